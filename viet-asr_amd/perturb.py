"""Audio perturbation on the device: the counterpart of nemo/collections/asr/parts/perturb.py for robustness sweeps.

The reference perturbs one ``AudioSegment`` at a time on the host (``WaveformFeaturizer.process``: after the trim, in front of
the features).  Here a padded batch that already sits on the device is perturbed there: the random PARAMETERS are drawn on
the host, per row in batch order, consuming every generator exactly as the reference's per-utterance calls do --
``rng.random() < prob`` per pipeline entry on the augmentor's generator, then that perturbation's own ``uniform`` / ``sample``
draws in the reference's order (the noise start takes the single ``random()`` that ``uniform(0.0, .)`` consumes) -- and
uploaded as small per-row arrays; the ARITHMETIC runs in the kernels of csrc/perturb.hip (``audio.mean_square``,
``audio.noise_plan``, ``audio.mix``, ``audio.convolve``; include/vasr.h has the semantics).  A row that does not draw a
perturbation gets its identity parameters (gain 1, shift 0, scale 0, response -1), which leave it bit for bit as it was.

Stated differences from the reference:
  * white noise: the level is drawn as the reference draws it (``RandomState.randint``), the SAMPLES come from the device's
    own generator (``torch.randn`` on the batch's device, as ``dither`` does): ``numpy.RandomState.randn`` is not reproduced;
  * a noise recording that is not longer than the utterance wraps around (the reference raises);
  * ``rms_db`` takes the mean square in float64 (the reference in float32) and the gain in product form; silence gets no
    noise (the reference: 0 or NaN);
  * noise and impulse recordings are read once, when the perturbation is built (``audio.read_wav``, PCM WAV), resampled on
    the device where their rate differs (``audio.resample``, not librosa's resampler) and kept as padded device banks with
    their lengths, and their mean squares / partition spectra, computed once per device and sample rate;
  * ``max_augmentation_length`` adds the longest impulse response - 1, which the reference forgets;
  * ``SpeedPerturbation`` (librosa's phase vocoder) is not implemented and raises NotImplementedError.
"""
import json
import math
import random

import numpy as np
import torch

from . import audio


def _manifest_files(manifest_path):
    files = []
    for path in str(manifest_path).split(","):
        with open(path, encoding="utf-8") as f:
            files += [json.loads(line)["audio_filepath"] for line in f if line.strip()]
    return files


class Perturbation(object):
    kind = None

    def max_augmentation_length(self, length):
        return length

    def draw(self, n, sample_rate):
        """The reference's draws for one utterance of n samples -> a dict of parameters."""
        raise NotImplementedError


class SpeedPerturbation(Perturbation):
    def __init__(self, min_speed_rate=0.85, max_speed_rate=1.15, rng=None):
        raise NotImplementedError("SpeedPerturbation (librosa.effects.time_stretch, a phase vocoder) is not implemented")


class GainPerturbation(Perturbation):
    kind = "gain"

    def __init__(self, min_gain_dbfs=-10, max_gain_dbfs=10, rng=None):
        self._min_gain_dbfs = min_gain_dbfs
        self._max_gain_dbfs = max_gain_dbfs
        self._rng = random.Random() if rng is None else rng

    def draw(self, n, sample_rate):
        return dict(gain_db=self._rng.uniform(self._min_gain_dbfs, self._max_gain_dbfs))


class ShiftPerturbation(Perturbation):
    kind = "shift"

    def __init__(self, min_shift_ms=-5.0, max_shift_ms=5.0, rng=None):
        self._min_shift_ms = min_shift_ms
        self._max_shift_ms = max_shift_ms
        self._rng = random.Random() if rng is None else rng

    def draw(self, n, sample_rate):
        shift_ms = self._rng.uniform(self._min_shift_ms, self._max_shift_ms)
        samples = 0                                         # perturb.py:71-74: ignored when longer than the utterance
        if not abs(shift_ms) / 1000 > n / float(sample_rate):
            samples = int(shift_ms * sample_rate // 1000)
        return dict(shift_ms=shift_ms, shift=samples)


class _Bank(object):
    """Recordings read once on the host; padded device banks per (device, sample rate)."""

    def __init__(self, manifest_path, signals):
        if signals is None:
            if manifest_path is None:
                raise ValueError("a manifest_path (or signals=[(samples, sample_rate), ...]) is required")
            signals = [audio.read_wav(p) for p in _manifest_files(manifest_path)]
        self._host = [(np.ascontiguousarray(x, dtype=np.float32), int(sr)) for x, sr in signals]
        if not self._host:
            raise ValueError("the manifest holds no recording")
        self._banks = {}

    def __len__(self):
        return len(self._host)

    def host_length(self, i, sample_rate):
        x, sr = self._host[i]
        return len(x) if sr == sample_rate else int(math.ceil(len(x) * (float(sample_rate) / sr)))

    def rows(self, device, sample_rate):
        """-> (bank [R, L] float32 on the device, zero padded; lengths [R] int64 there)"""
        key = (str(device), int(sample_rate))
        if key not in self._banks:
            rows = []
            for x, sr in self._host:
                t = torch.from_numpy(x).to(device)
                if sr != sample_rate:
                    y, n = audio.resample(t[None], torch.tensor([len(x)], device=device), sr, sample_rate)
                    t = y[0, : int(n[0])]
                rows.append(t)
            width = max(1, max(int(t.numel()) for t in rows))
            bank = torch.zeros((len(rows), width), dtype=torch.float32, device=device)
            for i, t in enumerate(rows):
                bank[i, : t.numel()] = t
            lens = torch.tensor([int(t.numel()) for t in rows], dtype=torch.int64, device=device)
            self._banks[key] = self._finish(bank, lens)
        return self._banks[key]

    def _finish(self, bank, lens):
        return bank, lens


class _NoiseBank(_Bank):
    def _finish(self, bank, lens):
        return bank, lens, audio.mean_square(bank, lens)


class _ImpulseBank(_Bank):
    def _finish(self, bank, lens):
        return audio.ImpulseBank(bank, lens)


class NoisePerturbation(Perturbation):
    kind = "noise"

    def __init__(self, manifest_path=None, min_snr_db=40, max_snr_db=50, max_gain_db=300.0, rng=None, signals=None):
        """signals (not in the reference): [(samples, sample_rate), ...] instead of a manifest of files."""
        self._bank = _NoiseBank(manifest_path, signals)
        self._rng = random.Random() if rng is None else rng
        self._min_snr_db = min_snr_db
        self._max_snr_db = max_snr_db
        self._max_gain_db = max_gain_db

    def draw(self, n, sample_rate):
        snr_db = self._rng.uniform(self._min_snr_db, self._max_snr_db)
        row = self._rng.sample(range(len(self._bank)), 1)[0]
        return dict(snr_db=snr_db, row=row, u=self._rng.random())      # uniform(0.0, d) is 0.0 + d * random()


class ImpulsePerturbation(Perturbation):
    kind = "impulse"

    def __init__(self, manifest_path=None, rng=None, signals=None):
        """signals (not in the reference): [(samples, sample_rate), ...] instead of a manifest of files."""
        self._bank = _ImpulseBank(manifest_path, signals)
        self._rng = random.Random() if rng is None else rng

    def max_augmentation_length(self, length, sample_rate=None):
        longest = max(self._bank.host_length(i, sample_rate or self._bank._host[i][1]) for i in range(len(self._bank)))
        return length + longest - 1

    def draw(self, n, sample_rate):
        return dict(row=self._rng.sample(range(len(self._bank)), 1)[0])


class WhiteNoisePerturbation(Perturbation):
    kind = "white_noise"

    def __init__(self, min_level=-90, max_level=-46, rng=None):
        self.min_level = int(min_level)
        self.max_level = int(max_level)
        self._rng = np.random.RandomState() if rng is None else rng

    def draw(self, n, sample_rate):
        return dict(level_db=int(self._rng.randint(self.min_level, self.max_level, dtype="int32")))


perturbation_types = {
    "speed": SpeedPerturbation,
    "gain": GainPerturbation,
    "impulse": ImpulsePerturbation,
    "shift": ShiftPerturbation,
    "noise": NoisePerturbation,
    "white_noise": WhiteNoisePerturbation,
}


class AudioAugmentor(object):
    def __init__(self, perturbations=None, rng=None):
        self._rng = random.Random() if rng is None else rng
        self._pipeline = perturbations if perturbations is not None else []

    @classmethod
    def from_config(cls, config):
        ptbs = []
        for p in config:
            if p["aug_type"] not in perturbation_types:
                continue                                    # the reference warns and skips
            ptbs.append((p["prob"], perturbation_types[p["aug_type"]](**p["cfg"])))
        return cls(perturbations=ptbs)

    def max_augmentation_length(self, length, sample_rate=None):
        """The longest a signal of ``length`` samples can become.  sample_rate: the batch's, where impulse responses are
        stored at another rate."""
        newlen = length
        for _, p in self._pipeline:
            if isinstance(p, ImpulsePerturbation):
                newlen = p.max_augmentation_length(newlen, sample_rate)
            else:
                newlen = p.max_augmentation_length(newlen)
        return newlen

    def draw_batch(self, lengths, sample_rate):
        """The host half: -> per pipeline entry, a list of B parameter dicts (None where the row did not draw the entry).  Rows
        in batch order, entries in pipeline order inside a row, as B calls of the reference's ``perturb`` would consume the
        generators.  An impulse changes the length the entries behind it see."""
        plan = [[None] * len(lengths) for _ in self._pipeline]
        for b, n in enumerate(lengths):
            n = int(n)
            for k, (prob, p) in enumerate(self._pipeline):
                if self._rng.random() < prob:
                    d = p.draw(n, sample_rate)
                    plan[k][b] = d
                    if p.kind == "impulse" and n > 0:
                        n = n + p._bank.host_length(d["row"], sample_rate) - 1
        return plan

    def perturb_batch(self, signal, length, sample_rate, lengths_host=None):
        """signal [B, L] float32 cuda (rows zero padded or not: the padding is never read), length [B] int64 ->
        (signal' [B, L'], length' [B] int64 on the device), L' = L unless an impulse response was drawn.  Everything is enqueued
        on the current stream.  lengths_host: the lengths as a sequence where the caller has them (the shift's duration rule
        and the order of the draws need them on the host); without it ``length`` is read back, which synchronises."""
        if lengths_host is None:
            lengths_host = length.cpu().tolist()
        plan = self.draw_batch(lengths_host, sample_rate)
        dev = signal.device
        B = signal.shape[0]
        x, ln = signal, length
        k = 0
        while k < len(self._pipeline):
            p = self._pipeline[k][1]
            rows = plan[k]
            if all(d is None for d in rows):
                k += 1
                continue
            if p.kind in ("gain", "shift"):
                # a gain and a shift next to each other are one pass (a row's gain commutes with its shift)
                gain = shift = None
                while k < len(self._pipeline):
                    q = self._pipeline[k][1]
                    if q.kind == "gain" and gain is None:
                        gain = [1.0 if d is None else 10.0 ** (d["gain_db"] / 20.0) for d in plan[k]]
                    elif q.kind == "shift" and shift is None:
                        shift = [0 if d is None else d["shift"] for d in plan[k]]
                    else:
                        break
                    k += 1
                x = audio.mix(x, ln, gain=gain, shift=shift)
                continue
            if p.kind == "noise":
                bank, bank_len, ms_v = p._bank.rows(dev, sample_rate)
                ms_x = audio.mean_square(x, ln)
                row = [-1 if d is None else d["row"] for d in rows]
                scale, start = audio.noise_plan(ln, ms_x, row, [0.0 if d is None else d["snr_db"] for d in rows],
                                                [0.0 if d is None else d["u"] for d in rows], bank_len, ms_v, p._max_gain_db,
                                                sample_rate)
                x = audio.mix(x, ln, add=bank, add_len=bank_len, add_row=row, scale=scale, start=start)
            elif p.kind == "white_noise":
                noise = torch.randn(x.shape, dtype=torch.float32, device=dev)
                scale = [0.0 if d is None else 10.0 ** (d["level_db"] / 20.0) for d in rows]
                x = audio.mix(x, ln, add=noise, add_len=[x.shape[1]] * B, add_row=list(range(B)), scale=scale)
            elif p.kind == "impulse":
                x, ln = audio.convolve(x, ln, p._bank.rows(dev, sample_rate), [-1 if d is None else d["row"] for d in rows])
            else:
                raise NotImplementedError(f"{type(p).__name__} has no device form")
            k += 1
        return x, ln
