"""Audio ingest for the callers of the path: WAV decoding, int -> float scaling, device resampling.

Reference behaviour being mirrored:
  * ``AudioSegment`` (nemo/collections/asr/parts/segment.py:19-32, 61-74): integer samples scaled by
    2^-(bits-1) to float32, multi-channel averaged to mono, optional resample to the target rate;
  * the CLI / web app decode with ``librosa.load(path, sr=16000)`` (infer.py:200, app.py:66,82), whose default
    resampler is resampy's ``kaiser_best`` -- third-party and absent here (parity unpinned); ``sinc_table`` /
    ``resample`` implement that published scheme on the device (csrc/audio.hip).
File decoding uses the standard library ``wave`` module (PCM WAV only; the reference's soundfile/librosa stack is
not in this image).
"""
import wave

import numpy as np
import torch

from . import _lib

KAISER_BEST = dict(num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492)
KAISER_FAST = dict(num_zeros=16, precision=9, rolloff=0.85, beta=8.555504641634386)


def read_wav(path):
    """-> (samples float32 mono in [-1, 1), sample_rate).  8/16/24/32-bit PCM."""
    with wave.open(path, "rb") as w:
        sr, nch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) * (1.0 / 2 ** 15)
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(np.float32) * (1.0 / 2 ** 23)
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) * (1.0 / 2 ** 31)
    else:
        raise TypeError(f"Unsupported sample width: {width} bytes")
    if nch > 1:
        x = x.reshape(-1, nch).mean(axis=1)          # segment.py:31-32
    return x.astype(np.float32), sr


def write_wav(path, samples, sr):
    """float32 [-1,1) -> 16-bit PCM WAV (test / tooling helper)."""
    pcm = np.clip(np.round(np.asarray(samples, dtype=np.float64) * 32768.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.writeframes(pcm.tobytes())


def sinc_table(ratio=1.0, num_zeros=64, precision=9, rolloff=0.9475937167399596, beta=14.769656459379492):
    """One-sided Kaiser-windowed sinc + forward differences, as [n+1, 2] float32 (resampy ``sinc_window``)."""
    num_bits = 2 ** precision
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    win = taper * sinc_win
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    return np.stack([win, delta], axis=1).astype(np.float32), num_bits


_tables = {}


def resample(signal, length, sr_in, sr_out, filter="kaiser_best"):
    """signal [B, L] float32 cuda (padding: anything, it is never read), length [B] int64 cuda -> (signal' [B, L'], length'),
    rows of signal' zero from int(n * ratio) on.

    Lengths follow ``librosa.load(sr=...)`` -> ``librosa.resample(fix=True)`` (infer.py:200): resampy computes
    ``int(n * ratio)`` samples, librosa pads them with zeros to ``ceil(n * ratio)`` (both in float64: 5 000 samples at
    11 025 -> 16 000 Hz come out as 7 257, the last one zero)."""
    if sr_in == sr_out:
        return signal, length
    if signal.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    params = {"kaiser_best": KAISER_BEST, "kaiser_fast": KAISER_FAST}[filter]
    ratio = float(sr_out) / float(sr_in)
    key = (signal.device, filter, ratio < 1 and ratio)
    if key not in _tables:
        tab, num_table = sinc_table(ratio, **params)
        _tables[key] = (torch.from_numpy(tab).to(signal.device), num_table)
    tab, num_table = _tables[key]
    x = signal.to(torch.float32).contiguous()
    ln = length.to(torch.int64).contiguous()
    B, L = x.shape
    L_out = int(np.ceil(L * ratio))
    y = torch.empty((B, max(L_out, 1)), dtype=torch.float32, device=x.device)
    ln_out = torch.empty((B,), dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().vasr_resample_f32(x.data_ptr(), L, ln.data_ptr(), B, tab.data_ptr(), tab.shape[0], num_table,
                                            ratio, y.data_ptr(), y.shape[1], ln_out.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    return y, ln_out


def trim_silence(signal, length, top_db=60.0, frame_length=2048, hop_length=512, out=None, start=None, workspace=None):
    """signal [B, L] float32 or int16 cuda (padding: anything), length [B] int64 cuda ->
    (trimmed [B, L] of the same dtype, zero behind each row, length' [B] int64, start [B] int64).

    ``AudioSegment(trim=True)`` -> ``librosa.effects.trim(samples, top_db)`` (parts/segment.py:19-32; librosa < 0.10,
    third-party arithmetic restated from its published form, parity unpinned) on the device: vasr_trim_silence_f32 / _pcm16 in
    include/vasr.h have the semantics.  Three launches on the current stream, no synchronisation: the padded width stays L.
    out / start / workspace: buffers of the caller's to write into ([B, L] of signal's dtype; [B] int64; uint8 of at least
    vasr_trim_silence_workspace_bytes) instead of fresh ones."""
    if signal.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    if signal.dtype not in (torch.float32, torch.int16) or signal.dim() != 2:
        raise ValueError("trim_silence expects a [B, L] float32 or int16 cuda tensor")
    x = signal.contiguous()
    ln = length.to(device=x.device, dtype=torch.int64).contiguous()
    B, L = x.shape
    L_lib = _lib.lib()
    if out is None:
        out = torch.empty((B, L), dtype=x.dtype, device=x.device)
    if out.dtype != x.dtype or out.device != x.device or tuple(out.shape) != (B, L) or not out.is_contiguous():
        raise ValueError("out must be a contiguous [B, L] tensor of signal's dtype on its device")
    ln_out = torch.empty((B,), dtype=torch.int64, device=x.device)
    if start is None:
        start = torch.empty((B,), dtype=torch.int64, device=x.device)
    need = int(L_lib.vasr_trim_silence_workspace_bytes(B, L, int(frame_length), int(hop_length)))
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
    entry = L_lib.vasr_trim_silence_pcm16 if x.dtype == torch.int16 else L_lib.vasr_trim_silence_f32
    _lib.check(entry(x.data_ptr(), L, ln.data_ptr(), B, float(top_db), int(frame_length), int(hop_length), out.data_ptr(),
                     out.shape[1], ln_out.data_ptr(), start.data_ptr(), workspace.data_ptr(), workspace.numel(),
                     torch.cuda.current_stream(x.device).cuda_stream))
    return out, ln_out, start


def split_silence(signal, length, top_db=60.0, frame_length=2048, hop_length=512, min_silence_frames=1, max_segment_frames=0,
                  max_segments=None, workspace=None):
    """signal [B, L] float32 or int16 cuda (padding: anything), length [B] int64 cuda ->
    (bounds [B, N, 2] int64: (start, end) in samples, ascending; count [B] int64), device tensors, no synchronisation.

    The non-silent intervals of every row: ``librosa.effects.split(y, top_db, ref=np.max, frame_length, hop_length)`` (librosa
    < 0.10, third-party arithmetic restated from its published form, parity unpinned) with two rules on top: a pause of fewer
    than ``min_silence_frames`` frames is bridged, and a run longer than ``max_segment_frames`` frames (0: no limit) is cut at
    its quietest frame; vasr_split_silence_f32 / _pcm16 in include/vasr.h have the semantics.  Entries of ``bounds`` at and
    behind ``min(count, N)`` are not written; ``count`` is the row's total also where it exceeds N.  max_segments=None takes
    N = 1 + L // hop_length, the most a row can have.  workspace: a uint8 buffer of the caller's of at least
    vasr_split_silence_workspace_bytes."""
    if signal.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    if signal.dtype not in (torch.float32, torch.int16) or signal.dim() != 2:
        raise ValueError("split_silence expects a [B, L] float32 or int16 cuda tensor")
    x = signal.contiguous()
    ln = length.to(device=x.device, dtype=torch.int64).contiguous()
    B, L = x.shape
    L_lib = _lib.lib()
    N = 1 + L // max(int(hop_length), 1) if max_segments is None else int(max_segments)
    bounds = torch.empty((B, max(N, 1), 2), dtype=torch.int64, device=x.device)      # never NULL, also for a count-only call
    count = torch.empty((B,), dtype=torch.int64, device=x.device)
    need = int(L_lib.vasr_split_silence_workspace_bytes(B, L, int(frame_length), int(hop_length)))
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
    entry = L_lib.vasr_split_silence_pcm16 if x.dtype == torch.int16 else L_lib.vasr_split_silence_f32
    _lib.check(entry(x.data_ptr(), L, ln.data_ptr(), B, float(top_db), int(frame_length), int(hop_length), int(min_silence_frames),
                     int(max_segment_frames), bounds.data_ptr(), N, count.data_ptr(),
                     workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(x.device).cuda_stream))
    return bounds[:, : max(N, 0)], count


def gather_segments(signal, rows, starts, lengths, width=None):
    """signal [B, L] float32 or int16 cuda; rows [S] (int32), starts [S], lengths [S] (int64): tensors or sequences ->
    out [S, width] of signal's dtype: out[s] = signal[rows[s], starts[s] : starts[s] + lengths[s]] and zeros behind it
    (vasr_gather_segments_f32 / _pcm16; a descriptor that does not lie inside its row, or is longer than ``width``, gives a row
    of zeros).  width=None takes the longest length, which reads ``lengths`` on the host when it is a device tensor."""
    if signal.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    if signal.dtype not in (torch.float32, torch.int16) or signal.dim() != 2:
        raise ValueError("gather_segments expects a [B, L] float32 or int16 cuda tensor")
    x = signal.contiguous()
    B, L = x.shape
    r = torch.as_tensor(rows).to(device=x.device, dtype=torch.int32).contiguous()
    s = torch.as_tensor(starts).to(device=x.device, dtype=torch.int64).contiguous()
    n = torch.as_tensor(lengths)
    S = int(r.numel())
    if int(s.numel()) != S or int(n.numel()) != S:
        raise ValueError("rows, starts and lengths must have one entry per segment")
    if width is None:
        width = int(n.max()) if S else 0
    width = max(int(width), 1)
    n = n.to(device=x.device, dtype=torch.int64).contiguous()
    out = torch.empty((S, width), dtype=x.dtype, device=x.device)
    if S == 0:
        return out
    entry = _lib.lib().vasr_gather_segments_pcm16 if x.dtype == torch.int16 else _lib.lib().vasr_gather_segments_f32
    _lib.check(entry(x.data_ptr(), L, B, r.data_ptr(), s.data_ptr(), n.data_ptr(), S, out.data_ptr(), width,
                     torch.cuda.current_stream(x.device).cuda_stream))
    return out


def plan_segments(bounds, count, lengths, pad=0, min_samples=0):
    """The host side between ``split_silence`` and ``gather_segments``: bounds [B, N, 2], count [B], lengths [B] (tensors on any
    device, arrays or lists) -> (segments, dropped): the flat list of (row, start, length) in row order, ascending inside a row,
    and the number of segments dropped per row (a list of B integers).  Integers only.  Reading ``count`` is the one
    synchronisation of the long-recording path: the shape of the batches depends on it.

    Every segment is widened by ``pad`` samples on both sides, then clamped to its row [0, lengths[b]) and to the midpoint of
    the gap to its neighbour -- the midpoint (start of the next + end of this) // 2 belongs to the next one --, so segments
    never overlap; a segment of ``min_samples`` or fewer samples after that is dropped.  A count beyond N (the device table
    overflowed) raises ValueError."""
    def host(t):
        return t.cpu().tolist() if isinstance(t, torch.Tensor) else np.asarray(t).tolist()
    c_host, n_host = host(count), host(lengths)
    held = int(bounds.shape[1]) if isinstance(bounds, torch.Tensor) else len(bounds[0]) if len(bounds) else 0
    used = min(held, max([int(c) for c in c_host], default=0))
    b_host = host(bounds[:, :used]) if isinstance(bounds, torch.Tensor) else bounds     # only the entries that were written
    pad, min_samples = int(pad), int(min_samples)
    segments, dropped = [], []
    for b, c in enumerate(c_host):
        c, n = int(c), max(int(n_host[b]), 0)
        if c > held:
            raise ValueError(f"row {b} has {c} segments, the table holds {held}: pass a larger max_segments")
        segs = [(int(s), int(e)) for s, e in b_host[b][:c]]
        lost = 0
        for k, (s, e) in enumerate(segs):
            lo = (segs[k - 1][1] + s) // 2 if k > 0 else 0
            hi = (e + segs[k + 1][0]) // 2 if k + 1 < c else n
            s2, e2 = max(s - pad, lo, 0), min(e + pad, hi, n)
            if e2 - s2 > min_samples:
                segments.append((b, s2, e2 - s2))
            else:
                lost += 1
        dropped.append(lost)
    return segments, dropped


def _f32_batch(signal, length, what):
    if signal.device.type != "cuda":
        raise _lib.VasrError("viet-asr_amd kernels need HIP-resident tensors; there is no CPU fallback for this path")
    if signal.dtype != torch.float32 or signal.dim() != 2:
        raise ValueError(f"{what} expects a [B, L] float32 cuda tensor (int16 PCM: pcm16_to_float first)")
    x = signal.contiguous()
    return x, length.to(device=x.device, dtype=torch.int64).contiguous()


def _opt(t, device, dtype):
    return None if t is None else torch.as_tensor(t).to(device=device, dtype=dtype).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def mean_square(signal, length, workspace=None):
    """signal [B, L] float32 cuda (padding: anything), length [B] int64 -> mean(x^2) per row, [B] float64 on the device: the
    argument of ``AudioSegment.rms_db`` (vasr_mean_square_f32: float64 sums in a fixed order; an empty row gives 0).  Two launches,
    no synchronisation."""
    x, ln = _f32_batch(signal, length, "mean_square")
    B, L = x.shape
    ms = torch.empty((B,), dtype=torch.float64, device=x.device)
    need = int(_lib.lib().vasr_mean_square_workspace_bytes(B, L))
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().vasr_mean_square_f32(x.data_ptr(), L, ln.data_ptr(), B, ms.data_ptr(), workspace.data_ptr(),
                                               workspace.numel(), torch.cuda.current_stream(x.device).cuda_stream))
    return ms


def noise_plan(length, ms_x, rows, snr_db, u, noise_len, ms_v, max_gain_db, sample_rate):
    """NoisePerturbation's gain and start per row on the device (vasr_noise_plan_f64): length [B] i64, ms_x [B] f64, rows [B]
    i32 (-1: no noise), snr_db [B] f64, u [B] f64 in [0, 1), noise_len [R] i64, ms_v [R] f64 -> (scale [B] f32, start [B] i64)."""
    dev = ms_x.device
    ln, mx = _opt(length, dev, torch.int64), _opt(ms_x, dev, torch.float64)
    r, s, uu = _opt(rows, dev, torch.int32), _opt(snr_db, dev, torch.float64), _opt(u, dev, torch.float64)
    nl, mv = _opt(noise_len, dev, torch.int64), _opt(ms_v, dev, torch.float64)
    B = int(ln.numel())
    if any(int(t.numel()) != B for t in (mx, r, s, uu)) or int(nl.numel()) != int(mv.numel()):
        raise ValueError("noise_plan: one entry per row (length, ms_x, rows, snr_db, u) and per noise (noise_len, ms_v)")
    scale = torch.empty((B,), dtype=torch.float32, device=dev)
    start = torch.empty((B,), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().vasr_noise_plan_f64(ln.data_ptr(), mx.data_ptr(), r.data_ptr(), s.data_ptr(), uu.data_ptr(), B,
                                              nl.data_ptr(), mv.data_ptr(), int(nl.numel()), float(max_gain_db), int(sample_rate),
                                              scale.data_ptr(), start.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return scale, start


def mix(signal, length, gain=None, shift=None, add=None, add_len=None, add_row=None, scale=None, start=None, out=None):
    """out[b][t] = gain[b] * x[b][t + shift[b]] + scale[b] * add[add_row[b]][(start[b] + t) mod add_len] for t < length[b], zeros
    behind; the lengths do not change (vasr_mix_f32: GainPerturbation, ShiftPerturbation, NoisePerturbation's and
    WhiteNoisePerturbation's sum in one pass).  gain [B] f32, shift [B] i64 (samples), add [R, La] f32 with add_len [R] i64,
    add_row [B] i32, scale [B] f32, start [B] i64; gain, shift, add and start may be None (1, 0, nothing, 0).  out: a
    contiguous float32 [B, >= L] tensor of the caller's."""
    x, ln = _f32_batch(signal, length, "mix")
    B, L = x.shape
    dev = x.device
    if out is None:
        out = torch.empty((B, L), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.device != dev or out.dim() != 2 or out.shape[0] != B or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [B, >= L] tensor on signal's device")
    g, sh = _opt(gain, dev, torch.float32), _opt(shift, dev, torch.int64)
    a = al = ar = sc = st = None
    ld_add = rows = 0
    if add is not None:
        if add.dim() != 2 or add.dtype != torch.float32 or add.device != dev:
            raise ValueError("add must be a [R, La] float32 tensor on signal's device")
        a = add.contiguous()
        rows, ld_add = a.shape
        al, ar = _opt(add_len, dev, torch.int64), _opt(add_row, dev, torch.int32)
        sc, st = _opt(scale, dev, torch.float32), _opt(start, dev, torch.int64)
    _lib.check(_lib.lib().vasr_mix_f32(x.data_ptr(), L, ln.data_ptr(), B, _ptr(g), _ptr(sh), _ptr(a), ld_add, rows, _ptr(al),
                                       _ptr(ar), _ptr(sc), _ptr(st), out.data_ptr(), out.shape[1],
                                       torch.cuda.current_stream(dev).cuda_stream))
    return out


class ImpulseBank:
    """Impulse responses [R, Lh] float32 cuda with their lengths, and their partition spectra computed once
    (vasr_convolve_prepare_f32)."""

    def __init__(self, responses, lengths):
        h, ln = _f32_batch(responses, lengths, "ImpulseBank")
        self.responses, self.lengths = h, ln
        self.R, self.ld = int(h.shape[0]), int(h.shape[1])
        L = _lib.lib()
        # the refusals (too many taps: NotImplementedError) come from the call itself
        need = int(L.vasr_convolve_spectra_bytes(self.R, self.ld))
        self.spectra = torch.empty(max(need, 8), dtype=torch.uint8, device=h.device)
        _lib.check(L.vasr_convolve_prepare_f32(h.data_ptr(), self.ld, ln.data_ptr(), self.R, self.spectra.data_ptr(),
                                               self.spectra.numel(), torch.cuda.current_stream(h.device).cuda_stream))


def convolve(signal, length, bank, rows, out=None):
    """signal [B, L] float32 cuda, length [B] i64, bank: an ImpulseBank, rows [B] i32 (-1: the row is copied) ->
    (out [B, L + bank.ld - 1], length' [B] i64): ``scipy.signal.fftconvolve(x, h, "full")`` per row, length n + m - 1
    (vasr_convolve_f32: partitioned overlap-save in one kernel).  One launch, no synchronisation."""
    x, ln = _f32_batch(signal, length, "convolve")
    B, L = x.shape
    r = _opt(rows, x.device, torch.int32)
    width = max(L + bank.ld - 1, 1)
    if out is None:
        out = torch.empty((B, width), dtype=torch.float32, device=x.device)
    if out.dtype != torch.float32 or out.device != x.device or out.dim() != 2 or out.shape[0] != B or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [B, >= L + bank.ld - 1] tensor on signal's device")
    ln_out = torch.empty((B,), dtype=torch.int64, device=x.device)
    _lib.check(_lib.lib().vasr_convolve_f32(x.data_ptr(), L, ln.data_ptr(), B, r.data_ptr(), bank.lengths.data_ptr(),
                                            bank.spectra.data_ptr(), bank.R, bank.ld, out.data_ptr(), out.shape[1],
                                            ln_out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream))
    return out, ln_out


def pcm16_to_float(pcm):
    """int16 cuda tensor -> float32 / 32768 on the device (halves the host->device bytes of a batch)."""
    if pcm.device.type != "cuda" or pcm.dtype != torch.int16:
        raise ValueError("pcm16_to_float expects an int16 cuda tensor")
    p = pcm.contiguous()
    out = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    _lib.check(_lib.lib().vasr_pcm16_to_f32(p.data_ptr(), p.numel(), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out
