"""Cost of the audio perturbations (csrc/perturb.hip): every launch alone -- ``audio.mean_square``, ``audio.noise_plan``,
``audio.mix`` (gain + shift + noise in one pass) and ``audio.convolve`` with impulse responses of 0.25 s, 0.5 s and 1 s -- at
64 x 10 s and at the 512 x 30 s shard, beside
  * the same convolution as a ``torch.fft.rfft * irfft`` composition on the same device tensors (one transform of the next power
    of two per row, the whole batch at once where it fits in memory, in slices of rows otherwise),
  * ``scipy.signal.fftconvolve`` (numpy where scipy is absent) over the rows on the host, at the small shape,
  * one read plus one write of the tensor at the box's measured streaming rate, the floor of the mix
    (bench.py's ``box_normalisers``, measured in the same run, after the timed windows),
  * the step of bench.py's workload (``QuartzNetCTC.forward`` on QuartzNet15x5, synthetic audio), of which every figure is given
    as a share.
Timed device-only: HIP events around --steps calls after --warmup, three windows (median, min, max), nothing synchronises inside
a window.  The convolution is compared with the torch.fft composition before anything is timed.  Single-run figures; the windows
give the spread.  One JSON line (and --out FILE).

    python tools/bench_perturb.py [--steps 20] [--warmup 3] [--skip-step] [--out profiles/perturb_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import _lib, audio, configs, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402

SHAPES = ((64, 10.0), (512, 30.0))
IR_SECONDS = (0.25, 0.5, 1.0)
SR = 16000


def _window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _timed(fn, steps, warmup, windows=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = sorted(_window(fn, steps) for _ in range(windows))
    return dict(ms=round(ms[len(ms) // 2], 5), ms_min=round(ms[0], 5), ms_max=round(ms[-1], 5))


def normalisers():
    import bench
    box = bench.box_normalisers(torch.device("cuda:0"))
    return {k: box.get(k) for k in ("measured_mfma_tflops", "measured_copy_gbs")}


def torch_fft_convolve(x, h, rows_per_slice):
    """x [B, L] (zero behind the rows), h [B, m] -> [B, L + m - 1]: one rfft / irfft of the next power of two per row"""
    B, L = x.shape
    m = h.shape[1]
    nfft = 1 << (L + m - 2).bit_length()
    out = torch.empty((B, L + m - 1), dtype=torch.float32, device=x.device)
    for lo in range(0, B, rows_per_slice):
        hi = min(B, lo + rows_per_slice)
        spec = torch.fft.rfft(x[lo:hi], nfft) * torch.fft.rfft(h[lo:hi], nfft)
        out[lo:hi] = torch.fft.irfft(spec, nfft)[:, : L + m - 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true", help="leave out the model's step (the shares are then not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_perturb.py measures on a HIP device; none found")
    cfg = configs.builtin("quartznet15x5")
    eng = None
    if not args.skip_step:
        jas = cfg["JasperEncoder"]["jasper"]
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(cfg["labels"]) + 1, 0))
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", sample_rate=SR, runs=[])
    rng = np.random.RandomState(0)
    for batch, seconds in SHAPES:
        samples = int(seconds * SR)
        sig, lens = synth.audio_batch(batch, samples, 0, ragged=True)
        x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
        steps = max(3, args.steps if batch <= 64 else args.steps // 5)
        run = dict(batch=batch, seconds=seconds, tensor_bytes=sig.nbytes)
        if eng is not None:
            per = max(3, min(args.steps, int(2000 / (2.0 * batch * seconds / 64))))
            run["step"] = _timed(lambda: eng.forward(x, n, want_pred=False), per, 2)
        # the memory-bound launches
        noise = torch.from_numpy((rng.standard_normal((4, samples + 16000)) * 0.05).astype(np.float32)).cuda()
        noise_len = torch.full((4,), samples + 16000, dtype=torch.int64, device="cuda")
        ms_v = audio.mean_square(noise, noise_len)
        row = torch.arange(batch, dtype=torch.int32, device="cuda") % 4
        snr = torch.full((batch,), 10.0, dtype=torch.float64, device="cuda")
        u = torch.rand(batch, dtype=torch.float64, device="cuda")
        gain = torch.full((batch,), 0.7, dtype=torch.float32, device="cuda")
        shift = torch.full((batch,), 80, dtype=torch.int64, device="cuda")
        ws = torch.empty(int(_lib.lib().vasr_mean_square_workspace_bytes(batch, samples)), dtype=torch.uint8, device="cuda")
        buf = torch.empty_like(x)
        run["mean_square"] = _timed(lambda: audio.mean_square(x, n, workspace=ws), steps, args.warmup)
        ms_x = audio.mean_square(x, n)
        run["noise_plan"] = _timed(lambda: audio.noise_plan(n, ms_x, row, snr, u, noise_len, ms_v, 300.0, SR), steps, args.warmup)
        scale, start = audio.noise_plan(n, ms_x, row, snr, u, noise_len, ms_v, 300.0, SR)
        run["mix_gain_shift_noise"] = _timed(lambda: audio.mix(x, n, gain=gain, shift=shift, add=noise, add_len=noise_len,
                                                               add_row=row, scale=scale, start=start, out=buf), steps, args.warmup)
        run["mix_gain_only"] = _timed(lambda: audio.mix(x, n, gain=gain, out=buf), steps, args.warmup)
        del noise, buf
        # the convolution
        run["convolve"] = []
        for ir_s in IR_SECONDS:
            m = int(ir_s * SR)
            h = (rng.standard_normal((8, m)) * np.exp(-np.arange(m) / (m / 6.0))).astype(np.float32)
            bank = audio.ImpulseBank(torch.from_numpy(h).cuda(), torch.full((8,), m, dtype=torch.int64, device="cuda"))
            rows = torch.arange(batch, dtype=torch.int32, device="cuda") % 8
            obuf = torch.empty((batch, samples + m - 1), dtype=torch.float32, device="cuda")
            xz = x.clone()                                     # zero behind the rows for the composition (synth pads with zeros)
            hb = bank.responses[rows.long()]
            per_slice = batch if batch * samples <= 64 * 10 * SR * 2 else 64
            got, _ = audio.convolve(x, n, bank, rows, out=obuf)
            want = torch_fft_convolve(xz, hb, per_slice)
            err = float((got - want).abs().max() / want.abs().max())
            assert err < 1e-4, err
            c = dict(ir_seconds=ir_s, taps=m, max_rel_diff_to_torch_fft=err)
            c["prepare"] = _timed(lambda: audio.ImpulseBank(bank.responses, bank.lengths), 3, 1)
            c["device"] = _timed(lambda: audio.convolve(x, n, bank, rows, out=obuf), steps, args.warmup)
            c["torch_fft"] = _timed(lambda: torch_fft_convolve(xz, hb, per_slice), max(3, steps // 2), 2)
            c["torch_fft_over_device"] = round(c["torch_fft"]["ms"] / c["device"]["ms"], 3)
            if batch <= 64:
                try:
                    from scipy.signal import fftconvolve as host_conv
                    c["host"] = "scipy.signal.fftconvolve"
                except ImportError:
                    host_conv = lambda a, b, mode: np.convolve(a, b)       # noqa: E731
                    c["host"] = "numpy.convolve"
                t0 = time.perf_counter()
                for b in range(batch):
                    host_conv(sig[b, : lens[b]], h[b % 8], "full")
                c["host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            run["convolve"].append(c)
            del bank, obuf, xz, hb, got, want
            torch.cuda.empty_cache()
        out["runs"].append(run)
        del x, n
        torch.cuda.empty_cache()
    out["box"] = normalisers()
    copy = out["box"].get("measured_copy_gbs")
    for run in out["runs"]:
        if copy:
            run["floor_ms_read_plus_write_at_measured_copy"] = round(2.0 * run["tensor_bytes"] / (copy * 1e9) * 1e3, 5)
        if "step" in run:
            for k in ("mean_square", "noise_plan", "mix_gain_shift_noise", "mix_gain_only"):
                run[k]["share_of_step"] = round(run[k]["ms"] / run["step"]["ms"], 5)
            for c in run["convolve"]:
                c["device"]["share_of_step"] = round(c["device"]["ms"] / run["step"]["ms"], 5)
                c["torch_fft"]["share_of_step"] = round(c["torch_fft"]["ms"] / run["step"]["ms"], 5)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
