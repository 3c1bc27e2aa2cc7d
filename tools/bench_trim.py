"""Cost of the silence trim: the three launches of ``audio.trim_silence`` alone (vasr_trim_silence_f32 / _pcm16: chunk
energies, bounds, shifted copy) at 64 x 10 s -- float32 and int16 PCM -- and at the 512 x 30 s shard, beside the step of
bench.py's workload (``QuartzNetCTC.forward`` on QuartzNet15x5, synthetic audio) without and with ``trim_silence=True``, and
beside a numpy restatement of the trim on the host for the same batch (the librosa recipe: reflect pad, framed mean of
squares, threshold, slice and collate again).  One JSON line (and --out FILE).

The floor recorded next to each device figure is three passes over the tensor -- one read for the energies, one read and one
write for the copy -- at the box's own measured streaming rate (bench.py's ``box_normalisers``, measured in the same run,
after the timed windows).  The rows are noise with silent margins of 5-20 % on both sides, so the trim really cuts.  Timed
device-only: HIP events around --steps calls after --warmup, three windows (median, min, max), nothing synchronises inside a
window; the host restatement is timed with perf_counter over one pass (two at the small shape).  The device result is compared
with the host restatement's bounds before anything is timed.  Single-run figures; the windows give the spread.

    python tools/bench_trim.py [--steps 50] [--warmup 5] [--skip-step] [--out profiles/trim_bench.json]
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

SHAPES = ((64, 10.0, "float32"), (64, 10.0, "int16"), (512, 30.0, "float32"))
TOP_DB, FRAME, HOP, AMIN = 60.0, 2048, 512, 1e-10


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


def host_trim_bounds(x, n):
    """librosa.effects.trim's recipe in numpy on one row (float64 energies) -> (start, end)"""
    y = x[:n].astype(np.float64) * (2.0 ** -15 if x.dtype == np.int16 else 1.0)
    y = np.pad(y, FRAME // 2, mode="reflect")
    frames = np.lib.stride_tricks.sliding_window_view(y, FRAME)[::HOP][: 1 + n // HOP]
    mse = np.mean(frames ** 2, axis=1)
    db = 10.0 * np.log10(np.maximum(AMIN, mse)) - 10.0 * np.log10(max(AMIN, mse.max()))
    nz = np.flatnonzero(db > -TOP_DB)
    return (int(nz[0]) * HOP, min(n, (int(nz[-1]) + 1) * HOP)) if nz.size else (0, 0)


def host_trim(batch, lens):
    """the whole host pass: bounds per row, then a second collate of the trimmed rows"""
    bounds = [host_trim_bounds(batch[b], int(lens[b])) for b in range(batch.shape[0])]
    out = np.zeros_like(batch)
    for b, (s, e) in enumerate(bounds):
        out[b, : e - s] = batch[b, s:e]
    return out, bounds


def with_margins(sig, lens, seed):
    """silence (1e-5 of the level) over 5-20 % of every row at both ends"""
    rng = np.random.default_rng(seed)
    sig = sig.copy()
    for b, n in enumerate(lens):
        lead, tail = (int(n * f) for f in rng.uniform(0.05, 0.2, 2))
        sig[b, :lead] *= 1e-5
        sig[b, n - tail : n] *= 1e-5
    return sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true", help="leave out the model's step (the shares are then not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trim.py measures on a HIP device; none found")
    cfg = configs.builtin("quartznet15x5")
    eng = None
    if not args.skip_step:
        jas = cfg["JasperEncoder"]["jasper"]
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(cfg["labels"]) + 1, 0))
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", top_db=TOP_DB, frame_length=FRAME, hop_length=HOP, runs=[])
    for batch, seconds, dtype in SHAPES:
        samples = int(seconds * 16000)
        sig, lens = synth.audio_batch(batch, samples, 0, ragged=True)
        sig = with_margins(sig, lens, batch)
        if dtype == "int16":
            sig = np.clip(np.round(sig.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
        x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
        t0 = time.perf_counter()
        reps = 2 if batch <= 64 else 1
        for _ in range(reps):
            _, bounds = host_trim(sig, lens)
        host_ms = (time.perf_counter() - t0) / reps * 1e3
        got, got_len, got_start = audio.trim_silence(x, n, TOP_DB, FRAME, HOP)
        assert got_start.cpu().tolist() == [s for s, _ in bounds] and got_len.cpu().tolist() == [e - s for s, e in bounds]
        kept = float(got_len.sum()) / float(n.sum())
        nbytes = sig.nbytes
        buf = (torch.empty_like(x), torch.empty_like(n), torch.empty(
            int(_lib.lib().vasr_trim_silence_workspace_bytes(batch, samples, FRAME, HOP)), dtype=torch.uint8, device="cuda"))
        steps = max(5, args.steps if batch <= 64 else args.steps // 5)
        run = dict(batch=batch, seconds=seconds, dtype=dtype, tensor_bytes=nbytes, workspace_bytes=int(buf[2].numel()),
                   kept_fraction=round(kept, 4), host_numpy_ms=round(host_ms, 2))
        run["trim"] = _timed(lambda: audio.trim_silence(x, n, TOP_DB, FRAME, HOP, out=buf[0], start=buf[1], workspace=buf[2]),
                             steps, args.warmup)
        run["host_over_trim"] = round(host_ms / run["trim"]["ms"], 1)
        if eng is not None:
            per = max(3, min(args.steps, int(2000 / (2.0 * batch * seconds / 64))))
            run["step"] = _timed(lambda: eng.forward(x, n, want_pred=False), per, 2)
            run["step_with_trim"] = _timed(lambda: eng.forward(x, n, want_pred=False, trim_silence=True), per, 2)
            run["trim_share_of_step"] = round(run["trim"]["ms"] / run["step"]["ms"], 5)
        out["runs"].append(run)
        del x, n, got, buf
        torch.cuda.empty_cache()
    out["box"] = normalisers()
    copy = out["box"].get("measured_copy_gbs")
    for run in out["runs"]:
        if copy:
            run["floor_ms_three_passes_at_measured_copy"] = round(3.0 * run["tensor_bytes"] / (copy * 1e9) * 1e3, 5)
            run["floor_over_trim"] = round(run["floor_ms_three_passes_at_measured_copy"] / run["trim"]["ms"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
