"""Cost of the split at silences: the two launches of ``vasr_split_silence_f32 / _pcm16`` alone (chunk energies; flags, runs,
cuts and bounds) at 64 x 60 s and at 1 x 3 600 s -- float32 and int16 PCM --, each beside ``audio.trim_silence`` (three launches:
the same chunk energies, bounds, shifted copy) at the same shape in the same run, and beside the floor of ONE read of the tensor
at the box's own measured streaming rate (bench.py's ``box_normalisers``, measured in the same run, after the timed windows).
Then ``VietASR.transcribe_long`` (greedy, QuartzNet15x5, synthetic weights) on a synthetic one-hour recording of noise bursts and
pauses, beside ``QuartzNetCTC.forward_long`` on the same recording.  One JSON line (and --out FILE).

The split is timed in the form ``transcribe_long`` runs by default (pauses under 0.3 s bridged: 9 frames; runs cut at 16.7 s: 521
frames) and in librosa's own form (1, 0).  Device figures: HIP events around --steps calls after --warmup, three windows (median,
min, max), the calls reuse their buffers, nothing synchronises inside a window.  ``transcribe_long`` and ``forward_long`` are
wall-clock (perf_counter around the call and a device synchronisation), a first call and then the median, minimum and maximum
of three.  The device's counts are compared with ``audio.trim_silence``'s bounds (the first start and the last end of a row are
the trim's) before anything is timed.  Single-run figures; the windows give the spread.

    python tools/bench_split.py [--steps 50] [--warmup 5] [--skip-model] [--out profiles/split_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import _lib, audio, configs, synth  # noqa: E402

SHAPES = ((64, 60.0), (1, 3600.0))
RATE, TOP_DB, FRAME, HOP = 16000, 60.0, 2048, 512
FORMS = (("split", 9, 521), ("split_librosa_form", 1, 0))


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


def _wall(fn, repeats=3):
    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r
    first, r = once()
    ms = sorted(once()[0] for _ in range(repeats))
    return dict(first_ms=round(first, 2), ms=round(ms[len(ms) // 2], 2), ms_min=round(ms[0], 2), ms_max=round(ms[-1], 2)), r


def normalisers():
    import bench
    box = bench.box_normalisers(torch.device("cuda:0"))
    return {k: box.get(k) for k in ("measured_mfma_tflops", "measured_copy_gbs")}


def bursts_and_pauses(samples, seed):
    """float32 noise: bursts of 2-12 s at level 0.1 (one in eight 20-30 s long, with quieter stretches of 0.2 s every 5 s for
    the cuts to land on), pauses of 0.4-1.5 s at 1e-5 of that"""
    rng = np.random.default_rng(seed)
    amp = np.full(samples, 1e-6, np.float32)
    at, k = int(0.5 * RATE), 0
    while at < samples:
        long_one = k % 8 == 7
        n = int(rng.uniform(20.0, 30.0) * RATE) if long_one else int(rng.uniform(2.0, 12.0) * RATE)
        amp[at : at + n] = 0.1
        if long_one:
            for dip in range(at + 5 * RATE, min(at + n, samples) - RATE, 5 * RATE):
                amp[dip : dip + RATE // 5] = 0.01
        at += n + int(rng.uniform(0.4, 1.5) * RATE)
        k += 1
    x = rng.standard_normal(samples, dtype=np.float32)
    x *= amp
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-model", action="store_true", help="leave out transcribe_long and forward_long")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_split.py measures on a HIP device; none found")
    L = _lib.lib()
    out = dict(device=torch.cuda.get_device_name(0), top_db=TOP_DB, frame_length=FRAME, hop_length=HOP,
               forms={name: dict(min_silence_frames=m, max_segment_frames=M) for name, m, M in FORMS}, runs=[])
    hour = bursts_and_pauses(int(3600 * RATE), 0)
    for batch, seconds in SHAPES:
        samples = int(seconds * RATE)
        base = hour if batch == 1 else np.stack([bursts_and_pauses(samples, 100 + b) for b in range(batch)])
        base = base.reshape(batch, samples)
        for dtype in ("float32", "int16"):
            sig = base if dtype == "float32" else np.clip(np.round(base.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
            x = torch.from_numpy(sig).cuda()
            n = torch.full((batch,), samples, dtype=torch.int64, device="cuda")
            N = 1 + samples // HOP
            bounds = torch.empty((batch, N, 2), dtype=torch.int64, device="cuda")
            count = torch.empty((batch,), dtype=torch.int64, device="cuda")
            ws = torch.empty(int(L.vasr_split_silence_workspace_bytes(batch, samples, FRAME, HOP)), dtype=torch.uint8, device="cuda")
            entry = L.vasr_split_silence_pcm16 if dtype == "int16" else L.vasr_split_silence_f32
            stream = torch.cuda.current_stream().cuda_stream

            def split(m, M):
                _lib.check(entry(x.data_ptr(), samples, n.data_ptr(), batch, TOP_DB, FRAME, HOP, m, M, bounds.data_ptr(), N,
                                 count.data_ptr(), ws.data_ptr(), ws.numel(), stream))

            tbuf = (torch.empty_like(x), torch.empty_like(n), torch.empty(
                int(L.vasr_trim_silence_workspace_bytes(batch, samples, FRAME, HOP)), dtype=torch.uint8, device="cuda"))
            _, t_len, t_start = audio.trim_silence(x, n, TOP_DB, FRAME, HOP, out=tbuf[0], start=tbuf[1], workspace=tbuf[2])
            run = dict(batch=batch, seconds=seconds, dtype=dtype, tensor_bytes=int(sig.nbytes), workspace_bytes=int(ws.numel()))
            for name, m, M in FORMS:
                split(m, M)
                c, b_host = count.cpu().numpy(), bounds.cpu().numpy()
                assert (c >= 1).all() and (c <= N).all()
                assert [int(b_host[r, 0, 0]) for r in range(batch)] == t_start.cpu().tolist()          # the trim's outer bounds
                assert [int(b_host[r, c[r] - 1, 1]) for r in range(batch)] == (t_start + t_len).cpu().tolist()
                run[name + "_segments"] = int(c.sum())
            steps = max(5, args.steps)
            for name, m, M in FORMS:
                run[name] = _timed(lambda: split(m, M), steps, args.warmup)
            run["trim"] = _timed(lambda: audio.trim_silence(x, n, TOP_DB, FRAME, HOP, out=tbuf[0], start=tbuf[1], workspace=tbuf[2]),
                                 steps, args.warmup)
            run["split_over_trim"] = round(run["split"]["ms"] / run["trim"]["ms"], 3)
            out["runs"].append(run)
            del x, bounds, ws, tbuf
            torch.cuda.empty_cache()
    if not args.skip_model:
        from viet_asr_amd.infer import VietASR
        cfg = configs.builtin("quartznet15x5")
        jas = cfg["JasperEncoder"]["jasper"]
        tmp = tempfile.mkdtemp(prefix="vasr_split_bench_")
        enc_p, dec_p = os.path.join(tmp, "JasperEncoder-STEP-1.pt"), os.path.join(tmp, "JasperDecoderForCTC-STEP-1.pt")
        torch.save({k: torch.as_tensor(v) for k, v in synth.encoder_state_dict(jas, 64, 0).items()}, enc_p)
        torch.save({k: torch.as_tensor(v) for k, v in synth.decoder_state_dict(1024, len(cfg["labels"]) + 1, 0).items()}, dec_p)
        asr = VietASR("quartznet15x5", enc_p, dec_p, device="gpu", decoder="greedy")
        eng = asr._fused_engine()
        long_run, res = _wall(lambda: asr.transcribe_long(hour))
        seg = [s["end"] - s["start"] for s in res["segments"]]
        wav = torch.from_numpy(hour).cuda()
        fl_run, fl = _wall(lambda: eng.forward_long(wav))
        out["one_hour"] = dict(model="quartznet15x5", decoder="greedy", batch_size=64, segments=len(seg), dropped=res["dropped"],
                               segment_seconds_total=round(float(sum(seg)), 1), segment_seconds_max=round(float(max(seg)), 2),
                               transcribe_long=long_run, forward_long=fl_run,
                               forward_long_workspace_bytes=int(fl["workspace_bytes"]),
                               peak_memory_bytes=int(torch.cuda.max_memory_allocated()))
    out["box"] = normalisers()
    copy = out["box"].get("measured_copy_gbs")
    for run in out["runs"]:
        if copy:
            run["floor_ms_one_read_at_measured_copy"] = round(run["tensor_bytes"] / (copy * 1e9) * 1e3, 5)
            run["floor_over_split"] = round(run["floor_ms_one_read_at_measured_copy"] / run["split"]["ms"], 3)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
