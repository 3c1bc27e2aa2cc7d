"""Cost of the feature masks (csrc/spec_augment.hip) with the shipped SpectrogramAugmentation (rect_masks 5, rect_time 120,
rect_freq 50) at [64, 64, 1001] (64 x 10 s) and at the 512 x 30 s shard's [512, 64, 3001]:
  * the in-place launch (stores only) and the out-of-place launch (one masked copy), rectangles already on the device;
  * the whole ``SpectrogramAugmentation.forward`` (host draws, one pinned upload, the out-of-place launch), wall clock;
  * the same masks through ``torch.masked_fill`` as the reference runs it: the byte mask filled rectangle by rectangle on the
    host, converted to bool, uploaded, then ``x.masked_fill(mask, 0)`` -- wall clock for all of it, and the device part alone;
  * the fused call (``QuartzNetCTC.forward`` on QuartzNet15x5, synthetic audio) without and with ``spec_augment=``;
beside the floors: masked cells x 4 B of stores (in place) and one read plus one write of the tensor (out of place), both at
the box's measured copy rate (bench.py's ``box_normalisers``, measured in the same run, after the timed windows).
Device figures: HIP events around --steps calls after --warmup, three windows (median, min, max), nothing synchronises inside a
window.  Wall-clock figures: perf_counter around calls that end in a synchronisation.  Single-run figures; the windows give the
spread.  One JSON line (and --out FILE).

    python tools/bench_specaug.py [--steps 20] [--warmup 3] [--skip-step] [--out profiles/specaug_bench.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import asr, configs, stages, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402

SHAPES = ((64, 10.0), (512, 30.0))
SR, HOP, FEAT = 16000, 160, 64


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


def _wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return dict(ms=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4))


def normalisers():
    import bench
    box = bench.box_normalisers(torch.device("cuda:0"))
    return {k: box.get(k) for k in ("measured_mfma_tflops", "measured_copy_gbs")}


def host_mask(rects, row_begin, shape):
    """the reference's mask: a byte tensor filled slice by slice on the host, then bool"""
    mask = torch.zeros(shape).byte()
    for b in range(shape[0]):
        for f0, f1, t0, t1 in rects[row_begin[b]:row_begin[b + 1]]:
            mask[b, f0:f1, t0:t1] = 1
    return mask.type(torch.bool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true", help="leave out the fused call (the shares are then not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_specaug.py measures on a HIP device; none found")
    cfg = configs.builtin("quartznet15x5")
    section = configs.spectrogram_augmentation("quartznet15x5")
    eng = None
    if not args.skip_step:
        jas = cfg["JasperEncoder"]["jasper"]
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(cfg["labels"]) + 1, 0))
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", augmentation=section, runs=[])
    dev = torch.device("cuda:0")
    for batch, seconds in SHAPES:
        samples = int(seconds * SR)
        T = 1 + samples // HOP
        steps = max(3, args.steps if batch <= 64 else args.steps // 4)
        x = torch.randn((batch, FEAT, T), dtype=torch.float32, device=dev)
        rects, row_begin = asr.SpectrogramAugmentation(rng=random.Random(0), **section).draw(batch, FEAT, T)
        mask = host_mask(rects, row_begin, x.shape)
        cells = int(mask.sum())
        run = dict(batch=batch, seconds=seconds, shape=[batch, FEAT, T], tensor_bytes=x.numel() * 4, rectangles=int(len(rects)),
                   masked_cells=cells, masked_share=round(cells / x.numel(), 5))
        dr, db = stages.upload_masks(rects, row_begin, dev)
        buf, work = torch.empty_like(x), x.clone()
        got = stages.spec_mask(x, dr, db, out=buf)
        want = x.masked_fill(mask.to(dev), 0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(stages.spec_mask(work, dr, db, out=work).view(torch.int32), want.view(torch.int32))
        run["in_place"] = _timed(lambda: stages.spec_mask(work, dr, db, out=work), steps, args.warmup)
        run["out_of_place"] = _timed(lambda: stages.spec_mask(x, dr, db, out=buf), steps, args.warmup)
        module = asr.SpectrogramAugmentation(rng=random.Random(1), **section)
        run["module_forward_wall"] = _wall(lambda: module.forward(x), steps, args.warmup)
        dmask = mask.to(dev)
        run["torch_masked_fill_device_only"] = _timed(lambda: x.masked_fill(dmask, 0), steps, args.warmup)
        run["torch_masked_fill_reference_wall"] = _wall(lambda: x.masked_fill(host_mask(rects, row_begin, x.shape).to(dev), 0),
                                                        max(3, steps // 4), 1)
        del buf, work, got, want, dmask
        if eng is not None:
            sig, lens = synth.audio_batch(batch, samples, 0, ragged=True)
            wav, n = torch.from_numpy(sig).to(dev), torch.from_numpy(lens).to(dev)
            per = max(3, min(args.steps, int(2000 / (2.0 * batch * seconds / 64))))
            aug = asr.SpectrogramAugmentation(rng=random.Random(2), **section)
            run["step"] = _timed(lambda: eng.forward(wav, n, want_pred=False), per, 2)
            run["step_with_masks"] = _timed(lambda: eng.forward(wav, n, want_pred=False, spec_augment=aug), per, 2)
            launches = []
            for a in (None, aug):
                eng.handle.profile_begin()
                eng.forward(wav, n, want_pred=False, spec_augment=a)
                launches.append(sum(v["launches"] for v in eng.handle.profile_end().values()))
            run["launch_brackets_without_and_with_masks"] = launches
            del wav, n
        out["runs"].append(run)
        del x
        torch.cuda.empty_cache()
    out["box"] = normalisers()
    copy = out["box"].get("measured_copy_gbs")
    for run in out["runs"]:
        if copy:
            run["floor_ms_in_place_masked_cells_x_4B"] = round(4.0 * run["masked_cells"] / (copy * 1e9) * 1e3, 6)
            run["floor_ms_out_of_place_read_plus_write"] = round(2.0 * run["tensor_bytes"] / (copy * 1e9) * 1e3, 5)
        if "step" in run:
            for k in ("in_place", "out_of_place", "torch_masked_fill_device_only"):
                run[k]["share_of_step"] = round(run[k]["ms"] / run["step"]["ms"], 6)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
