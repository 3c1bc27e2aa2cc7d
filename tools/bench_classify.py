"""Cost of the speech-classification path: a 128-filter separable encoder with audio_length 128 on the fused call
(engine.QuartzNetClassifier, vasr_classify_f32), batch 1 and batch 128 of 1 s clips, f16x2 (the default arithmetic): ms per
call, and the pool + linear launches' own time from the per-class profile of one pass (vasr_profile_end, class "head")
beside their floor -- the B * C * T' * 4 bytes the pool has to read over a copy rate (--copy-gbs: what ``bench.py --full``
reports as box.measured_copy_gbs) -- one JSON line.  Single-run figures.

    python tools/bench_classify.py [--steps 50] [--warmup 10] [--copy-gbs 0]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetClassifier  # noqa: E402

AUDIO_LENGTH, CLASSES, FILTERS = 128, 35, 128


def _blk(kernel, repeat, residual):
    return dict(filters=FILTERS, repeat=repeat, kernel=[kernel], stride=[1], dilation=[1], dropout=0.0, residual=residual,
                separable=True)


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--copy-gbs", type=float, default=0.0, help="device copy rate in GB/s for the pool's floor (0: not given)")
    args = ap.parse_args()
    jas = [_blk(11, 1, False), _blk(13, 2, True), _blk(15, 2, True), _blk(17, 1, False)]
    cfg = configs.jasper_definition(jas)
    eng = QuartzNetClassifier(cfg, synth.encoder_state_dict(jas, 64, 0), synth.classifier_state_dict(FILTERS, CLASSES, 0),
                              AUDIO_LENGTH)
    out = dict(model=f"separable 4 x {FILTERS}", audio_length=AUDIO_LENGTH, classes=CLASSES, gemm=eng.handle.gemm_mode_name(),
               device=torch.cuda.get_device_name(0), runs=[])
    for batch in (1, 128):
        sig, lens = synth.audio_batch(batch, 16000, 0)
        x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
        ms = _time(lambda: eng.forward(x, n), args.steps, args.warmup)
        eng.handle.profile_begin()
        eng.forward(x, n)
        torch.cuda.synchronize()
        prof = eng.handle.profile_end()
        t1 = eng.handle.encoded_frames(AUDIO_LENGTH)
        pool_bytes = batch * FILTERS * t1 * 4
        run = dict(batch=batch, ms_per_call=round(ms, 4), pool_linear_us=round(prof["head"]["ms"] * 1e3, 2),
                   pool_linear_launches=prof["head"]["launches"], pool_bytes=pool_bytes,
                   classes_ms={k: round(v["ms"], 4) for k, v in prof.items()})
        if args.copy_gbs > 0:
            run["pool_floor_us"] = round(pool_bytes / (args.copy_gbs * 1e9) * 1e6, 3)
        out["runs"].append(run)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
