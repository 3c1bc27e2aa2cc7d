"""Cost of the forced CTC alignment: the align launch (``stages.ctc_align``, one vasr_ctc_align_f32 and its workspace
allocation) beside the scoring launch (``stages.ctc_loss``, one vasr_ctc_loss_f32) on the same device tensors, at the two
shapes of tools/bench_ctc.py: 64 x 10 s of QuartzNet15x5 (T' = 501, about 150 ids per row) and the 512 x 30 s shard (T' = 1501,
about 450 ids), 29 classes.  The back-pointer workspace of each shape is recorded.  One JSON line (and --out FILE).

The log-probs and targets are bench_ctc.py's synthetic ones; every row has a path.  Timed device-only: HIP events around
--steps calls after --warmup, three windows (median, min, max), nothing synchronises inside a window.  Before anything is
timed the best path is checked to score no more than the sum over paths, and every token to have a span.  The box's
normalisers (bench.py's ``box_normalisers``) are measured in the same run, after the timed windows.  Single-run figures; the
windows give the spread.

    python tools/bench_ctc_align.py [--steps 50] [--warmup 5] [--out profiles/ctc_align_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from bench_ctc import CHARS_PER_SECOND, SHAPES, _timed, normalisers, synthetic  # noqa: E402
from viet_asr_amd import _lib, configs, stages  # noqa: E402

FRAMES_PER_SECOND = 50          # a hop of 160 samples at 16 kHz and the encoder's stride of 2; + 1 frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_align.py measures on a HIP device; none found")
    classes = len(configs.builtin("quartznet15x5")["labels"]) + 1
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", classes=classes, runs=[])
    for batch, seconds in SHAPES:
        t1 = int(seconds * FRAMES_PER_SECOND) + 1
        logp, frames, tgt, tgt_len = synthetic(batch, t1, classes, CHARS_PER_SECOND * seconds, seed=batch)
        loss = stages.ctc_loss(logp, frames, tgt, tgt_len, classes - 1)
        got = stages.ctc_align(logp, frames, tgt, tgt_len, classes - 1, want_path=True)
        assert bool(torch.isfinite(got["score"]).all()) and bool((got["score"] <= -loss + 1e-3).all())
        inside = torch.arange(tgt.shape[1], device="cuda")[None] < tgt_len[:, None]
        assert bool((got["end"] > got["start"])[inside].all()) and bool((got["start"][~inside] == -1).all())
        run = dict(batch=batch, seconds=seconds, frames=t1, tgt_width=int(tgt.shape[1]), mean_ids=round(float(tgt_len.float().mean()), 1),
                   mean_score=round(float(got["score"].mean()), 3), mean_loss=round(float(loss.mean()), 3),
                   workspace_bytes=int(_lib.lib().vasr_ctc_align_workspace_bytes(batch, t1, int(tgt.shape[1]))))
        steps = max(5, args.steps if batch <= 64 else args.steps // 5)
        run["loss"] = _timed(lambda: stages.ctc_loss(logp, frames, tgt, tgt_len, classes - 1), steps, args.warmup)
        run["align"] = _timed(lambda: stages.ctc_align(logp, frames, tgt, tgt_len, classes - 1), steps, args.warmup)
        run["align_with_path"] = _timed(lambda: stages.ctc_align(logp, frames, tgt, tgt_len, classes - 1, want_path=True), steps,
                                        args.warmup)
        run["align_over_loss"] = round(run["align"]["ms"] / run["loss"]["ms"], 2)
        out["runs"].append(run)
        del logp, got
        torch.cuda.empty_cache()
    out["box"] = normalisers()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
