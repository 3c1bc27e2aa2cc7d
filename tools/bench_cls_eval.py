"""Cost of one ``TopKAccuracy.update`` (metrics.py: one vasr_class_scores_f32 launch + the device-side sums) beside what the
parent commit would run for the same result -- ``logits.topk`` + ``F.cross_entropy`` in torch on the device, summed the same
way -- at (B, C) = (128, 35) and (4096, 1000) with top_k = (1, 5).  One JSON line (and --out FILE).

Both sides are timed device-only: HIP events around --steps calls after --warmup, three windows (median, min, max), nothing
synchronises inside a window.  `kernel` is the scoring launch alone (stages.classification_scores).  The two results are
compared before anything is timed: the counts exactly, the loss to 1e-5 relative.  The box's normalisers (bench.py's
``box_normalisers``: sustained MFMA TFLOP/s and copy GB/s) are measured in the same run, after the timed windows.
Single-run figures; the windows give the spread.

    python tools/bench_cls_eval.py [--steps 200] [--warmup 20] [--out profiles/cls_eval_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import stages  # noqa: E402
from viet_asr_amd.metrics import TopKAccuracy  # noqa: E402

SHAPES = ((128, 35), (4096, 1000))
TOP_K = (1, 5)


class TorchTopK:
    """The same accumulators from torch's own operators: what a caller of the parent commit would write."""

    def __init__(self, top_k):
        self.top_k, self._acc, self._loss = sorted(top_k), None, None

    def update(self, logits, targets):
        _, pred = logits.topk(max(self.top_k), dim=1, largest=True, sorted=True)
        correct = pred.eq(targets.view(-1, 1))
        hits = torch.stack([correct[:, :k].sum(dtype=torch.int64) for k in self.top_k])
        n = torch.full((1,), logits.shape[0], dtype=torch.int64, device=logits.device)
        bad = ((targets < 0) | (targets >= logits.shape[1])).sum(dtype=torch.int64).reshape(1)
        row = torch.cat([hits, n, bad])
        pair = torch.stack([F.cross_entropy(logits, targets), torch.ones((), device=logits.device)])
        self._acc = row if self._acc is None else self._acc + row
        self._loss = pair if self._loss is None else self._loss + pair

    def compute(self):
        host, (s, b) = self._acc.cpu().tolist(), self._loss.cpu().tolist()
        return dict(correct={k: host[i] for i, k in enumerate(self.top_k)}, samples=host[len(self.top_k)], eval_loss=s / b)


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
    """What this box sustains, now: bench.py's own two figures (its f16x2 MFMA stream, a streaming pass over 2 x 1 GiB)."""
    import bench
    box = bench.box_normalisers(torch.device("cuda:0"))
    return {k: box.get(k) for k in ("measured_mfma_tflops", "measured_copy_gbs")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cls_eval.py measures on a HIP device; none found")
    out = dict(device=torch.cuda.get_device_name(0), top_k=list(TOP_K), runs=[])
    for B, Cn in SHAPES:
        rng = np.random.default_rng(B)
        logits = torch.from_numpy(rng.standard_normal((B, Cn)).astype(np.float32)).cuda()
        targets = torch.from_numpy(rng.integers(0, Cn, B)).cuda()
        ours, theirs = TopKAccuracy(TOP_K), TorchTopK(TOP_K)
        ours.update(logits, targets); theirs.update(logits, targets)
        a, b = ours.compute(), theirs.compute()
        assert a["correct"] == b["correct"] and a["samples"] == b["samples"] == B, (a, b)
        assert abs(a["eval_loss"] - b["eval_loss"]) <= 1e-5 * abs(b["eval_loss"]), (a, b)
        run = dict(batch=B, classes=Cn, result=dict(correct=a["correct"], eval_loss=a["eval_loss"]),
                   kernel=_timed(lambda: stages.classification_scores(logits, targets), args.steps, args.warmup),
                   update=_timed(lambda: ours.update(logits, targets), args.steps, args.warmup),
                   torch_update=_timed(lambda: theirs.update(logits, targets), args.steps, args.warmup))
        run["torch_over_update"] = round(run["torch_update"]["ms"] / run["update"]["ms"], 2)
        out["runs"].append(run)
    out["box"] = normalisers()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
