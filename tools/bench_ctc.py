"""Cost of the CTC forward score: the scoring launch alone (``stages.ctc_loss``, one vasr_ctc_loss_f32) and one
``CTCEvalLoss.update`` (the launch + the device-side sums), beside ``torch.nn.functional.ctc_loss(reduction='none')`` on the
same device tensors, at the two shapes of the other scoring benches: 64 x 10 s of QuartzNet15x5 (T' = 500, about 150 ids per
row) and the 512 x 30 s shard (T' = 1500, about 450 ids), 29 classes.  Each figure is also given as a share of that
workload's step (``QuartzNetCTC.forward`` on synthetic audio, timed here).  One JSON line (and --out FILE).

The log-probs are synthetic (a log_softmax of normal logits at scale 3), the targets random ids with a fifth of the neighbours
equal and lengths within 10 % of the mean; every row has a path.  Timed device-only: HIP events around --steps calls after
--warmup, three windows (median, min, max), nothing synchronises inside a window.  The two results are compared before
anything is timed (1e-4 relative).  Where torch's own call cannot run on the box, its error is recorded in place of a number.
The box's normalisers (bench.py's ``box_normalisers``) are measured in the same run, after the timed windows.  Single-run
figures; the windows give the spread.

    python tools/bench_ctc.py [--steps 50] [--warmup 5] [--skip-step] [--out profiles/ctc_bench.json]
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
from viet_asr_amd import configs, stages, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402
from viet_asr_amd.metrics import CTCEvalLoss  # noqa: E402

SHAPES = ((64, 10.0), (512, 30.0))
CHARS_PER_SECOND = 15.0


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


def synthetic(batch, frames, classes, mean_len, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(int(mean_len * 0.9), int(mean_len * 1.1) + 1, batch)
    tgt = rng.integers(0, classes - 1, (batch, int(lens.max())))
    same = rng.random(tgt.shape) < 0.2
    for i in range(1, tgt.shape[1]):
        tgt[:, i] = np.where(same[:, i], tgt[:, i - 1], tgt[:, i])
    gen = torch.Generator(device="cuda").manual_seed(seed)
    logp = torch.log_softmax(torch.randn((batch, frames, classes), device="cuda", generator=gen) * 3.0, dim=-1)
    full = torch.full((batch,), frames, dtype=torch.int64, device="cuda")
    return logp, full, torch.from_numpy(tgt).cuda(), torch.from_numpy(lens).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true", help="leave out the model's step (the shares are then not given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc.py measures on a HIP device; none found")
    cfg = configs.builtin("quartznet15x5")
    labels = cfg["labels"]
    classes = len(labels) + 1
    eng = None
    if not args.skip_step:
        jas = cfg["JasperEncoder"]["jasper"]
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, classes, 0))
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", classes=classes, runs=[])
    for batch, seconds in SHAPES:
        samples = int(seconds * 16000)
        t1 = int(seconds * 50) if eng is None else eng.frames(samples)[1]
        logp, frames, tgt, tgt_len = synthetic(batch, t1, classes, CHARS_PER_SECOND * seconds, seed=batch)
        ours = stages.ctc_loss(logp, frames, tgt, tgt_len, classes - 1)
        run = dict(batch=batch, seconds=seconds, frames=t1, tgt_width=int(tgt.shape[1]), mean_ids=round(float(tgt_len.float().mean()), 1),
                   mean_loss=round(float(ours.mean()), 3))
        assert bool(torch.isfinite(ours).all())
        steps = max(5, args.steps if batch <= 64 else args.steps // 5)
        run["kernel"] = _timed(lambda: stages.ctc_loss(logp, frames, tgt, tgt_len, classes - 1), steps, args.warmup)
        metric = CTCEvalLoss(classes - 1)
        run["update"] = _timed(lambda: metric.update(logp, frames, tgt, tgt_len), steps, args.warmup)
        metric.reset()
        lp_t = logp.transpose(0, 1)                     # [T', B, C], a view: what CTCLossNM hands nn.CTCLoss
        try:
            with torch.no_grad():
                call = lambda: F.ctc_loss(lp_t, tgt, frames, tgt_len, blank=classes - 1, reduction="none")  # noqa: E731
                theirs = call()
                run["max_rel_diff_vs_torch"] = float(((ours - theirs).abs() / theirs.abs()).max())
                assert run["max_rel_diff_vs_torch"] <= 1e-4, run
                run["torch"] = _timed(call, steps, args.warmup)
            run["torch_over_kernel"] = round(run["torch"]["ms"] / run["kernel"]["ms"], 2)
        except RuntimeError as e:                       # torch's own call cannot run here: recorded instead of a number
            run["torch"] = dict(error=str(e).splitlines()[0][:200])
        if eng is not None:
            sig, lens = synth.audio_batch(batch, samples, 0)
            x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
            fwd = lambda: eng.forward(x, n, want_pred=False)  # noqa: E731
            per = max(3, min(args.steps, int(2000 / (2.0 * batch * seconds / 64))))
            run["step"] = _timed(fwd, per, 2)
            run["kernel_share_of_step"] = round(run["kernel"]["ms"] / run["step"]["ms"], 5)
            run["update_share_of_step"] = round(run["update"]["ms"] / run["step"]["ms"], 5)
            del x, n
        out["runs"].append(run)
        del logp
        torch.cuda.empty_cache()
    out["box"] = normalisers()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
