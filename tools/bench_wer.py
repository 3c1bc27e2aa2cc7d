"""Cost of scoring WER / CER on the device (stages.error_counts, metrics.ErrorRate) beside the host scorer it replaces, at the
transcript shapes of 64 x 10 s and 512 x 30 s -- one JSON line (and --out FILE).

Inputs are synthetic id batches: the reference is random text over the labels at 13.3 characters per second (400 per 30 s
clip) with one character in six a space (five-letter words); the hypothesis is the reference with about 10 % random
substitutions, insertions and deletions, in a [B, T'] batch as wide as the encoder's output for that clip length.

  (a) device time of one scoring launch: HIP events around --steps launches after --warmup, three windows (median, min, max);
      and of one bare 4096 x 4096 pair, the widest the entry point takes;
  (b) wall time of data_layer.word_error_rate on the same pairs as strings, use_cer False and True (one pass each: seconds);
  (c) the QuartzNetCTC step (quartznet15x5, f16x2) with and without ErrorRate.update enqueued behind it, alternating windows:
      scoring's share of a step.  Scored are the realistic synthetic ids of (a); `own_ids` scores the synthetic model's own
      output instead (what evaluate_manifest enqueues), whose rows are far longer than speech gives -- mean length reported.
Single-run figures; the windows give the spread.

    python tools/bench_wer.py [--steps 50] [--warmup 10] [--skip-host] [--out profiles/wer_bench.json]
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
from viet_asr_amd import configs, stages, synth  # noqa: E402
from viet_asr_amd.data_layer import word_error_rate  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402
from viet_asr_amd.metrics import ErrorRate  # noqa: E402

CHARS_PER_SECOND, SPACE_P, EDIT_P = 400 / 30.0, 1 / 6.0, 0.10
SHAPES = ((64, 10.0), (512, 30.0))


def synthetic_pairs(labels, batch, seconds, width, seed):
    """-> (hyp [B, width] i32, hyp_len, ref [B, R] i32, ref_len) numpy, and the same pairs as strings."""
    rng = np.random.default_rng(seed)
    space = labels.index(" ")
    letters = [i for i in range(len(labels)) if i != space]
    n_ref = int(round(CHARS_PER_SECOND * seconds))
    hyps, refs = [], []
    for _ in range(batch):
        ref = np.where(rng.random(n_ref) < SPACE_P, space, rng.choice(letters, n_ref))
        hyp = []
        for c in ref.tolist():
            u = rng.random()
            if u < EDIT_P / 3:
                continue
            hyp.append(int(rng.integers(len(labels))) if u < 2 * EDIT_P / 3 else c)
            if u > 1 - EDIT_P / 3:
                hyp.append(int(rng.integers(len(labels))))
        refs.append(ref.tolist())
        hyps.append(hyp[:width])
    def pad(rows, w):
        out = np.zeros((len(rows), w), dtype=np.int32)
        for k, r in enumerate(rows):
            out[k, : len(r)] = r
        return out, np.array([len(r) for r in rows], dtype=np.int32)
    hyp, hn = pad(hyps, width)
    ref, rn = pad(refs, n_ref)
    text = lambda rows: ["".join(labels[c] for c in r) for r in rows]  # noqa: E731
    return (hyp, hn, ref, rn), (text(hyps), text(refs))


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
    return dict(ms=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true", help="leave out (b), the host scorer (minutes at 512 x 30 s)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wer.py measures on a HIP device; none found")
    cfg = configs.builtin("quartznet15x5")
    labels = cfg["labels"]
    jas = cfg["JasperEncoder"]["jasper"]
    eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(labels) + 1, 0))
    metric = ErrorRate(labels)
    out = dict(device=torch.cuda.get_device_name(0), model="quartznet15x5", gemm=eng.handle.gemm_mode_name(),
               chars_per_second=round(CHARS_PER_SECOND, 2), space_p=round(SPACE_P, 4), edit_p=EDIT_P, runs=[])
    cuda = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    for batch, seconds in SHAPES:
        samples = int(seconds * 16000)
        _, t1 = eng.frames(samples)
        arrays, (hyps, refs) = synthetic_pairs(labels, batch, seconds, t1, seed=batch)
        hyp, hn, ref, rn = (cuda(a) for a in arrays)
        run = dict(batch=batch, seconds=seconds, hyp_width=t1, ref_width=int(ref.shape[1]),
                   cells_char=int((arrays[1].astype(np.int64) * arrays[3]).sum()))
        # (a) the scoring launch alone
        score = lambda: stages.error_counts(hyp, hn, ref, rn, metric.space_ids)  # noqa: E731
        run["device_scoring"] = _timed(score, args.steps, args.warmup)
        metric.reset()
        metric.update(hyp, hn, ref, rn)
        dev = metric.compute()
        run["device_result"] = dev
        # (b) the host scorer on the same pairs
        if not args.skip_host:
            t0 = time.perf_counter(); wer = word_error_rate(hyps, refs); t1_ = time.perf_counter()
            cer = word_error_rate(hyps, refs, use_cer=True); t2 = time.perf_counter()
            assert (wer, cer) == (dev["wer"], dev["cer"]), (wer, cer, dev)
            run["host_scorer"] = dict(wer_ms=round((t1_ - t0) * 1e3, 1), cer_ms=round((t2 - t1_) * 1e3, 1),
                                      both_ms=round((t2 - t0) * 1e3, 1))
            run["host_over_device"] = round(run["host_scorer"]["both_ms"] / run["device_scoring"]["ms"], 1)
        # (c) the step with and without scoring enqueued behind it
        sig, lens = synth.audio_batch(batch, samples, 0)
        x, n = cuda(sig), cuda(lens)
        steps = max(3, min(args.steps, int(2000 / (2.0 * batch * seconds / 64))))     # about half a second per window

        def plain():
            return eng.forward(x, n, want_pred=False)

        def scored():
            eng.forward(x, n, want_pred=False)
            metric.update(hyp, hn, ref, rn)

        def scored_own():
            r = eng.forward(x, n, want_pred=False)
            metric.update(r["ids"], r["id_len"], ref, rn)

        for fn in (plain, scored, scored_own):
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        w = {"plain": [], "scored": [], "scored_own": []}
        for _ in range(3):                                      # alternate: drift hits all three alike
            for name, fn in (("plain", plain), ("scored", scored), ("scored_own", scored_own)):
                w[name].append(_window(fn, steps))
        med = {k: sorted(v)[1] for k, v in w.items()}
        own_len = float(plain()["id_len"].float().mean())
        run["step"] = dict(steps_per_window=steps, plain_ms=round(med["plain"], 4), scored_ms=round(med["scored"], 4),
                           scored_own_ids_ms=round(med["scored_own"], 4),
                           plain_windows_ms=[round(v, 4) for v in w["plain"]], scored_windows_ms=[round(v, 4) for v in w["scored"]],
                           scoring_share_of_step=round((med["scored"] - med["plain"]) / med["plain"], 5),
                           own_ids_share_of_step=round((med["scored_own"] - med["plain"]) / med["plain"], 5),
                           own_ids_mean_len=round(own_len, 1))
        metric.reset()
        out["runs"].append(run)
    # the widest pair the entry point takes, alone on the device
    rng = np.random.default_rng(4096)
    wide = rng.integers(0, len(labels), (1, 4096)).astype(np.int32)
    other = np.where(rng.random((1, 4096)) < 0.1, rng.integers(0, len(labels), (1, 4096)), wide).astype(np.int32)
    full = cuda(np.array([4096], dtype=np.int32))
    a, b = cuda(wide), cuda(other)
    out["pair_4096x4096"] = _timed(lambda: stages.error_counts(a, full, b, full, metric.space_ids), max(5, args.steps // 5), 3)
    out["pair_4096x4096"]["over_512x30s_step"] = round(out["pair_4096x4096"]["ms"] / out["runs"][-1]["step"]["plain_ms"], 4)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
