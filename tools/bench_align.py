"""Cost of the S/D/I breakdown, the word edit script and the n-best oracle scoring on the device beside the yardstick they
share a table with, stages.error_counts (vasr_error_counts_i32), on the inputs of tools/bench_wer.py: 64 x 10 s and 512 x 30 s
of synthetic transcripts (its ``synthetic_pairs``), hypothesis buffers as wide as the encoder's output for the clip length
(hop 160, stride 2: 501 and 1501 ids).  One JSON line (and --out FILE).

  error_counts          the yardstick, unchanged by this tool;
  error_ops             vasr_error_ops_i32, counts only: the same cells and barriers, one more count per cell;
  error_ops_script      the same with the word edit script; the script form takes widths up to 1024, so the 1501-wide
                        hypothesis buffer of the 30 s shape is cut to 1024 columns (its rows are about 400 ids long) -- the
                        yardstick is timed on the cut buffer too (`error_counts_cut`), since the LDS a workgroup asks for, and
                        with it the workgroups per compute unit, follow the WIDTH;
  nbest_error_counts    vasr_nbest_error_counts_i32 at nbest 8: slot 0 is the hypothesis, slots 1..7 carry 5 % more
                        substitutions each; all 8 filled.

Device time: HIP events around --steps calls after --warmup, three windows per form, the forms alternating window by window
so that drift hits all alike (median, min, max); nothing synchronises inside a window.  Every call includes what the stages
wrapper does per call (the output allocation).  Before anything is timed the results are checked against each other: sub + del
+ ins = the yardstick's edits, slot 0 of the n-best counts = the yardstick's rows, the script's op counts = the word counts.
The box's normalisers (bench.py's ``box_normalisers``) are measured in the same run, after the timed windows.  Single-run
figures; the windows give the spread.

    python tools/bench_align.py [--steps 50] [--warmup 10] [--out profiles/align_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, stages  # noqa: E402
from viet_asr_amd.metrics import space_ids  # noqa: E402
from bench_wer import SHAPES, _window, synthetic_pairs  # noqa: E402

NBEST, SCRIPT_WIDTH = 8, 1024


def encoded_frames(seconds):
    """QuartzNet's output frames for a clip: samples // hop + 1 mel frames (hop 160), halved (rounded up) by the stride-2 block"""
    return (int(seconds * 16000) // 160 + 1 + 1) // 2


def nbest_batch(hyp, hn, n_labels, seed):
    rng = np.random.default_rng(seed)
    slots = [hyp]
    for s in range(1, NBEST):
        noise = rng.random(hyp.shape) < 0.05 * s
        slots.append(np.where(noise, rng.integers(0, n_labels, hyp.shape), hyp).astype(np.int32))
    return np.ascontiguousarray(np.stack(slots, axis=1)), np.ascontiguousarray(np.repeat(hn[:, None], NBEST, axis=1))


def timed_together(forms, steps, warmup, windows=3):
    """forms: {name: fn} -> {name: dict(ms, ms_min, ms_max)}; the forms alternate window by window"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    w = {k: [] for k in forms}
    for _ in range(windows):
        for k, fn in forms.items():
            w[k].append(_window(fn, steps))
    out = {}
    for k, v in w.items():
        v = sorted(v)
        out[k] = dict(ms=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4))
    return out


def normalisers():
    """What this box sustains, now: bench.py's own two figures (its f16x2 MFMA stream, a streaming pass over 2 x 1 GiB)."""
    import bench
    box = bench.box_normalisers(torch.device("cuda:0"))
    return {k: box.get(k) for k in ("measured_mfma_tflops", "measured_copy_gbs")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py measures on a HIP device; none found")
    labels = configs.builtin("quartznet15x5")["labels"]
    sp = space_ids(labels)
    out = dict(device=torch.cuda.get_device_name(0), nbest=NBEST, script_width=SCRIPT_WIDTH, runs=[])
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for batch, seconds in SHAPES:
        width = encoded_frames(seconds)
        (hyp_h, hn_h, ref_h, rn_h), _ = synthetic_pairs(labels, batch, seconds, width, seed=batch)
        assert int(hn_h.max()) <= SCRIPT_WIDTH
        ids_h, idn_h = nbest_batch(hyp_h, hn_h, len(labels), batch)
        hyp, hn, ref, rn = cuda(hyp_h), cuda(hn_h), cuda(ref_h), cuda(rn_h)
        cut = cuda(hyp_h[:, :SCRIPT_WIDTH])
        ids, idn = cuda(ids_h), cuda(idn_h)
        count = torch.full((batch,), NBEST, dtype=torch.int32, device="cuda")
        # the forms agree with the yardstick before anything is timed
        want = stages.error_counts(hyp, hn, ref, rn, sp)
        ops = stages.error_ops(hyp, hn, ref, rn, sp)
        ops_s, script, script_len = stages.error_ops(cut, hn, ref, rn, sp, script=True)
        nb = stages.nbest_error_counts(ids, idn, count, ref, rn, sp)
        assert bool((ops == ops_s).all())
        assert bool((ops[:, 0:3].sum(1) == want[:, 0]).all()) and bool((ops[:, 4:7].sum(1) == want[:, 2]).all())
        assert bool((ops[:, 3] + ops[:, 0] + ops[:, 1] == want[:, 1]).all()) and bool((ops[:, 7] + ops[:, 4] + ops[:, 5] == want[:, 3]).all())
        assert bool((nb["slot_counts"][:, 0] == want).all()) and bool((nb["counts"][:, 0] <= want[:, 0]).all())
        steps_ok = torch.arange(script.shape[1], device="cuda")[None, :] < script_len[:, None]
        for code in range(4):
            assert bool((((script == code) & steps_ok).sum(1) == ops[:, (3, 0, 1, 2)[code]]).all()), code
        tot = ops.sum(0, dtype=torch.int64).cpu().tolist()
        run = dict(batch=batch, seconds=seconds, hyp_width=width, ref_width=int(ref.shape[1]),
                   cells_char=int((hn_h.astype(np.int64) * rn_h).sum()),
                   totals=dict(zip(("word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del", "char_ins", "char_hits"), tot)))
        forms = {
            "error_counts": lambda: stages.error_counts(hyp, hn, ref, rn, sp),
            "error_ops": lambda: stages.error_ops(hyp, hn, ref, rn, sp),
            "error_counts_cut": lambda: stages.error_counts(cut, hn, ref, rn, sp),
            "error_ops_script": lambda: stages.error_ops(cut, hn, ref, rn, sp, script=True),
            "nbest_error_counts": lambda: stages.nbest_error_counts(ids, idn, count, ref, rn, sp),
        }
        run.update(timed_together(forms, args.steps, args.warmup))
        run["ops_over_counts"] = round(run["error_ops"]["ms"] / run["error_counts"]["ms"], 3)
        run["script_over_counts_cut"] = round(run["error_ops_script"]["ms"] / run["error_counts_cut"]["ms"], 3)
        run["nbest_over_counts"] = round(run["nbest_error_counts"]["ms"] / run["error_counts"]["ms"], 3)
        out["runs"].append(run)
    out["box"] = normalisers()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
