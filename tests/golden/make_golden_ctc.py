#!/usr/bin/env python3
"""Generate tests/golden/ctc_cases.npz by running the REAL reference code on the CPU -- dev container only: ``CTCLossNM._loss``
and its ``_criterion`` (nemo/collections/asr/losses.py: nn.CTCLoss(blank=num_classes, reduction='none')) for the per-row losses
and the batch mean, and ``process_evaluation_batch`` / ``process_evaluation_epoch`` (helpers.py:146-204) for an epoch of
three batches.  Shims from make_golden.py.

    python tests/golden/make_golden_ctc.py     # needs the reference checkout

Stored, per case ``c<i>`` (C in {2, 5, 29, 96} x ragged batches of 1, 3 and 5 rows): seeded float32 log-probs [B][T][C] (a
log_softmax of normal logits at scale 0.1 -- flat posteriors -- or 8 -- peaked ones --, valid behind every row's length too),
int64 targets [B][W] and both lengths, the reference's per-row float32 losses and its batch mean.  The rows walk through L in
{0, 1, 2, 31, 32, 33}, targets with runs of equal labels and without (C = 2 has one label: every pair is equal), and T one
frame too few (+inf), exactly feasible (a single path), in between, and about 3 L.  One row has -inf among its log-probs.
And an epoch of 5, 3 and 1 rows at C = 29 -- unequal sizes, so the mean of the batch means is not the sample mean -- with
greedy predictions, through the reference's own bookkeeping: its dict, its strings, its batch losses.

Asserted here: the reference is defined (not NaN) on EVERY stored row, +inf exactly where a row has fewer frames than its
target needs, the float64 restatement (tests/ctc_reference.py) agrees on every +inf, and the reference's float32 losses lie
inside the restatement's bound.  No row is excused."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import ctc_reference as CR  # noqa: E402

CLASSES = (2, 5, 29, 96)
BATCHES = (1, 3, 5)
LENGTHS = (0, 1, 2, 31, 32, 33)
KINDS = ("too_few", "exact", "between", "long")
SCALES = (0.1, 8.0)
EPOCH = (5, 3, 1)
EPOCH_LABELS = list(" abcdefghijklmnopqrstuvwxyz'")


def draw_target(rng, L, labels, repeats):
    """L ids below ``labels``; with repeats about a third of the neighbours are equal, without none are (given two labels)"""
    y = rng.integers(0, labels, L)
    for i in range(1, L):
        if repeats and rng.random() < 0.35:
            y[i] = y[i - 1]
        elif not repeats and labels > 1:
            while y[i] == y[i - 1]:
                y[i] = rng.integers(0, labels)
    return y.astype(np.int64)


def frames_for(kind, y):
    need, L = CR.min_frames(y, len(y)), len(y)
    return {"too_few": max(need - 1, 0), "exact": need, "between": need + L // 2 + 1, "long": 3 * L + 2}[kind]


def log_softmax(rng, shape, scale):
    return torch.log_softmax(torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)), dim=-1).numpy()


def make_batch(rng, rows, C, scale):
    """rows: [(L, kind, repeats)] -> logp [B][T][C] f32, frames [B] i64, tgt [B][W] i64, tgt_len [B] i64"""
    ys = [draw_target(rng, L, C - 1, rep) for L, _, rep in rows]
    frames = np.array([frames_for(kind, y) for (_, kind, _), y in zip(rows, ys)], dtype=np.int64)
    T, W = max(int(frames.max()) + 2, 1), max(max(len(y) for y in ys), 1) + 1      # something real behind every length
    tgt = rng.integers(0, C - 1, (len(rows), W)).astype(np.int64)
    for b, y in enumerate(ys):
        tgt[b, : len(y)] = y
    return log_softmax(rng, (len(rows), T, C), scale), frames, tgt, np.array([len(y) for y in ys], dtype=np.int64)


def main():
    assert os.path.isdir(MG.REF), "reference checkout required (dev container only)"
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    import nemo
    import nemo.collections.asr.helpers as H
    from nemo.collections.asr.losses import CTCLossNM
    nemo.core.NeuralModuleFactory(placement=nemo.core.DeviceType.CPU)

    rng = np.random.default_rng(20261019)
    fx, n, walk, seen_inf_row = {}, 0, 0, False

    def reference(nm, logp, frames, tgt, tgt_len):
        lt, ft, tt, nt = (torch.from_numpy(a) for a in (logp, frames, tgt, tgt_len))
        rows = nm._criterion(lt.transpose(1, 0), tt, ft, nt).numpy()
        mean = nm._loss(lt, tt, ft, nt)
        assert rows.dtype == np.float32 and mean.dtype == torch.float32
        return rows, mean

    def check(logp, frames, tgt, tgt_len, blank, rows):
        l64, bound = CR.batch(logp, frames, tgt, tgt_len, blank)
        for b in range(len(frames)):
            assert not np.isnan(rows[b]), "the reference has to be defined on every stored row"
            infeasible = frames[b] < CR.min_frames(tgt[b], tgt_len[b])
            assert np.isinf(l64[b]) == infeasible or np.isneginf(logp[b, : frames[b]]).any()
            assert CR.close(rows[b], l64[b], bound[b]), (b, float(rows[b]), l64[b], bound[b])
            assert CR.close(CR.loss32(logp[b], frames[b], tgt[b], tgt_len[b], blank), l64[b], bound[b])

    for C in CLASSES:
        nm = CTCLossNM(num_classes=C - 1)
        for B in BATCHES:
            rows = []
            for _ in range(B):
                rows.append((LENGTHS[walk % 6], KINDS[(walk // 6 + walk) % 4], (walk // 2) % 2 == 0))
                walk += 1
            scale = SCALES[n % 2]
            logp, frames, tgt, tgt_len = make_batch(rng, rows, C, scale)
            if C == 5 and B == 3:            # one row with -inf among its log-probs: a class that never occurs in two frames,
                b = int(np.argmax(frames))   # and one entry of a label the row does use
                logp[b, 1:3, 3] = -np.inf
                logp[b, 0, int(tgt[b, 1])] = -np.inf
                seen_inf_row = True
            ref_rows, ref_mean = reference(nm, logp, frames, tgt, tgt_len)
            check(logp, frames, tgt, tgt_len, C - 1, ref_rows)
            fx.update({f"c{n}_logp": logp, f"c{n}_frames": frames, f"c{n}_tgt": tgt, f"c{n}_tgt_len": tgt_len,
                       f"c{n}_loss": ref_rows, f"c{n}_mean": np.float32(ref_mean.item()), f"c{n}_scale": np.float64(scale),
                       f"c{n}_kinds": np.array([KINDS.index(k) for _, k, _ in rows], dtype=np.int64)})
            n += 1
    assert seen_inf_row
    fx["cases"] = np.int64(n)

    # one epoch of three unequal batches through the reference's own bookkeeping
    C = len(EPOCH_LABELS) + 1
    nm, gv = CTCLossNM(num_classes=C - 1), {}
    for j, B in enumerate(EPOCH):
        rows = [(int(rng.integers(4, 13)), "between" if b % 2 else "long", b % 2 == 0) for b in range(B)]
        logp, frames, tgt, tgt_len = make_batch(rng, rows, C, 2.0)
        ref_rows, ref_mean = reference(nm, logp, frames, tgt, tgt_len)
        check(logp, frames, tgt, tgt_len, C - 1, ref_rows)
        pred = torch.from_numpy(logp).argmax(dim=-1)
        H.process_evaluation_batch({"loss": [ref_mean], "predictions": [pred], "transcript": [torch.from_numpy(tgt)],
                                    "transcript_length": [torch.from_numpy(tgt_len)], "output": [torch.from_numpy(logp)]},
                                   gv, labels=EPOCH_LABELS)
        fx.update({f"epoch{j}_logp": logp, f"epoch{j}_frames": frames, f"epoch{j}_tgt": tgt, f"epoch{j}_tgt_len": tgt_len,
                   f"epoch{j}_pred": pred.numpy().astype(np.int64), f"epoch{j}_loss": ref_rows})
    logs = H.process_evaluation_epoch(gv, eval_metric="WER", tag=None)
    tagged = H.process_evaluation_epoch(gv, eval_metric="cer", tag="dev")
    assert sorted(logs) == ["Evaluation_Loss", "Evaluation_Valid_CER", "Evaluation_Valid_WER"]
    assert sorted(tagged) == ["Evaluation_Loss_dev", "Evaluation_Valid_CER", "Evaluation_Valid_WER"]
    assert tagged["Evaluation_Loss_dev"] == logs["Evaluation_Loss"]
    fx["epoch_labels"] = np.array(EPOCH_LABELS)
    fx["epoch_loss"] = np.float64(logs["Evaluation_Loss"])
    fx["epoch_wer"], fx["epoch_cer"] = np.float64(logs["Evaluation_Valid_WER"]), np.float64(logs["Evaluation_Valid_CER"])
    fx["epoch_batch_losses"] = np.array([float(v) for v in gv["EvalLoss"]], dtype=np.float64)
    fx["epoch_predictions"], fx["epoch_transcripts"] = np.array(gv["predictions"]), np.array(gv["transcripts"])
    assert len(gv["predictions"]) == len(gv["transcripts"]) == sum(EPOCH) and len(gv["logits"]) == 3
    every = np.concatenate([fx[f"epoch{j}_loss"] for j in range(3)]).astype(np.float64)
    assert abs(every.mean() - float(fx["epoch_loss"])) > 1e-2, "the mean of batch means has to differ from the sample mean"

    path = os.path.join(HERE, "ctc_cases.npz")
    np.savez_compressed(path, **fx)
    print(f"ctc_cases: {n} cases + an epoch of {EPOCH}, eval loss {float(fx['epoch_loss']):.6f}, wer {float(fx['epoch_wer']):.4f} "
          f"cer {float(fx['epoch_cer']):.4f}, bytes={os.path.getsize(path)}")
    assert os.path.getsize(path) < 600 * 1000


if __name__ == "__main__":
    main()
