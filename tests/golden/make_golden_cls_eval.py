#!/usr/bin/env python3
"""Generate tests/golden/cls_eval_cases.npz by running the REAL reference functions on the CPU -- dev container only:
``classification_accuracy`` (nemo/collections/asr/metrics.py:66-99), ``process_classification_evaluation_batch`` / ``_epoch``
(helpers.py:215-288) and ``nn.CrossEntropyLoss`` as CrossEntropyLossNM builds it (backends/pytorch/common/losses.py:136-141;
reduction 'none' for the per-row values, its default 'mean' for the epoch's batch losses).  Shims from make_golden.py.

    python tests/golden/make_golden_cls_eval.py     # needs the reference checkout

Stored, per case ``c<i>`` (C in {1, 2, 35, 64, 65, 257, 1000} x batches of 1, 3, 4 and 5 rows, and 67 rows at C in {2, 35, 65,
257}; logit scales 0.01, 1 and 100 in turn): seeded float32 logits, int64 targets (half of them drawn among the row's six
best classes, so that the accuracies are not all zero at large C), the reference's ``logits.topk(min(5, C))`` indices, its
per-row float32 losses, and ``classification_accuracy`` for top_k [1], [1, 5] and [5, 1, 3] (each k capped at C; the last is
the unsorted list).  And the logs of a three-batch epoch of 67, 5 and 1 rows at C = 35 -- unequal sizes, so the mean of the
batch means is not the sample mean -- with top_k [5, 1], next to its inputs.

One shim beyond make_golden.py's: ``classification_accuracy`` calls ``correct[:k].view(-1)`` on the transposed comparison
matrix, which the torch of its day allowed (``eq`` returned a contiguous tensor) and today's refuses for k > 1; ``view`` falls
back to ``reshape`` here while the reference runs -- the same elements in the same order.

The condition the tests rest on is asserted here: NO row holds a tie among its six largest values or at its target's value, so
the reference's answer is unambiguous on every row and no row is ever excused.  The restatement (tests/cls_eval_reference.py)
has to reproduce every stored integer, and the reference's float32 losses have to lie inside its bound."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import cls_eval_reference as ER  # noqa: E402

CLASSES = (1, 2, 35, 64, 65, 257, 1000)
BATCHES = (1, 3, 4, 5)
WIDE = (2, 35, 65, 257)              # these also get a 67-row batch
SCALES = (0.01, 1.0, 100.0)
TOP_K = ([1], [1, 5], [5, 1, 3])
EPOCH = (67, 5, 1)


def draw(rng, rows, C, scale):
    logits = (rng.standard_normal((rows, C)) * scale).astype(np.float32)
    targets = rng.integers(0, C, rows)
    for b in range(rows):
        if rng.random() < 0.5:
            targets[b] = ER.order(logits[b])[int(rng.integers(0, min(6, C)))]
    return logits, targets.astype(np.int64)


def assert_no_ties(logits, targets):
    for x, t in zip(logits, targets):
        top = np.sort(x)[::-1][: min(6, x.size)]
        assert len(set(top.tolist())) == top.size, "tie among the six largest values"
        assert int((x == x[t]).sum()) == 1, "tie at the target's value"
        assert np.isfinite(x).all()


def main():
    assert os.path.isdir(MG.REF), "reference checkout required (dev container only)"
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    import nemo.collections.asr.helpers as H
    from nemo.collections.asr.metrics import classification_accuracy

    view = torch.Tensor.view

    def view_or_reshape(self, *a, **k):
        try:
            return view(self, *a, **k)
        except RuntimeError:
            return self.reshape(*a, **k)
    torch.Tensor.view = view_or_reshape

    rng = np.random.default_rng(20261019)
    ce_rows = torch.nn.CrossEntropyLoss(weight=None, reduction="none")
    ce_mean = torch.nn.CrossEntropyLoss(weight=None, reduction="mean")
    fx, n = {}, 0
    shapes = [(C, B) for C in CLASSES for B in BATCHES] + [(C, 67) for C in WIDE]
    for i, (C, B) in enumerate(shapes):
        scale = SCALES[(CLASSES.index(C) + i) % 3]
        logits, targets = draw(rng, B, C, scale)
        assert_no_ties(logits, targets)
        lt, tt = torch.from_numpy(logits), torch.from_numpy(targets)
        top5 = lt.topk(min(5, C), dim=1, largest=True, sorted=True)[1].numpy()
        loss = ce_rows(lt, tt).numpy()
        r, tk, l64 = ER.batch(logits, targets, min(5, C))
        assert (tk == top5).all() and loss.dtype == np.float32
        for b in range(B):
            assert abs(float(loss[b]) - l64[b]) <= ER.loss_bound(logits[b], targets[b])
        fx.update({f"c{i}_logits": logits, f"c{i}_targets": targets, f"c{i}_top5": top5.astype(np.int64), f"c{i}_loss": loss,
                   f"c{i}_scale": np.float64(scale)})
        for j, ks in enumerate(TOP_K):
            ks = [min(k, C) for k in ks]
            acc = np.array([float(a) for a in classification_accuracy(lt, tt, top_k=ks)], dtype=np.float64)
            assert acc.tolist() == [float(a) for a in ER.reference_accuracy(r, ks)]
            fx[f"c{i}_acc{j}"], fx[f"c{i}_acc{j}_k"] = acc, np.array(ks, dtype=np.int64)
        n += 1
    fx["cases"] = np.int64(n)

    # one epoch of three unequal batches through the reference's own bookkeeping
    gv, top_k = {}, [5, 1]
    for j, B in enumerate(EPOCH):
        logits, targets = draw(rng, B, 35, 1.0)
        assert_no_ties(logits, targets)
        lt, tt = torch.from_numpy(logits), torch.from_numpy(targets)
        H.process_classification_evaluation_batch({"loss": [ce_mean(lt, tt)], "logits": [lt], "labels": [tt]}, gv, top_k=top_k)
        fx[f"epoch{j}_logits"], fx[f"epoch{j}_targets"] = logits, targets
    logs = H.process_classification_evaluation_epoch(gv, eval_metric=top_k, tag="t")
    fx["epoch_top_k"] = np.array(top_k, dtype=np.int64)
    fx["epoch_loss"] = np.float64(logs["Evaluation_Loss t"])
    for k in top_k:
        fx[f"epoch_acc{k}"] = np.float64(float(logs[f"Evaluation_Accuracy_Top@{k} t"]))
        fx[f"epoch_counts{k}"] = np.array([float(v) for v in gv[f"CorrectCount@{k}"]], dtype=np.float64)
    fx["epoch_batch_losses"] = np.array([float(v) for v in gv["EvalLoss"]], dtype=np.float64)
    assert gv["batchsize"] == list(EPOCH) and sorted(logs) == sorted(
        ["Evaluation_Loss t", "Evaluation_Accuracy_Top@1 t", "Evaluation_Accuracy_Top@5 t"])
    rows = np.concatenate([ER.batch(fx[f"epoch{j}_logits"], fx[f"epoch{j}_targets"], 0)[2] for j in range(3)])
    assert abs(float(rows.mean()) - float(fx["epoch_loss"])) > 1e-3, "the mean of batch means has to differ from the sample mean"
    torch.Tensor.view = view

    path = os.path.join(HERE, "cls_eval_cases.npz")
    np.savez_compressed(path, **fx)
    print(f"cls_eval_cases: {n} cases + an epoch of {EPOCH}, eval loss {float(fx['epoch_loss']):.6f}, "
          f"top@1 {float(fx['epoch_acc1']):.4f} top@5 {float(fx['epoch_acc5']):.4f}, bytes={os.path.getsize(path)}")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
