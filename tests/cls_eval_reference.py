"""What the classification-scoring tests and tests/golden/make_golden_cls_eval.py share: a float64 / integer restatement of
vasr_class_scores_f32 (include/vasr.h) -- the order on a row's classes, the target's rank, the top-k and the cross-entropy
loss -- and the bound on the float32 loss.

The order: larger value first; a NaN above every number; -0 equal to +0; among equal values, and among NaNs, the lower class
index first.  rank = the number of classes that come before the target; a target outside [0, C) gives rank -1 and loss 0.

The bound, per row, on |loss32 - loss64|:

    eps * [(R(C) + 8) + 2 * (|max| + |x_target| + |loss64|)],   eps = 2^-24,   R(C) = ceil(log2 max(C, 2))

R(C): the roundings on the longest path of a tree sum of C positive terms, each a relative error of the sum and so an
absolute error of its logarithm; 8: a few ulps for expf / logf and the subtraction in front of expf; the last term: the
roundings of max + log(sum), of that minus x_target, and of the result, at their magnitudes.

The kernel's summation order (csrc/cls_eval.hip): class c goes to accumulator (c / 64) % 8 of lane c % 64; an accumulator
takes its ceil(C / 512) terms one after the other (ceil(C / 512) - 1 roundings; none while it holds one term, adding to the
initial zero is exact), the eight are merged pairwise (3) and the 64 lanes by a butterfly (6); a merge with an empty
accumulator or lane adds zero and rounds nothing.  The longest path therefore has

    K(C) = (ceil(C / 512) - 1) + min(3, ceil(log2 max(1, min(8, ceil(C / 64))))) + min(6, ceil(log2 min(C, 64)))

roundings, which is <= R(C) for every C <= 1536 (checked exhaustively in tests/test_cls_eval_host.py) and exceeds it above
(C = 2048: 12 against 11; C = 65536: 136 against 16).  ``sum_roundings`` is max(R(C), K(C)): the issue's constant at every
size the tests use, the kernel's own depth where that is larger.  Derived from the code's order, not from its output."""
import math

import numpy as np

EPS = 2.0 ** -24


def _ceil_log2(n):
    return int(math.ceil(math.log2(n))) if n > 1 else 0


def tree_roundings(C):
    """R(C) = ceil(log2 max(C, 2))."""
    return _ceil_log2(max(int(C), 2))


def kernel_roundings(C):
    """K(C): the longest path of the kernel's sum (module docstring)."""
    C = int(C)
    per_acc = -(-C // 512)
    accs = min(8, -(-C // 64))
    return (per_acc - 1) + min(3, _ceil_log2(accs)) + min(6, _ceil_log2(min(C, 64)))


def sum_roundings(C):
    return max(tree_roundings(C), kernel_roundings(C))


def order(row):
    """Class indices of one row in the documented order (all C of them)."""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    val = np.where(nan, np.inf, row) + 0.0                      # -0 + 0 = +0; NaN handled by the first key
    # lexsort: last key first -- NaN first, then value descending, then index ascending
    return np.lexsort((np.arange(row.size), -val, ~nan)).astype(np.int64)


def rank(row, target):
    """0-based position of ``target`` in the order, -1 for a target outside [0, C)."""
    C = len(row)
    if not 0 <= int(target) < C:
        return -1
    return int(np.nonzero(order(row) == int(target))[0][0])


def topk(row, k):
    return order(row)[: int(k)]


def logsumexp64(row):
    x = np.asarray(row, dtype=np.float64)
    m = x.max()
    return m + math.log(np.exp(x - m).sum())


def loss64(row, target):
    """logsumexp(row) - row[target] in float64; 0 for a target outside [0, C)."""
    if not 0 <= int(target) < len(row):
        return 0.0
    return logsumexp64(row) - float(row[int(target)])


def loss_bound(row, target):
    """The bound on |loss32 - loss64| of one row with finite values (module docstring)."""
    x = np.asarray(row, dtype=np.float64)
    return EPS * ((sum_roundings(x.size) + 8) + 2.0 * (abs(x.max()) + abs(x[int(target)]) + abs(loss64(x, target))))


def prob64(row, classes):
    x = np.asarray(row, dtype=np.float64)
    return np.exp(x[np.asarray(classes, dtype=np.int64)] - logsumexp64(x))


def prob_bound(row, classes):
    """Bound on |p32 - p64| of expf(x - logsumexp32): the loss bound taken at each class as the absolute error of the
    exponent -- a relative error of the probability -- plus one expf (2 ulps) and the rounding of the result."""
    x = np.asarray(row, dtype=np.float64)
    p = prob64(x, classes)
    rel = np.array([loss_bound(x, c) for c in classes]) + 3 * EPS
    return p * rel + 2.0 ** -126                # (below the smallest normal number a result may be denormal or flushed)


def batch(logits, targets, k):
    """Rows of logits [B][C] -> (rank [B] i64, topk [B][k] i64, loss64 [B])."""
    logits = np.asarray(logits)
    r = np.array([rank(x, t) for x, t in zip(logits, targets)], dtype=np.int64)
    tk = np.stack([topk(x, k) for x in logits]) if k else np.zeros((len(logits), 0), dtype=np.int64)
    ls = np.array([loss64(x, t) for x, t in zip(logits, targets)], dtype=np.float64)
    return r, tk, ls


def hits(ranks, k):
    ranks = np.asarray(ranks)
    return int(((ranks >= 0) & (ranks < k)).sum())


def reference_accuracy(ranks, top_k):
    """classification_accuracy (metrics.py:66-99) from ranks, as the reference computes it: correct[:k].float().mean() runs
    over the k x B comparison matrix, so the value is hits / (k * B) in float32 -- the top-k accuracy divided by k."""
    n = len(ranks)
    return [np.float32(hits(ranks, k)) / np.float32(k * n) for k in top_k]


def mean_of_means_bound(rows_per_batch, bounds_per_batch, means64):
    """Bound on |eval_loss32 - mean of the float64 batch means| where every batch mean is a float32 mean of float32 losses
    within ``bounds`` of their float64 values and the batch means are summed in float32: the mean of the per-batch mean
    bounds, plus the roundings of each batch's sum and division (B at most, whatever the order of the sum) and of the sum
    over the batches and its division (one per batch, and one) at the magnitude of the means."""
    nb = len(rows_per_batch)
    out = 0.0
    for n, b, m in zip(rows_per_batch, bounds_per_batch, means64):
        out += float(np.mean(b)) + EPS * (n + 1) * abs(m)
    return out / nb + EPS * (nb + 1) * float(np.mean(np.abs(means64)))
