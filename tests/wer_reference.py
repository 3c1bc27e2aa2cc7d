"""NumPy restatement of word_error_rate (nemo/collections/asr/metrics.py:30-63) on label-id rows: what
vasr_error_counts_i32 has to return, integer for integer.

``counts(hyp, ref, space_ids)`` -> [word_edits, ref_words, char_edits, ref_chars] of one pair; ``batch_counts`` does a padded
batch over its lengths.  The distance is the unit-cost Levenshtein distance of metrics.py:7-27, computed row by row: the
candidates that come from the previous row are one vector expression, and the dependency on the left neighbour,
cur[j] = min(c[j], cur[j - 1] + 1), resolves to min over k <= j of (c[k] - k) + j = np.minimum.accumulate(c - arange) + arange
-- so a 4096 x 4096 pair costs 4096 vector steps, not 16.8 million interpreted cells.  Words are ``str.split()`` written on
ids: maximal runs of ids outside ``space_ids``; equal words are equal tuples of ids.
"""
import numpy as np


def levenshtein(a, b):
    """Unit-cost edit distance between two 1-D integer arrays."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return int(n + m)
    ar = np.arange(m + 1, dtype=np.int64)
    prev = ar.copy()
    c = np.empty(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        c[0] = i
        np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1, out=c[1:])
        prev = np.minimum.accumulate(c - ar) + ar
    return int(prev[m])


def split_ids(row, space_ids):
    """``str.split()`` on ids: the maximal runs of ids that are not in ``space_ids``, as tuples."""
    row = np.asarray(row, dtype=np.int64)
    if len(row) == 0:
        return []
    sp = np.isin(row, np.asarray(list(space_ids), dtype=np.int64))
    prev_sp = np.concatenate([[True], sp[:-1]])
    next_sp = np.concatenate([sp[1:], [True]])
    starts = np.flatnonzero(~sp & prev_sp)
    ends = np.flatnonzero(~sp & next_sp) + 1
    return [tuple(row[s:e].tolist()) for s, e in zip(starts, ends)]


def counts(hyp, ref, space_ids):
    """-> [word_edits, ref_words, char_edits, ref_chars] of one (hypothesis, reference) pair of id rows."""
    hw, rw = split_ids(hyp, space_ids), split_ids(ref, space_ids)
    number = {}
    hn = [number.setdefault(w, len(number)) for w in hw]
    rn = [number.setdefault(w, len(number)) for w in rw]
    return [levenshtein(hn, rn), len(rw), levenshtein(hyp, ref), len(ref)]


def batch_counts(hyp, hyp_len, ref, ref_len, space_ids):
    """Padded batches [B, Th] / [B, Tr] with lengths [B] -> int32 [B, 4]; a negative length gives four -1 (vasr.h)."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    out = np.empty((len(hyp_len), 4), dtype=np.int32)
    for b, (n, m) in enumerate(zip(np.asarray(hyp_len).tolist(), np.asarray(ref_len).tolist())):
        if n < 0 or m < 0:
            out[b] = -1
            continue
        n, m = min(n, hyp.shape[1]), min(m, ref.shape[1])
        out[b] = counts(hyp[b, :n], ref[b, :m], space_ids)
    return out


def rates(total):
    """[word_edits, ref_words, char_edits, ref_chars] sums -> (wer, cer) as metrics.py:59-62 divides them."""
    we, rw, ce, rc = (int(v) for v in total)
    return (1.0 * we / rw if rw else float("inf")), (1.0 * ce / rc if rc else float("inf"))
