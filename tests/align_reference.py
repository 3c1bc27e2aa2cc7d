"""Plain restatement of the alignment rule of include/vasr.h: what vasr_error_ops_i32 and vasr_nbest_error_counts_i32 have to
return, integer for integer, scripts included.

The full (n + 1) x (m + 1) table with one predecessor per cell, row by row -- the rule only looks at a cell's three neighbours, so
the order of the walk does not matter:
    borders   D[i][0] = i (insertions), D[0][j] = j (deletions)
    interior  diag = D[i-1][j-1] + (h[i-1] != r[j-1]);  dele = D[i][j-1] + 1;  ins = D[i-1][j] + 1
    tie-break diag if diag <= min(dele, ins), else dele if dele <= ins, else ins
``align(h, r)`` -> the ops from the first element to the last (0 hit, 1 substitution, 2 deletion, 3 insertion);
``ops(hyp, ref, space_ids)`` -> (eight counts, word script) of one pair of id rows; ``batch_ops`` / ``nbest_counts`` do padded
batches.  Words are ``wer_reference.split_ids``.
"""
import numpy as np

from wer_reference import counts as wer_counts
from wer_reference import split_ids

HIT, SUB, DEL, INS = 0, 1, 2, 3
NAMES = ("hit", "sub", "del", "ins")


def align(h, r):
    """The edit script of sequences h (hypothesis) against r (reference), first step first."""
    n, m = len(h), len(r)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    P = [[DEL] * (m + 1) for _ in range(n + 1)]
    for i in range(1, n + 1):
        D[i][0], P[i][0] = i, INS
    for j in range(1, m + 1):
        D[0][j] = j
    for i in range(1, n + 1):
        hi, Di, Dp, Pi = h[i - 1], D[i], D[i - 1], P[i]
        for j in range(1, m + 1):
            ne = 1 if hi != r[j - 1] else 0
            diag, dele, ins = Dp[j - 1] + ne, Di[j - 1] + 1, Dp[j] + 1
            if diag <= dele and diag <= ins:
                Di[j], Pi[j] = diag, ne          # HIT or SUB
            elif dele <= ins:
                Di[j], Pi[j] = dele, DEL
            else:
                Di[j], Pi[j] = ins, INS
    i, j, rev = n, m, []
    while i > 0 or j > 0:
        op = P[i][j]
        rev.append(op)
        if op != DEL:
            i -= 1
        if op != INS:
            j -= 1
    assert len([o for o in rev if o != HIT]) == D[n][m]
    return rev[::-1]


def op_counts(script):
    """-> [sub, del, ins, hits]"""
    return [script.count(SUB), script.count(DEL), script.count(INS), script.count(HIT)]


def ops(hyp, ref, space_ids):
    """One pair of id rows -> ([word_sub, word_del, word_ins, word_hits, char_sub, char_del, char_ins, char_hits], word script)."""
    hw, rw = split_ids(hyp, space_ids), split_ids(ref, space_ids)
    words = align(hw, rw)
    chars = align(list(np.asarray(hyp).tolist()), list(np.asarray(ref).tolist()))
    return op_counts(words) + op_counts(chars), words


def batch_ops(hyp, hyp_len, ref, ref_len, space_ids):
    """Padded batches -> (int32 [B, 8], list of word scripts; None for a row with a negative length, whose counts are -1)."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    out = np.empty((len(hyp_len), 8), dtype=np.int32)
    scripts = []
    for b, (n, m) in enumerate(zip(np.asarray(hyp_len).tolist(), np.asarray(ref_len).tolist())):
        if n < 0 or m < 0:
            out[b] = -1
            scripts.append(None)
            continue
        n, m = min(n, hyp.shape[1]), min(m, ref.shape[1])
        out[b], s = ops(hyp[b, :n], ref[b, :m], space_ids)
        scripts.append(s)
    return out, scripts


def replay(script, hyp_words, ref_words):
    """Walk a script over the two word lists -> [(op name, hyp word | None, ref word | None)]; raises when the script does not
    consume both lists exactly or calls unequal words a hit (or equal words a substitution)."""
    i = j = 0
    out = []
    for op in script:
        hw = rw = None
        if op != DEL:
            hw, i = hyp_words[i], i + 1
        if op != INS:
            rw, j = ref_words[j], j + 1
        if op in (HIT, SUB):
            assert (hw == rw) == (op == HIT), (op, hw, rw)
        out.append((NAMES[op], hw, rw))
    assert i == len(hyp_words) and j == len(ref_words), (i, len(hyp_words), j, len(ref_words))
    return out


def nbest_counts(ids, id_len, count, ref, ref_len, space_ids):
    """ids [B, N, T], id_len [B, N], count [B], ref [B, Tr], ref_len [B] -> (slot_counts int32 [B, N, 4], counts int32 [B, 4],
    slot int32 [B, 2]) as include/vasr.h states them for vasr_nbest_error_counts_i32."""
    ids, id_len, ref = np.asarray(ids), np.asarray(id_len), np.asarray(ref)
    B, N = id_len.shape
    slot_counts = np.full((B, N, 4), -1, dtype=np.int32)
    counts = np.full((B, 4), -1, dtype=np.int32)
    slot = np.full((B, 2), -1, dtype=np.int32)
    for b in range(B):
        filled, m = min(int(count[b]), N), int(ref_len[b])
        if filled < 1 or m < 0 or (id_len[b, :filled] < 0).any():
            continue
        m = min(m, ref.shape[1])
        for s in range(filled):
            n = min(int(id_len[b, s]), ids.shape[2])
            slot_counts[b, s] = wer_counts(ids[b, s, :n], ref[b, :m], space_ids)
        w, c = slot_counts[b, :filled, 0], slot_counts[b, :filled, 2]
        slot[b] = [int(np.argmin(w)), int(np.argmin(c))]          # argmin: the first (lowest) among equals
        counts[b] = [w.min(), slot_counts[b, 0, 1], c.min(), slot_counts[b, 0, 3]]
    return slot_counts, counts, slot
