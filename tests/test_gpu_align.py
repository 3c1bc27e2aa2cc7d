"""GPU checks of the S/D/I breakdown, the word edit script and the n-best oracle scoring (vasr_error_ops_i32,
vasr_nbest_error_counts_i32, stages.error_ops / nbest_error_counts, metrics.ErrorBreakdown / OracleErrorRate / word_alignment,
VietASR.evaluate_manifest(breakdown=, nbest=)): every integer, scripts included, equals tests/align_reference.py.

Ids are drawn from THREE symbols plus two separator ids: almost every cell of either table then has tied predecessors, and a
tie-break slip changes the split or the script.  As in test_gpu_wer.py every batch is wider than its rows and the ids behind
a length are poison.  The shapes are the smallest at which the kernel's paths change: 64 lanes (word compaction), 256 lanes
(cells of a diagonal per pass) at both levels, lopsided tables, the 1024-id script limit, the 4096-id counts limit."""
import json

import numpy as np
import pytest
import torch

import align_reference as AR
import wer_reference as WR

pytestmark = pytest.mark.gpu

POISON = (2 ** 31 - 1, -1, -(2 ** 31), -7)
SP = [3, 4]                      # ids 0..2 are symbols


def pack(rows, width=None, poison=POISON):
    longest = max([len(r) for r in rows] + [0])
    width = longest + 3 if width is None else width
    out = np.empty((len(rows), width), dtype=np.int64)
    out[:] = np.resize(np.asarray(poison, dtype=np.int64), width)[None, :]
    for k, r in enumerate(rows):
        out[k, : len(r)] = r
    return out.astype(np.int32), np.array([len(r) for r in rows], dtype=np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_ops(hyp, hn, ref, rn, sp, script=True):
    """-> (ops [B, 8], scripts: per row a list of op codes, or None for a -1 row)"""
    from viet_asr_amd import stages
    if not script:
        return stages.error_ops(dev(hyp), dev(hn), dev(ref), dev(rn), sp).cpu().numpy(), None
    ops, steps, steps_len = stages.error_ops(dev(hyp), dev(hn), dev(ref), dev(rn), sp, script=True)
    ops, steps, steps_len = ops.cpu().numpy(), steps.cpu().numpy(), steps_len.cpu().numpy()
    assert steps.shape[1] == max(1, (hyp.shape[1] + 1) // 2 + (ref.shape[1] + 1) // 2)
    return ops, [None if n < 0 else steps[b, :n].tolist() for b, n in enumerate(steps_len.tolist())]


def check_rows(hyps, refs, sp=SP, hyp_width=None, ref_width=None):
    """Both forms of the kernel against the restatement, and sub + del + ins against vasr_error_counts_i32."""
    from viet_asr_amd import stages
    hyp, hn = pack(hyps, hyp_width)
    ref, rn = pack(refs, ref_width)
    want, want_scripts = AR.batch_ops(hyp, hn, ref, rn, sp)
    got, scripts = device_ops(hyp, hn, ref, rn, sp)
    plain, _ = device_ops(hyp, hn, ref, rn, sp, script=False)
    assert got.dtype == np.int32 and got.shape == (len(hyps), 8)
    bad = np.flatnonzero((got != want).any(axis=1) | (plain != want).any(axis=1))
    assert bad.size == 0, [(int(b), len(hyps[b]), len(refs[b]), got[b].tolist(), plain[b].tolist(), want[b].tolist()) for b in bad[:6]]
    for b, (s, w) in enumerate(zip(scripts, want_scripts)):
        assert s == w, (b, len(hyps[b]), len(refs[b]), s[:40], w[:40])
        assert AR.op_counts(s) == got[b, :4].tolist()                    # the script's op counts are the row's word counts
    edits = stages.error_counts(dev(hyp), dev(hn), dev(ref), dev(rn), sp).cpu().numpy()
    assert (got[:, 0:3].sum(axis=1) == edits[:, 0]).all() and (got[:, 4:7].sum(axis=1) == edits[:, 2]).all()
    assert (got[:, 3] + got[:, 0] + got[:, 1] == edits[:, 1]).all() and (got[:, 7] + got[:, 4] + got[:, 5] == edits[:, 3]).all()
    return got, scripts


def seq(rng, n, symbols=5):
    return rng.integers(0, symbols, n).tolist()


def words(rng, k):
    """k one-id words: 2k - 1 ids (0 for k = 0)"""
    out = []
    for w in rng.integers(0, 3, k).tolist():
        out += [w, 3]
    return out[:-1]


def noisy(rng, row, p=0.1):
    return [c if rng.random() > p else int(rng.integers(5)) for c in row]


def test_smallest_tables(gpu):
    rng = np.random.default_rng(1)
    hyps, refs = [], []
    for n in (0, 1, 2):
        for m in (0, 1, 2):
            for _ in range(4):
                hyps.append(seq(rng, n, 3)); refs.append(seq(rng, m, 3))          # symbols only
                hyps.append(seq(rng, n)); refs.append(seq(rng, m))
    got, scripts = check_rows(hyps, refs)
    check_rows(hyps, refs, hyp_width=2, ref_width=2)                              # rows as wide as the buffer
    # the hand-written pairs of test_align_host.py, on the device: words 0 1 2 = a b c
    a, b, c, s = 0, 1, 2, 3
    H, S, D, I = AR.HIT, AR.SUB, AR.DEL, AR.INS
    cases = [([a, s, b], [b, s, a], [S, S]), ([a, s, a, s, b], [a, s, b, s, b], [H, S, H]), ([a], [b, s, c], [D, S]),
             ([b, s, c], [a], [I, S]), ([a, s, b, s, a], [b, s, a, s, b], [I, H, H, D]), ([a], [a, s, a], [D, H]),
             ([a, s, a], [a], [I, H]), ([], [a, s, b], [D, D]), ([a, s, b], [], [I, I]), ([], [], [])]
    _, scripts = check_rows([h for h, _, _ in cases], [r for _, r, _ in cases])
    assert scripts == [w for _, _, w in cases]
    # width 0 on either side and on both
    z, zl = np.zeros((2, 0), dtype=np.int32), np.zeros(2, dtype=np.int32)
    ref, rn = pack([[a, s, b], [c]])
    ops, sc = device_ops(z, zl, ref, rn, SP)
    assert ops.tolist() == [[0, 2, 0, 0, 0, 3, 0, 0], [0, 1, 0, 0, 0, 1, 0, 0]] and sc == [[D, D], [D]]
    ops, sc = device_ops(ref, rn, z, zl, SP)
    assert ops.tolist() == [[0, 0, 2, 0, 0, 0, 3, 0], [0, 0, 1, 0, 0, 0, 1, 0]] and sc == [[I, I], [I]]
    ops, sc = device_ops(z, zl, z, zl, SP)
    assert ops.tolist() == [[0] * 8] * 2 and sc == [[], []]


def test_lengths_around_the_lane_and_workgroup_boundaries(gpu):
    """63 / 64 / 65 and 255 / 256 / 257 ids (the character table's diagonals against 64 and 256 lanes) and as many WORDS
    (the ballot of the word compaction, the word table's diagonals), 300 x 7 and 7 x 300."""
    rng = np.random.default_rng(2)
    hyps, refs = [], []
    for n, m in ((63, 64), (64, 65), (65, 63), (64, 64), (255, 256), (256, 257), (257, 255), (300, 7), (7, 300)):
        hyps.append(seq(rng, n)); refs.append(seq(rng, m))
    base = seq(rng, 257)
    hyps += [base, noisy(rng, base)[:-1]]; refs += [noisy(rng, base), base]
    for k, j in ((63, 64), (64, 65), (65, 63), (255, 256), (256, 257), (257, 255), (150, 4), (4, 150)):
        hyps.append(words(rng, k)); refs.append(words(rng, j))
    wbase = words(rng, 257)
    hyps += [wbase]; refs += [noisy(rng, wbase)]
    check_rows(hyps, refs)
    check_rows(refs[:9], hyps[:9], hyp_width=310, ref_width=304)                  # the other order, other strides


def test_the_script_limit_1024(gpu):
    """One 1024 x 1024 pair with a script: 512 words per side, the largest LDS carve-up of the script form."""
    from viet_asr_amd import stages
    rng = np.random.default_rng(3)
    h = words(rng, 512) + [4]                                                     # 1024 ids, 512 words
    r = words(rng, 512) + [3]
    r[200:700] = h[200:700]
    assert len(h) == len(r) == 1024
    got, scripts = check_rows([h], [r], hyp_width=1024, ref_width=1024)
    assert len(scripts[0]) >= 512 and got[0, 3] > 0 and got[0, 0] + got[0, 1] + got[0, 2] > 0
    # one id wider on either side: the script is refused, the counts are not
    wide = torch.zeros((1, 1025), dtype=torch.int32, device="cuda")
    ok = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    n = torch.ones(1, dtype=torch.int32, device="cuda")
    for a, b in ((wide, ok), (ok, wide)):
        with pytest.raises(NotImplementedError, match="1024"):
            stages.error_ops(a, n, b, n, SP, script=True)
        assert stages.error_ops(a, n, b, n, SP).shape == (1, 8)


def test_word_boundaries(gpu):
    labels = " abcdefg\t"
    sp = [0, 8]
    ids = lambda t: [labels.index(c) for c in t]  # noqa: E731
    long_a, long_b = "abcdefg" * 43, "abcdefg" * 42 + "abcdefa"                   # one word of 301 characters
    pairs = [("", "ab cd"), ("ab cd", ""), ("", ""), ("ab cd", "ab cd"), (" \t  ", "\t"), (" \t ", "ab"), ("ab", "\t \t"),
             ("  ab cd", "ab cd"), ("ab cd  ", "ab cd"), ("ab  cd", "ab cd"), ("ab \t cd", "abcd"), (long_a, long_b),
             (long_a, long_a), (long_a, "ab"), ("a b c d e f g", "a b d d e g"), ("abcd abce abc", "abce abcd abcd"),
             ("ab ab ab ab", "ab ab ab"), ("ab ab", "ab ab ab ab"), ("a b a b a", "b a b a b")]
    hyps, refs = [ids(h) for h, _ in pairs], [ids(r) for _, r in pairs]
    got, scripts = check_rows(hyps, refs, sp)
    H, S, D, I = AR.HIT, AR.SUB, AR.DEL, AR.INS
    assert scripts[0] == [D, D] and scripts[1] == [I, I] and scripts[2] == [] and scripts[3] == [H, H] and scripts[4] == []
    assert scripts[7] == scripts[8] == scripts[9] == [H, H] and scripts[11] == [S] and scripts[12] == [H]
    assert got[11].tolist() == [1, 0, 0, 0, 1, 0, 0, 300]
    check_rows(hyps, refs, [0])                       # the tab is part of a word
    check_rows(hyps, refs, [])                        # a non-empty row is one word


def test_lengths_padding_and_batching(gpu):
    rng = np.random.default_rng(5)
    hyps, refs = [seq(rng, int(rng.integers(20, 60))) for _ in range(5)], [seq(rng, int(rng.integers(20, 60))) for _ in range(5)]
    got, scripts = check_rows(hyps, refs)
    # each row alone gives what it gives inside the batch of 5
    for b in range(5):
        one, one_script = check_rows([hyps[b]], [refs[b]])
        assert one[0].tolist() == got[b].tolist() and one_script[0] == scripts[b]
    # other strides and other garbage behind the lengths
    hyp, hn = pack(hyps, width=97, poison=(-5, 0, 1, 2 ** 31 - 1, 3))
    ref, rn = pack(refs, width=64, poison=(4,))
    again, again_scripts = device_ops(hyp, hn, ref, rn, SP)
    assert (again == got).all() and again_scripts == scripts
    # a negative length on either side: eight -1 and a script length of -1, the other rows untouched
    hn2 = hn.copy(); hn2[1] = -1; hn2[4] = -3
    rn2 = rn.copy(); rn2[3] = -1
    ops, sc = device_ops(hyp, hn2, ref, rn2, SP)
    ops0, sc0 = ops, sc
    assert ops[[1, 3, 4]].tolist() == [[-1] * 8] * 3 and [sc[b] for b in (1, 3, 4)] == [None] * 3
    assert (ops[[0, 2]] == got[[0, 2]]).all() and [sc[0], sc[2]] == [scripts[0], scripts[2]]
    assert (device_ops(hyp, hn2, ref, rn2, SP, script=False)[0] == ops).all()
    # lengths above the width are clamped to it
    full_h, _ = pack([h[:20] for h in hyps[:2]], width=20)
    full_r, _ = pack([r[:20] for r in refs[:2]], width=20)
    big = np.array([21, 1 << 30], dtype=np.int32)
    ops, sc = device_ops(full_h, big, full_r, big, SP)
    want, want_sc = AR.batch_ops(full_h, [20, 20], full_r, [20, 20], SP)
    assert (ops == want).all() and sc == want_sc
    # entries of the script at or beyond a row's length are not written, and nothing is written outside the buffers
    from viet_asr_amd import _lib
    L = (hyp.shape[1] + 1) // 2 + (ref.shape[1] + 1) // 2
    script = torch.full((5, L + 1), -77, dtype=torch.int32, device="cuda")
    slen = torch.full((6,), -77, dtype=torch.int32, device="cuda")
    out = torch.full((6, 8), -77, dtype=torch.int32, device="cuda")
    arr = (_lib.C.c_int32 * 2)(*SP)
    t = [dev(x) for x in (hyp, hn2, ref, rn2)]
    _lib.check(_lib.lib().vasr_error_ops_i32(t[0].data_ptr(), hyp.shape[1], t[1].data_ptr(), t[2].data_ptr(), ref.shape[1],
                                             t[3].data_ptr(), 5, arr, 2, out.data_ptr(), script.data_ptr(), slen.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    flat, slen, out = script.cpu().numpy().reshape(-1), slen.cpu().numpy(), out.cpu().numpy()
    assert slen[5] == -77 and (out[5] == -77).all() and (flat[5 * L:] == -77).all() and (out[:5] == ops0).all()
    for b in range(5):
        row = flat[b * L: (b + 1) * L]
        n = max(0, slen[b])
        assert (row[n:] == -77).all() and (sc0[b] is None and slen[b] == -1 or row[:n].tolist() == sc0[b])


def test_the_widest_rows_counts_only(gpu):
    """4096 x 4096, counts only (the script form stops at 1024).  The cell-by-cell restatement is too slow here: the distances
    come from wer_reference.levenshtein, the split is held to its identities."""
    rng = np.random.default_rng(4096)
    base = seq(rng, 4096)
    other = noisy(rng, base, 0.15)[5:] + seq(rng, 5)
    hyp, hn = pack([base, base[:4000], [2]], width=4096)
    ref, rn = pack([other, base, base], width=4096)
    got, _ = device_ops(hyp, hn, ref, rn, SP, script=False)
    for b in range(3):
        h, r = hyp[b, : hn[b]], ref[b, : rn[b]]
        we, rw, ce, rc = WR.counts(h, r, SP)
        nw = len(WR.split_ids(h, SP))
        ws, wd, wi, wh, cs, cd, ci, ch = got[b].tolist()
        assert min(got[b].tolist()) >= 0
        assert ws + wd + wi == we and wd - wi == rw - nw and wh + ws + wd == rw
        assert cs + cd + ci == ce and cd - ci == rc - len(h) and ch + cs + cd == rc
    assert got[0, 4] > 0 and got[0, 7] > 2048 and got[1].tolist()[4:] == [0, 96, 0, 4000]


# --------------------------------------------------------------------------------------------------------------- n-best
def device_nbest(ids, id_len, count, ref, ref_len, sp):
    from viet_asr_amd import stages
    out = stages.nbest_error_counts(dev(ids), dev(id_len), dev(count), dev(ref), dev(ref_len), sp)
    return tuple(out[k].cpu().numpy() for k in ("slot_counts", "counts", "slot"))


def check_nbest(ids, id_len, count, ref, ref_len, sp=SP):
    got = device_nbest(ids, id_len, count, ref, ref_len, sp)
    want = AR.nbest_counts(ids, id_len, count, ref, ref_len, sp)
    for g, w, name in zip(got, want, ("slot_counts", "counts", "slot")):
        assert g.dtype == np.int32 and g.shape == w.shape and (g == w).all(), (name, g.tolist(), w.tolist())
    return got


def pack_nbest(lists, width=None):
    """lists[b][s]: id rows -> (ids [B, N, width] with poison behind every length, id_len [B, N])"""
    N = max(len(l) for l in lists)
    flat = [r for l in lists for r in (l + [[]] * (N - len(l)))]
    ids, n = pack(flat, width)
    return ids.reshape(len(lists), N, -1), n.reshape(len(lists), N)


def test_nbest_1_is_error_counts(gpu):
    from viet_asr_amd import stages
    rng = np.random.default_rng(6)
    hyps, refs = [seq(rng, int(rng.integers(0, 90))) for _ in range(7)], [seq(rng, int(rng.integers(0, 90))) for _ in range(7)]
    hyp, hn = pack(hyps)
    ref, rn = pack(refs)
    sc, c, s = check_nbest(hyp[:, None, :], hn[:, None], np.ones(7, np.int32), ref, rn)
    plain = stages.error_counts(dev(hyp), dev(hn), dev(ref), dev(rn), SP).cpu().numpy()
    assert (sc[:, 0] == plain).all() and (c == plain).all() and (s == 0).all()


def test_nbest_minima_ties_and_unfilled_slots(gpu):
    a, b, c, s = 0, 1, 2, 3
    ref_row = [a, a, s, b, b, s, c, c]                                            # "aa bb cc"
    lists = [
        # a tie takes the lower slot: every slot has one word edit, slots 1, 2 and 3 one character edit (slot 0 three)
        [[a, a, s, b, b], [a, a, s, b, b, s, c, a], [a, b, s, b, b, s, c, c], [a, a, s, b, b, s, c, a]],
        # the word minimum and the character minimum on different slots: slot 0 = one wrong word (4 characters off),
        # slot 1 = two wrong words (2 characters off)
        [[a, a, s, b, b, s, a, a, a, a], [a, b, s, b, b, s, c, b], [c]],
        # count < nbest: slots 2 and 3 hold the reference itself and are NOT filled
        [[a, a], [b, b], ref_row, ref_row],
        # empty reference, every filled hypothesis non-empty: the unfilled length-0 slots would win
        [[a, s, b], [a], [], []],
    ]
    ids, n = pack_nbest(lists)
    count = np.array([4, 3, 2, 2], dtype=np.int32)
    n[2, 2:] = 8
    refs = [ref_row, ref_row, ref_row, []]
    ref, rn = pack(refs)
    sc, cnt, slot = check_nbest(ids, n, count, ref, rn)
    assert cnt[0].tolist() == [1, 3, 1, 8] and slot[0].tolist() == [0, 1]
    assert cnt[1].tolist() == [1, 3, 2, 8] and slot[1].tolist() == [0, 1]
    assert sc[2, 2:].tolist() == [[-1] * 4] * 2 and cnt[2].tolist() == [2, 3, 6, 8] and slot[2].tolist() == [0, 0]
    assert cnt[3].tolist() == [1, 0, 1, 0] and slot[3].tolist() == [1, 1] and sc[3, 2:].tolist() == [[-1] * 4] * 2
    # a count above nbest is clamped to it; garbage lengths behind the count are never used
    n2 = n.copy(); n2[3, 2:] = -1; n2[2, 3] = 1 << 30
    check_nbest(ids, n2, np.array([9, 3, 2, 2], np.int32), ref, rn)
    # rows that cannot be scored: -1 everywhere, the other rows as before
    bad_n = n.copy(); bad_n[1, 2] = -1                                            # a filled slot with a negative length
    got = check_nbest(ids, bad_n, np.array([4, 3, 0, 2], np.int32), ref, np.array([8, 8, 8, -1], np.int32))
    assert (got[0][1:] == -1).all() and (got[1][1:] == -1).all() and (got[2][1:] == -1).all()
    assert (got[0][0] == sc[0]).all() and got[1][0].tolist() == cnt[0].tolist()
    # more slots than a wavefront has lanes, the minimum late in the list and repeated
    many = [[[c] * (9 + k % 5) for k in range(70)]]
    many[0][66] = ref_row[:-1]; many[0][68] = ref_row[:-1]; many[0][69] = ref_row
    ids, n = pack_nbest(many)
    _, cnt, slot = check_nbest(ids, n, np.array([69], np.int32), *pack([ref_row]))
    assert cnt[0].tolist() == [1, 3, 1, 8] and slot[0].tolist() == [66, 66]


def test_nbest_of_a_real_beam_search(gpu):
    """decode_beams_ids' outputs go in as they are; per row the oracle counts are the minimum of host-computed distances over
    the returned slots and no larger than slot 0's."""
    from viet_asr_amd.beam import BeamSearchDecoder
    from viet_asr_amd.metrics import ErrorRate, OracleErrorRate
    from test_beam import LABELS, random_posteriors
    B, T, nbest = 4, 40, 8
    lp = np.stack([random_posteriors(T + 7 * b, len(LABELS) + 1, 60 + b)[:T] for b in range(B)])
    dec = BeamSearchDecoder(LABELS)
    ids, n, count, _, _ = dec.decode_beams_ids(torch.from_numpy(lp).to(gpu), 16, nbest)
    sp = [0]
    # references: slot min(2, count - 1) of each row with an edit, so that slot 0 is rarely the best
    ids_h, n_h, count_h = ids.cpu().numpy(), n.cpu().numpy(), count.cpu().numpy()
    assert (count_h >= 1).all() and (count_h > 1).any()
    refs = []
    for b in range(B):
        k = min(2, count_h[b] - 1)
        refs.append(ids_h[b, k, : n_h[b, k]].tolist() + [0, 5])
    ref, rn = pack(refs)
    sc, cnt, slot = check_nbest(ids_h, n_h, count_h, ref, rn, sp)
    for b in range(B):
        host = [WR.counts(ids_h[b, s, : n_h[b, s]], refs[b], sp) for s in range(count_h[b])]
        assert cnt[b, 0] == min(h[0] for h in host) and cnt[b, 2] == min(h[2] for h in host)
        assert cnt[b, 0] <= sc[b, 0, 0] and cnt[b, 2] <= sc[b, 0, 2]
    # the running metric, without a synchronisation in update
    m, one = OracleErrorRate(LABELS), ErrorRate(LABELS)
    ref_d, rn_d = dev(ref.astype(np.int64)), dev(rn.astype(np.int64))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(ids, n, count, ref_d, rn_d)
        one.update(ids[:, 0], n[:, 0], ref_d, rn_d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    r, r1 = m.compute(), one.compute()
    tot = cnt.astype(np.int64).sum(axis=0)
    assert [r[k] for k in ("word_edits", "ref_words", "char_edits", "ref_chars")] == tot.tolist()
    assert (r["oracle_wer"], r["oracle_cer"]) == WR.rates(tot) and r["oracle_wer"] <= r1["wer"] and r["oracle_cer"] <= r1["cer"]


# ------------------------------------------------------------------------------------------------------ Python surface
def test_breakdown_and_word_alignment(gpu):
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import ErrorBreakdown, ErrorRate, confusion_pairs, word_alignment
    labels = list(" abcd\te")
    rng = np.random.default_rng(12)
    m, e = ErrorBreakdown(labels), ErrorRate(labels)
    assert m.space_ids == [0, 5]
    total = np.zeros(8, dtype=np.int64)
    batches = []
    for B, wh, wr in ((3, 50, 40), (9, 130, 300), (1, 7, 9)):
        hyp, hn = pack([seq(rng, int(rng.integers(0, wh)), 7) for _ in range(B)], width=wh)
        ref, rn = pack([seq(rng, int(rng.integers(0, wr)), 7) for _ in range(B)], width=wr)
        total += AR.batch_ops(hyp, hn, ref, rn, m.space_ids)[0].astype(np.int64).sum(axis=0)
        batches.append((dev(hyp), dev(hn), dev(ref.astype(np.int64)), dev(rn.astype(np.int64))))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            m.update(*b)
            e.update(*b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    r, r0 = m.compute(), e.compute()
    keys = ("word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del", "char_ins", "char_hits")
    assert [r[k] for k in keys] == total.tolist()
    assert {k: r[k] for k in r0} == r0 and m.compute(reduce=True) == r
    hyp, hn, ref, rn = batches[0]
    bad = hn.clone(); bad[2] = -1
    m.update(hyp, bad, ref, rn)
    with pytest.raises(VasrError):
        m.compute()
    with pytest.raises(VasrError):
        word_alignment(hyp, bad, ref, rn, labels)
    # word_alignment: strings, first word to last
    ids = lambda t: [labels.index(c) for c in t]  # noqa: E731
    pairs = [("ab cd e", "ab ce e"), ("a b", "b a"), ("\tab  ba", "ab"), ("", "dd"), ("cab", ""), ("a b a", "b a b")]
    hyp, hn = pack([ids(h) for h, _ in pairs])
    ref, rn = pack([ids(t) for _, t in pairs])
    rows = word_alignment(dev(hyp), dev(hn), dev(ref.astype(np.int64)), dev(rn.astype(np.int64)), labels)
    assert rows[0] == [("hit", "ab", "ab"), ("sub", "cd", "ce"), ("hit", "e", "e")]
    assert rows[1] == [("sub", "a", "b"), ("sub", "b", "a")]
    assert rows[2] == [("hit", "ab", "ab"), ("ins", "ba", None)]
    assert rows[3] == [("del", None, "dd")] and rows[4] == [("ins", "cab", None)]
    assert rows[5] == [("ins", "a", None), ("hit", "b", "b"), ("hit", "a", "a"), ("del", None, "b")]
    assert confusion_pairs(rows) == {("ce", "cd"): 1, ("b", "a"): 1, ("a", "b"): 1}


def test_evaluate_manifest_breakdown_and_nbest(gpu, tmp_path):
    """The default call returns what it returned before (the six keys, the restatement's values on the returned transcripts);
    breakdown=True agrees on those six and adds the split; nbest=N scores the beam search's slot 0 and adds the oracle."""
    from viet_asr_amd import audio, configs, synth
    from viet_asr_amd.infer import VietASR
    cfg = configs.builtin("quartznet12x1_vi")
    labels = cfg["labels"]
    jas = cfg["JasperEncoder"]["jasper"]
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in synth.encoder_state_dict(jas, 64, 3).items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in synth.decoder_state_dict(1024, len(labels) + 1, 3).items()}, dec_p)
    asr = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy")
    rng = np.random.default_rng(8)
    lens = [9000, 16000, 4000, 12000, 20000]
    paths = []
    for i, n in enumerate(lens):
        paths.append(str(tmp_path / f"u{i}.wav"))
        audio.write_wav(paths[-1], (0.1 * rng.standard_normal(n)).astype(np.float32), 16000)

    def manifest(name, texts):
        p = str(tmp_path / name)
        with open(p, "w", encoding="utf-8") as f:
            for w, n, t in zip(paths, lens, texts):
                e = {"audio_filepath": w, "duration": n / 16000}
                if t is not None:
                    e["text"] = t
                f.write(json.dumps(e, ensure_ascii=False) + "\n")
        return p

    own, none = asr.transcribe_manifest(manifest("plain.json", [None] * 5), batch_size=3)
    assert none is None and any(own)
    refs = list(own)
    refs[0] = own[0][2:] + " " + labels[5] + labels[7]
    refs[1] = " ".join(own[1].split()[1:])
    refs[3] = None                                            # no text: transcribed, not scored
    refs[4] = own[4][: len(own[4]) // 2] + labels[3]
    man = manifest("refs.json", refs)
    sp = [i for i, c in enumerate(labels) if c.isspace()]
    ids = lambda t: [labels.index(c) for c in t if c in labels]  # noqa: E731
    scored = [i for i, t in enumerate(refs) if t]
    six = ("wer", "cer", "word_edits", "ref_words", "char_edits", "ref_chars")

    hyps, res = asr.evaluate_manifest(man, batch_size=3)
    assert hyps == own and tuple(res) == six
    total = np.sum([WR.counts(ids(hyps[i]), ids(refs[i]), sp) for i in scored], axis=0)
    assert [res[k] for k in six[2:]] == total.tolist() and (res["wer"], res["cer"]) == WR.rates(total) and res["char_edits"] > 0

    hyps_b, res_b = asr.evaluate_manifest(man, batch_size=3, breakdown=True)
    assert hyps_b == own and {k: res_b[k] for k in six} == res and len(res_b) == 14
    split = np.sum([AR.ops(ids(hyps[i]), ids(refs[i]), sp)[0] for i in scored], axis=0)
    names = ("word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del", "char_ins", "char_hits")
    assert [res_b[k] for k in names] == split.tolist()
    with pytest.raises(ValueError, match="beam"):
        asr.evaluate_manifest(man, batch_size=3, nbest=4)

    beam = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="beam", beam_width=8)
    hyps_n, res_n = beam.evaluate_manifest(man, batch_size=3, nbest=4, breakdown=True)
    assert set(res_n) == set(six) | set(names) | {"oracle_wer", "oracle_cer"}
    order = sorted(range(5), key=lambda i: lens[i])            # the batches evaluate_manifest cuts: by duration, three at a time
    for lo in (0, 3):
        idx = order[lo: lo + 3]
        texts = beam.transcribe_batch([audio.read_wav(paths[i])[0] for i in idx], row_independent=True, decoder="beam")
        assert [hyps_n[i] for i in idx] == texts
    total_n = np.sum([WR.counts(ids(hyps_n[i]), ids(refs[i]), sp) for i in scored], axis=0)
    assert [res_n[k] for k in six[2:]] == total_n.tolist()
    assert res_n["oracle_wer"] <= res_n["wer"] and res_n["oracle_cer"] <= res_n["cer"]
