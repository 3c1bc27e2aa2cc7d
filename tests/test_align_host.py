"""CPU checks of the S/D/I breakdown, the word alignment and the n-best oracle scoring: the restatement of the alignment rule
(tests/align_reference.py) on the fixture the reference's own metric wrote (tests/golden/wer_cases.npz, read only) and on
hand-written pairs whose optimal alignments are not unique; the two exported symbols, their signatures and header
declarations with the ABI still 8; every refusal of vasr_error_ops_i32 and vasr_nbest_error_counts_i32 before a device is
touched; the host arithmetic of ErrorBreakdown / OracleErrorRate fed CPU counts; confusion_pairs."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest
import torch

import align_reference as AR
import wer_reference as WR
from conftest import GOLDEN_DIR, ROOT

INVALID, UNSUPPORTED = -1, -5
HIT, SUB, DEL, INS = AR.HIT, AR.SUB, AR.DEL, AR.INS


def test_breakdown_identities_on_the_reference_metrics_fixture():
    g = np.load(os.path.join(GOLDEN_DIR, "wer_cases.npz"), allow_pickle=False)
    sp = g["space_ids"].tolist()
    got, scripts = AR.batch_ops(g["hyp"], g["hyp_len"], g["ref"], g["ref_len"], sp)
    ws, wd, wi, wh, cs, cd, ci, ch = (got[:, k].astype(np.int64) for k in range(8))
    assert (ws + wd + wi).tolist() == g["word_edits"].tolist() and (cs + cd + ci).tolist() == g["char_edits"].tolist()
    assert (wh + ws + wd).tolist() == g["ref_words"].tolist() and (ch + cs + cd).tolist() == g["ref_len"].tolist()
    assert (ch + cs + ci).tolist() == g["hyp_len"].tolist()
    for b, script in enumerate(scripts):
        hw = WR.split_ids(g["hyp"][b, : g["hyp_len"][b]], sp)
        rw = WR.split_ids(g["ref"][b, : g["ref_len"][b]], sp)
        assert wh[b] + ws[b] + wi[b] == len(hw)
        steps = AR.replay(script, hw, rw)                   # consumes both lists exactly; hits are equal words, subs are not
        assert [w for _, w, _ in steps if w is not None] == hw and [w for _, _, w in steps if w is not None] == rw
        names = [op for op, _, _ in steps]
        assert [names.count(k) for k in ("sub", "del", "ins", "hit")] == got[b, :4].tolist()


def test_tie_break_on_pairs_with_more_than_one_optimal_alignment():
    """Worked by hand from the rule in include/vasr.h: diagonal first, then deletion, then insertion."""
    cases = [
        ("a b", "b a", [SUB, SUB]),                          # not del-hit-ins, not ins-hit-del
        ("a a b", "a b b", [HIT, SUB, HIT]),
        ("a", "b c", [DEL, SUB]),                            # (1,2): diag = dele = 2 -> diag, which leaves the deletion in front
        ("b c", "a", [INS, SUB]),
        ("a b a", "b a b", [INS, HIT, HIT, DEL]),            # (3,3): dele = ins = 2 < diag = 3 -> dele; del-hit-hit-ins loses
        ("a", "a a", [DEL, HIT]),                            # (1,2): diag = dele = 1 -> the hit goes to the LAST reference word
        ("a a", "a", [INS, HIT]),
        ("a b", "c a b c", [DEL, HIT, HIT, DEL]),
        ("", "a b", [DEL, DEL]),
        ("a b", "", [INS, INS]),
        ("", "", []),
    ]
    for h, r, want in cases:
        assert AR.align(h.split(), r.split()) == want, (h, r)
    # on ids, through ops(): words "1 2" against "2 1" with 0 as the separator
    counts, script = AR.ops([1, 0, 2], [2, 0, 1], [0])
    assert script == [SUB, SUB] and counts == [2, 0, 0, 0, 2, 0, 0, 1]
    # any script of the rule has the distance of the plain recurrence, on three symbols where almost every cell ties
    rng = np.random.default_rng(0)
    for _ in range(40):
        a, b = rng.integers(0, 3, int(rng.integers(0, 30))).tolist(), rng.integers(0, 3, int(rng.integers(0, 30))).tolist()
        s = AR.align(a, b)
        sub, dele, ins, hits = AR.op_counts(s)
        assert sub + dele + ins == WR.levenshtein(a, b) and dele - ins == len(b) - len(a) and hits + sub + dele == len(b)
        AR.replay(s, a, b)


def test_nbest_restatement():
    ids = np.array([[[1, 0, 2, 9], [1, 0, 3, 9], [7, 7, 7, 7]], [[1, 9, 9, 9], [2, 9, 9, 9], [9, 9, 9, 9]]])
    id_len = np.array([[3, 3, 0], [1, 1, 0]])
    ref = np.array([[1, 0, 3], [5, 5, 5]])
    sc, c, s = AR.nbest_counts(ids, id_len, [2, 3], ref, [3, 0], [0])
    assert sc[0].tolist() == [[1, 2, 1, 3], [0, 2, 0, 3], [-1] * 4] and c[0].tolist() == [0, 2, 0, 3] and s[0].tolist() == [1, 1]
    # an empty reference: the filled empty slot 2 wins here because count says it IS filled
    assert c[1].tolist() == [0, 0, 0, 0] and s[1].tolist() == [2, 2]
    sc, c, s = AR.nbest_counts(ids, id_len, [2, 2], ref, [3, 0], [0])
    assert c[1].tolist() == [1, 0, 1, 0] and s[1].tolist() == [0, 0] and sc[1, 2].tolist() == [-1] * 4
    for count, rl, il in (([0, 2], [3, 0], id_len), ([2, 2], [-1, 0], id_len), ([2, 2], [3, 0], np.array([[3, -1, 0], [1, 1, 0]]))):
        sc, c, s = AR.nbest_counts(ids, il, count, ref, rl, [0])
        assert (sc[0] == -1).all() and (c[0] == -1).all() and (s[0] == -1).all() and (c[1] >= 0).all()


def test_new_symbols_are_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    for n in ("vasr_error_ops_i32", "vasr_nbest_error_counts_i32"):
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    assert "diag <= min(dele, ins)" in header                # the rule is written into the header


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_error_ops_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f = L.vasr_error_ops_i32
    p = 4096                                   # a non-NULL, 16-byte aligned "device pointer"
    sp = (C.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    ok = dict(hyp=p, hw=16, hl=p, ref=p, rw=16, rl=p, batch=2, sp=sp, ns=1, out=p, script=None, slen=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["hyp"], a["hw"], a["hl"], a["ref"], a["rw"], a["rl"], a["batch"], a["sp"], a["ns"], a["out"], a["script"],
                 a["slen"], None)

    for name in ("hyp", "hl", "ref", "rl", "out"):
        assert call(**{name: None}) == INVALID, name
        assert call(**{name: None}, script=p, slen=p) == INVALID, name
    assert call(batch=0) == INVALID and call(batch=-3) == INVALID
    assert call(hw=-1) == INVALID and call(rw=-1) == INVALID
    assert call(ns=-1) == INVALID and call(ns=9) == INVALID and call(sp=None, ns=1) == INVALID
    assert call(out=p + 4) == INVALID and call(out=p + 8) == INVALID       # two 16-byte vector stores per row
    assert call(hw=4097) == UNSUPPORTED and call(rw=4097) == UNSUPPORTED and call(hw=1 << 40) == UNSUPPORTED
    assert b"4096" in L.vasr_last_error()
    # one script pointer without the other
    assert call(script=p) == INVALID and call(slen=p) == INVALID
    # a script: both widths at most 1024; the counts alone keep 4096 (checked on the GPU, where it can run)
    assert call(script=p, slen=p, hw=1025) == UNSUPPORTED and call(script=p, slen=p, rw=1025) == UNSUPPORTED
    assert b"1024" in L.vasr_last_error()
    assert call(script=p, slen=p, hw=4097) == UNSUPPORTED and call(script=p, slen=p, batch=0, hw=1025) == INVALID
    with pytest.raises(NotImplementedError):
        _lib.check(call(script=p, slen=p, rw=4096), L)
    with pytest.raises(ValueError):
        _lib.check(call(script=p), L)


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_nbest_refusals_come_before_a_device_is_touched(which):
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f = L.vasr_nbest_error_counts_i32
    p = 4096
    sp = (C.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    ok = dict(ids=p, w=16, il=p, count=p, nbest=4, ref=p, rw=16, rl=p, batch=2, sp=sp, ns=1, sc=p, counts=p, slot=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["ids"], a["w"], a["il"], a["count"], a["nbest"], a["ref"], a["rw"], a["rl"], a["batch"], a["sp"], a["ns"],
                 a["sc"], a["counts"], a["slot"], None)

    for name in ("ids", "il", "count", "ref", "rl", "sc"):
        assert call(**{name: None}) == INVALID, name
    assert call(batch=0) == INVALID and call(batch=-3) == INVALID
    assert call(nbest=0) == INVALID and call(nbest=-1) == INVALID
    assert call(nbest=65536) == UNSUPPORTED and b"65535" in L.vasr_last_error()   # the launch grid is batch x nbest
    assert call(w=-1) == INVALID and call(rw=-1) == INVALID
    assert call(ns=-1) == INVALID and call(ns=9) == INVALID and call(sp=None, ns=1) == INVALID
    assert call(sc=p + 4) == INVALID and call(counts=p + 8) == INVALID
    assert call(w=4097) == UNSUPPORTED and call(rw=4097) == UNSUPPORTED and call(w=1 << 40) == UNSUPPORTED
    assert b"4096" in L.vasr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(rw=5000), L)
    with pytest.raises(ValueError):
        _lib.check(call(nbest=0), L)


def test_error_breakdown_host_arithmetic():
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import ErrorBreakdown, ErrorRate
    keys = ("word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del", "char_ins", "char_hits")
    m = ErrorBreakdown(list(" ab\tc"))
    assert m.space_ids == [0, 3]
    empty = m.compute()
    assert empty["wer"] == float("inf") and empty["cer"] == float("inf") and all(empty[k] == 0 for k in keys)
    assert set(empty) == set(ErrorRate(list(" ab")).compute()) | set(keys)
    m._add(torch.tensor([[1, 0, 2, 3, 4, 1, 0, 9], [0, 2, 0, 1, 2, 2, 2, 5]], dtype=torch.int32))
    m._add(torch.tensor([[0, 0, 1, 0, 0, 0, 3, 0]], dtype=torch.int32))       # a hypothesis against an empty reference
    r = m.compute()
    assert [r[k] for k in keys] == [1, 2, 3, 4, 6, 3, 5, 14]
    # edits = sub + del + ins, reference count = hits + sub + del: ErrorRate's six keys with ErrorRate's values
    assert (r["word_edits"], r["ref_words"], r["char_edits"], r["ref_chars"]) == (6, 7, 14, 23)
    assert r["wer"] == 6 / 7 and r["cer"] == 14 / 23
    e = ErrorRate(list(" ab"))
    e._add(torch.tensor([[6, 7, 14, 23]], dtype=torch.int32))
    assert {k: r[k] for k in e.compute()} == e.compute()
    assert m.compute(reduce=True) == r                                          # no process group: the identity
    m._add(torch.tensor([[5] * 8, [-1] * 8], dtype=torch.int32))
    with pytest.raises(VasrError):
        m.compute()
    m.reset()
    m._add(torch.full((3, 8), 2 ** 30, dtype=torch.int32))                      # the sums are 64-bit
    assert m.compute()["char_hits"] == 3 * 2 ** 30 and m.compute()["ref_chars"] == 9 * 2 ** 30
    with pytest.raises(NotImplementedError):
        ErrorBreakdown([" ", "a", "ch"])


def test_oracle_error_rate_host_arithmetic():
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import OracleErrorRate
    m = OracleErrorRate(list(" abc"))
    assert m.compute() == dict(oracle_wer=float("inf"), oracle_cer=float("inf"), word_edits=0, ref_words=0, char_edits=0,
                               ref_chars=0)
    m._add(torch.tensor([[1, 3, 2, 7], [0, 4, 1, 9]], dtype=torch.int32))
    m._add(torch.tensor([[2, 0, 5, 5]], dtype=torch.int32))
    assert m.compute() == dict(oracle_wer=3 / 7, oracle_cer=8 / 21, word_edits=3, ref_words=7, char_edits=8, ref_chars=21)
    assert m.compute(reduce=True) == m.compute()
    m._add(torch.tensor([[-1, -1, -1, -1]], dtype=torch.int32))
    with pytest.raises(VasrError):
        m.compute()
    m.reset()
    m._add(torch.tensor([[0, 2, 0, 5]], dtype=torch.int32))
    assert m.compute()["oracle_wer"] == 0.0 and m.compute()["ref_chars"] == 5


def test_confusion_pairs():
    from viet_asr_amd.metrics import confusion_pairs
    rows = [[("hit", "a", "a"), ("sub", "bat", "cat"), ("del", None, "on"), ("sub", "teh", "the")],
            [("ins", "uh", None), ("sub", "bat", "cat"), ("sub", "cat", "bat")], []]
    got = confusion_pairs(rows)
    assert isinstance(got, Counter)
    assert got == Counter({("cat", "bat"): 2, ("the", "teh"): 1, ("bat", "cat"): 1})          # (ref_word, hyp_word)
    assert confusion_pairs([]) == Counter()
    # from the restatement's replay: the same shape word_alignment returns
    sp = [0]
    h, r = [1, 0, 2, 2, 0, 3], [1, 0, 2, 0, 3, 0, 4]
    steps = AR.replay(AR.ops(h, r, sp)[1], WR.split_ids(h, sp), WR.split_ids(r, sp))
    assert confusion_pairs([steps]) == Counter({((2,), (2, 2)): 1})
