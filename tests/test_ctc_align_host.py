"""CPU checks of the forced CTC alignment: the float64 and float32 restatements (tests/ctc_align_reference.py) against
brute-force enumeration of every valid path of every tiny row, each broken rule caught there, the best path below the sum
over paths (tests/ctc_reference.py), the greedy transcript's alignment equal to the argmax path, the exported symbols /
signatures / header declarations with the ABI still 8, every refusal of vasr_ctc_align_f32 before a device is touched, the
workspace size, the stage's refusals, and the host arithmetic of ``VietASR.align``."""
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_align_reference as AR
import ctc_reference as CR
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -5
BLANK, LABELS = 3, 3


def tiny_cases():
    """Every target with L <= 3 over 3 labels at every T <= 6, on log-probs that are multiples of 1/8 (every sum is exact in
    both formats: ties are real ties, and frequent), a third of the cases with -inf entries."""
    rng = np.random.default_rng(5)
    n = 0
    for L in range(4):
        for y in itertools.product(range(LABELS), repeat=L):
            for T in range(1, 7):
                lp = -(rng.integers(0, 9, (T, LABELS + 1)).astype(np.float32)) / np.float32(8)
                if n % 3 == 2:
                    lp[rng.random(lp.shape) < 0.25] = -np.inf
                n += 1
                yield lp, T, np.array(y, dtype=np.int64)


@pytest.fixture(scope="module")
def enumerated():
    """(logp, T, y, brute-force score, brute-force path) of every tiny case, enumerated once"""
    return [(lp, T, y) + AR.brute_force(lp, T, y, BLANK) for lp, T, y in tiny_cases()]


def test_restatements_equal_brute_force_enumeration(enumerated):
    paths = ties = none = 0
    for lp, T, y, want, want_path in enumerated:
        for run in (AR.align64, AR.align32):
            r = run(lp, T, y, len(y), BLANK)
            assert float(r["score"]) == want, (y, T, float(r["score"]), want)
            if want_path is None:
                assert (r["path"] == -1).all() and (r["start"] == -1).all() and (r["token_logp"] == 0).all()
                continue
            assert (r["path"][:T] == want_path).all(), (y, T, r["path"], want_path)
            AR.validate(r["path"], r["start"], r["end"], T, y, len(y))
            assert AR.path_score64(lp, r["path"], T, y, BLANK) == want
            for j in range(len(y)):
                assert float(r["token_logp"][j]) == float(lp[r["start"][j] : r["end"][j], y[j]].astype(np.float64).sum())
        none += want_path is None
        paths += want_path is not None
        ties += want_path is not None and float(AR.align64(lp, T, y, len(y), BLANK, broken="tie_reversed")["score"]) == want \
            and (AR.align64(lp, T, y, len(y), BLANK, broken="tie_reversed")["path"][:T] != want_path).any()
    assert paths >= 100 and none >= 20 and ties >= 20, (paths, none, ties)


@pytest.mark.parametrize("rule", AR.BROKEN)
def test_each_broken_rule_is_caught(enumerated, rule):
    """The validator or the comparison of the score with the enumeration catches the three rules that change which paths
    count; the reversed tie-break keeps score and validity and is caught by the comparison of the path."""
    caught = {"validator": 0, "score": 0, "path": 0}
    for lp, T, y, want, want_path in enumerated:
        r = AR.align64(lp, T, y, len(y), BLANK, broken=rule)
        if float(r["score"]) != want:
            caught["score"] += 1
        elif want_path is not None:
            try:
                AR.validate(r["path"], r["start"], r["end"], T, y, len(y))
            except AssertionError:
                caught["validator"] += 1
            else:
                caught["path"] += int((r["path"][:T] != want_path).any())
    print(rule, caught)
    if rule == "tie_reversed":
        assert caught["path"] and not caught["validator"] and not caught["score"]
    else:
        assert caught["validator"] + caught["score"] > 0


def random_rows(seed, n, C=6, T=30):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        L = int(rng.integers(0, 12))
        y = rng.integers(0, C - 1, max(L, 1)).astype(np.int64)
        for i in range(1, L):
            if rng.random() < 0.3:
                y[i] = y[i - 1]
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32) * 2), dim=-1).numpy()
        yield lp, int(rng.integers(max(AR.min_frames(y, L), 1), T + 1)), y, L


def test_best_path_is_no_more_than_the_sum_over_paths():
    n = 0
    for lp, T, y, L in random_rows(6, 40):
        r64, r32 = AR.align64(lp, T, y, L, 5), AR.align32(lp, T, y, L, 5)
        total = -CR.loss64(lp, T, y, L, 5)
        assert math.isfinite(total) and float(r64["score"]) <= total + 1e-12, (float(r64["score"]), total)
        AR.validate(r64["path"], r64["start"], r64["end"], T, y, L)
        AR.validate(r32["path"], r32["start"], r32["end"], T, y, L)
        b = AR.bound(r64)
        assert AR.close(r32["score"], r64["score"], b) and b < 1e-4
        assert abs(AR.path_score64(lp, r64["path"], T, y, 5) - float(r64["score"])) <= 1e-12
        assert AR.path_score64(lp, r32["path"], T, y, 5) >= float(r64["score"]) - 2 * b
        n += 1
    assert n == 40


def test_conventions():
    lp = next(random_rows(7, 1))[0]
    tgt = np.array([0, 1, 1, 2])
    nan = lambda r: math.isnan(float(r["score"])) and (r["path"] == -1).all() and (r["start"] == -1).all()  # noqa: E731
    assert nan(AR.align64(lp, -1, tgt, 2, 5)) and nan(AR.align64(lp, 3, tgt, -2, 5))
    assert nan(AR.align64(lp, 6, np.array([0, 5, 1]), 3, 5)) and nan(AR.align64(lp, 6, np.array([0, 6]), 2, 5))
    assert nan(AR.align32(lp, 6, np.array([-1, 0]), 2, 5))
    assert not nan(AR.align64(lp, 6, np.array([0, 5, 9, -5]), 1, 5))          # ids behind the length are not looked at
    assert float(AR.align64(lp, 0, tgt, 0, 5)["score"]) == 0.0 and float(AR.align64(lp, 0, tgt, 1, 5)["score"]) == -np.inf
    assert float(AR.align64(lp, 4, tgt, 4, 5)["score"]) == -np.inf            # 4 ids, one repeat: 5 frames
    one = AR.align64(lp, 5, tgt, 4, 5)                                        # the unique path
    assert one["path"][:5].tolist() == [1, 3, 4, 5, 7] and one["start"].tolist() == [0, 1, 3, 4] and one["end"].tolist() == [1, 2, 4, 5]
    empty = AR.align64(lp, 4, tgt, 0, 5)                                      # L == 0: the blank's sum
    assert abs(float(empty["score"]) - float(lp[:4, 5].astype(np.float64).sum())) < 1e-12 and empty["path"][:4].tolist() == [0] * 4
    assert AR.align64(lp, 99, tgt, 99, 5)["path"].tolist() == AR.align64(lp, 30, tgt, 4, 5)["path"].tolist()   # clamped
    dead = lp.copy()
    dead[:, 5] = -np.inf                                                      # no blank: the repeat has no path, others do
    assert float(AR.align32(dead, 6, tgt, 4, 5)["score"]) == -np.inf
    assert math.isfinite(float(AR.align32(dead, 3, np.array([0, 1, 2]), 3, 5)["score"]))


def test_greedy_transcript_aligns_to_the_argmax_path():
    rng = np.random.default_rng(8)
    rows = 0
    for _ in range(20):
        T, C = 40, 5
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32) * 3), dim=-1).numpy()
        top = np.sort(lp, axis=1)
        assert (top[:, -1] > top[:, -2]).all()                               # a unique argmax in every frame
        k = lp.argmax(axis=1)
        y, states, prev = [], [], C - 1
        for c in k:
            if c != C - 1 and c != prev:
                y.append(int(c))
            states.append(2 * len(y) if c == C - 1 else 2 * len(y) - 1)
            prev = c
        L, y = len(y), np.array(y or [0], dtype=np.int64)
        for run in (AR.align64, AR.align32):
            r = run(lp, T, y, L, C - 1)
            assert r["path"][:T].tolist() == states
            assert abs(float(r["score"]) - float(lp.max(axis=1).astype(np.float64).sum())) <= AR.bound(AR.align64(lp, T, y, L, C - 1))
        rows += 1
    assert rows == 20


NAMES = ("vasr_ctc_align_f32", "vasr_ctc_align_workspace_bytes")


def test_new_symbols_are_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == 17 and len(_lib.SIGNATURES[NAMES[1]][1]) == 3
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    decl = header[header.index(f" {NAMES[0]}("):]
    decl = decl[: decl.index(";")]
    assert decl.count(",") == 16 and "wins only STRICTLY" in header and "EVERY element of every non-NULL output is written" in header


def source_constants():
    src = open(os.path.join(ROOT, "viet-asr_amd", "csrc", "vasr_internal.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (kCtc\w+) = (\d+);", src)}


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f, size = L.vasr_ctc_align_f32, L.vasr_ctc_align_workspace_bytes
    p = 4096
    ok = dict(x=p, fr=p, b=2, t=10, c=5, blank=4, tgt=p, w=3, tl=p, score=p, start=p, end=p, tok=p, path=p, ws=p, wsb=None)

    def call(**kw):
        a = dict(ok, **kw)
        wsb = a["wsb"] if a["wsb"] is not None else max(size(a["b"], a["t"], a["w"]), 1)
        return f(a["x"], a["fr"], a["b"], a["t"], a["c"], a["blank"], a["tgt"], a["w"], a["tl"], a["score"], a["start"], a["end"],
                 a["tok"], a["path"], a["ws"], wsb, None)

    for name in ("x", "fr", "tgt", "tl", "score", "start", "end", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert call(b=0) == INVALID and call(b=-3) == INVALID and call(t=-1) == INVALID and call(w=-1) == INVALID
    assert call(c=1, blank=0) == INVALID and call(c=0, blank=0) == INVALID
    assert call(blank=-1) == INVALID and call(blank=5) == INVALID
    need = size(2, 10, 3)
    assert need > 0 and call(wsb=need - 1) == INVALID and call(wsb=0) == INVALID
    assert str(need).encode() in L.vasr_last_error()
    assert call(w=4097) == UNSUPPORTED and call(w=1 << 40) == UNSUPPORTED
    assert b"4096" in L.vasr_last_error()
    assert call(w=4097, b=0) == INVALID and call(w=4097, ws=None) == INVALID      # an argument error wins over the size limit
    with pytest.raises(NotImplementedError):
        _lib.check(call(w=5000), L)
    with pytest.raises(ValueError):
        _lib.check(call(b=0), L)


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_workspace_bytes_is_monotone_and_within_two_bits_per_slot(which):
    from viet_asr_amd import _lib
    size = getattr(_lib, which)().vasr_ctc_align_workspace_bytes
    k = source_constants()
    lanes, narrow, wide, align = k["kCtcLossLanes"], k["kCtcLossNarrowSlots"], k["kCtcLossWideSlots"], k["kCtcAlignWorkspaceAlign"]
    assert (lanes, narrow, wide, k["kCtcLossMaxWidth"]) == (256, 4, 33, 4096)
    assert size(0, 10, 3) == size(-1, 10, 3) == size(2, -1, 3) == size(2, 10, -1) == size(2, 10, 4097) == 0
    batches, frames, widths = (1, 2, 7, 512), (0, 1, 2, 63, 64, 65, 1501, 100000), (0, 1, 151, 511, 512, 513, 4096)
    for b, t, w in itertools.product(batches, frames, widths):
        slots = narrow if 2 * w + 1 <= lanes * narrow else wide
        n = size(b, t, w)
        assert 0 < n <= b * t * (lanes * slots * 2 // 8) + align, (b, t, w, n)
        assert n >= b * t * ((2 * w + 1) * 2 // 8)                              # and room for 2 bits per state that exists
    for (b0, t0, w0), (b1, t1, w1) in itertools.product(itertools.product(batches, frames, widths), repeat=2):
        if b0 <= b1 and t0 <= t1 and w0 <= w1:
            assert size(b0, t0, w0) <= size(b1, t1, w1)
    assert size(2 ** 31 - 1, 2 ** 62, 4096) == 2 ** 64 - 1                      # what does not fit fits no workspace


def test_stage_refuses_host_tensors_and_bad_shapes():
    from viet_asr_amd import stages
    from viet_asr_amd._lib import VasrError
    i64, z = torch.int64, torch.zeros
    with pytest.raises(VasrError):
        stages.ctc_align(z(2, 3, 4), torch.tensor([3, 3]), z(2, 1, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3), torch.tensor([3, 3]), z(2, 1, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3, 4, dtype=i64), torch.tensor([3, 3]), z(2, 1, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3, 4), torch.tensor([3, 3]), z(2, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3, 4), torch.tensor([3, 3]), z(3, 1, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3, 4), torch.tensor([3]), z(2, 1, dtype=i64), torch.tensor([1, 1]), 3)
    with pytest.raises(ValueError):
        stages.ctc_align(z(2, 3, 4), torch.tensor([3, 3]), z(2, 1, dtype=i64), torch.tensor([1, 1, 1]), 3)


def test_word_grouping_and_seconds_of_align():
    from viet_asr_amd.infer import alignment_entries
    chars = list(" ab  c d")
    start = np.array([0, 2, 5, 9, 10, 12, 20, 21], dtype=np.int32)
    end = np.array([1, 4, 6, 10, 12, 13, 21, 25], dtype=np.int32)
    logp = np.array([-0.5, -1.0, -0.25, -2.0, -0.125, -4.0, -0.0625, -8.0], dtype=np.float32)
    cs, ws = alignment_entries(chars, start, end, logp, 0.02)
    assert [c["char"] for c in cs] == chars and [c["logp"] for c in cs] == logp.tolist()
    assert [c["start"] for c in cs] == [int(s) * 0.02 for s in start] and [c["end"] for c in cs] == [int(e) * 0.02 for e in end]
    assert ws == [{"word": "ab", "start": 2 * 0.02, "end": 6 * 0.02, "logp": -1.25},
                  {"word": "c", "start": 12 * 0.02, "end": 13 * 0.02, "logp": -4.0},
                  {"word": "d", "start": 21 * 0.02, "end": 25 * 0.02, "logp": -8.0}]
    assert "".join(c["char"] for c in cs).split() == [w["word"] for w in ws]
    assert alignment_entries([], start[:0], end[:0], logp[:0], 0.02) == ([], [])
    cs, ws = alignment_entries(["x"], start[:1], end[:1], logp[:1], 0.04)
    assert ws == [{"word": "x", "start": 0.0, "end": 0.04, "logp": -0.5}]
