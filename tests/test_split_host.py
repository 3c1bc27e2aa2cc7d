"""CPU checks of the split at silences: the float64 restatement (tests/split_reference.py) against a literal transcription of
librosa.effects.split's published form and against its own invariants, the decidability of every frame and of every cut of
every table case, what the table has to contain, audio.plan_segments on hand-made tables, the exported symbols / signatures /
header declarations with the ABI still 8, and every refusal of the new entry points before a device is touched."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import split_reference as S
import trim_reference as T
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -5
ALL = [(i, d) for i in range(len(S.TABLE)) for d in S.DTYPES]


def test_hand_computed_rows():
    # frame 2, hop 2, n = 12: frames (b,a) (b,c) (d,e) (f,g) (h,i) (j,k) (l,k): y = [b | a .. l | k]
    x = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0], np.float32)
    flags, sums = S.frame_flags(x, 60.0, 2, 2)
    assert flags.tolist() == [False, False, True, False, False, True, True] and sums.tolist() == [0, 0, 1, 0, 0, 2, 1]
    assert S.split(x, 60.0, 2, 2) == [(4, 6), (10, 12)] == S.librosa_split(x, 60.0, 2, 2)       # the last end is min(n, 14)
    assert S.split(x, 60.0, 2, 2, m=2) == [(4, 6), (10, 12)] and S.split(x, 60.0, 2, 2, m=3) == [(4, 12)]   # a gap of two frames
    # cuts: a run of 7 frames with sums 5 4 3 2 2 4 5, M = 4: window frames 2 .. 4 -> the first 2 (frame 3); the rest is 4 long
    assert S.cut_run(0, 7, np.array([5.0, 4, 3, 2, 2, 4, 5]), 4)[0] == [(0, 3), (3, 7)]
    assert S.cut_run(0, 7, np.zeros(7), 4)[0] == [(0, 2), (2, 4), (4, 7)]                       # ties: s + ceil(M / 2)
    assert S.cut_run(0, 7, np.zeros(7), 3)[0] == [(0, 2), (2, 4), (4, 7)] and S.cut_run(0, 7, np.zeros(7), 2)[0] == \
        [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 7)]
    assert S.cut_run(2, 6, np.arange(9.0), 4)[0] == [(2, 6)] and S.cut_run(2, 6, np.arange(9.0), 0)[0] == [(2, 6)]
    # n == 0 has no segment; the empty last interval of librosa: one frame per hop, the only loud frame starts at n
    assert S.split(np.zeros(0, np.float32)) == [] and S.librosa_split(np.zeros(0, np.float32)) == []
    last = np.zeros(8192, np.float32)
    last[-1] = 0.9
    assert S.split(last, 60.0, 256, 256) == [(8192, 8192)] == S.librosa_split(last, 60.0, 256, 256)
    assert S.bridged_runs([1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0], 1) == [(0, 1), (2, 3), (5, 6), (9, 10)]
    assert S.bridged_runs([1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0], 2) == [(0, 3), (5, 6), (9, 10)]
    assert S.bridged_runs([1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0], 3) == [(0, 6), (9, 10)]
    assert S.bridged_runs([0, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1, 0], 4) == [(1, 11)] and S.bridged_runs([0, 0], 1) == []


def test_the_table_holds_what_it_has_to():
    names = [t[0] for t in S.TABLE]
    assert len(set(names)) == len(names) and {(t[3], t[4]) for t in S.TABLE} == set(S.FORMS) == set(T.FORMS)
    assert S.PAIRS == ((1, 0), (8, 0), (1, 40), (8, 40), (3, 7), (1, 2)) and S.DTYPES == ("float32", "int16")
    assert set().union(*S.groups().values()) == set(range(len(names)))
    assert max(t[2] for t in S.TABLE) <= 400000                     # a few hundred thousand samples at the most
    for fl, hop in S.FORMS:
        mine = [i for i, t in enumerate(S.TABLE) if (t[3], t[4]) == (fl, hop)]
        fams = {S.TABLE[i][1] for i in mine}
        assert set(T.NOISE_FAMILIES) <= fams and {"pauses", "dips", "zeros", "below_amin_flat", "last_burst", "click_last"} <= fams
        lens = {S.TABLE[i][2] for i in mine}
        assert {1, hop - 1, hop, hop + 1} <= lens and (0 in lens or (fl, hop) == (2048, 512))
        for dtype in S.DTYPES:
            # pauses of m - 1, m and m + 1 silent frames between two non-silent ones, for every m of the pairs
            gaps = set()
            for i in mine:
                if S.TABLE[i][1] == "pauses" and S.TABLE[i][5] == 60.0:
                    c = S.case(i, dtype)
                    nz = np.flatnonzero(S.frame_flags(c["x"], 60.0, fl, hop)[0])
                    gaps |= set((np.diff(nz) - 1).tolist())
            assert {1, 2, 3, 4, 7, 8, 9} <= gaps, (fl, hop, dtype, sorted(gaps))
            # a row of more than 256 frames and more than 256 segments; an empty [n, n) interval where the form has one
            assert any(1 + S.TABLE[i][2] // hop > 256 and len(S.expected(i, dtype, m, M)) > 256 for i in mine for m, M in S.PAIRS)
            if fl == hop:
                assert any((c, c) in S.expected(i, dtype, 1, 0) for i in mine for c in [S.TABLE[i][2]] if c % hop == 0 and c)
            # the dips take the cuts: every cut of the long dips row under M = 40 falls on a frame of the quieter stretches
            i = names.index(f"dips-n{120 * hop + 7}-f{fl}h{hop}-db60")
            c = S.case(i, dtype)
            segs = S.split_frames(c["x"], 60.0, fl, hop, 1, 40)[0]
            assert len(segs) >= 3 and segs[0][0] == 0
            sums = S.frame_flags(c["x"], 60.0, fl, hop)[1]
            assert all(sums[f1] < 0.5 * np.median(sums) for _, f1 in segs[:-1])
            # ties fall at s + ceil(M / 2): all-zero rows and the +-2^-20 rows, longer than M frames
            for fam in ("zeros", "below_amin_flat"):
                i = names.index(f"{fam}-n{100 * hop + 5}-f{fl}h{hop}-db60")
                for m, M in S.PAIRS:
                    want, s = [], 0
                    while M > 0 and 101 - s > M:
                        want.append((s, s + (M + 1) // 2))
                        s += (M + 1) // 2
                    want.append((s, 101))
                    n = 100 * hop + 5
                    assert list(S.expected(i, dtype, m, M)) == [(min(n, a * hop), min(n, b * hop)) for a, b in want], (fam, m, M)


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_librosa_form_and_invariants(dtype):
    for i in range(len(S.TABLE)):
        c = S.case(i, dtype)
        fl, hop, n = c["frame_length"], c["hop_length"], c["n"]
        assert list(S.expected(i, dtype, 1, 0)) == S.librosa_split(c["x"], c["top_db"], fl, hop), c["name"]
        for m, M in S.PAIRS:
            segs, runs, _, flags = S.split_frames(c["x"], c["top_db"], fl, hop, m, M)
            assert [(min(n, a * hop), min(n, b * hop)) for a, b in segs] == list(S.expected(i, dtype, m, M))
            # ascending and disjoint, at most M frames, contiguous inside a run: the union is exactly the bridged runs
            assert all(a < b for a, b in segs) and all(segs[k][1] <= segs[k + 1][0] for k in range(len(segs) - 1)), c["name"]
            if M:
                assert all(b - a <= M for a, b in segs) and all(e - s <= M * hop for s, e in S.expected(i, dtype, m, M))
            covered = np.zeros(flags.size + 1, int)
            for a, b in segs:
                covered[a:b] += 1
            in_runs = np.zeros(flags.size + 1, int)
            for a, b in runs:
                in_runs[a:b] += 1
            assert np.array_equal(covered, in_runs) and covered.max(initial=0) <= 1, c["name"]
            assert covered[:-1][flags].all(), c["name"]                         # every non-silent frame is inside a segment
            # a run starts and ends on a non-silent frame and holds no m silent frames in a row; between runs there are m
            for a, b in runs:
                assert flags[a] and flags[b - 1]
                quiet = np.flatnonzero(flags[a:b])
                assert (np.diff(quiet) - 1 < m).all()
            for (_, b), (a2, _) in zip(runs, runs[1:]):
                assert a2 - b >= m and not flags[b:a2].any()
            assert len(segs) <= flags.size


def test_every_frame_and_every_cut_is_decidable():
    """The condition on the GPU tests: every frame of the table falls on the same side of the threshold in any summation order
    and in either form of the comparison, and every cut has one smallest frame sum by more than 2^-40 relative -- or sums that
    are exact in any order, where equal sums are equal bits."""
    closest, frames, cuts, ties, tight = np.inf, 0, 0, 0, np.inf
    for i, dtype in ALL:
        c = S.case(i, dtype)
        if c["n"] == 0:
            assert all(S.expected(i, dtype, m, M) == () for m, M in S.PAIRS)
            continue
        mse = T.frame_energies(c["x"], c["frame_length"], c["hop_length"])
        ratio = T.threshold_ratios(mse, c["top_db"])
        dist = np.abs(ratio - 1.0).min()
        assert dist > T.band(c["frame_length"]), (c["name"], dtype, dist)
        closest, frames = min(closest, dist), frames + ratio.size
        flags, sums = S.frame_flags(c["x"], c["top_db"], c["frame_length"], c["hop_length"])
        assert np.array_equal(flags, ratio > 1.0), c["name"]                    # the product form decides as the log form does
        exact = S.sums_exact(c["x"], sums.max())
        assert exact or dtype == "float32"                                      # every int16 row is exact
        for m, M in S.PAIRS:
            for window, _ in S.split_frames(c["x"], c["top_db"], c["frame_length"], c["hop_length"], m, M)[2]:
                margin = S.cut_margin(window)
                cuts += 1
                if exact:
                    ties += margin == 0.0
                    continue
                assert margin > S.CUT_MARGIN, (c["name"], dtype, m, M, margin)
                tight = min(tight, margin)
    print(f"{frames} frames, closest ratio to the threshold |r - 1| = {closest:.3g} (band {T.band(2048):.3g}); {cuts} cuts, "
          f"{ties} of them ties between exact sums, smallest margin of the others {tight:.3g} (needed {S.CUT_MARGIN:.3g})")
    assert cuts > 1000 and ties > 100 and S.CUT_MARGIN == 2.0 ** -40


def test_sums_exact():
    assert S.sums_exact(np.zeros(10, np.float32), 0.0) and S.sums_exact(np.array([3, -32768, 77], np.int16), 2048.0)
    assert S.sums_exact(np.full(9, 2.0 ** -20, np.float32), 2048 * 2.0 ** -40)
    assert S.sums_exact(np.array([0.1, 0.2], np.float32), 0.05)                 # squares of odd * 2^-27, 2^-26: multiples of 2^-54
    assert not S.sums_exact(np.array([0.1, 1e-5], np.float32), 0.0101)          # 1e-5f squared reaches below 2^-70
    assert S.sums_exact(np.array([0.9, 0.0], np.float32), 1.62)                 # one click, mirrored once at the most
    assert S.cut_margin(np.array([3.0, 1.0, 2.0])) == 0.5 and S.cut_margin(np.array([1.0, 1.0, 2.0])) == 0.0
    assert S.cut_margin(np.zeros(3)) == 0.0


# ---- audio.plan_segments ----------------------------------------------------------------------------------------------
def test_plan_segments_on_hand_made_tables():
    from viet_asr_amd import audio
    bounds = [[[100, 200], [260, 300], [1000, 1500], [-1, -1]],
              [[0, 50], [50, 90], [-1, -1], [-1, -1]],
              [[-1, -1]] * 4]
    count, lengths = [3, 2, 0], [1520, 95, 700]
    segs, dropped = audio.plan_segments(bounds, count, lengths, pad=0, min_samples=0)
    assert segs == [(0, 100, 100), (0, 260, 40), (0, 1000, 500), (1, 0, 50), (1, 50, 40)] and dropped == [0, 0, 0]
    # pad 50: clamped at the row's start / end and at the midpoint (200 + 260) // 2 = 230 of a gap narrower than 2 pad
    segs, dropped = audio.plan_segments(bounds, count, lengths, pad=50, min_samples=0)
    assert segs == [(0, 50, 180), (0, 230, 120), (0, 950, 570), (1, 0, 50), (1, 50, 45)] and dropped == [0, 0, 0]
    for (r0, s0, n0), (r1, s1, n1) in zip(segs, segs[1:]):
        assert r0 != r1 or s0 + n0 <= s1                                        # never overlapping
    # short segments are dropped AFTER padding, the order of the others is kept
    segs, dropped = audio.plan_segments(bounds, count, lengths, pad=50, min_samples=120)
    assert segs == [(0, 50, 180), (0, 950, 570)] and dropped == [1, 2, 0]
    segs, dropped = audio.plan_segments(bounds, count, lengths, pad=0, min_samples=40)
    assert segs == [(0, 100, 100), (0, 1000, 500), (1, 0, 50)] and dropped == [1, 1, 0]
    # librosa's empty last interval [n, n) is widened like any other; tensors are accepted; integers come back
    segs, dropped = audio.plan_segments(torch.tensor([[[0, 256], [512, 512]]]), torch.tensor([2]), torch.tensor([512]), 100, 0)
    assert segs == [(0, 0, 356), (0, 412, 100)] and dropped == [0]
    assert all(isinstance(v, int) for s in segs for v in s)
    segs, dropped = audio.plan_segments(np.zeros((2, 0, 2), np.int64), np.zeros(2, np.int64), [5, 6], 3, 0)
    assert segs == [] and dropped == [0, 0]
    with pytest.raises(ValueError):
        audio.plan_segments(bounds, [5, 0, 0], lengths, 0, 0)                   # the device table overflowed
    d = {k: v.default for k, v in inspect.signature(audio.split_silence).parameters.items()}
    assert (d["top_db"], d["frame_length"], d["hop_length"], d["min_silence_frames"], d["max_segment_frames"], d["max_segments"]) \
        == (60.0, 2048, 512, 1, 0, None)
    assert list(inspect.signature(audio.gather_segments).parameters) == ["signal", "rows", "starts", "lengths", "width"]
    for f in (audio.split_silence, audio.gather_segments):
        with pytest.raises(Exception):
            f(torch.zeros(2, 100), torch.tensor([100, 50]), [0, 0], [1, 1]) if f is audio.gather_segments else \
                f(torch.zeros(2, 100), torch.tensor([100, 50]))


def test_transcribe_long_keywords():
    from viet_asr_amd import configs, infer
    d = {k: v.default for k, v in inspect.signature(infer.VietASR.transcribe_long).parameters.items()}
    assert (d["sample_rate"], d["top_db"], d["min_silence"], d["max_seconds"], d["pad"], d["batch_size"], d["decoder"], d["align"]) \
        == (None, 60.0, 0.3, None, None, 64, "greedy", False)
    assert "convention" in infer.VietASR.transcribe_long.__doc__.lower()
    for name in ("quartznet15x5", "quartznet12x1_vi"):
        assert configs.builtin(name)["AudioToTextDataLayer"]["max_duration"] == 16.7


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
NAMES = ("vasr_split_silence_f32", "vasr_split_silence_pcm16", "vasr_gather_segments_f32", "vasr_gather_segments_pcm16",
         "vasr_split_silence_workspace_bytes")


def test_new_symbols_are_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    want = {NAMES[0]: 15, NAMES[1]: 15, NAMES[2]: 10, NAMES[3]: 10, NAMES[4]: 4}
    for n, args in want.items():
        assert len(_lib.SIGNATURES[n][1]) == args
        decl = header[header.rindex(f" {n}("):]                                 # the declaration, behind the comment
        assert decl[: decl.index(";")].count(",") == args - 1
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    assert "parity unpinned" in header[header.index("Split at silences"): header.index(f" {NAMES[0]}(")]


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    size = L.vasr_split_silence_workspace_bytes
    assert size(0, 10, 64, 16) == size(-1, 10, 64, 16) == size(2, -1, 64, 16) == 0
    assert size(2, 10, 64, 0) == size(2, 10, 60, 16) == size(2, 10, 8704, 512) == size(2, 10, 16, 64) == 0
    for b, ld, (fl, hop) in itertools.product((1, 7), (0, 17, 160000), ((64, 16), (256, 256), (2048, 512))):
        chunks, runs = ld // hop + fl // hop, (ld // hop + 1) // 2 + 1          # one float64 per hop, two int64 per run
        assert b * (chunks * 8 + runs * 16) <= size(b, ld, fl, hop) <= b * (chunks * 8 + runs * 16) + 768
        assert size(b, ld, fl, hop) >= L.vasr_trim_silence_workspace_bytes(b, ld, fl, hop) - 512
    assert size(2 ** 31 - 1, 2 ** 62, 8192, 1) == 2 ** 64 - 1
    p, q = 4096, 8192
    for entry in NAMES[:2]:
        f = getattr(L, entry)
        ok = dict(x=p, ld=1000, ln=p, b=2, db=60.0, fl=2048, hop=512, m=1, M=0, bd=q, ms=8, ct=q, ws=p, wsb=None)

        def call(**kw):
            a = dict(ok, **kw)
            wsb = a["wsb"] if a["wsb"] is not None else max(size(a["b"], max(a["ld"], 0), a["fl"], a["hop"]), 1)
            return f(a["x"], a["ld"], a["ln"], a["b"], a["db"], a["fl"], a["hop"], a["m"], a["M"], a["bd"], a["ms"], a["ct"],
                     a["ws"], wsb, None)

        for name in ("x", "ln", "bd", "ct", "ws"):
            assert call(**{name: None}) == INVALID, name
        assert call(b=0) == INVALID and call(b=-3) == INVALID and call(ld=-1) == INVALID
        assert call(m=0) == INVALID and call(m=-2) == INVALID and call(M=1) == INVALID and call(M=-1) == INVALID
        assert call(ms=-1) == INVALID
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert call(db=bad) == INVALID
        need = size(2, 1000, 2048, 512)
        assert need > 0 and call(wsb=need - 1) == INVALID and call(wsb=0) == INVALID
        assert str(need).encode() in L.vasr_last_error()
        for fl, hop in ((2048, 0), (2048, -512), (2048, 500), (0, 512), (8704, 512), (512, 1024)):
            assert call(fl=fl, hop=hop) == UNSUPPORTED, (fl, hop)
            assert call(fl=fl, hop=hop, b=0) == INVALID and call(fl=fl, hop=hop, m=0) == INVALID    # an argument error wins
        with pytest.raises(NotImplementedError):
            _lib.check(call(fl=2048, hop=500), L)
        with pytest.raises(ValueError):
            _lib.check(call(M=1), L)
    for entry in NAMES[2:4]:
        f = getattr(L, entry)
        ok = dict(x=p, ld=1000, b=2, row=p, st=p, ln=p, s=3, out=q, ldo=100)

        def call(**kw):
            a = dict(ok, **kw)
            return f(a["x"], a["ld"], a["b"], a["row"], a["st"], a["ln"], a["s"], a["out"], a["ldo"], None)

        for name in ("x", "row", "st", "ln", "out"):
            assert call(**{name: None}) == INVALID, name
        assert call(out=p) == INVALID                                           # d_out must not alias d_in
        assert call(b=0) == INVALID and call(ld=-1) == INVALID and call(s=0) == INVALID and call(s=-1) == INVALID
        assert call(ldo=0) == INVALID and call(ldo=-5) == INVALID
