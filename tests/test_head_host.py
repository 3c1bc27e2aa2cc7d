"""CPU checks of tests/head_reference.py, the float64 reference, error bound, case tables and kernel-choice restatement
tests/test_gpu_head.py judges the CTC head by: the bound against honest float32 arithmetic in the kernel's order (not
tighter than that) and against nine planted defects (tighter than those, on every case a defect can occur in; the smallest
factor per defect is printed), the tables against the list of paths they claim to reach, the share of near-tie frames, and the
refusals that need no device."""
import numpy as np
import pytest
import torch

import head_reference as H

CUS = 256          # the table's claims are stated for an MI355X's 256 compute units
EPI_MUTANTS = tuple(m for m in H.MUTANTS if m not in H.GEMM_MUTANTS)
_smallest = {}


def _note(mutant, case, factor):
    if mutant not in _smallest or factor < _smallest[mutant][0]:
        _smallest[mutant] = (factor, case.name)


def _pred_rule_broken(logp, pred):
    """What test_gpu_head.py asserts of the prediction: the first index of the maximum of the kernel's own log-probs."""
    return not np.array_equal(pred, H.first_argmax(logp))


@pytest.mark.parametrize("case", H.EPI_CASES, ids=repr)
def test_epilogue_restatement_inside_the_bound_and_defects_outside(case):
    z, expect = H.logits(case)
    T = case.frames
    assert z.shape == (case.B, case.V, H.SEP.padded(T)) and np.isnan(z[:, :, T:]).all()
    z64 = torch.from_numpy(z[:, :, :T]).double()
    ref, bound = H.epilogue_bound(z64)
    lp, pred = H.f32_epilogue(z[:, :, :T])
    worst, msg = H.judge(lp, ref, bound)
    assert msg is None, msg
    assert not _pred_rule_broken(lp, pred)
    for (b, t), c in expect.items():
        assert int(pred[b, t]) == c, (b, t, int(pred[b, t]), c)
    fin = torch.isfinite(ref)
    if case.kind == "gauss":
        crude = float(torch.where(fin, (torch.from_numpy(lp).double() - ref).abs() / H.crude_epilogue_bound(z64), torch.zeros_like(ref)).max())
        assert crude <= 0.75, crude          # the calibration of the docstring: 0.62 at worst on 4000 frames a shape
    if case.kind == "nonfinite":
        rows = ~fin.all(-1)
        assert int(rows.sum()) >= 5 * case.B and bool(torch.isnan(ref[0, 3]).all()) and bool(torch.isinf(ref[0, 40, case.V - 1]))
    if not case.planted:                      # the near-tie cap, from the float64 reference alone
        excluded = float(1 - H.decided(ref, bound).double().mean())
        assert excluded <= H.NEAR_TIE_CAP, excluded
    missed = []
    for m in EPI_MUTANTS:
        if not H.applies(m, case):
            continue
        lpm, predm = H.f32_epilogue(z[:, :, :T], m)
        if m == "tie_later":
            factor = float("inf") if _pred_rule_broken(lpm, predm) else 0.0
        else:
            factor = H.judge(lpm, ref, bound)[0]
        _note(m, case, factor)
        if not factor > 1.0:
            missed.append((m, factor))
    assert not missed, missed


@pytest.mark.parametrize("case", H.GEMM_CASES, ids=repr)
def test_head_restatement_inside_the_bound_and_defects_outside(case):
    x = H.head_input(case)
    sd = H.head_weights(case)
    assert x.shape == (case.B, case.K, case.T) and float(x.min()) >= 0
    if case.B > 1:                            # one utterance far above the others: the f16x2 scale is per utterance
        level = np.abs(x[:, :, 1:] if case.T > 1 else x).reshape(case.B, -1).max(1)
        assert level[1] > 50 * np.delete(level, 1).max()
    ref, bounds = H.head_reference(case, x)
    lp, pred = H.f32_head(x, sd)
    worst, msg = H.judge(lp, ref, bounds["fp32"])
    assert msg is None, msg
    for a in ("f16x2", "bf16x3"):
        assert (bounds[a] >= bounds["fp32"]).all(), a
    assert (H.first_argmax(ref.numpy())[:, 0] == case.V - 1).all()          # the steered frame
    for a in H.ARITHS:                        # the near-tie cap per arithmetic, from the float64 reference alone
        excluded = float(1 - H.decided(ref, bounds[a]).double().mean())
        assert excluded <= H.NEAR_TIE_CAP, (a, excluded)
    if case.wgain > 1:
        assert float(ref.abs().max()) > 200
    missed = []
    for m in H.MUTANTS:
        if m == "tie_later" or not H.applies(m, case):
            continue
        lpm, _ = H.f32_head(x, sd, m)
        factor = min(H.judge(lpm, ref, bounds[a])[0] for a in H.ARITHS)
        _note(m, case, factor)
        if not factor > 1.0:
            missed.append((m, factor))
    assert not missed, missed


def test_every_defect_was_tried_and_its_smallest_factor():
    """(Runs after the two parametrised tests of this file.)  Every defect of the list met cases it applies to."""
    tried = {m: [c.name for c in H.EPI_CASES + H.GEMM_CASES if H.applies(m, c)] for m in H.MUTANTS}
    assert all(len(v) >= 3 for v in tried.values()), {m: len(v) for m, v in tried.items()}
    for m in H.MUTANTS:
        if m in _smallest:
            f, name = _smallest[m]
            print(f"{m}: smallest |y - ref| / bound = {f:.3g} ({name}; {len(tried[m])} cases)")
    # above the depth at which w_hi is asserted it is the bit equalities' business: the rule is the stated one
    assert all(c.K <= H.W_HI_MAX_K for c in H.GEMM_CASES if H.applies("w_hi", c))


def test_the_tables_meet_every_path():
    plans = {(c.name, a): H.head_plan(c.V, c.K, c.B, c.T, a, CUS) for c in H.GEMM_CASES for a in H.ARITHS}
    by = lambda a, **kw: [c for c in H.GEMM_CASES if all(plans[(c.name, a)][k] == v for k, v in kw.items())]
    # every class count meets every kernel of every arithmetic
    for V in H.CLASS_COUNTS:
        mine = lambda cs: any(c.V == V for c in cs)
        assert mine(by("f16x2", kernel="lat")) and mine(by("f16x2", kernel="64x32")) and mine(by("f16x2", kernel="128x64")), V
        assert mine(by("bf16x3", kernel="64x32")) and mine(by("bf16x3", kernel="128x64")) and mine(by("fp32", kernel="fp32")), V
        assert not by("bf16x3", kernel="lat")
    assert {c.V for c in H.GEMM_CASES} == set(H.CLASS_COUNTS) == {c.V for c in H.EPI_CASES if not c.planted}
    # every epilogue instantiation, both sides of every edge, every VMAX at 1, 64 and 65 frames
    assert {H.vmax_of(V) for V in H.CLASS_COUNTS} == {32, 64, 96, 128}
    for edge in (32, 64, 96):
        assert {edge, edge + 1} <= set(H.CLASS_COUNTS) and H.vmax_of(edge) + 32 == H.vmax_of(edge + 1)
    for vmax in (32, 64, 96, 128):
        seen = {c.frames for c in H.EPI_CASES if not c.planted and H.vmax_of(c.V) == vmax}
        assert {1, 64, 65} <= seen, (vmax, seen)
    assert {c.frames for c in H.EPI_CASES} == set(H.EPI_FRAMES) and {c.B for c in H.EPI_CASES} == {1, 3}
    assert {H.vmax_of(c.V) for c in H.EPI_CASES if c.kind == "tie_quarters"} == {32, 64, 96, 128}
    assert {c.kind for c in H.EPI_CASES} == {"gauss", "tie_quarters", "tie_ends", "all_equal", "nonfinite", "span170"}
    # every split tile the head can take, with and without a full row block
    for a in ("f16x2", "bf16x3"):
        assert {plans[(c.name, a)]["blocks"] for c in by(a, kernel="128x64")} == {("full",), ("partial",)}
        got = {plans[(c.name, a)]["blocks"] for c in by(a, kernel="64x32")}
        assert got == {("partial", "empty"), ("full", "empty"), ("full", "partial"), ("full", "full")}, got
    assert {plans[(c.name, "f16x2")]["blocks"] for c in by("f16x2", kernel="lat")} == {("full",), ("partial",)}
    assert {plans[(c.name, "fp32")]["blocks"] for c in by("fp32", kernel="fp32")} == {("full",), ("partial",)}
    # V = 64 (block 0 full, block 1 empty), V = 65 (block 1 stores one row), V = 128 (all full) on the 64 x 32 tile
    for V, blocks in ((64, ("full", "empty")), (65, ("full", "partial")), (128, ("full", "full"))):
        assert any(c.V == V and plans[(c.name, "bf16x3")]["blocks"] == blocks for c in by("bf16x3", kernel="64x32")), V
    # the latency kernel at all three depths, the chunked kernel at depths it refuses (in f16x2) and at its own (in bf16x3)
    assert {c.K for c in by("f16x2", kernel="lat")} == {256, 512, 1024}
    assert {c.K for c in by("f16x2", kernel="64x32")} == {64, 192}
    assert {c.K for c in by("bf16x3", kernel="64x32")} == set(H.GEMM_K)
    assert {c.T for c in H.GEMM_CASES} == set(H.GEMM_FRAMES) and {c.B for c in H.GEMM_CASES} == {1, 2, 3, H.BIG[0]}
    # the large batch is the smallest that takes the 128 x 64 tile at T' = 100
    B, T = H.BIG
    assert H.SEP.split_tile(128, H.SEP.padded(T), B, CUS) == 3 and H.SEP.split_tile(128, H.SEP.padded(T), B - 1, CUS) == 4
    # the forced settings of the bit-equality test move every one of its cases to another kernel in at least one arithmetic
    for c in H.BITS_CASES:
        own = H.head_plan(c.V, c.K, c.B, c.T, "f16x2", CUS)["kernel"]
        assert own == "lat" and H.head_plan(c.V, c.K, c.B, c.T, "f16x2", CUS, lat=False)["kernel"] == "64x32"
        assert H.head_plan(c.V, c.K, c.B, c.T, "bf16x3", CUS, force_tile=3)["kernel"] == "128x64"
    assert {c.V for c in H.BITS_CASES} == {29, 64, 65, 128} and {c.K for c in H.BITS_CASES} == {256, 1024}


def test_restated_choice_equals_the_librarys_host_arithmetic():
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    for T in list(H.EPI_FRAMES) + list(H.GEMM_FRAMES):
        assert H.SEP.padded(T) == int(L.vasr_padded_frames(T))


def test_refusals_that_need_no_device():
    from viet_asr_amd import _lib, synth
    with pytest.raises(NotImplementedError):                               # VASR_ERR_UNSUPPORTED
        _lib.Handle(dec_feat_in=1024, num_classes=129)
    h = _lib.Handle(dec_feat_in=96, num_classes=29)
    h.load_state_dict(synth.decoder_state_dict(96, 29, 1))
    with pytest.raises((NotImplementedError, ValueError, _lib.VasrError), match="64"):
        h.finalize()
    h.close()
    L = _lib.dev_lib()
    INVALID = -1
    assert H.null_pointer_call(L, 1, 10, 0) == INVALID
    assert H.null_pointer_call(L, 1, 10, -3) == INVALID
    assert H.null_pointer_call(L, 1, 10, 129) == INVALID
    assert H.null_pointer_call(L, 1, 0, 29) == INVALID
    assert H.null_pointer_call(L, 1, -5, 29) == INVALID
    assert H.null_pointer_call(L, 0, 10, 29) == INVALID
    assert H.null_pointer_call(L, 1, 10, 29, logp=False, pred=False) == INVALID
    assert b"bench_ctc_head" in L.vasr_last_error()
    assert int(L.vasr_bench_ctc_head(None, 1, 10, 29, _lib.C.c_void_p(4096), None, None)) == INVALID
