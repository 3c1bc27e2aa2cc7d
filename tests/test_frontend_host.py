"""CPU checks of tests/frontend_reference.py, the float64 chain and the two error bounds tests/test_gpu_frontend.py judges the
mel front end by: the oracle's float32 melspec_forward (torch.stft) and an honest float32 restatement stay inside the bounds
on every case and element, every structural defect a rewrite of csrc/frontend.hip could make leaves them on every case it
can occur in, the bounds are not vacuous, and the case table reaches what it claims to reach."""
import functools

import numpy as np
import pytest
import torch

import frontend_reference as FE

CASES = FE.CASES


@functools.lru_cache(maxsize=None)
def _ref(name):
    """The float64 chain and bound of a case, computed once and shared (read only)."""
    case = FE.BY_NAME[name]
    x, lens = FE.inputs(case)
    r = FE.case_chain(case, x, lens)
    for a in r.values():
        a.setflags(write=False)
    return x, lens, r


def _oracle_raw(case, x, lens, normalize=None):
    from oracle import quartznet_oracle as O
    d = FE.description(case)
    kw = dict(n_window_size=case.win, n_window_stride=case.hop, preemph=case.preemph, log_zero_guard_value=case.guard,
              log_zero_guard_type=case.guard_type, fb=d["filterbank"], window=torch.from_numpy(d["window"]), normalize=normalize)
    if not case.own:
        m, s = O.melspec_forward(x, lens, **kw)
        return m.numpy(), s.numpy()
    # row-independent mode: each row as the batch of one the reference would run it as (rows the reference cannot pad stay 0)
    out = np.zeros((case.B, FE.NMELS, case.T), np.float32)
    for b in range(case.B):
        if lens[b] > FE.NFFT // 2:
            m, _ = O.melspec_forward(x[b:b + 1, :lens[b]], lens[b:b + 1], **kw)
            out[b, :, :m.shape[2]] = m[0].numpy()
    return out, FE.seq_len(lens, case.hop)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_and_float32_restatement_inside_the_raw_bound(case):
    x, lens, r = _ref(case.name)
    got, seq = _oracle_raw(case, x, lens)
    assert np.array_equal(seq, r["seq"])
    t = np.arange(case.T)[None, :]
    assert (got[np.broadcast_to((t >= seq[:, None])[:, None, :], got.shape)] == 0).all()      # masked frames exactly 0
    worst, big, fails = FE.judge(got, r["raw"], r["bound"], r["judged"])
    f32 = FE.case_chain(case, x, lens, dtype=np.float32)
    w32, _, fails32 = FE.judge(f32["raw"], r["raw"], r["bound"], r["judged"])
    print(f"{case}: form {case.form}, largest bound {big:.3e}, oracle / bound {worst:.3f}, float32 restatement / bound {w32:.3f}")
    assert not fails and not fails32, (fails, fails32)
    assert np.isfinite(r["bound"]).all()
    if case.signal == "white" and case.guard == 2.0 ** -24 and case.guard_type == "add":
        # white noise at 0.1: the bound is not vacuous on any judged element.  A one-hot bank judges single bins, whose
        # power is exponentially distributed and comes as close to 0 as there are elements to look at: there the logarithm
        # itself is ill-conditioned and a true bound is large, so the cap holds for all but one element in a hundred.
        b = np.broadcast_to(r["judged"][:, None, :], r["bound"].shape)
        cap = np.quantile(r["bound"][b], 0.99) if case.bank.startswith("onehot") else big
        assert cap < 1e-3, (big, cap)


@pytest.mark.parametrize("mode", ("per_feature", "all_features"))
@pytest.mark.parametrize("case", [c for c in CASES if c.norm], ids=repr)
def test_oracle_inside_the_normalisation_bound(case, mode):
    """The oracle's float32 normalisation of ITS raw log-mel against the float64 normalisation of the same values, inside the
    bound with the term for statistics summed in float32 (the device sums in double and is judged without that term)."""
    x, lens, r = _ref(case.name)
    raw, seq = _oracle_raw(case, x, lens)
    got, _ = _oracle_raw(case, x, lens, normalize=mode)
    ref, bound = FE.normalize(raw, seq, mode, float32_sums=True)
    worst, big, fails = FE.judge(got, ref, bound)
    print(f"{case} {mode}: largest bound {big:.3e}, oracle / bound {worst:.3f}")
    assert not fails, fails
    if mode == "per_feature":
        for b in np.flatnonzero(seq == 1):
            assert np.isnan(got[b, :, 0]).all() and (got[b, :, 1:] == 0).all()
    for b in np.flatnonzero(seq == 0):
        assert (got[b] == 0).all()


@pytest.mark.parametrize("defect", sorted(FE.DEFECTS))
def test_structural_defect_leaves_the_raw_bound(defect):
    """A float32 restatement with the defect is outside the bound on every case the defect can occur in (FE.DEFECTS says
    which), by the printed factor."""
    hit = 0
    for case in CASES:
        if not FE.DEFECTS[defect](case):
            continue
        x, lens, r = _ref(case.name)
        bad = FE.case_chain(case, x, lens, dtype=np.float32, defect=defect)
        worst, _, _ = FE.judge(bad["raw"], r["raw"], r["bound"], r["judged"])
        print(f"{defect} on {case}: {worst:.3g} times the bound")
        assert worst > 2.0, (defect, case.name, worst)
        hit += 1
    assert hit


@pytest.mark.parametrize("defect", FE.NORM_DEFECTS)
def test_normalisation_defect_leaves_its_bound(defect):
    for case in (c for c in CASES if c.norm):
        x, lens, r = _ref(case.name)
        raw = r["raw"].astype(np.float32)
        mode = "per_feature" if defect != "all_padded" else "all_features"
        ref, bound = FE.normalize(raw, r["seq"], mode)
        bad, _ = FE.normalize(raw, r["seq"], mode, defect=defect)
        keep = ~np.isnan(ref) & ~np.isnan(bad)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(keep & (bad != ref), np.abs(bad - ref) / bound, 0.0)
        # std_biased, eps_under_root: every row with at least two valid frames and a deviation;  all_padded: every row
        # shorter than the batch
        rows = [b for b in range(case.B) if (2 <= r["seq"][b] if defect != "all_padded" else 1 <= r["seq"][b] < case.T)
                and np.ptp(raw[b, :, :r["seq"][b]]) > 0]
        print(f"{defect} on {case}: {min(ratio[b].max() for b in rows):.3g} times the bound on the mildest of {len(rows)} rows")
        assert rows and all(ratio[b].max() > 2.0 for b in rows)


def test_table_reaches_what_it_claims():
    forms = {c.form for c in CASES}
    assert forms == {8, 32}
    prod = {-(-c.T // 32) * c.B for c in CASES}
    assert 127 in prod and 128 in prod                                        # the threshold from both sides
    assert any(c.form == 32 and c.hop > 236 and FE.lds_bytes(32, c.hop) > 65536 for c in CASES)
    assert FE.lds_bytes(32, 236) <= 65536 < FE.lds_bytes(32, 237) and FE.lds_bytes(32, 512) == 99712
    assert FE.lds_bytes(8, 512) < 65536
    assert any(c.win % 2 for c in CASES)
    assert any(c.T % 8 for c in CASES if c.form == 8) and any(c.T % 32 for c in CASES if c.form == 32)
    alone = set()
    for j in range(5):
        fb = FE.one_hot_bank(j)
        assert ((fb != 0).sum(1) == 1).all()
        alone |= set(np.flatnonzero(fb.any(0)).tolist())
    assert alone == set(range(FE.NBINS)) and all(f"onehot{j}" in {c.bank for c in CASES} for j in range(5))
    box = FE.boxcar_bank()
    assert max(np.flatnonzero(r)[-1] - np.flatnonzero(r)[0] + 1 for r in box) == FE.MEL_TAPS
    assert {c.preemph for c in CASES} >= {0.97, 0.0, None}
    assert {(c.guard_type, c.guard) for c in CASES} >= {("add", 2.0 ** -24), ("clamp", 1e-5), ("clamp", FE.TINY32)}
    for a, b in FE.PAIRS:
        ca, cb = FE.BY_NAME[a], FE.BY_NAME[b]
        n = min(ca.B, cb.B)
        xa, la = FE.inputs(ca)
        xb, lb = FE.inputs(cb)
        assert ca.L == cb.L and np.array_equal(xa[:n], xb[:n]) and np.array_equal(la[:n], lb[:n])
    assert {FE.BY_NAME[a].form for a, b in FE.PAIRS} == {8} and 32 in {FE.BY_NAME[b].form for a, b in FE.PAIRS}
    # the mixed batch: every signal kind and every length option, with the gap's all-zero frames below the row's seq
    mix = FE.BY_NAME["mix_f8"]
    x, lens, r = _ref("mix_f8")
    assert {k for k, _ in FE.MIX_ROWS} == set(FE.KINDS) and {o for _, o in FE.MIX_ROWS} == set(range(7))
    gap = [k for k, _ in FE.MIX_ROWS].index("gap")
    assert (r["raw"][gap][:, r["judged"][gap]] == np.log(mix.guard)).any()
    # the valid-frame counts of the normalisation case
    n = FE.BY_NAME["norm_counts"]
    assert sorted(set(_ref("norm_counts")[2]["seq"].tolist())) == [0, 1, 2, 255, 256, 257, n.T]


def test_form_rule_and_seq_quirk():
    assert FE.form(127, 5) == 8 and FE.form(128, 5) == 32 and FE.form(1, 32 * 127 + 1) == 32 and FE.form(1, 32 * 127) == 8
    # float32: 16777217 samples round to 16777216 before the division
    assert FE.seq_len([16777217], 1)[0] == 16777216
    from oracle import quartznet_oracle as O
    lens = np.array([0, 1, 159, 160, 161, 16777217, 2 ** 31 + 129], np.int64)
    for hop in (1, 3, 160, 237, 512):
        assert np.array_equal(FE.seq_len(lens, hop), O.featurizer_seq_len(torch.from_numpy(lens), hop).numpy())
