"""CPU checks of tests/resample_reference.py, the float64 reference tests/test_gpu_resample.py holds csrc/audio.hip to: the
reference against the oracle and librosa's length rule, the float32 emulation of the three kernels inside the bound, mutants of
that emulation outside it, and the restated kernel choice against the library's own (vasr_resample_form, host arithmetic).

What the mutants show (``impulse`` batches, worst |y - y64| / bound over the rows; the unmutated emulation stays <= 0.63):
every mutant is caught at every table entry where it changes a bit, by factors of 8 (17 / 1, wing capped) to 1e9.  Against
the tolerance the suite had before -- |y - oracle| < 2e-6 absolute on noise -- the same mutants at 8 -> 16 kHz and 48 -> 16 kHz:
    drop_outer    8.6e-8, 3.1e-8   PASSES the old tolerance
    cap_wing      7.8e-8, 3.1e-8   PASSES the old tolerance
    eta_zero      no-op at p = 2 (eta is 0 there); 8.6e-4 at 1 / 3: caught
    phase_shift   0.73 at p = 2: caught; no-op at p = 1
    seam_n        0.51, 3.3e-3: caught
    right_from_n  1.04, 0.36: caught
so the outermost taps of a wing were the gap: they could vanish unnoticed (on noise even the elementwise bound lets them, at
0.78 and 0.15 of it: the ``impulse`` signal is what judges a tap at its own scale).  The emulation also found a defect that no
tolerance had met because no test ran the ratio: the phase kernel took a phase's filter from the first output of the tile with
that phase and n from ``(double)t / ratio``, and at 100 / 99 (7 / 3, 9 / 7) that quotient lands one ulp under an integer for
some t (100 / 99: t = 500, 900, 1000 ...), so those outputs met a filter built for the next sample: errors of the size of the
signal (``parent_floor`` below; 1.0 on noise at amplitude 0.3).  The kernel now takes n and the phase from integers.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import resample_reference as R
from oracle import audio_oracle as AO

OLD_TOL = 2e-6          # tests/test_audio_data.py::test_device_resampler_matches_oracle
EXISTING_PAIRS = [(8000, 16000), (16000, 8000), (11025, 16000), (16000, 24000), (48000, 16000)]
_IDS = [R.case_id(c) for c in R.ALL_CASES]


def test_every_case_has_the_form_it_was_written_for():
    for kind, sr_in, sr_out in R.ALL_CASES:
        assert R.form(sr_in, sr_out)[0] == kind, (kind, sr_in, sr_out, R.form(sr_in, sr_out))
    # the pairs that straddle each limit: p = 16 | 17, and the 60 KB of LDS from both directions
    assert [R.form(1000, 1000 * p)[0] for p in (16, 17)] == ["up", "phase"]
    assert [R.form(1000 * q, 1000 * p)[0] for p, q in ((100, 99), (112, 111))] == ["phase", "generic"]
    assert [R.form(1000 * q, 1000)[0] for q in (11, 12)] == ["phase", "generic"]
    assert R.form(22051, 16000) == ("generic", 0, 0)


@pytest.mark.parametrize("sr_in,sr_out", EXISTING_PAIRS)
def test_reference_agrees_with_the_oracle(sr_in, sr_out):
    """Both accumulate in float64 over the same float64 window; the oracle floors ``t / ratio`` in doubles and hands its sum
    back rounded to float32, so the comparison is at 1e-9 max |x| plus that one rounding, 2^-24 |y|."""
    x = R.signal("noise", 600, 3)
    want = AO.resample(x, sr_in, sr_out)
    y, A, n_comp, n_ret = R.resample64(x, sr_in, sr_out)
    ratio = float(sr_out) / sr_in
    assert (n_comp, n_ret) == (int(600 * ratio), int(np.ceil(600 * ratio))) and len(want) == n_ret == len(y)
    assert not y[n_comp:].any()
    tol = 1e-9 * float(np.abs(x).max()) + R.U * np.abs(y)
    assert (np.abs(y - want) <= tol).all(), float(np.abs(y - want).max())


def test_reference_length_rule():
    y, A, n_comp, n_ret = R.resample64(np.ones(5000, dtype=np.float32), 11025, 16000)
    assert (n_comp, n_ret, len(y), len(A)) == (7256, 7257, 7257, 7256) and y[7256] == 0.0
    for n in (0, 1, 2):
        for sr_in, sr_out in ((16000, 8000), (8000, 16000), (12000, 1000)):
            y, A, n_comp, n_ret = R.resample64(np.ones(n, dtype=np.float32), sr_in, sr_out)
            assert (n_comp, n_ret) == R.out_counts(n, float(sr_out) / sr_in) and len(y) == n_ret


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_IDS)
def test_emulation_stays_inside_the_bound(case):
    """Float32 table, eta and weights, with (phase, generic) and without (up) the float32 product, float64 sum: every signal, the
    two smallest tile lengths of the entry (one below a tile seam, one at it)."""
    kind, sr_in, sr_out = case
    worst = 0.0
    for sig in R.SIGNALS:
        for n in R.tile_lengths(sr_in, sr_out)[:2]:
            x = R.signal(sig, n, 11, R.seams(sr_in, sr_out, n) + R.outer_taps(sr_in, sr_out, n))
            y, A, n_comp, _ = R.resample64(x, sr_in, sr_out)
            e = R.emulate(x, sr_in, sr_out)
            assert np.isfinite(e).all() and not e[n_comp:].any()
            worst = max(worst, R.worst(e, y, A))
    print(f"{R.case_id(case)}: emulation worst err / bound {worst:.3f}")
    assert worst <= 1.0, (case, worst)


def _noop(mutant, sr_in, sr_out):
    """Where a mutant cannot change a bit: eta is 0 at every phase when max(p, q) divides the 512 table entries per zero
    crossing; with one phase there is no other phase's filter; and the wing cap only bites phase 0's left wing, whose second
    output (t = 640) lies past the rows of 640 / 441."""
    f = Fraction(sr_out, sr_in)
    return ((mutant == "eta_zero" and R.NUM_TABLE % max(f.numerator, f.denominator) == 0)
            or (mutant == "phase_shift" and f.numerator == 1)
            or (mutant == "cap_wing" and f == Fraction(640, 441)))


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_IDS)
def test_mutants_break_the_bound_on_impulse(case):
    """The ragged ``impulse`` batch the GPU test launches, each mutant of the emulation over all its rows: some row has to leave
    the bound -- or the mutant provably changes nothing at this ratio, then every bit is equal."""
    kind, sr_in, sr_out = case
    x, lens, rows = R.reference(sr_in, sr_out, "impulse")
    base = [R.emulate(x[b, :n], sr_in, sr_out) for b, n in enumerate(lens)]
    assert max(R.worst(base[b], rows[b][0], rows[b][1]) for b in range(len(lens))) <= 1.0
    for mutant in R.MUTANTS:
        out = [R.emulate(x[b, :n], sr_in, sr_out, mutant=mutant) for b, n in enumerate(lens)]
        if _noop(mutant, sr_in, sr_out):
            assert all(np.array_equal(o, e) for o, e in zip(out, base)), (case, mutant)
            continue
        worst = max(R.worst(out[b], rows[b][0], rows[b][1]) for b in range(len(lens)))
        print(f"{R.case_id(case)} {mutant}: worst err / bound {worst:.3g}")
        assert worst > 1.0, (case, mutant, worst)


def test_old_absolute_tolerance_let_the_outer_taps_vanish():
    """The same mutants on ``noise`` against the tolerance the suite had: which of them 2e-6 absolute lets through (module
    docstring).  Dropping or capping a wing's outermost taps passes it; the others, where they change anything, do not."""
    for sr_in, sr_out in ((8000, 16000), (48000, 16000)):
        n = R.tile_lengths(sr_in, sr_out)[3]
        x = R.signal("noise", n, 5)
        y, A, n_comp, _ = R.resample64(x, sr_in, sr_out)
        base = R.emulate(x, sr_in, sr_out)
        assert float(np.abs(base - y).max()) < OLD_TOL
        for mutant in R.MUTANTS:
            e = R.emulate(x, sr_in, sr_out, mutant=mutant)
            err = float(np.abs(e - y).max())
            print(f"{sr_in} -> {sr_out} {mutant}: max |y - y64| {err:.2e}, err / bound {R.worst(e, y, A):.3g}")
            if mutant in ("drop_outer", "cap_wing"):
                assert not np.array_equal(e, base) and err < OLD_TOL, (mutant, err)     # wrong, and it passed
            elif not _noop(mutant, sr_in, sr_out):
                assert err > OLD_TOL, (mutant, err)


def test_double_quotient_in_the_phase_kernel_was_a_defect():
    """100 / 99: ``t / ratio`` in doubles is one ulp under t q / p at t = 500, 900, 1000, ...; the phase kernel as it stood
    (``parent_floor``) is off by a whole sample there, the integer form is inside the bound."""
    sr_in, sr_out = 99000, 100000
    t = np.arange(2048, dtype=np.int64)
    low = np.nonzero((t.astype(np.float64) / (100000.0 / 99000.0)).astype(np.int64) != t * 99 // 100)[0]
    assert low.size and low[0] == 500
    x = R.signal("noise", 1100, 2)
    y, A, n_comp, _ = R.resample64(x, sr_in, sr_out)
    assert R.worst(R.emulate(x, sr_in, sr_out), y, A) <= 1.0
    parent = R.emulate(x, sr_in, sr_out, mutant="parent_floor")
    err = np.abs(parent - y)[:n_comp]
    assert R.worst(parent, y, A) > 1e3 and err[500] > 1e-3 and float(err.max()) > 0.1
    # the generic kernel floors the same quotient, but takes filter and n from it together: continuity covers it
    assert R.worst(R.emulate(x, sr_in, sr_out, kind="generic"), y, A) <= 1.0


def test_form_equals_the_librarys_choice():
    """vasr_resample_form (devtools build; launch_resample calls the same function) against the restatement: every table
    entry, then p / q over 1 .. 128 x 1 .. 16."""
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    code = {0: "generic", 1: "phase", 2: "up"}
    pairs = [(sr_in, sr_out) for _, sr_in, sr_out in R.ALL_CASES] + [(q, p) for p in range(1, 129) for q in range(1, 17)]
    seen = set()
    for sr_in, sr_out in pairs:
        p, q = C.c_int(-1), C.c_int(-1)
        rc = L.vasr_resample_form(float(sr_out) / float(sr_in), R.NWIN, R.NUM_TABLE, C.byref(p), C.byref(q))
        assert rc in code, (sr_in, sr_out, rc)
        assert (code[rc], p.value, q.value) == R.form(sr_in, sr_out), (sr_in, sr_out)
        seen.add(code[rc])
    assert seen == {"generic", "phase", "up"}
    assert L.vasr_resample_form(2.0, R.NWIN, R.NUM_TABLE, None, None) == 2
    assert L.vasr_resample_form(0.0, R.NWIN, R.NUM_TABLE, None, None) == -1          # what vasr_resample_f32 refuses
    assert L.vasr_resample_form(1e-4, R.NWIN, R.NUM_TABLE, None, None) == -1         # index_step 0
