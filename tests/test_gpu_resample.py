"""-m gpu: csrc/audio.hip alone against float64 (tests/resample_reference.py): vasr_resample_f32 through ctypes in its three
kernel forms -- integer up-sampling p = 2 ... 16, the phase kernel, the generic gather --, every table entry asserting the form it
was written for (p = 16 | 17 and the 60 KB LDS limit from both sides straddled), and vasr_pcm16_to_f32.

Per table entry and signal (noise, impulses six decades over a noise floor, noise at 300 x) ONE ragged launch of every length of
the ratio: 0, 1, 2, around one wing's input span, around the output-tile seams.  d_out pre-filled with NaN, ld_out 300 columns
past ceil(L * ratio) (into another tile), the input NaN from each row's length to the pitch.  Per row: len_out as the reference's,
every stored value finite, |y - y64| inside the ELEMENTWISE bound C * 2^-24 * sum |w_i| |x_i| + 2^-24 |y64| with the derived C = 4
(resample_reference's docstring has the count), exact zeros from the computed count to ld_out.  Then: NaN padding against zero
padding, each row alone against its row in the batch, and a repeated launch, bit for bit; audio.resample against the ctypes
call, with two ratios < 1 in its table cache; lengths above the pitch and below zero clamped.

Largest |y - y64| / bound seen on an MI355X, per form (the figure is reported through _record, not a threshold):
    up       0.500 (p = 5, impulse; 0.34 ... 0.50 on impulse over the five p, 0.22 ... 0.31 on noise and loud)
    phase    0.615 (3 / 2, impulse; 0.44 ... 0.62 on impulse over the ten ratios, 0.13 ... 0.43 on noise and loud)
    generic  0.526 (16 000 / 22 051, impulse; 0.45 ... 0.53 on impulse, 0.11 ... 0.41 on noise and loud)
The numpy emulation of the kernels' arithmetic (tests/test_resample_host.py) predicts these to the second digit: 0.61 at 17 / 1
and 3 / 2.  The long sums of the down-sampling ratios sit lowest (1 / 11, 1 / 12 on noise: 0.11 ... 0.14), the worst-case count
per tap averaging out over their 1400 and more taps.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_reference as R
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

_IDS = [R.case_id(c) for c in R.ALL_CASES]
_tables = {}


def _table(gpu, ratio):
    key = ratio if ratio < 1 else 1.0
    if key not in _tables:
        _tables[key] = torch.from_numpy(R.table32(ratio)).to(gpu)
    return _tables[key]


def _resample(gpu, x, lens, sr_in, sr_out, ld_out=None, pad=float("nan"), spare_rows=0):
    """vasr_resample_f32 on x [B, L] with row lengths lens (any int64: the library clamps them) -> (y [B, ld_out], len_out [B]).
    The input is `pad` wherever a row has no sample (and in `spare_rows` whole rows behind the batch); d_out starts as NaN."""
    from viet_asr_amd import _lib
    L_ = _lib.lib()
    B, L = x.shape
    ratio = float(sr_out) / float(sr_in)
    if ld_out is None:
        ld_out = int(np.ceil(L * ratio)) + 300
    host = np.full((B + spare_rows, L), pad, dtype=np.float32)
    for b in range(B):
        n = int(min(max(int(lens[b]), 0), L))
        host[b, :n] = x[b, :n]
    xd = torch.from_numpy(host).to(gpu)
    ld = torch.from_numpy(np.asarray(lens, dtype=np.int64)).to(gpu)
    tab = _table(gpu, ratio)
    yd = torch.full((B, ld_out), float("nan"), dtype=torch.float32, device=gpu)
    lo = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    rc = L_.vasr_resample_f32(C.c_void_p(xd.data_ptr()), L, C.c_void_p(ld.data_ptr()), B, C.c_void_p(tab.data_ptr()),
                              tab.shape[0], R.NUM_TABLE, ratio, C.c_void_p(yd.data_ptr()), ld_out, C.c_void_p(lo.data_ptr()),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, L_)
    torch.cuda.synchronize()
    return yd.cpu().numpy(), lo.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_IDS)
def test_every_length_and_signal_inside_the_bound(gpu, case):
    kind, sr_in, sr_out = case
    assert R.form(sr_in, sr_out)[0] == kind              # (the library's own choice equals form(): test_resample_host.py)
    for sig in R.SIGNALS:
        x, lens, rows = R.reference(sr_in, sr_out, sig)
        y, ln = _resample(gpu, x, lens, sr_in, sr_out)
        worst, at = 0.0, None
        for b, n in enumerate(lens):
            y64, A, n_comp, n_ret = rows[b]
            assert ln[b] == n_ret, (case, sig, int(n), int(ln[b]), n_ret)
            assert np.isfinite(y[b]).all(), (case, sig, int(n), np.argwhere(~np.isfinite(y[b]))[:5])
            w = R.worst(y[b], y64, A)
            if w > worst:
                worst, at = w, int(n)
            assert not y[b, n_comp:].any(), (case, sig, int(n), np.argwhere(y[b, n_comp:] != 0)[:5] + n_comp)
        print(f"{R.case_id(case)} {sig}: worst err / bound {worst:.3f} (row of {at} samples)")
        _record("resample_bound", case=R.case_id(case), form=kind, signal=sig, worst=worst, row=at)
        assert worst <= 1.0, (case, sig, worst, at)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=_IDS)
def test_padding_is_never_read_and_rows_are_independent(gpu, case):
    """NaN behind every row's length gives the bits zero padding gives; a launch repeated gives the same bits; each row alone
    (batch 1, the same pitch) is bit-equal to its row in the ragged batch."""
    kind, sr_in, sr_out = case
    for sig in R.SIGNALS:
        x, lens, _ = R.reference(sr_in, sr_out, sig)
        y, ln = _resample(gpu, x, lens, sr_in, sr_out)
        y0, ln0 = _resample(gpu, x, lens, sr_in, sr_out, pad=0.0)
        assert np.array_equal(_bits(y), _bits(y0)) and np.array_equal(ln, ln0), (case, sig, "padding")
        y2, ln2 = _resample(gpu, x, lens, sr_in, sr_out)
        assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(ln, ln2), (case, sig, "repeat")
        if sig == "impulse":
            for b, n in enumerate(lens):
                y1, ln1 = _resample(gpu, x[b:b + 1], lens[b:b + 1], sr_in, sr_out, ld_out=y.shape[1])
                assert np.array_equal(_bits(y1[0]), _bits(y[b])) and ln1[0] == ln[b], (case, int(n), "row alone")


def test_wrapper_agrees_with_the_c_call(gpu):
    """audio.resample against vasr_resample_f32, bit for bit, one ratio per form -- and again once a second ratio < 1 has
    populated the wrapper's table cache, which keys on the ratio only when it is < 1."""
    from viet_asr_amd import audio
    order = [(8000, 16000, "up"), (48000, 16000, "phase"), (44100, 16000, "generic"), (48000, 16000, "phase"),
             (16000, 24000, "phase"), (8000, 16000, "up"), (44100, 16000, "generic")]
    lens = np.array([1500, 0, 777, 1], dtype=np.int64)
    x = np.zeros((4, 1500), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = R.signal("noise", int(n), 40 + b)
    for sr_in, sr_out, kind in order:
        assert R.form(sr_in, sr_out)[0] == kind
        ld_out = max(int(np.ceil(1500 * (float(sr_out) / sr_in))), 1)
        want, want_len = _resample(gpu, x, lens, sr_in, sr_out, ld_out=ld_out, pad=0.0)
        y, ln = audio.resample(torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu), sr_in, sr_out)
        assert tuple(y.shape) == want.shape and np.array_equal(ln.cpu().numpy(), want_len), (sr_in, sr_out)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(want)), (sr_in, sr_out)


@pytest.mark.parametrize("sr_in,sr_out,kind", [(8000, 16000, "up"), (3000, 2000, "phase"), (44100, 16000, "generic")])
def test_lengths_are_clamped_to_the_pitch(gpu, sr_in, sr_out, kind):
    """A length above ld_in counts as ld_in, a negative one as 0 (an all-zero row, len_out 0).  The input has one spare row behind
    the batch and holds finite samples everywhere, so that code without the clamp would over-read inside the allocation."""
    assert R.form(sr_in, sr_out)[0] == kind
    B, L = 3, 1301
    x = np.stack([R.signal("noise", L, 60 + b) for b in range(B)])
    full = np.full(B, L, dtype=np.int64)
    want, want_len = _resample(gpu, x, full, sr_in, sr_out, pad=0.25, spare_rows=1)
    assert (want_len == R.out_counts(L, float(sr_out) / sr_in)[1]).all()
    y, ln = _resample(gpu, x, full + 5, sr_in, sr_out, pad=0.25, spare_rows=1)
    assert np.array_equal(_bits(y), _bits(want)) and np.array_equal(ln, want_len)
    lens = full.copy()
    lens[1] = -3
    y, ln = _resample(gpu, x, lens, sr_in, sr_out, pad=0.25, spare_rows=1)
    assert ln[1] == 0 and not y[1].any() and np.isfinite(y[1]).all()
    for b in (0, 2):
        assert np.array_equal(_bits(y[b]), _bits(want[b])) and ln[b] == want_len[b]


def _pcm(gpu, pcm, guard=8):
    """vasr_pcm16_to_f32 on the first len(pcm) elements of buffers `guard` elements longer -> the whole float buffer."""
    from viet_asr_amd import _lib
    L_ = _lib.lib()
    n = len(pcm)
    src = torch.from_numpy(np.concatenate([pcm, np.full(guard, 12345, dtype=np.int16)])).to(gpu)
    out = torch.full((n + guard,), float("nan"), dtype=torch.float32, device=gpu)
    _lib.check(L_.vasr_pcm16_to_f32(C.c_void_p(src.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), L_)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_pcm16_every_value_and_every_tail(gpu):
    """All 65 536 int16 values == int / 32768 (float64, cast to float32: exact, a 16-bit integer times 2^-15); element counts
    around the short4 body's scalar tail, with nothing written past n."""
    every = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    out = _pcm(gpu, every)
    assert np.array_equal(out[:65536], (every.astype(np.float64) / 32768.0).astype(np.float32))
    assert np.isnan(out[65536:]).all()
    rng = np.random.default_rng(9)
    for n in (1, 2, 3, 4, 5, 7, 1023, 1024, 1025):
        pcm = rng.integers(-32768, 32768, size=n).astype(np.int16)
        out = _pcm(gpu, pcm)
        assert np.array_equal(out[:n], (pcm.astype(np.float64) / 32768.0).astype(np.float32)), n
        assert np.isnan(out[n:]).all(), n
