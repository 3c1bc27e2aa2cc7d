"""-m gpu: the mel front end (csrc/frontend.hip) against float64 at every window, hop, form, signal, filterbank and option of
tests/frontend_reference.py's table, through _lib.Handle(frontend=...) and stages.melspec (vasr_melspec_f32).

Per case: the kernel form by the restated rule; seq equal to the float32 rule; every frame >= seq exactly 0; every stored
element of the raw log-mel inside the elementwise bound around the float64 chain (nothing sampled or averaged); two calls
bit-equal; for a 32-frame case the first rows run alone (8-frame form) bit-equal; in row-independent mode every row bit-equal
to the batch of one on x[:len].  For the cases marked so, per_feature and all_features of a second and third handle against
the float64 normalisation of the FIRST handle's raw output inside the normalisation bound alone, with the NaN and zero rules.
Then the refusal of a 33-bin filter, and the guard regions around the outputs of a direct call.

Largest |device - float64| / bound on an MI355X, from a single run:
    cases                                                        8-frame form   32-frame form
    forms a-e (320 / 160)                                        0.27           0.27
    windows and hops, LDS <= 64 KB                               0.27           0.40
    hops 237, 320, 512 (LDS 65616, 75904, 99712 bytes)                          0.32
    mixed signals, lengths, row-independent mode                 0.69           0.73
    filterbanks (one-hot, boxcar, empty rows, 300-3400 Hz)       0.31           0.41
    preemph 0 / None, clamp 1e-5, clamp at tiny                  0.64
    normalisation alone: per_feature 0.99, all_features 0.93 (the half-ulp rounding of the float32 mean is attained)
(The mixed batches' 0.73 is the logf term on the rows of noise at 1e-4: 1.5 ulp of a result near -16, of the 2 that d allows.)
The launches above 64 KB of dynamic LDS are accepted without an opt-in and give the 8-frame form's bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_reference as FE
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

_CACHE = {}


def _handle(case, normalize="none", bank=None):
    from viet_asr_amd import _lib
    h = _lib.Handle(frontend=FE.description(case, normalize, bank))
    h.finalize()
    if case.own:
        h.set_row_independent(True)
    return h


def _melspec(h, gpu, x, lens):
    from viet_asr_amd import stages
    mel, seq = stages.melspec(h, torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu))
    torch.cuda.synchronize()
    return mel.cpu(), seq.cpu()


def _raw(case, gpu):
    """The raw log-mel of a case on the device, computed once (read only afterwards) -> (x, lens, mel, seq, handle)."""
    if case.name not in _CACHE:
        x, lens = FE.inputs(case)
        h = _handle(case)
        mel, seq = _melspec(h, gpu, x, lens)
        _CACHE[case.name] = (x, lens, mel, seq, h)
    return _CACHE[case.name]


@pytest.mark.parametrize("case", FE.CASES, ids=repr)
def test_raw_logmel_against_float64(gpu, case):
    x, lens, mel, seq, h = _raw(case, gpu)
    assert case.form == FE.form(case.B, h.mel_frames(case.L)) and tuple(mel.shape) == (case.B, FE.NMELS, case.T)
    ref = FE.case_chain(case, x, lens)
    assert seq.dtype == torch.int64 and np.array_equal(seq.numpy(), ref["seq"])
    got = mel.numpy()
    t = np.arange(case.T)[None, :]
    masked = np.broadcast_to((t >= ref["seq"][:, None])[:, None, :], got.shape)
    assert (got[masked] == 0).all() and not np.signbit(got[masked]).any()
    worst, big, fails = FE.judge(got, ref["raw"], ref["bound"], ref["judged"])
    at = FE.worst_element(got, ref["raw"], ref["bound"], ref["judged"])
    print(f"{case}: form {case.form}, LDS {FE.lds_bytes(case.form, case.hop)} bytes, worst |y - ref| / bound {worst:.4f} at "
          f"(row, bin, frame) {at}, largest bound {big:.3e}")
    _record("frontend_f64", case=case.name, form=case.form, lds=FE.lds_bytes(case.form, case.hop), ratio=worst, bound=big,
            at=list(at))
    assert not fails, fails
    # exact values where the arithmetic leaves no room: no power at all under the add guard, and under the clamp at tiny
    if case.signal == "mix":
        zero = [k for k, _ in FE.MIX_ROWS].index("zero")
        n = int(ref["seq"][zero])
        want = np.float32(np.log(np.float64(np.float32(case.guard))))
        assert n > 0 and np.abs(got[zero, :, :n] - want).max() <= FE.D_LOG * FE.U * abs(float(want))
    again, seq2 = _melspec(h, gpu, x, lens)
    assert torch.equal(again.view(torch.int32), mel.view(torch.int32)) and torch.equal(seq2, seq)     # two calls, the same bits
    # the first rows alone take the 8-frame form: a frame's arithmetic does not depend on the block it is in
    if case.form == 32:
        n = min(3, case.B - 1)
        assert FE.form(n, case.T) == 8
        few, _ = _melspec(h, gpu, x[:n], lens[:n])
        same = torch.equal(few.view(torch.int32), mel[:n].view(torch.int32))
        _record("frontend_bits", case=case.name, what=f"rows 0..{n - 1} alone in the 8-frame form", same=same)
        assert same
    # row-independent mode: a row is the batch of one on its own samples
    if case.own:
        for b in np.flatnonzero(lens > FE.NFFT // 2):
            one, s1 = _melspec(h, gpu, x[b:b + 1, :lens[b]], lens[b:b + 1])
            n = int(ref["seq"][b])
            assert int(s1[0]) == n and torch.equal(one[0, :, :n].view(torch.int32), mel[b, :, :n].view(torch.int32)), int(b)


@pytest.mark.parametrize("mode", ("per_feature", "all_features"))
@pytest.mark.parametrize("case", [c for c in FE.CASES if c.norm], ids=repr)
def test_normalisation_alone_against_float64(gpu, case, mode):
    """A second handle that differs only in `normalize`, judged against the float64 normalisation of the first handle's raw
    output: the STFT's error is on both sides and does not compound."""
    x, lens, mel, seq, _ = _raw(case, gpu)
    got, seq_n = _melspec(_handle(case, mode), gpu, x, lens)
    assert torch.equal(seq_n, seq)
    got, raw, s = got.numpy(), mel.numpy(), seq.numpy()
    ref, bound = FE.normalize(raw, s, mode)
    worst, big, fails = FE.judge(got, ref, bound)
    print(f"{case} {mode}: worst |y - ref| / bound {worst:.4f}, largest bound {big:.3e}")
    _record("frontend_norm_f64", case=case.name, mode=mode, ratio=worst, bound=big)
    assert not fails, fails
    t = np.arange(case.T)[None, :]
    assert (got[np.broadcast_to((t >= s[:, None])[:, None, :], got.shape)] == 0).all()
    seen = set()
    for b in range(case.B):
        n, v = int(s[b]), raw[b, :, :int(s[b])]
        if n == 0:
            assert (got[b] == 0).all()                                   # no valid frame: exactly 0 everywhere
            seen.add("none")
        elif n == 1 and mode == "per_feature":
            assert np.isnan(got[b, :, 0]).all() and (got[b, :, 1:] == 0).all()     # NaN in exactly the valid frame of every bin
            seen.add("one")
        elif (np.ptp(v, axis=1) == 0).all() if mode == "per_feature" else np.ptp(v) == 0:
            assert (got[b] == 0).all()                                   # a constant row: the double sums give its mean exactly
            seen.add("constant")
        else:
            assert np.isfinite(got[b]).all()
    if case.signal != "white":
        assert seen >= ({"none", "constant"} | ({"one"} if mode == "per_feature" else set())), seen
    if mode == "all_features":
        # a short row's statistics exclude its padding: over the padded width they would be far outside the bound
        bad, _ = FE.normalize(raw, s, mode, defect="all_padded")
        short = [b for b in range(case.B) if 1 <= s[b] < case.T and np.ptp(raw[b, :, :s[b]]) > 0]
        assert short and all(np.nanmax(np.abs(bad[b] - got[b]) / np.maximum(bound[b], 1e-300)) > 100 for b in short)


@pytest.mark.parametrize("a,b", FE.PAIRS)
def test_common_rows_bit_equal_across_forms_and_batches(gpu, a, b):
    ca, cb = FE.BY_NAME[a], FE.BY_NAME[b]
    ma, mb = _raw(ca, gpu)[2], _raw(cb, gpu)[2]
    n = min(ca.B, cb.B)
    same = torch.equal(ma[:n].view(torch.int32), mb[:n].view(torch.int32))
    _record("frontend_bits", case=f"{a} / {b}", what=f"forms {ca.form} / {cb.form}, rows 0..{n - 1}", same=same)
    assert same, (a, b)


def test_filter_of_33_bins_is_refused(gpu):
    from viet_asr_amd import _lib
    case = FE.BY_NAME["bank_boxcar"]
    h = _lib.Handle(frontend=FE.description(case, bank="boxcar33"))
    with pytest.raises(NotImplementedError, match="spans 33 bins"):         # VASR_ERR_UNSUPPORTED
        h.finalize()


@pytest.mark.parametrize("name", ("form_b", "form_e"))
def test_direct_call_writes_its_outputs_and_nothing_else(gpu, name):
    """vasr_melspec_f32 with d_mel and d_seq inside larger pattern-filled tensors (T = 14 and T = 134, the 8- and the
    32-frame form): every element of [B, 64, T] and of seq written, the guard regions untouched."""
    from viet_asr_amd import _lib
    case = FE.BY_NAME[name]
    x, lens, mel, seq, h = _raw(case, gpu)
    G, PAT, IPAT = 1003, -12345.678, -7777
    n = case.B * FE.NMELS * case.T
    big = torch.full((n + 2 * G,), PAT, dtype=torch.float32, device=gpu)
    sbig = torch.full((case.B + 2 * 5,), IPAT, dtype=torch.int64, device=gpu)
    xd, ld = torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu)
    _lib.check(_lib.lib().vasr_melspec_f32(h.h, xd.data_ptr(), ld.data_ptr(), case.B, case.L, big.data_ptr() + 4 * G,
                                           sbig.data_ptr() + 8 * 5, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    big, sbig = big.cpu(), sbig.cpu()
    pat = torch.tensor(PAT, dtype=torch.float32)
    assert (big[:G] == pat).all() and (big[G + n:] == pat).all() and (sbig[:5] == IPAT).all() and (sbig[-5:] == IPAT).all()
    assert torch.equal(big[G:G + n].view(torch.int32), mel.reshape(-1).view(torch.int32)) and not (big[G:G + n] == pat).any()
    assert torch.equal(sbig[5:-5], seq)
