"""CPU checks of tests/dw_reference.py, the float64 restatement and error bound tests/test_gpu_dw.py judges the depthwise
kernels by: the restatement against torch's own float64 conv1d, the length formula against the oracle's MaskedConv1d, the bound
against honest float32 arithmetic (not tighter than that) and against a wrong convolution (far tighter than that)."""
import numpy as np
import pytest
import torch

import dw_reference as DW

TRIPLES = [(33, 1, 1), (11, 2, 1), (29, 1, 2)]          # (K, stride, dilation)
B, C, T = 3, 8, 300


def _case(K, stride, dil):
    lens = DW.ragged(B, T, floor=1)
    x, w = DW.inputs(K, stride, dil, C, B, T, lens)
    lo = DW.lens_out(lens, K, stride, dil)
    return lens, lo, x, w, DW.reference(x, w, lens, lo, T, stride, dil)


def _masked(x, lens):
    """The reference's own words (jasper.py:113-118): x.masked_fill(arange >= lens, 0)."""
    mask = torch.arange(T).expand(B, T) >= torch.tensor(lens).unsqueeze(1)
    return x[:, :, :T].masked_fill(mask.unsqueeze(1), 0)


@pytest.mark.parametrize("K,stride,dil", TRIPLES)
def test_reference_equals_float64_conv1d_on_the_masked_input(K, stride, dil):
    lens, lo, x, w, (ref, bound) = _case(K, stride, dil)
    assert torch.isnan(x[:, :, T:]).all() and not torch.isnan(x[:, :, :T]).any()
    assert float(x[2, :, lens[2]:T].abs().min()) > 0                # garbage past the length, and it is not small
    want = torch.nn.functional.conv1d(_masked(x, lens).double(), w.double()[:, None, :], stride=stride,
                                      padding=DW.same_padding(K, stride, dil), dilation=dil, groups=C)
    assert want.shape == ref.shape == bound.shape == (B, C, DW.out_frames(T, K, stride, dil))
    for b in range(B):
        assert torch.equal(ref[b, :, : lo[b]], want[b, :, : lo[b]])
        assert not ref[b, :, lo[b]:].any()
    assert torch.isfinite(ref).all() and (bound >= DW.TINY).all()


@pytest.mark.parametrize("K,stride,dil", TRIPLES + [(33, 8, 1), (87, 1, 2), (13, 1, 3), (1, 1, 1), (99, 1, 1)])
def test_length_formula_equals_the_oracles_masked_conv(K, stride, dil):
    from oracle import quartznet_oracle as O
    lens = torch.arange(1, 601)
    _, got = O.masked_conv1d(torch.zeros(600, 1, 600), lens, torch.zeros(1, 1, K), stride, O.get_same_padding(K, stride, dil), dil)
    assert got.dtype == torch.float32
    assert np.array_equal(DW.lens_out(lens.numpy(), K, stride, dil), got.to(torch.long).numpy())
    # len_chain.h: float(li + 2 pad - dil (K - 1) - 1) / stride + 1, truncated -- the same integers
    p = DW.same_padding(K, stride, dil)
    chain = [int(np.float32(np.float32(n + 2 * p - dil * (K - 1) - 1) / np.float32(stride)) + np.float32(1)) for n in range(1, 601)]
    assert DW.lens_out(lens.numpy(), K, stride, dil).tolist() == chain
    assert DW.out_frames(600, K, stride, dil) == int(chain[-1])


def test_same_padding_refuses_stride_with_dilation():
    with pytest.raises(ValueError):
        DW.same_padding(33, 2, 2)


@pytest.mark.parametrize("K,stride,dil", TRIPLES)
def test_float32_conv1d_stays_inside_the_bound(K, stride, dil):
    """The bound is not tighter than honest float32 arithmetic: torch's float32 conv1d of the same masked input."""
    lens, lo, x, w, (ref, bound) = _case(K, stride, dil)
    y = torch.nn.functional.conv1d(_masked(x, lens), w[:, None, :], stride=stride, padding=DW.same_padding(K, stride, dil),
                                   dilation=dil, groups=C).double()
    keep = (torch.arange(y.shape[-1])[None, :] < torch.from_numpy(lo).long()[:, None])[:, None, :]
    err = (torch.where(keep, y, torch.zeros((), dtype=torch.float64)) - ref).abs()
    assert (err <= bound).all(), float((err / bound).max())
    assert float((err / bound).max()) > 1e-4                        # ... and float32 really differs from float64 here


@pytest.mark.parametrize("K,stride,dil", TRIPLES)
def test_a_wrong_convolution_breaks_the_bound_a_hundredfold(K, stride, dil):
    """One tap dropped, the taps shifted by one place, or the output one frame late: each leaves the bound by more than 100 x,
    in every row (300 x level included) and in the channel whose taps are a thousand times smaller."""
    lens, lo, x, w, (ref, bound) = _case(K, stride, dil)
    dropped = w.clone()
    dropped[:, K // 2] = 0
    shifted = torch.roll(w, 1, dims=1)
    for wrong_w in (dropped, shifted):
        wrong, _ = DW.reference(x, wrong_w, lens, lo, T, stride, dil)
        ratio = (wrong - ref).abs() / bound
        for b in range(B):
            for ch in (0, 3):
                assert float(ratio[b, ch, : lo[b]].max()) > 100, (b, ch)
    late = torch.roll(ref, 1, dims=2)
    assert float(((late - ref).abs() / bound).max()) > 100
    # an input column past the length consumed (the garbage inputs() puts there)
    leak, _ = DW.reference(x, w, [T] * B, lo, T, stride, dil)
    assert float(((leak - ref).abs() / bound)[2].max()) > 100
