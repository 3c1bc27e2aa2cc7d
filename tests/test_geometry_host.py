"""CPU checks of what the engines' Python layer says once: the conv chain's arithmetic (viet_asr_amd.geometry) and the
zero-pad collate with its refusals (engine.collate, engine.check_lengths).  Nothing here loads the library.

The float length chain is held to the reference's recorded ``enc_len``, the integer frame chain to the output widths torch's
own conv1d gives, step by step; the two are different things (500.0 and 501 for one and the same 10 s row) and the goldens
contain rows on which they differ."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from viet_asr_amd import configs, geometry
from viet_asr_amd.engine import _pcm_to_float, blocks_from_config, check_lengths, collate

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOP = 160
LENGTHS = (257, 319, 320, 321, 16000, 160077)


def _builtin_blocks(name):
    return blocks_from_config(configs.builtin(name)["JasperEncoder"]["jasper"])


def _golden_blocks(name):
    src = json.loads(str(np.load(os.path.join(GOLDEN, name + ".npz"))["definition"]))
    return blocks_from_config(configs.jasper_definition(src)["JasperEncoder"]["jasper"])


def test_float_length_chain_equals_the_recorded_enc_len():
    used, differ = 0, 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        g = np.load(path)
        if not {"seq", "enc_len", "cfg_file"} <= set(g.keys()):
            continue
        try:
            blocks = _builtin_blocks(str(g["cfg_file"]))
        except ValueError:            # (not a built-in config)
            continue
        used += 1
        for b, (seq, want) in enumerate(zip(g["seq"], g["enc_len"])):
            got = np.float32(geometry.encoded_length(blocks, int(seq)))
            assert got == want and got.dtype == want.dtype, (os.path.basename(path), int(seq), got, want)
            if "lens" in g.keys():
                own = int(geometry.frames_of(blocks, HOP, torch.tensor([int(g["lens"][b])]))[0])
                differ += own != want
    assert used >= 11, used
    assert differ > 0                 # a merged chain would pass nowhere: e.g. 160000 samples are 501 frames and 500.0


def test_the_two_chains_differ_on_a_ten_second_row():
    blocks = _builtin_blocks("quartznet15x5")
    assert geometry.encoded_length(blocks, 1000) == 500.0
    assert geometry.frames_of(blocks, HOP, torch.tensor([160000])).tolist() == [501]


def _conv1d_widths(blocks, t):
    """Frames after every sub-block's K-tap conv, from torch's conv1d itself.  The kernel and padding rules are restated here
    (parts/jasper.py:52-65): an even kernel grows by one; padding (dilation * K) // 2 - 1 when dilated, K // 2 otherwise."""
    for b in blocks:
        k = b["kernel"] if b["kernel"] % 2 else b["kernel"] + 1
        pad = (b["dilation"] * k) // 2 - 1 if b["dilation"] > 1 else k // 2
        for _ in range(b["repeat"]):
            t = torch.nn.functional.conv1d(torch.zeros(1, 1, t), torch.zeros(1, 1, k), stride=b["stride"], padding=pad,
                                           dilation=b["dilation"]).shape[-1]
    return t


@pytest.mark.parametrize("model", ["quartznet12x1_vi", "quartznet15x5", "jasper_k11_s2_b3", "jasper_k29_d2_b3"])
def test_integer_frame_chain_equals_conv1d_output_widths(model):
    blocks = _golden_blocks(model) if model.startswith("jasper_") else _builtin_blocks(model)
    if model == "jasper_k11_s2_b3":
        assert any(b["stride"] == 2 for b in blocks)
    if model == "jasper_k29_d2_b3":
        assert any(b["dilation"] == 2 for b in blocks)
    got = geometry.frames_of(blocks, HOP, torch.tensor(LENGTHS, dtype=torch.int64))
    assert got.dtype == torch.int32
    assert got.tolist() == [_conv1d_widths(blocks, 1 + n // HOP) for n in LENGTHS]


def test_stride_product_and_halo():
    vi = _builtin_blocks("quartznet12x1_vi")
    assert geometry.stride_product(vi) == 2
    assert geometry.halo_mel_frames(vi) == 636                                   # tests/test_gpu_parity.py, forward_long
    dr3 = _golden_blocks("jasper_dr3_from_mel_b3")
    assert geometry.halo_mel_frames(dr3) == 36                                   # tests/test_gpu_jasper.py, forward_long
    assert geometry.stride_product(_golden_blocks("jasper_k11_s2_b3")) == 2
    with pytest.raises(NotImplementedError):
        geometry.halo_mel_frames([dict(vi[0], repeat=2)])                        # a strided block with repeat > 1
    assert [geometry.odd_kernel(k) for k in (1, 2, 11, 32, 33)] == [1, 3, 11, 33, 33]


# ---- collate ------------------------------------------------------------------------------------------------------------------

def _rows():
    rng = np.random.default_rng(3)
    return [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (700, 300, 513, 1)]


def _pcm_rows():
    rng = np.random.default_rng(4)
    return [rng.integers(-2 ** 15, 2 ** 15, size=n).astype(np.int16) for n in (700, 300, 513, 1)]


def test_collate_pads_float_rows_with_zeros():
    rows = _rows()
    batch, lens = collate(rows)
    assert batch.dtype == np.float32 and batch.shape == (4, 700) and lens == [700, 300, 513, 1]
    for b, s in enumerate(rows):
        assert np.array_equal(batch[b, : len(s)], s) and not batch[b, len(s):].any()


def test_collate_keeps_an_all_int16_batch_only_when_asked():
    rows = _pcm_rows()
    kept, lens = collate(rows, keep_int16=True)
    assert kept.dtype == np.int16 and lens == [700, 300, 513, 1]
    scaled, _ = collate(rows)
    assert scaled.dtype == np.float32
    for b, s in enumerate(rows):
        assert np.array_equal(kept[b, : len(s)], s) and not kept[b, len(s):].any()
        assert np.array_equal(scaled[b, : len(s)], s.astype(np.float32) * np.float32(2.0 ** -15)) and not scaled[b, len(s):].any()


def test_collate_scales_the_integer_rows_of_a_mixed_batch():
    rows = [_rows()[0], _pcm_rows()[1], _rows()[2], _pcm_rows()[3].astype(np.int32) * 2 ** 16]
    batch, lens = collate(rows, keep_int16=True)
    assert batch.dtype == np.float32 and lens == [700, 300, 513, 1]
    for b, s in enumerate(rows):
        want = _pcm_to_float(s)
        assert want.dtype == np.float32
        assert np.array_equal(batch[b, : len(s)], want) and not batch[b, len(s):].any()
    assert np.array_equal(batch[1, :300], rows[1].astype(np.float32) * np.float32(2.0 ** -15))
    assert np.array_equal(batch[3, :1], rows[3].astype(np.float32) * np.float32(2.0 ** -31))


@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_collate_overwrites_a_dirty_buffer(dtype):
    rows = _rows() if dtype == np.float32 else _pcm_rows()
    out = np.full((4, 700), 77, dtype=dtype)
    batch, lens = collate(rows, out=out)
    assert batch is out and lens == [700, 300, 513, 1]
    fresh, _ = collate(rows, keep_int16=True)
    assert fresh.dtype == dtype and np.array_equal(out, fresh)


def test_the_three_refusals():
    rows = _rows()
    n_fft = 512
    with pytest.raises(ValueError, match="empty batch"):
        collate([], n_fft)
    with pytest.raises(ValueError, match="empty signal"):
        collate(rows + [np.zeros(0, dtype=np.float32)], n_fft)
    text = "row-independent batching needs more than n_fft/2 = 256 samples per signal (got 1): an unbatched call refuses such input too"
    for call in (lambda: collate(rows, n_fft, True), lambda: collate(rows, n_fft, row_independent=True, keep_int16=True),
                 lambda: check_lengths([len(s) for s in rows], n_fft, True)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    with pytest.raises(ValueError, match="got 256"):
        check_lengths([700, 256], n_fft, True)
    check_lengths([700, 257], n_fft, True)
    collate(rows, n_fft)                     # a short row is refused under row_independent only
    collate(rows)                            # and nothing is refused where no front end is named
