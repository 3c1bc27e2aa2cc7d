"""-m gpu: the 16-wavefront form of the fused depthwise + pointwise kernel's 128-frame tile (csrc/encoder_fused.hip, template
parameter NW) against its 8-wavefront form and against float64, at the cases of tests/fused16_child.py: one 256-channel block
of two sub-layers, K = 33 / 39, with and without the folded residual, batch 3 x 200 frames (two tiles a row), lengths
200 / 129 / 37, NaN past every row's length.

Two child processes on the devtools build (VASR_FUSED_MIN_TILES=1, VASR_FUSED_TILE=128; VASR_FUSED_WAVES=8 and 16) run every
case once; the tests share their arrays.  Both forms give an accumulator the same products in the same order and a depthwise
output the same FMA chain, so the encoder outputs -- what the trailing GEMM makes of the block's output AND of the maxima it
published, on 4 slots a tile in one form and 8 in the other -- must be equal bit for bit, under ReLU, hardtanh and SELU.  The
16-wavefront outputs are then held to the elementwise float64 bound of tests/sep_reference.py, every stored element judged.

Seen on an MI355X: all six comparisons bit-equal; worst |y - ref| / bound 1e-4 (k33, k39, k39_res) and 2e-4 (k33_res); the
module takes 13 s, almost all of it the two child processes.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fused16_child as F16
import sep_reference as SEP

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RELU = sorted(F16.CASES)
ACTS = ["k33_res:hardtanh", "k39_res:selu"]


@pytest.fixture(scope="module")
def outs(gpu, tmp_path_factory):
    """{waves: arrays of every case} -- one child process per VASR_FUSED_WAVES value."""
    from viet_asr_amd import _lib
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    tmp = tmp_path_factory.mktemp("fused16")
    got = {}
    for waves in ("8", "16"):
        path = str(tmp / f"waves{waves}.npz")
        env = {**os.environ, "VASR_LIB_PATH": dev, "VASR_FUSED_MIN_TILES": "1", "VASR_FUSED_TILE": "128", "VASR_FUSED_WAVES": waves}
        p = subprocess.run([sys.executable, os.path.join(HERE, "fused16_child.py"), path] + RELU + ACTS, env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "FUSED16_CHILD_OK" in p.stdout, (waves, p.stdout[-2000:], p.stderr[-2000:])
        got[waves] = dict(np.load(path))
    return got


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _both_fused(outs, item):
    for waves in ("8", "16"):       # both sub-layers of the block took the fused kernel, nothing took the depthwise kernels
        assert outs[waves][f"{item}/counts"].tolist()[:2] == [2, 0], (item, waves, outs[waves][f"{item}/counts"])


@pytest.mark.parametrize("name", RELU)
def test_16_wavefronts_give_the_bits_of_8(outs, name):
    _both_fused(outs, name)
    y8, y16 = outs["8"][f"{name}/y"], outs["16"][f"{name}/y"]
    assert y16.shape == (F16.B, 256, F16.T) and np.isfinite(y16).all()
    assert _same_bits(y8, y16), (name, int((y8.view(np.uint32) != y16.view(np.uint32)).sum()))
    assert torch.equal(torch.from_numpy(y8), torch.from_numpy(y16))
    assert np.array_equal(outs["8"][f"{name}/lens"], outs["16"][f"{name}/lens"])


@pytest.mark.parametrize("name", RELU)
def test_16_wavefronts_against_float64(outs, name):
    """The judged chain is the block and the identity trailing block on the device's own leading-block output (sep_reference's
    reference and bound, unchanged).  The plan it needs -- which arithmetic every launch ran -- is the restated product choice
    for a device of 7 units, where the rule itself picks 128-frame tiles for these 6 tiles, as the switches force here."""
    _both_fused(outs, name)
    case = F16.CASES[name]
    res = case.blocks[1]["residual"]
    plans = SEP.plan(case, "f16x2", 7)
    assert SEP.form_names(plans[1]) == ["fused128", "fused128+res" if res else "fused128"]
    sd = SEP.weights(case)
    _, lens = F16.inputs(case)
    lead = torch.from_numpy(outs["16"][f"{name}/lead"]).double()
    assert torch.isfinite(lead).all()
    ref, bounds, lens_out = SEP.chain(lead, SEP.lens_chain(lens, case.blocks[:1]), sd, case.blocks[1:], 1, {"f16x2": plans[1:]})
    assert np.array_equal(outs["16"][f"{name}/lens"].astype(np.float32), lens_out.astype(np.float32))
    worst, msg = SEP.judge(torch.from_numpy(outs["16"][f"{name}/y"]), ref, bounds["f16x2"])
    print(f"{name}: worst |y - ref| / bound = {worst:.4f}")
    assert msg is None, (name, msg)


@pytest.mark.parametrize("item", ACTS)
def test_16_wavefronts_give_the_bits_of_8_under_hardtanh_and_selu(outs, item):
    _both_fused(outs, item)
    y8, y16 = outs["8"][f"{item}/y"], outs["16"][f"{item}/y"]
    assert np.isfinite(y16).all()
    assert _same_bits(y8, y16), (item, int((y8.view(np.uint32) != y16.view(np.uint32)).sum()))
    # the activation really is another one: a ReLU output has no negative element
    assert (y16 < 0).any(), item
