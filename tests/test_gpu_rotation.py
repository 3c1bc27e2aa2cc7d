"""-m gpu: the two buffer rotations of run_encoder (csrc/vasr_host.h BufRotation; VASR_BUF_ROTATE=pingpong|inplace) give the
same bits.  They launch the same kernels with the same arguments at other addresses, so the encoder output of the per-module
entry point, the log-probs, the encoded lengths, the predictions and the collapsed ids of the transcribe path must be equal
bit for bit -- unless a launch stored over something another launch still had to read.

Two child processes on the devtools build (tests/rotation_child.py; VASR_FUSED_MIN_TILES=1 and VASR_FUSED_TILE=128, so that the
256-channel sub-blocks take the fused kernel's 128-frame tile at every batch) run every case once; the workspace is filled with
NaN before each call.  Cases: the seven models at batch 6 and batch 3 (the latency GEMM) on ragged clips of 2.0 / 1.3 / 0.6 s
(101 frames: one 128-column tile), row-independent mode, two slices of 8 rows, and 64 x 2 s (the 512 x 128 GEMM tile, the
16-wavefront fused kernel).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rotation_child as RC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("enc", "enc_len_module", "logp", "enc_len", "pred", "ids", "id_len")


@pytest.fixture(scope="module")
def outs(gpu, tmp_path_factory):
    from viet_asr_amd import _lib
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    tmp = tmp_path_factory.mktemp("rotation")
    got = {}
    for mode in ("pingpong", "inplace"):
        path = str(tmp / f"{mode}.npz")
        env = {**os.environ, "VASR_LIB_PATH": dev, "VASR_FUSED_MIN_TILES": "1", "VASR_FUSED_TILE": "128", "VASR_BUF_ROTATE": mode}
        p = subprocess.run([sys.executable, os.path.join(HERE, "rotation_child.py"), "run", path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "ROTATION_CHILD_OK" in p.stdout, (mode, p.stdout[-2000:], p.stderr[-2000:])
        got[mode] = dict(np.load(path))
    return got


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.mark.parametrize("case", sorted(RC.GPU_CASES))
def test_both_rotations_give_the_same_bits(outs, case):
    model, batch, row_independent, _ = RC.GPU_CASES[case]
    for k in KEYS:
        a, b = outs["pingpong"][f"{case}/{k}"], outs["inplace"][f"{case}/{k}"]
        assert a.shape == b.shape and a.dtype == b.dtype, (case, k)
        assert np.array_equal(_bits(a), _bits(b)), (case, k, int((_bits(a) != _bits(b)).sum()))
    enc, logp = outs["inplace"][f"{case}/enc"], outs["inplace"][f"{case}/logp"]
    assert enc.shape == (batch, 512, 101) and logp.shape[:2] == (batch, 101)
    # nothing of the NaN the workspace was filled with reaches a result, and the model is not dead
    assert np.isfinite(enc).all() and np.isfinite(logp).all(), case
    assert float(np.abs(enc).max()) > 0
    lens = outs["inplace"][f"{case}/enc_len"]
    assert lens.shape == (batch,) and (lens > 0).all() and (lens <= 101).all() and len(set(lens[:3].tolist())) == 3, (case, lens)
    assert np.array_equal(lens, outs["inplace"][f"{case}/enc_len_module"])
    assert (outs["inplace"][f"{case}/id_len"] >= 0).all()
