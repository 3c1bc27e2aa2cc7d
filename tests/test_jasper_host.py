"""CPU-side checks of the Jasper layouts: non-separable K-tap convolutions and dense residuals (JasperEncoder's
residual_dense).  Configuration parsing, the reference's state_dict layout, the layouts the reference cannot run, the
implicit GEMM's weight order and ABI 8."""
import json
import os
import re

import numpy as np
import pytest

from viet_asr_amd import _lib, configs, synth
from viet_asr_amd.engine import blocks_from_config

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _blk(filters, kernel=11, repeat=1, stride=1, dilation=1, residual=True, dense=False):
    d = dict(filters=filters, repeat=repeat, kernel=[kernel], stride=[stride], dilation=[dilation], dropout=0.0,
             residual=residual)
    if dense:
        d["residual_dense"] = True
    return d


def test_jasper10x5dr_block_list_is_accepted():
    cfg = configs.builtin("jasper10x5dr")
    blocks = blocks_from_config(cfg["JasperEncoder"]["jasper"])
    assert len(blocks) == 13
    assert blocks[0] == dict(filters=256, repeat=1, kernel=11, stride=2, dilation=1, residual=0, separable=0, residual_dense=0)
    assert [b["filters"] for b in blocks[1:11]] == [256, 256, 384, 384, 512, 512, 640, 640, 768, 768]
    assert [b["kernel"] for b in blocks[1:11]] == [11, 11, 13, 13, 17, 17, 21, 21, 25, 25]
    assert all(b["residual_dense"] == 1 and b["residual"] == 1 and b["repeat"] == 5 for b in blocks[1:11])
    assert blocks[11]["kernel"] == 29 and blocks[11]["dilation"] == 2 and blocks[12]["kernel"] == 1
    assert cfg["labels"] == configs.LABELS_EN


def test_module_state_dict_equals_the_reference_layout():
    """asr.JasperEncoder(jasper10x5dr) has the keys and shapes of the reference's own module (fixture written by
    tests/golden/make_golden_jasper.py from nemo.collections.asr.JasperEncoder); synth generates exactly those."""
    from viet_asr_amd import asr
    with open(os.path.join(HERE, "golden", "jasper10x5dr_state_dict_keys.json"), encoding="utf-8") as f:
        want = json.load(f)
    cfg = configs.builtin("jasper10x5dr")
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    have = {k: list(v.shape) for k, v in enc.state_dict().items()}
    assert have == want
    assert "encoder.10.res.9.0.conv.weight" in have and have["encoder.10.res.9.0.conv.weight"] == [768, 768, 1]
    assert have["encoder.10.res.0.0.conv.weight"] == [768, 256, 1]     # pane 0: the prologue's output
    jas = cfg["JasperEncoder"]["jasper"]
    sd = synth.encoder_state_dict(jas[:3], 64, 0)        # the first dense blocks: same key set as the module's prefix
    assert {k: list(np.shape(v)) for k, v in sd.items()} == {k: v for k, v in want.items() if k.split(".")[1] in ("0", "1", "2")}


def test_synthetic_streams_of_quartznet_layouts_are_unchanged():
    """The Jasper gains apply to keys the QuartzNet layouts never have: their weights (and so every existing golden) stay."""
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    sd = synth.encoder_state_dict(jas, 64, 3)
    w = synth._conv_weight("encoder.17.mconv.0.conv.weight", 3, 1024, 512, 1, gain=synth.G_MAIN)
    assert np.array_equal(sd["encoder.17.mconv.0.conv.weight"], w)
    w = synth._conv_weight("encoder.1.res.0.0.conv.weight", 3, 256, 256, 1, gain=synth.G_RES)
    assert np.array_equal(sd["encoder.1.res.0.0.conv.weight"], w)


@pytest.mark.parametrize("layout, what", [
    ([_blk(256, dense=True), _blk(256, residual=True), _blk(256, dense=True)], "contiguous"),     # a break in the run
    ([_blk(256, dense=True, residual=False), _blk(256, dense=True)], "contiguous"),               # dense without residual
    ([_blk(256, dense=True), _blk(256, stride=2, dense=True)], "strided"),
])
def test_layouts_the_reference_cannot_run_raise_at_construction(layout, what):
    from viet_asr_amd import asr
    with pytest.raises(ValueError, match=what):
        blocks_from_config(layout)
    with pytest.raises(ValueError, match=what):
        asr.JasperEncoder(jasper=layout, activation="relu", feat_in=64)


def test_layouts_the_reference_runs_are_accepted():
    from viet_asr_amd import asr
    ok = [[_blk(256, dense=True), _blk(256, dense=True), _blk(384, dense=True, residual=False)],   # last one without residual
          [_blk(256, dense=True, residual=False), _blk(256, residual=False)],
          [_blk(256, residual=False, stride=2), _blk(256, dense=True), _blk(256, dense=True)]]
    for layout in ok:
        blocks_from_config(layout)
        enc = asr.JasperEncoder(jasper=layout, activation="relu", feat_in=64)
        assert set(enc.state_dict()) == set(synth.encoder_state_dict(layout, 64, 0))
    enc = asr.JasperEncoder(jasper=ok[0], activation="relu", feat_in=64)
    assert enc.state_dict()["encoder.1.res.1.0.conv.weight"].shape == (256, 256, 1)
    assert "encoder.2.res.0.0.conv.weight" not in enc.state_dict()


def test_residual_block_after_a_dense_run_takes_the_runs_input():
    """A residual block that is not dense right after a dense run receives the run's pane list and takes its residual from
    xs[0] (parts/jasper.py:428-436): accepted when that pane has the block's input width (the reference runs it; GPU fixture
    jasper_dense_then_plain_b3), refused where the reference's 1x1 conv cannot take it."""
    from viet_asr_amd import asr
    ok = [_blk(256, residual=False), _blk(256, dense=True), _blk(256, dense=True), _blk(256)]
    blocks_from_config(ok)
    asr.JasperEncoder(jasper=ok, activation="relu", feat_in=64)
    desc = lambda l: [dict(filters=b["filters"], repeat=b["repeat"], kernel=b["kernel"][0], stride=b["stride"][0],
                           dilation=b["dilation"][0], residual=int(b["residual"]), separable=0,
                           residual_dense=int(b.get("residual_dense", False))) for b in l]     # (no Python-side check)
    _lib.Handle(feat_in=64, blocks=desc(ok)).close()
    for bad in ([_blk(384, residual=False), _blk(256, dense=True), _blk(256, dense=True), _blk(256)],    # run input 384 != 256
                [_blk(256, residual=False), _blk(256, dense=True), _blk(256, dense=True), _blk(256, stride=2)]):
        with pytest.raises(ValueError, match="run's input"):
            asr.JasperEncoder(jasper=bad, activation="relu", feat_in=64)
        with pytest.raises(ValueError, match="run's input"):
            _lib.Handle(feat_in=64, blocks=desc(bad))
    # the run starting at block 0: pane 0 is the encoder input (64 channels here, 256 needed)
    with pytest.raises(ValueError, match="run's input"):
        asr.JasperEncoder(jasper=[_blk(256, dense=True), _blk(256, dense=True), _blk(256)], activation="relu", feat_in=64)


def test_library_refuses_the_same_layouts():
    """vasr_create makes the same decision for callers of the C ABI (no weights needed: it fails before them)."""
    bad = [dict(filters=256, repeat=1, kernel=11, stride=1, dilation=1, residual=1, separable=0, residual_dense=1),
           dict(filters=256, repeat=1, kernel=11, stride=1, dilation=1, residual=1, separable=0, residual_dense=0),
           dict(filters=256, repeat=1, kernel=11, stride=1, dilation=1, residual=1, separable=0, residual_dense=1)]
    with pytest.raises(ValueError, match="contiguous"):
        _lib.Handle(feat_in=256, blocks=bad)      # (256: block 1 may take its residual from the encoder input)
    strided = [dict(filters=256, repeat=1, kernel=11, stride=2, dilation=1, residual=1, separable=0, residual_dense=1)]
    with pytest.raises(ValueError, match="strided"):
        _lib.Handle(feat_in=64, blocks=strided)


def test_conv_weight_packing_layout():
    """A K-tap conv's [cout][cin][K] weights become the implicit GEMM's [cout][K * cin] with the input channel inner (k = tap *
    cin + c), which the pointwise packers then put in fragment order."""
    L = _lib.dev_lib()
    cout, cin, K = 5, 64, 3
    w = np.arange(cout * cin * K, dtype=np.float32).reshape(cout, cin, K)
    g = np.empty((cout, K * cin), dtype=np.float32)
    _lib.check(L.vasr_conv_gemm_weights(w.ctypes.data, cout, cin, K, g.ctypes.data), L)
    for m, tap, c in [(0, 0, 0), (1, 2, 5), (4, 1, 63), (3, 0, 17)]:
        assert g[m, tap * cin + c] == w[m, c, tap]
    assert np.array_equal(g, w.transpose(0, 2, 1).reshape(cout, K * cin))
    with pytest.raises(ValueError):
        _lib.check(L.vasr_conv_gemm_weights(w.ctypes.data, cout, cin, 0, g.ctypes.data), L)


def test_abi_8_is_consistent():
    hdr = open(os.path.join(ROOT, "include", "vasr.h"), encoding="utf-8").read()
    assert int(re.search(r"#define VASR_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.lib().vasr_abi_version() == 8
    body = re.search(r"typedef struct \{(.*?)\} vasr_block_desc;", hdr, re.S).group(1)
    fields = re.findall(r"int32_t (\w+);", body)
    assert fields == [f for f, _ in _lib.BlockDesc._fields_]
    assert fields[-1] == "residual_dense"


JASPER_FIXTURES = ("jasper_10x5dr_b2_ragged", "jasper_dr3_from_mel_b3", "jasper_k11_s2_b3", "jasper_k29_d2_b3",
                   "jasper_dense_then_plain_b3")


@pytest.mark.parametrize("name", JASPER_FIXTURES)
def test_oracle_runs_dense_residuals_like_the_reference(name):
    """oracle.encoder_forward + decoder_forward on the reference's own mel features reproduce what the imported reference
    computed (tests/golden/make_golden_jasper.py): float32 log-probs to float32 round-off, its greedy predictions and
    encoded lengths, and in float64 its argmax and top-2 margins.  Three fixtures carry dense residuals (a run after a
    strided prologue, a run that starts at the mel input, a plain residual block after a run): this pins the oracle's pane
    list, which the GPU tests of the Jasper layouts then use as their reference at shapes no fixture has."""
    import torch
    from oracle import quartznet_oracle as O
    g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
    src = json.loads(str(g["definition"]))
    cfg = configs.builtin(src) if isinstance(src, str) else configs.jasper_definition(src)
    jas = cfg["JasperEncoder"]["jasper"]
    seed = int(g["seed"])
    enc_sd = synth.encoder_state_dict(jas, 64, seed)
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, seed)
    seq = torch.from_numpy(np.ceil(g["lens"] / 160).astype(np.int64))     # get_seq_len (features.py:238-239)
    enc, enc_len = O.encoder_forward(g["mel"], seq, enc_sd, jas)
    logp = O.decoder_forward(enc, dec_sd).numpy()
    assert logp.shape == g["logp"].shape
    # (the same ATen CPU calls in the same order: measured bit-identical; the bound leaves room for another BLAS)
    assert np.abs(logp - g["logp"]).max() <= 2e-6 * np.abs(g["logp"]).max()
    assert np.array_equal(logp.argmax(-1), g["pred"])
    assert np.array_equal(enc_len.numpy().astype(np.float32), g["enc_len"].astype(np.float32))
    enc64, _ = O.encoder_forward(g["mel"], seq, enc_sd, jas, dtype=torch.float64)
    logp64 = O.decoder_forward(enc64, dec_sd)
    assert np.array_equal(logp64.argmax(-1).numpy(), g["pred64"])
    top2 = torch.topk(logp64, 2, dim=-1).values
    assert np.abs((top2[..., 0] - top2[..., 1]).numpy() - g["margin64"]).max() <= 1e-9


def test_oracle_dense_pane_list():
    """The pane list on a small layout, checked term by term: a dense block's residual sums one BN(1x1 conv) per pane it
    receives, and the plain residual block after the run takes pane 0 (the run's input)."""
    import torch
    import torch.nn.functional as F
    from oracle import quartznet_oracle as O
    jas = [_blk(64, kernel=3, residual=False), _blk(64, kernel=3, dense=True), _blk(64, kernel=5, dense=True),
           _blk(64, kernel=3)]
    sd = synth.encoder_state_dict(jas, 64, 5)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 64, 40)).astype(np.float64))
    lens = torch.tensor([40, 23])
    want, _ = O.encoder_forward(x, lens, sd, jas, dtype=torch.float64)

    def conv_bn(i, j, inp, k):        # block i's mconv.j conv (K taps, same padding) + BN, masked input
        mask = (torch.arange(inp.shape[2]) < lens[:, None])[:, None, :]
        w = torch.from_numpy(np.asarray(sd[f"encoder.{i}.mconv.{j}.conv.weight"])).double()
        y = F.conv1d(inp * mask, w, padding=k // 2)
        return O._bn_eval(y, sd, f"encoder.{i}.mconv.{j + 1}")

    def res(i, q, inp):
        mask = (torch.arange(inp.shape[2]) < lens[:, None])[:, None, :]
        w = torch.from_numpy(np.asarray(sd[f"encoder.{i}.res.{q}.0.conv.weight"])).double()
        return O._bn_eval(F.conv1d(inp * mask, w), sd, f"encoder.{i}.res.{q}.1")

    p0 = F.relu(conv_bn(0, 0, x, 3))
    p1 = F.relu(conv_bn(1, 0, p0, 3) + res(1, 0, p0))
    p2 = F.relu(conv_bn(2, 0, p1, 5) + res(2, 0, p0) + res(2, 1, p1))
    y = F.relu(conv_bn(3, 0, p2, 3) + res(3, 0, p0))
    assert "encoder.3.res.1.0.conv.weight" not in sd
    assert torch.allclose(want, y, rtol=0, atol=1e-12)
