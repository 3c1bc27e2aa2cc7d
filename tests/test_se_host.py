"""CPU checks of squeeze-and-excitation JasperBlocks (se / se_reduction_ratio): config parsing, the state_dict layout against the
reference's own (tests/golden/se_*_state_dict_keys.json, written by make_golden_se.py), vasr_set_block_se / vasr_finalize
refusals, forward_long's refusal, and a float64 restatement of the SE encoder checked against the reference's fixtures."""
import copy
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("se_15x5_rows3", "se_dense_rows3", "se_nores_k11s2_rows3")


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def _jas(name):
    return json.loads(str(_golden(name)["definition"]))


def test_blocks_from_config_output_is_unchanged_and_se_is_read_separately():
    from viet_asr_amd import configs, engine
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    plain = engine.blocks_from_config(jas)
    se = copy.deepcopy(jas)
    for i, b in enumerate(se):
        b["se"] = True
        if i == 2:
            b["se_reduction_ratio"] = 48
    assert engine.blocks_from_config(se) == plain
    assert engine.se_from_config(jas) == [0] * len(jas)
    assert engine.se_from_config(se) == [48 if i == 2 else 16 for i in range(len(jas))]
    assert engine.se_from_config([dict(jas[0], se=False, se_reduction_ratio=4)]) == [0]
    with pytest.raises(ValueError):
        engine.se_from_config([dict(jas[0], se=True, se_reduction_ratio=0)])
    with pytest.raises(ValueError):   # 256 // 512 == 0: the reference would build a zero-width Linear
        engine.se_from_config([dict(jas[0], se=True, se_reduction_ratio=512)])
    d = configs.jasper_definition(se)
    assert [b.get("se") for b in d["JasperEncoder"]["jasper"]] == [True] * len(jas)
    assert d["JasperEncoder"]["jasper"][2]["se_reduction_ratio"] == 48


@pytest.mark.parametrize("name", ["se_dense", "se_nores_k11s2"])
def test_state_dict_keys_equal_the_reference_layout(name):
    from viet_asr_amd import asr, configs, synth
    want = json.load(open(os.path.join(HERE, "golden", name + "_state_dict_keys.json"), encoding="utf-8"))
    jas = _jas(name + "_rows3")
    enc = asr.JasperEncoder(feat_in=64, **configs.jasper_definition(jas)["JasperEncoder"])
    got = {k: list(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    sd = synth.encoder_state_dict(jas, 64, 1)
    assert {k: list(np.shape(v)) for k, v in sd.items()} == want


def test_synthetic_weights_without_se_are_unchanged():
    """SE weights come from their own streams: a model's non-SE tensors do not move when SE is switched on (where the
    keys are the same, i.e. residual blocks), and a model without SE gets exactly the tensors it got before."""
    from viet_asr_amd import configs, synth
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    plain = synth.encoder_state_dict(jas, 64, 7)
    with_se = synth.encoder_state_dict([dict(b, se=True) for b in jas], 64, 7)
    assert not any(".fc." in k for k in plain)
    for i, b in enumerate(jas):
        if b["residual"]:
            for k in plain:
                if k.startswith(f"encoder.{i}."):
                    assert np.array_equal(plain[k], with_se[k]), k
    assert with_se["encoder.1.res.0.2.fc.0.weight"].shape == (16, 256)
    assert with_se["encoder.0.mconv.3.fc.2.weight"].shape == (256, 16)


def _handle(blocks, se):
    from viet_asr_amd import _lib
    return _lib.Handle(feat_in=64, blocks=blocks, se=se)


def test_set_block_se_and_finalize_refusals():
    from viet_asr_amd import _lib, engine
    jas = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                se=True, se_reduction_ratio=8)]
    blocks = engine.blocks_from_config(jas)
    L = _lib.lib()
    h = _handle(blocks, None)
    assert L.vasr_set_block_se(h.h, 1, 8) == -1            # no such block
    assert L.vasr_set_block_se(h.h, -1, 8) == -1
    assert L.vasr_set_block_se(h.h, 0, -2) == -1
    assert L.vasr_set_block_se(h.h, 0, 512) == 0
    with pytest.raises(ValueError):                          # VASR_ERR_INVALID: 256 // 512 == 0
        h.finalize()
    assert "hidden" in L.vasr_last_error().decode()
    h.close()
    # SE weights missing: VASR_ERR_STATE, before anything touches a device
    from viet_asr_amd import synth
    sd = synth.encoder_state_dict(jas, 64, 3)
    h = _handle(blocks, [8])
    h.load_state_dict({k: v for k, v in sd.items() if ".fc.2." not in k})
    with pytest.raises(_lib.VasrError) as e:
        h.finalize()
    assert "encoder.0.res.0.2.fc.2.weight" in str(e.value)
    assert L.vasr_finalize(h.h) == -2
    h.close()
    # wrong shape: VASR_ERR_INVALID
    h = _handle(blocks, [8])
    sd2 = dict(sd)
    sd2["encoder.0.res.0.2.fc.0.weight"] = np.zeros((16, 256), dtype=np.float32)
    h.load_state_dict(sd2)
    assert L.vasr_finalize(h.h) == -1
    h.close()
    # the SE keys are expected exactly where the reference puts them: a non-residual block's mconv entries shift
    jas_nr = [dict(jas[0], residual=False)]
    sd_nr = synth.encoder_state_dict(jas_nr, 64, 3)
    assert "encoder.0.mconv.5.fc.0.weight" in sd_nr and "encoder.0.mconv.9.fc.0.weight" in sd_nr
    assert "encoder.0.mconv.6.conv.weight" in sd_nr and "encoder.0.mconv.8.running_var" in sd_nr


def test_forward_long_refuses_se_models():
    from viet_asr_amd.engine import QuartzNetCTC
    with pytest.raises(NotImplementedError, match="squeeze-and-excitation"):
        QuartzNetCTC.forward_long(types.SimpleNamespace(_se=[0, 16]), torch.zeros(16000))


# ---- float64 restatement of the SE encoder (parts/jasper.py:113-132, :152-168, :214-288, :408-448) -----------------------

def _masked_conv(x, lens, w, stride, dil, groups):
    k = w.shape[-1]
    pad = (dil * k) // 2 - 1 if dil > 1 else k // 2
    t = torch.arange(x.shape[2])
    x = x.masked_fill(t[None, None, :] >= lens[:, None, None], 0.0)
    y = F.conv1d(x, w, stride=stride, padding=pad, dilation=dil, groups=groups)
    lens = ((lens.double() + 2 * pad - dil * (k - 1) - 1) / stride + 1).long()
    return y, lens


def _bn(x, sd, p):
    g, b, m, v = (torch.as_tensor(sd[f"{p}.{n}"]).double() for n in ("weight", "bias", "running_mean", "running_var"))
    return (x - m[:, None]) / torch.sqrt(v[:, None] + 1e-3) * g[:, None] + b[:, None]


def _se(x, sd, p):
    """SqueezeExcite; the mean is over the whole width, which is the row's length in these batch-1 fixtures."""
    y = x.mean(dim=2)
    y = torch.sigmoid(F.linear(torch.relu(F.linear(y, torch.as_tensor(sd[f"{p}.fc.0.weight"]).double())),
                               torch.as_tensor(sd[f"{p}.fc.2.weight"]).double()))
    return x * y[:, :, None]


def _encoder64(mel, lens, sd, jas):
    W = lambda k: torch.as_tensor(sd[k]).double()   # noqa: E731
    xs, panes = [torch.as_tensor(mel).double()], []
    for i, b in enumerate(jas):
        k = b["kernel"][0] + (1 - b["kernel"][0] % 2)
        s, d, sep, res, se = b["stride"][0], b["dilation"][0], b.get("separable", False), b["residual"], b.get("se", False)
        out, l, j = xs[-1], lens, 0
        for r in range(b["repeat"]):
            if sep:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, out.shape[1])
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j + 1}.conv.weight"), 1, 1, 1)
                j += 2
            else:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, 1)
                j += 1
            out = _bn(out, sd, f"encoder.{i}.mconv.{j}")
            j += 1
            if r != b["repeat"] - 1:
                out = torch.relu(out)
                j += 2
            if se and not res:
                out = _se(out, sd, f"encoder.{i}.mconv.{j}")
                j += 1
        if res:
            srcs = xs if b.get("residual_dense", False) else xs[:1]
            for q, src in enumerate(srcs):
                ro, _ = _masked_conv(src, lens, W(f"encoder.{i}.res.{q}.0.conv.weight"), 1, 1, 1)
                ro = _bn(ro, sd, f"encoder.{i}.res.{q}.1")
                if se:
                    ro = _se(ro, sd, f"encoder.{i}.res.{q}.2")
                out = out + ro
        out = torch.relu(out)
        xs = xs + [out] if (res and b.get("residual_dense", False)) else [out]
        lens = l
    return xs[-1], lens


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference_fixtures(name):
    from viet_asr_amd import synth
    g = _golden(name)
    jas = json.loads(str(g["definition"]))
    seed = int(g["seed"])
    sd = synth.encoder_state_dict(jas, 64, seed)
    dec = synth.decoder_state_dict(jas[-1]["filters"], 29, seed)
    for i in range(len(g["lens"])):
        mel = g[f"mel_{i}"]
        lens = torch.tensor([mel.shape[2]])
        e, el = _encoder64(mel, lens, sd, jas)
        logits = F.conv1d(e, torch.as_tensor(dec["decoder_layers.0.weight"]).double(),
                          torch.as_tensor(dec["decoder_layers.0.bias"]).double())
        logp = torch.log_softmax(logits.transpose(1, 2), dim=-1).numpy()
        want = g[f"logp_{i}"]
        assert logp.shape == want.shape
        tol = max(5e-4, 2e-5 * float(np.abs(want).max()))
        assert float(np.abs(logp - want).max()) <= tol, (name, i)
        assert np.array_equal(logp.argmax(-1), g[f"pred64_{i}"]), (name, i)
        assert int(el[0]) == int(g[f"enc_len_{i}"][0])


# ---- the oracle's SE (oracle.quartznet_oracle.squeeze_excite / jasper_block_forward): the three fixtures, ragged batches -----

@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_in_float64_matches_the_reference_fixtures(name):
    """oracle.encoder_forward (float64, row means) on each fixture row, as _encoder64 above: the oracle puts SE where the
    reference does, on every layout the fixtures hold (residual panes, dense panes, after every non-residual sub-layer)."""
    from viet_asr_amd import synth
    from oracle import quartznet_oracle as O
    g = _golden(name)
    jas = json.loads(str(g["definition"]))
    seed = int(g["seed"])
    sd = synth.encoder_state_dict(jas, 64, seed)
    dec = synth.decoder_state_dict(jas[-1]["filters"], 29, seed)
    for i in range(len(g["lens"])):
        mel = g[f"mel_{i}"]
        lens = torch.tensor([mel.shape[2]])
        e, el = O.encoder_forward(mel, lens, sd, jas, dtype=torch.float64)
        e2, _ = _encoder64(mel, lens, sd, jas)
        assert float((e - e2).abs().max()) <= 1e-9 * max(1.0, float(e2.abs().max())), (name, i)
        logp = O.decoder_forward(e, dec).numpy()
        want = g[f"logp_{i}"]
        assert logp.shape == want.shape
        tol = max(5e-4, 2e-5 * float(np.abs(want).max()))
        assert float(np.abs(logp - want).max()) <= tol, (name, i)
        assert np.array_equal(logp.argmax(-1), g[f"pred64_{i}"]), (name, i)
        assert int(el[0]) == int(g[f"enc_len_{i}"][0])


# layouts of every SE placement: separable residual, non-residual (SE after every sub-layer), a dense run, a strided K-tap
# non-separable prologue (pooled at the strided lengths), a plain block behind an SE block
SE_LAYOUT = [
    dict(filters=128, repeat=2, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, se=True,
         se_reduction_ratio=8),
    dict(filters=128, repeat=3, kernel=[7], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True, se=True,
         se_reduction_ratio=4),
    dict(filters=128, repeat=2, kernel=[5], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True, se=True,
         se_reduction_ratio=16),
    dict(filters=128, repeat=1, kernel=[3], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True, se=True,
         se_reduction_ratio=128),
    dict(filters=128, repeat=2, kernel=[9], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True, se=True,
         se_reduction_ratio=1),
    dict(filters=128, repeat=1, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True),
]


def _ragged_mel(lens, T, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((len(lens), 64, T))
    for b, n in enumerate(lens):
        x[b, :, n:] = 3.0 * rng.standard_normal((64, T - n))      # garbage past each row's length: the masks must hide it
    return x


def test_oracle_row_means_make_a_ragged_batch_equal_its_rows_alone():
    """Row means: every row of a ragged batch equals that row run alone at batch 1 (where the tensor is the row's own width),
    to float64 round-off, valid frames compared.  Lengths 1 and 2 reach a 1-frame row through the stride-2 prologue."""
    from viet_asr_amd import synth
    from oracle import quartznet_oracle as O
    sd = synth.encoder_state_dict(SE_LAYOUT, 64, 5)
    lens = np.array([90, 1, 2, 37, 64, 89], dtype=np.int64)
    x = _ragged_mel(lens, 90, 5)
    y, yl = O.encoder_forward(x, torch.from_numpy(lens), sd, SE_LAYOUT, dtype=torch.float64)
    for b, n in enumerate(lens):
        one, ol = O.encoder_forward(x[b:b + 1, :, :n], torch.from_numpy(lens[b:b + 1]), sd, SE_LAYOUT, dtype=torch.float64)
        f = int(ol[0])
        assert f == int(yl[b]) and one.shape[2] == f
        assert float((y[b, :, :f] - one[0]).abs().max()) <= 1e-12 * max(1.0, float(one.abs().max())), (b, n)


def test_oracle_width_means_differ_on_a_ragged_batch():
    """The reference's own mean (se_mean="width": the padded tensor width) is not the device's: on a ragged batch a short row
    differs from its batch-1 call, while the longest row (as long as the tensor) and any batch-1 call agree in both modes --
    the documented deviation (vasr.h vasr_set_block_se)."""
    from viet_asr_amd import synth
    from oracle import quartznet_oracle as O
    sd = synth.encoder_state_dict(SE_LAYOUT, 64, 5)
    lens = np.array([90, 37], dtype=np.int64)
    x = _ragged_mel(lens, 90, 6)
    L = torch.from_numpy(lens)
    rows = O.encoder_forward(x, L, sd, SE_LAYOUT, dtype=torch.float64)[0]
    width = O.encoder_forward(x, L, sd, SE_LAYOUT, dtype=torch.float64, se_mean="width")[0]
    f = int(O.encoder_forward(x[1:, :, :37], L[1:], sd, SE_LAYOUT, dtype=torch.float64)[1][0])
    scale = float(rows[1, :, :f].abs().max())
    assert float((width[1, :, :f] - rows[1, :, :f]).abs().max()) > 1e-3 * scale
    assert float((width[0] - rows[0]).abs().max()) <= 1e-12 * max(1.0, float(rows[0].abs().max()))
    one_w = O.encoder_forward(x[1:, :, :37], L[1:], sd, SE_LAYOUT, dtype=torch.float64, se_mean="width")[0]
    assert float((one_w[0] - rows[1, :, :f]).abs().max()) <= 1e-12 * max(1.0, scale)
    with pytest.raises(ValueError):
        O.encoder_forward(x, L, sd, SE_LAYOUT, dtype=torch.float64, se_mean="frames")


def test_finalize_refuses_se_wider_than_1024_channels():
    """1152 channels: past the two 1024-float LDS arrays of se_mlp_kernel -- VASR_ERR_UNSUPPORTED from vasr_finalize's first
    check, before any weight is looked at or anything touches a device (this runs without one).  1024 passes that check and
    stops at the missing weights instead (VASR_ERR_STATE).  The codes are read from include/vasr.h."""
    import re
    from viet_asr_amd import _lib, engine
    codes = dict(re.findall(r"(VASR_ERR_\w+) = (-\d+)", open(os.path.join(HERE, "..", "include", "vasr.h")).read()))
    unsupported, state = int(codes["VASR_ERR_UNSUPPORTED"]), int(codes["VASR_ERR_STATE"])
    L = _lib.lib()
    for filters, ratio, want in ((1152, 8, unsupported), (1152, 1152, unsupported), (1024, 1, state), (1024, 1024, state)):
        jas = [dict(filters=filters, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False, se=True,
                    se_reduction_ratio=ratio)]
        h = _handle(engine.blocks_from_config(jas), engine.se_from_config(jas))
        assert L.vasr_finalize(h.h) == want, (filters, ratio)
        if want == unsupported:
            assert "1152 channels" in L.vasr_last_error().decode()
        h.close()
