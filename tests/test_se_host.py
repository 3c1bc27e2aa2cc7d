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
