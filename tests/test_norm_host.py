"""CPU checks of GroupNorm JasperEncoders (normalization_mode "group" / "instance" / "layer", norm_groups): config parsing, the
state_dict layout against the reference's own (tests/golden/norm_*_state_dict_keys.json, written by make_golden_norm.py),
vasr_set_block_norm / vasr_finalize refusals, forward_long's refusal, and a float64 restatement of the normalized encoder
checked against the reference's fixtures and against the row rule (statistics over each row's own frames) in a ragged batch."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("norm_15x5_group32_rows3", "norm_dense_layer_rows3", "norm_se_instance_rows3", "norm_groups_group8_rows3")


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def _case(name):
    """(golden, model definition, block list, per-block GroupNorm group counts)."""
    from viet_asr_amd import configs, engine
    g = _golden(name)
    jas = json.loads(str(g["definition"]))
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(normalization_mode=str(g["normalization_mode"]), norm_groups=int(g["norm_groups"]))
    return g, cfg, jas, engine.norm_from_config(cfg["JasperEncoder"], jas)


def test_norm_from_config_maps_the_modes():
    from viet_asr_amd import engine
    jas = [dict(filters=256), dict(filters=512)]
    assert engine.norm_from_config({}, jas) == [0, 0]
    assert engine.norm_from_config(dict(normalization_mode="batch", norm_groups=7), jas) == [0, 0]
    assert engine.norm_from_config(dict(normalization_mode="group", norm_groups=32), jas) == [32, 32]
    assert engine.norm_from_config(dict(normalization_mode="group"), jas) == [256, 512]        # -1: the channels
    assert engine.norm_from_config(dict(normalization_mode="instance", norm_groups=32), jas) == [256, 512]
    assert engine.norm_from_config(dict(normalization_mode="layer", norm_groups=32), jas) == [1, 1]


def test_blocks_from_config_output_is_unchanged_by_normalization():
    from viet_asr_amd import configs, engine
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    plain = engine.blocks_from_config(jas)
    for name in FIXTURES:
        g, cfg, fj, norm = _case(name)
        assert engine.blocks_from_config(cfg["JasperEncoder"]["jasper"]) == engine.blocks_from_config(fj)
        assert all(n > 0 for n in norm)
    assert engine.blocks_from_config(jas) == plain
    assert set(plain[0]) == {"filters", "repeat", "kernel", "stride", "dilation", "residual", "separable", "residual_dense"}


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_equal_the_reference_layout(name):
    """asr.JasperEncoder and synth build the reference's keys and shapes (GroupNorm: weight / bias, no running statistics)."""
    from viet_asr_amd import asr, synth
    g, cfg, jas, norm = _case(name)
    with open(os.path.join(HERE, "golden", name.replace("_rows3", "") + "_state_dict_keys.json")) as f:
        want = json.load(f)
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == want
    sd = synth.encoder_state_dict(jas, 64, 1, norm=norm)
    assert {k: list(np.shape(v)) for k, v in sd.items()} == want
    assert not any("running_mean" in k for k in want)


def test_synthetic_weights_without_groupnorm_are_unchanged():
    """GroupNorm weights come from their own streams: a BatchNorm model's tensors are what they were (norm None or all 0),
    and a normalized model's conv weights equal the BatchNorm model's."""
    from viet_asr_amd import configs, synth
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    plain = synth.encoder_state_dict(jas, 64, 7)
    zero = synth.encoder_state_dict(jas, 64, 7, norm=[0] * len(jas))
    gn = synth.encoder_state_dict(jas, 64, 7, norm=[32] * len(jas))
    assert plain.keys() == zero.keys()
    for k in plain:
        assert np.array_equal(plain[k], zero[k]), k
        if k.endswith("conv.weight"):
            assert np.array_equal(plain[k], gn[k]), k
    assert not any(k.endswith("running_var") for k in gn)
    assert not np.array_equal(gn["encoder.0.mconv.2.weight"], plain["encoder.0.mconv.2.weight"])


def test_python_refusals():
    from viet_asr_amd import asr, engine
    jas = [dict(filters=256, repeat=1, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True),
           dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
    with pytest.raises(ValueError, match="Normalization method"):
        asr.JasperEncoder(jas, "relu", 64, normalization_mode="weight")
    with pytest.raises(ValueError, match="divisible"):
        asr.JasperEncoder(jas, "relu", 64, normalization_mode="group", norm_groups=256)   # 384 % 256
    with pytest.raises(ValueError):
        engine.norm_from_config(dict(normalization_mode="group", norm_groups=0), jas)
    asr.JasperEncoder(jas, "relu", 64, normalization_mode="group", norm_groups=128)
    # the options that stay unimplemented keep raising NotImplementedError
    with pytest.raises(NotImplementedError):
        asr.JasperEncoder(jas, "relu", 64, normalization_mode="layer", residual_mode="max")
    with pytest.raises(NotImplementedError):
        asr.JasperEncoder(jas, "relu", 64, normalization_mode="layer", conv_mask=False)


def test_set_block_norm_and_finalize_refusals():
    """vasr_finalize refuses a non-dividing group count and missing or misshaped gamma / beta with VASR_ERR_INVALID, before
    anything touches a device (the devtools build, as the tests of the alternate paths use it)."""
    from viet_asr_amd import _lib, engine, synth
    jas = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True)]
    blocks = engine.blocks_from_config(jas)
    sd = synth.encoder_state_dict(jas, 64, 3, norm=[8])
    L = _lib.dev_lib()

    def handle(norm, weights):
        h = _lib.Handle(feat_in=64, blocks=blocks)
        for i, g in enumerate(norm):
            assert L.vasr_set_block_norm(h.h, i, g) == 0
        h.load_state_dict(weights)
        return h

    h = _lib.Handle(feat_in=64, blocks=blocks)
    assert L.vasr_set_block_norm(h.h, 1, 8) == -1       # no such block
    assert L.vasr_set_block_norm(h.h, -1, 8) == -1
    assert L.vasr_set_block_norm(h.h, 0, -1) == -1
    h.close()
    h = handle([24], sd)                                  # 256 % 24
    assert L.vasr_finalize(h.h) == -1
    assert "norm_groups 24" in L.vasr_last_error().decode()
    h.close()
    h = handle([8], {k: v for k, v in sd.items() if k != "encoder.0.res.0.1.bias"})
    assert L.vasr_finalize(h.h) == -1
    assert "encoder.0.res.0.1.bias" in L.vasr_last_error().decode()
    h.close()
    bad = dict(sd)
    bad["encoder.0.mconv.7.weight"] = np.ones(128, dtype=np.float32)
    h = handle([8], bad)
    assert L.vasr_finalize(h.h) == -1
    assert "encoder.0.mconv.7.weight" in L.vasr_last_error().decode()
    h.close()


def test_forward_long_refuses_normalized_models():
    from viet_asr_amd.engine import QuartzNetCTC
    with pytest.raises(NotImplementedError, match="normalization"):
        QuartzNetCTC.forward_long(types.SimpleNamespace(_se=[0, 0], _norm=[0, 32]), torch.zeros(16000))


# ---- float64 restatement of the normalized encoder (parts/jasper.py:113-150, :152-168, :214-288, :385-448) -----------------
# GroupNorm's statistics and SE's mean are over each row's own frames t < len_b: the reference's whole-width statistics in
# the batch-1 fixtures (the width is the row's length there), the library's row rule in a ragged batch.

def _mask(x, lens):
    t = torch.arange(x.shape[2])
    return x.masked_fill(t[None, None, :] >= lens[:, None, None], 0.0)


def _masked_conv(x, lens, w, stride, dil, groups):
    k = w.shape[-1]
    pad = (dil * k) // 2 - 1 if dil > 1 else k // 2
    y = F.conv1d(_mask(x, lens), w, stride=stride, padding=pad, dilation=dil, groups=groups)
    lens = ((lens.double() + 2 * pad - dil * (k - 1) - 1) / stride + 1).long()
    return y, lens


def _gn(x, lens, G, sd, p):
    """GroupNorm(G, C), biased variance, eps 1e-5, over channels of the group x t < lens[b]."""
    B, Cn, T = x.shape
    g, b = (torch.as_tensor(sd[f"{p}.{n}"]).double() for n in ("weight", "bias"))
    m = (torch.arange(T)[None, :] < lens[:, None]).double()[:, None, None, :]     # [B, 1, 1, T]
    xg = x.reshape(B, G, Cn // G, T)
    n = (m.sum(dim=3, keepdim=True) * (Cn // G)).clamp(min=1)
    mean = (xg * m).sum(dim=(2, 3), keepdim=True) / n
    var = (((xg - mean) * m) ** 2).sum(dim=(2, 3), keepdim=True) / n
    y = ((xg - mean) / torch.sqrt(var + 1e-5)).reshape(B, Cn, T)
    return y * g[:, None] + b[:, None]


def _shuffle(x, G):
    B, Cn, T = x.shape
    return x.view(B, G, Cn // G, T).transpose(1, 2).reshape(B, Cn, T)


def _se(x, lens, sd, p):
    y = _mask(x, lens).sum(dim=2) / lens[:, None].double().clamp(min=1)
    y = torch.sigmoid(F.linear(torch.relu(F.linear(y, torch.as_tensor(sd[f"{p}.fc.0.weight"]).double())),
                               torch.as_tensor(sd[f"{p}.fc.2.weight"]).double()))
    return x * y[:, :, None]


def _encoder64(mel, lens, sd, jas, norm):
    W = lambda k: torch.as_tensor(sd[k]).double()   # noqa: E731
    xs = [torch.as_tensor(mel).double()]
    for i, (b, G) in enumerate(zip(jas, norm)):
        k = b["kernel"][0] + (1 - b["kernel"][0] % 2)
        s, d, sep, res, se = b["stride"][0], b["dilation"][0], b.get("separable", False), b["residual"], b.get("se", False)
        groups = b.get("groups", 1)
        out, l, j = xs[-1], lens, 0
        for r in range(b["repeat"]):
            if sep:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, out.shape[1])
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j + 1}.conv.weight"), 1, 1, groups)
                j += 2
            else:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, groups)
                j += 1
            out = _gn(out, l, G, sd, f"encoder.{i}.mconv.{j}")
            j += 1
            if groups > 1:
                out = _shuffle(out, groups)
                j += 1
            if r != b["repeat"] - 1:
                out = torch.relu(out)
                j += 2
            if se and not res:
                out = _se(out, l, sd, f"encoder.{i}.mconv.{j}")
                j += 1
        if res:
            srcs = xs if b.get("residual_dense", False) else xs[:1]
            for q, src in enumerate(srcs):
                ro, _ = _masked_conv(src, lens, W(f"encoder.{i}.res.{q}.0.conv.weight"), 1, 1, 1)
                ro = _gn(ro, lens, G, sd, f"encoder.{i}.res.{q}.1")
                if se:
                    ro = _se(ro, lens, sd, f"encoder.{i}.res.{q}.2")
                out = out + ro
        out = torch.relu(out)
        xs = xs + [out] if (res and b.get("residual_dense", False)) else [out]
        lens = l
    return xs[-1], lens


def _logp(e, dec):
    logits = F.conv1d(e, torch.as_tensor(dec["decoder_layers.0.weight"]).double(),
                      torch.as_tensor(dec["decoder_layers.0.bias"]).double())
    return torch.log_softmax(logits.transpose(1, 2), dim=-1).numpy()


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_restatement_matches_the_reference_fixtures(name):
    from viet_asr_amd import synth
    g, cfg, jas, norm = _case(name)
    seed = int(g["seed"])
    sd = synth.encoder_state_dict(jas, 64, seed, norm=norm)
    dec = synth.decoder_state_dict(jas[-1]["filters"], 29, seed)
    for i in range(len(g["lens"])):
        mel = g[f"mel_{i}"]
        e, el = _encoder64(mel, torch.tensor([mel.shape[2]]), sd, jas, norm)
        logp = _logp(e, dec)
        want = g[f"logp_{i}"]
        assert logp.shape == want.shape
        tol = max(5e-4, 2e-5 * float(np.abs(want).max()))
        assert float(np.abs(logp - want).max()) <= tol, (name, i)
        assert np.array_equal(logp.argmax(-1), g[f"pred64_{i}"]), (name, i)
        assert int(el[0]) == int(g[f"enc_len_{i}"][0])


@pytest.mark.parametrize("name", ["norm_dense_layer_rows3", "norm_groups_group8_rows3"])
def test_row_rule_makes_a_ragged_batch_equal_its_rows_alone(name):
    """Statistics over each row's own frames: the rows of a padded batch give what they give alone (float64), and the
    reference's whole-width rule would not -- it moves the shorter rows."""
    from viet_asr_amd import synth
    g, cfg, jas, norm = _case(name)
    seed = int(g["seed"])
    sd = synth.encoder_state_dict(jas, 64, seed, norm=norm)
    T = max(g[f"mel_{i}"].shape[2] for i in range(3))
    mel = np.zeros((3, 64, T))
    for i in range(3):
        mel[i, :, : g[f"mel_{i}"].shape[2]] = g[f"mel_{i}"][0]
    lens = torch.tensor([g[f"mel_{i}"].shape[2] for i in range(3)])
    e, el = _encoder64(mel, lens, sd, jas, norm)
    for i in range(3):
        one, ol = _encoder64(g[f"mel_{i}"], lens[i:i + 1], sd, jas, norm)
        f = int(ol[0])
        assert int(el[i]) == f
        assert torch.allclose(e[i, :, :f], one[0, :, :f], rtol=1e-9, atol=1e-9), (name, i)
    # the whole-width statistics of the reference differ for the shorter rows of the batch
    wide, _ = _encoder64(mel, torch.full((3,), T), sd, jas, norm)
    short = int(np.argmin(lens.numpy()))
    f = int(el[short])
    assert float((wide[short, :, :f] - e[short, :, :f]).abs().max()) > 1e-3
