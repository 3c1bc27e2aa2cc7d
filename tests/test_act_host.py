"""CPU checks of JasperEncoder's ``activation`` ("relu", "hardtanh", "selu") and ``residual_mode`` ("add", anything else = max):
config parsing, the constructors, the refusals (Python and vasr_set_activation / vasr_finalize on the devtools build, before
anything touches a device), the state_dict layout against the reference's own (tests/golden/act_*_state_dict_keys.json,
written by make_golden_act.py), the fixtures' own consistency, and the ABI version."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("act_15x5_selu_add_rows3", "act_15x5_hardtanh_max_rows3", "act_dense_selu_max_rows3",
            "act_dense_se_relu_max_rows3", "act_conv_selu_add_rows3", "act_groups_se_hardtanh_group_rows3")

_JAS = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True),
        dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def _cfg(name):
    from viet_asr_amd import configs
    g = _golden(name)
    jas = json.loads(str(g["definition"]))
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(activation=str(g["activation"]), residual_mode=str(g["residual_mode"]),
                                normalization_mode=str(g["normalization_mode"]), norm_groups=int(g["norm_groups"]))
    return g, cfg, jas


def test_activation_from_config_maps_the_options():
    from viet_asr_amd import engine
    assert engine.activation_from_config({}) == (0, 0)
    assert engine.activation_from_config(dict(activation="relu", residual_mode="add")) == (0, 0)
    assert engine.activation_from_config(dict(activation="hardtanh")) == (1, 0)
    assert engine.activation_from_config(dict(activation="selu", residual_mode="max")) == (2, 1)
    # the reference: `if self.residual_mode == "add": ... else: torch.max` -- any other string is max
    assert engine.activation_from_config(dict(residual_mode="maximum")) == (0, 1)
    with pytest.raises(KeyError):
        engine.activation_from_config(dict(activation="gelu"))


@pytest.mark.parametrize("activation", ["relu", "hardtanh", "selu"])
@pytest.mark.parametrize("residual_mode", ["add", "max"])
def test_constructors_accept_the_options(activation, residual_mode):
    from viet_asr_amd import asr
    enc = asr.JasperEncoder(_JAS, activation, 64, residual_mode=residual_mode)
    assert (enc._act, enc._res_mode) == ({"relu": 0, "hardtanh": 1, "selu": 2}[activation], int(residual_mode == "max"))
    # the activation has no parameters: the keys are the ReLU model's
    assert enc.state_dict().keys() == asr.JasperEncoder(_JAS, "relu", 64).state_dict().keys()


def test_python_refusals():
    from viet_asr_amd import asr
    with pytest.raises(KeyError):
        asr.JasperEncoder(_JAS, "tanh", 64)
    for mode in ("group", "instance", "layer"):
        with pytest.raises(NotImplementedError, match="max"):
            asr.JasperEncoder(_JAS, "selu", 64, normalization_mode=mode, residual_mode="max")
    asr.JasperEncoder(_JAS, "selu", 64, normalization_mode="group", residual_mode="add")
    with pytest.raises(NotImplementedError):
        asr.JasperEncoder(_JAS, "selu", 64, conv_mask=False)
    with pytest.raises(NotImplementedError):
        asr.JasperEncoder(_JAS, "hardtanh", 64, frame_splicing=3)


def test_set_activation_and_finalize_refusals():
    """vasr_set_activation refuses codes out of range with VASR_ERR_INVALID (ValueError in Python); vasr_finalize refuses a
    max residual beside any GroupNorm block with VASR_ERR_UNSUPPORTED before anything touches a device (the devtools
    build, as the tests of the alternate paths use it)."""
    from viet_asr_amd import _lib, engine, synth
    blocks = engine.blocks_from_config(_JAS)
    L = _lib.dev_lib()
    h = _lib.Handle(feat_in=64, blocks=blocks)
    for act, res in ((3, 0), (-1, 0), (0, 2), (0, -1)):
        assert L.vasr_set_activation(h.h, act, res) == -1, (act, res)
    for act in (0, 1, 2):
        for res in (0, 1):
            assert L.vasr_set_activation(h.h, act, res) == 0
    h.close()
    for act, res in ((3, 0), (0, 2)):
        with pytest.raises(ValueError):
            _lib.Handle(feat_in=64, blocks=blocks, activation=act, residual_mode=res)
    for norm in ([8, 0], [0, 8]):      # a GroupNorm block with or without a residual
        h = _lib.Handle(feat_in=64, blocks=blocks)
        for i, g in enumerate(norm):
            if g:
                assert L.vasr_set_block_norm(h.h, i, g) == 0
        assert L.vasr_set_activation(h.h, 2, 1) == 0
        h.load_state_dict(synth.encoder_state_dict(_JAS, 64, 3, norm=norm))
        assert L.vasr_finalize(h.h) == -5, norm
        assert "residual_mode max" in L.vasr_last_error().decode()
        h.close()


def test_abi_version_is_unchanged():
    from viet_asr_amd import _lib
    assert _lib.lib().vasr_abi_version() == 8
    assert "vasr_set_activation" in _lib.SIGNATURES


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_equal_the_reference_layout(name):
    """asr.JasperEncoder and synth build the reference's keys and shapes with the fixture's options."""
    from viet_asr_amd import asr, engine, synth
    g, cfg, jas = _cfg(name)
    with open(os.path.join(HERE, "golden", name.replace("_rows3", "") + "_state_dict_keys.json")) as f:
        want = json.load(f)
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == want
    sd = synth.encoder_state_dict(jas, 64, 1, norm=engine.norm_from_config(cfg["JasperEncoder"], jas))
    assert {k: list(np.shape(v)) for k, v in sd.items()} == want


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_hold_what_the_activation_allows(name):
    """The fixture's options are the ones its name says, and its outputs are normalized log-probs with their argmax."""
    g, cfg, jas = _cfg(name)
    assert "_" + str(g["activation"]) + "_" in name and ("_max_" in name) == (str(g["residual_mode"]) == "max")
    for i in range(len(g["lens"])):
        lp = g[f"logp_{i}"][0]
        assert np.allclose(np.exp(lp.astype(np.float64)).sum(-1), 1.0, atol=1e-4)
        assert np.array_equal(lp.argmax(-1), g[f"pred_{i}"][0])
