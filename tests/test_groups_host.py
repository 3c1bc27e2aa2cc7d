"""CPU checks of grouped JasperBlocks (groups + GroupShuffle), shared depthwise weights (heads) and kernel_size_factor: config
parsing, the state_dict layout against the reference's own (tests/golden/groups_*_state_dict_keys.json, written by
make_golden_groups.py), unchanged synthetic weights of ungrouped models, vasr_set_block_groups / vasr_finalize refusals, and a
float64 restatement (F.conv1d(groups=G) + the shuffle) checked against the reference's fixtures."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("groups_15x5_rows3", "groups_jasper_rows3", "groups_dense_rows3", "groups_se_rows3")


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name + ".npz")))


def _jas(name):
    return json.loads(str(_golden(name)["definition"]))


def test_blocks_from_config_reads_groups_heads_and_kernel_size_factor():
    from viet_asr_amd import configs, engine
    jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
    plain = engine.blocks_from_config(jas)
    g = copy.deepcopy(jas)
    for b in g:
        b["groups"] = 4
    g[1]["heads"] = 16
    assert engine.blocks_from_config(g) == plain                     # groups / heads: not in the block description
    assert engine.groups_from_config(jas) == [(1, -1)] * len(jas)
    assert engine.groups_from_config(g) == [(4, 16 if i == 1 else -1) for i in range(len(jas))]
    f = copy.deepcopy(jas)
    f[4]["kernel_size_factor"] = 0.5
    got = engine.blocks_from_config(f)
    assert got[4]["kernel"] == 19 and got[:4] == plain[:4] and got[5:] == plain[5:]
    for bad in (dict(groups=0), dict(groups=1.5), dict(heads=0), dict(heads=-2)):
        with pytest.raises(ValueError):
            engine.groups_from_config([dict(jas[1], **bad)])
    # heads on a block that is not separable: ignored, as the reference ignores it (only a separable block's depthwise conv
    # receives it, parts/jasper.py:353-386)
    assert engine.groups_from_config([dict(jas[17], heads=4), dict(jas[17], heads=4, groups=2)]) == [(1, -1), (2, -1)]


# (K, kernel_size_factor, compute_new_kernel_size(K, f)) -- values of the reference's function (parts/jasper.py:52-57)
KERNEL_TABLE = [(33, 1.0, 33), (33, 0.5, 17), (39, 0.5, 19), (11, 0.25, 3), (1, 0.1, 1), (3, 0.3, 1), (87, 1.5, 131),
                (13, 2.0, 27), (5, 0.2, 1), (51, 0.75, 39), (2, 1.0, 3), (7, 0.99, 7)]


@pytest.mark.parametrize("k,f,want", KERNEL_TABLE)
def test_kernel_size_factor_matches_compute_new_kernel_size(k, f, want):
    from viet_asr_amd import engine, synth
    assert engine.compute_new_kernel_size(k, f) == want
    l = dict(filters=256, repeat=1, kernel=[k], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
             kernel_size_factor=f)
    b = engine.blocks_from_config([l])[0]
    assert b["kernel"] + (1 - b["kernel"] % 2) == want                # the library makes an even kernel odd itself
    assert synth.kernel_of(l) == want


@pytest.mark.parametrize("name", ["groups_15x5", "groups_jasper", "groups_dense", "groups_se"])
def test_state_dict_keys_equal_the_reference_layout(name):
    from viet_asr_amd import asr, configs, synth
    want = json.load(open(os.path.join(HERE, "golden", name + "_state_dict_keys.json"), encoding="utf-8"))
    jas = _jas(name + "_rows3")
    enc = asr.JasperEncoder(feat_in=64, **configs.jasper_definition(jas)["JasperEncoder"])
    got = {k: list(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    sd = synth.encoder_state_dict(jas, 64, 1)
    assert {k: list(np.shape(v)) for k, v in sd.items()} == want


# heads on non-separable blocks (and a separable one), keys written by make_golden_groups.py from the reference's own modules
HEADS_NONSEP = [dict(filters=256, repeat=2, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, groups=2, heads=4),
                dict(filters=256, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=True, heads=8),
                dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                     heads=16)]


def test_heads_on_non_separable_blocks_are_ignored_like_the_reference():
    from viet_asr_amd import asr, configs, engine, synth
    want = json.load(open(os.path.join(HERE, "golden", "groups_heads_nonsep_state_dict_keys.json"), encoding="utf-8"))
    enc = asr.JasperEncoder(feat_in=64, **configs.jasper_definition(HEADS_NONSEP)["JasperEncoder"])
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == want
    sd = synth.encoder_state_dict(HEADS_NONSEP, 64, 1)
    assert {k: list(np.shape(v)) for k, v in sd.items()} == want
    plain = [dict(b) for b in HEADS_NONSEP[:2]]
    for b in plain:
        del b["heads"]
    same = synth.encoder_state_dict(plain, 64, 1)
    assert all(np.array_equal(same[k], sd[k]) for k in same)          # the same weights as without heads
    assert engine.groups_from_config(HEADS_NONSEP) == [(2, -1), (1, -1), (1, 16)]


# sha256 over (key, dtype, bytes) of synth.encoder_state_dict(builtin, 64, 0), sorted by key: the values before grouping existed
UNGROUPED_DIGESTS = {
    "quartznet12x1": "a7f5f528941fa102f6746bb16b27a70c589caaea257b44d227f9dad69e7dab86",
    "quartznet15x5": "e9c753ac7f26fee81ada12d653c37f93d91bdfe05f95d15d9f202c93b531436e",
    "jasper10x5dr": "b243f2259a247298823aea0911d4a6e379e95d1b9d288bce344f8b1002627499",
}


@pytest.mark.parametrize("name", sorted(UNGROUPED_DIGESTS))
def test_synthetic_weights_of_ungrouped_models_are_unchanged(name):
    from viet_asr_amd import configs, synth
    sd = synth.encoder_state_dict(configs.builtin(name)["JasperEncoder"]["jasper"], 64, 0)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(str(sd[k].dtype).encode())
        h.update(sd[k].tobytes())
    assert h.hexdigest() == UNGROUPED_DIGESTS[name]


def _handle(blocks, groups, se=None):
    from viet_asr_amd import _lib
    return _lib.Handle(feat_in=64, blocks=blocks, se=se, groups=groups)


def test_set_block_groups_and_finalize_refusals():
    """Refusals of vasr_set_block_groups and vasr_finalize's grouped checks -- all before anything touches a device (this runs
    without one): VASR_ERR_INVALID (-1) for groups / heads that do not divide the channels and wrongly shaped weights,
    VASR_ERR_STATE (-2) for missing ones, VASR_ERR_UNSUPPORTED (-5) for grouped filters that are not a multiple of 128."""
    from viet_asr_amd import _lib, engine, synth
    L = _lib.lib()
    jas = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                groups=4, heads=8)]
    blocks = engine.blocks_from_config(jas)
    h = _handle(blocks, None)
    assert L.vasr_set_block_groups(h.h, 1, 2, -1) == -1            # no such block
    assert L.vasr_set_block_groups(h.h, -1, 2, -1) == -1
    assert L.vasr_set_block_groups(h.h, 0, 0, -1) == -1            # groups < 1
    assert L.vasr_set_block_groups(h.h, 0, 2, 0) == -1             # heads: -1 or positive
    assert L.vasr_set_block_groups(h.h, 0, 2, -3) == -1
    assert L.vasr_set_block_groups(h.h, 0, 3, -1) == 0             # 3 divides neither 64 nor 256
    assert L.vasr_finalize(h.h) == -1
    assert "groups 3" in L.vasr_last_error().decode()
    h.close()
    h = _handle(blocks, [(2, 6)])                                  # 64 % 6 != 0
    assert L.vasr_finalize(h.h) == -1
    assert "heads 6" in L.vasr_last_error().decode()
    h.close()
    # heads handed to a non-separable block through the C ABI: ignored there, as by the reference -- no refusal, finalize goes
    # on to look for the plain weights (none loaded: VASR_ERR_STATE on the first one)
    nonsep = [dict(jas[0], separable=False, heads=-1)]
    h = _handle(engine.blocks_from_config(nonsep), [(1, 4)])
    assert L.vasr_finalize(h.h) == -2
    assert "encoder.0.mconv.0.conv.weight" in L.vasr_last_error().decode()
    h.close()
    # a grouped block whose filters are not a multiple of 128 (192 at G = 3: 64 per group, but the GEMM rows pad to 256):
    # VASR_ERR_UNSUPPORTED up front, the rule every block meets
    odd = [dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False),
           dict(filters=192, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False, groups=3)]
    h = _handle(engine.blocks_from_config(odd), engine.groups_from_config(odd))
    assert L.vasr_finalize(h.h) == -5
    assert "multiple of 128" in L.vasr_last_error().decode()
    h.close()
    sd = synth.encoder_state_dict(jas, 64, 3)
    # the shuffle entries shift the keys: a separable grouped sub-layer takes four slots (dw, pw, BN, shuffle) + act, drop
    assert sd["encoder.0.mconv.0.conv.weight"].shape == (8, 1, 11)
    assert sd["encoder.0.mconv.1.conv.weight"].shape == (256, 16, 1)
    assert "encoder.0.mconv.2.running_var" in sd and "encoder.0.mconv.6.conv.weight" in sd
    assert sd["encoder.0.mconv.7.conv.weight"].shape == (256, 64, 1)
    assert sd["encoder.0.res.0.0.conv.weight"].shape == (256, 64, 1)   # the residual branch is never grouped
    # missing grouped weight: VASR_ERR_STATE
    h = _handle(blocks, engine.groups_from_config(jas))
    h.load_state_dict({k: v for k, v in sd.items() if k != "encoder.0.mconv.7.conv.weight"})
    with pytest.raises(_lib.VasrError) as e:
        h.finalize()
    assert "encoder.0.mconv.7.conv.weight" in str(e.value)
    assert L.vasr_finalize(h.h) == -2
    h.close()
    # a dense (ungrouped) weight where the grouped one belongs, a per-channel depthwise weight where heads share rows, and
    # transposed shapes with the right element count: the shapes are checked, not only the sizes
    for key, shape in (("encoder.0.mconv.7.conv.weight", (256, 256, 1)), ("encoder.0.mconv.0.conv.weight", (64, 1, 11)),
                       ("encoder.0.mconv.7.conv.weight", (64, 256, 1)), ("encoder.0.mconv.0.conv.weight", (1, 8, 11))):
        h = _handle(blocks, engine.groups_from_config(jas))
        h.load_state_dict(dict(sd, **{key: np.zeros(shape, dtype=np.float32)}))
        assert L.vasr_finalize(h.h) == -1, (key, shape)
        assert key in L.vasr_last_error().decode() and "shape" in L.vasr_last_error().decode()
        h.close()


# ---- float64 restatement of grouped blocks (parts/jasper.py:70-150, :214-288, :329-448) -----------------------------------

def _masked_conv(x, lens, w, stride, dil, groups, heads=-1):
    k = w.shape[-1]
    pad = (dil * k) // 2 - 1 if dil > 1 else k // 2
    t = torch.arange(x.shape[2])
    x = x.masked_fill(t[None, None, :] >= lens[:, None, None], 0.0)
    sh = x.shape
    if heads != -1:
        x = x.reshape(-1, heads, sh[-1])
    y = F.conv1d(x, w, stride=stride, padding=pad, dilation=dil, groups=groups)
    if heads != -1:
        y = y.reshape(sh[0], sh[1], -1)
    lens = ((lens.double() + 2 * pad - dil * (k - 1) - 1) / stride + 1).long()
    return y, lens


def _shuffle(x, groups):
    b, c, t = x.shape
    return x.reshape(b, groups, c // groups, t).transpose(1, 2).reshape(b, c, t)


def _bn(x, sd, p):
    g, b, m, v = (torch.as_tensor(sd[f"{p}.{n}"]).double() for n in ("weight", "bias", "running_mean", "running_var"))
    return (x - m[:, None]) / torch.sqrt(v[:, None] + 1e-3) * g[:, None] + b[:, None]


def _se(x, sd, p):
    y = x.mean(dim=2)
    y = torch.sigmoid(F.linear(torch.relu(F.linear(y, torch.as_tensor(sd[f"{p}.fc.0.weight"]).double())),
                               torch.as_tensor(sd[f"{p}.fc.2.weight"]).double()))
    return x * y[:, :, None]


def _encoder64(mel, lens, sd, jas):
    from viet_asr_amd import synth
    W = lambda k: torch.as_tensor(sd[k]).double()   # noqa: E731
    xs = [torch.as_tensor(mel).double()]
    for i, b in enumerate(jas):
        k = synth.kernel_of(b)
        s, d, sep, res, se = b["stride"][0], b["dilation"][0], b.get("separable", False), b["residual"], b.get("se", False)
        G, H = b.get("groups", 1), b.get("heads", -1)
        out, l, j = xs[-1], lens, 0
        for r in range(b["repeat"]):
            if sep:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, H if H != -1 else out.shape[1], H)
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j + 1}.conv.weight"), 1, 1, G)
                j += 2
            else:
                out, l = _masked_conv(out, l, W(f"encoder.{i}.mconv.{j}.conv.weight"), s, d, G)
                j += 1
            out = _bn(out, sd, f"encoder.{i}.mconv.{j}")
            j += 1
            if G > 1:
                out = _shuffle(out, G)
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


def test_shuffle_is_the_reference_permutation():
    """Output channel j * G + g holds pre-shuffle channel g * (C / G) + j (GroupShuffle, parts/jasper.py:135-150)."""
    C, G = 12, 3
    x = torch.arange(C, dtype=torch.float64)[None, :, None]
    y = _shuffle(x, G)[0, :, 0]
    for g in range(G):
        for j in range(C // G):
            assert int(y[j * G + g]) == g * (C // G) + j
