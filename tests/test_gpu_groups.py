"""-m gpu: grouped JasperBlocks (groups + GroupShuffle, heads, kernel_size_factor; vasr_set_block_groups) against the imported
reference's own batch-1 outputs (tests/golden/make_golden_groups.py), and the grouped split GEMM (encoder_pw_split.hip GRP)
against its block-diagonal dense form and against float64.

Per fixture row and arithmetic (f16x2, bf16x3, fp32), through the fused path (QuartzNetCTC.forward) and the module path
(asr.JasperEncoder -> vasr_encoder_f32 on the reference's mel, then the CTC head): log-probs within max(5e-4, 2e-5 |log-prob|),
equal encoded lengths, equal predictions and transcripts.  Then: rows of different lengths batched together in row-independent
mode against each row's own fixture; that mode's bit-identical rows across batch compositions; run-to-run bits; forward_long
against the one-pass call; the grouped kernel's floats equal to VASR_NO_GROUPED's (devtools library, child processes); one
grouped layer against float64 at every tile the product picks.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOGP_REL = 2e-5
LOGP_ABS = 5e-4
ARITHMETICS = ("f16x2", "bf16x3", "fp32")
FIXTURES = ("groups_15x5_rows3", "groups_jasper_rows3", "groups_dense_rows3", "groups_se_rows3")
HOP = 160

_CACHE = {}


def _tol(logp):
    return max(LOGP_ABS, LOGP_REL * float(np.abs(np.asarray(logp)).max()))


def _case(name):
    """(golden, definition, jasper list, encoder sd, decoder sd, [row signals], lengths)."""
    if name not in _CACHE:
        from viet_asr_amd import configs, synth
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        jas = json.loads(str(g["definition"]))
        cfg = configs.jasper_definition(jas)
        seed = int(g["seed"])
        lens = g["lens"].astype(np.int64)
        enc_sd = synth.encoder_state_dict(jas, 64, seed)
        dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, seed)
        sig, _ = synth.audio_batch(len(lens), int(lens.max()), seed, ragged=False)
        rows = [sig[b, :n].copy() for b, n in enumerate(lens)]
        _CACHE[name] = (g, cfg, jas, enc_sd, dec_sd, rows, lens)
    return _CACHE[name]


def _check(tag, g, i, logp, pred, enc_len=None, hyp=None):
    """Row i of fixture g against logp [T, V] / pred [T] of the same row (frames past the row's own output cut off).  The
    fixtures have no frame whose float64 top-2 margin lies inside the tolerance: predictions must be equal."""
    want = g[f"logp_{i}"][0]
    logp, pred = np.asarray(logp)[: want.shape[0]], np.asarray(pred)[: want.shape[0]]
    assert logp.shape == want.shape, (tag, logp.shape, want.shape)
    tol = _tol(want)
    assert not (g[f"margin64_{i}"][0] < tol).any(), (tag, i)
    err = float(np.abs(logp - want).max())
    flips = int((pred != g[f"pred_{i}"][0]).sum())
    _record("groups_fixture", case=tag[0], gemm=tag[1], path=tag[2], row=i, err=err, tol=tol, flips=flips)
    assert err <= tol, (tag, i, err, tol)
    assert flips == 0, (tag, i)
    if enc_len is not None:
        assert np.float32(enc_len) == np.float32(g[f"enc_len_{i}"][0]), (tag, i)
    if hyp is not None:
        assert hyp == str(g[f"hyp_{i}"][0]), (tag, i)


def _batch(rows, order, gpu):
    n = max(len(rows[b]) for b in order)
    sig = np.zeros((len(order), n), dtype=np.float32)
    for k, b in enumerate(order):
        sig[k, :len(rows[b])] = rows[b]
    lens = np.array([len(rows[b]) for b in order], dtype=np.int64)
    return torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu)


@pytest.fixture(scope="module")
def engines(gpu):
    from viet_asr_amd.engine import QuartzNetCTC
    out = {}
    for name in FIXTURES:
        g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
        out[name] = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    yield out
    out.clear()


@pytest.mark.parametrize("name", FIXTURES)
def test_fused_path_matches_reference(gpu, engines, name):
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    for gemm in ARITHMETICS:
        eng.handle.set_gemm_mode(gemm)
        for i in range(len(rows)):
            w, l = _batch(rows, [i], gpu)
            r = eng.forward(w, l, want_logp=True)
            hyp = eng.texts(r["ids"], r["id_len"])[0]
            _check((name, gemm, "fused"), g, i, r["logp"][0].cpu(), r["pred"][0].cpu(), float(r["enc_len"][0]), hyp)
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("name", FIXTURES)
def test_module_path_matches_reference(gpu, name):
    """asr.JasperEncoder on the reference's own mel features (vasr_encoder_f32), then asr.JasperDecoderForCTC."""
    from viet_asr_amd import asr
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec = asr.JasperDecoderForCTC(feat_in=jas[-1]["filters"], num_classes=len(cfg["labels"]))
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    for gemm in ARITHMETICS:
        enc._get_handle().set_gemm_mode(gemm)
        dec._get_handle().set_gemm_mode(gemm)
        for i in range(len(rows)):
            mel = torch.from_numpy(g[f"mel_{i}"]).to(gpu)
            seq = torch.tensor([int(np.ceil(lens[i] / HOP))], dtype=torch.int64, device=gpu)
            e, el = enc.forward(mel, seq)
            logp = dec.forward(e)
            _check((name, gemm, "module"), g, i, logp[0].cpu(), logp[0].argmax(-1).cpu(), float(el[0]))


@pytest.mark.parametrize("name", FIXTURES)
def test_ragged_batch_rows_match_their_batch1_fixtures(gpu, engines, name):
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    for gemm in ("f16x2", "fp32"):
        eng.handle.set_gemm_mode(gemm)
        order = [1, 0, 2, 1]
        w, l = _batch(rows, order, gpu)
        r = eng.forward(w, l, want_logp=True, row_independent=True)
        hyp = eng.texts(r["ids"], r["id_len"])
        for k, i in enumerate(order):
            _check((name, gemm, "ragged"), g, i, r["logp"][k].cpu(), r["pred"][k].cpu(), hyp=hyp[k])
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("name", FIXTURES)
def test_row_independent_rows_are_bit_identical_across_batches(gpu, engines, name, gemm):
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    eng.handle.set_gemm_mode(gemm)
    one = []
    for i in range(len(rows)):
        w, l = _batch(rows, [i], gpu)
        one.append(eng.forward(w, l, want_logp=True, row_independent=True)["logp"][0])
    for order in ([2, 1, 0], [1, 2, 0, 0, 2, 1, 1, 0, 2, 2, 0, 1]):
        w, l = _batch(rows, order, gpu)
        r = eng.forward(w, l, want_logp=True, row_independent=True)
        for k, i in enumerate(order):
            f = one[i].shape[0]
            assert torch.equal(r["logp"][k, :f], one[i]), (name, gemm, order, k)
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("name", FIXTURES)
def test_runs_are_bit_identical(gpu, engines, name):
    """64 rows in the default mode (the grouped GEMMs take their throughput tiles): the same call twice, the same bits."""
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    w, l = _batch(rows, [k % 3 for k in range(64)], gpu)
    a = eng.forward(w, l, want_logp=True)["logp"].clone()
    b = eng.forward(w, l, want_logp=True)["logp"]
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["groups_15x5_rows3", "groups_jasper_rows3"])
def test_forward_long_equals_the_one_pass_result(gpu, engines, name):
    """Grouping is local in time: forward_long's windows give the one-pass log-probs bit for bit in bf16x3 (fp16 split: the
    operand scale follows the window, predictions equal here)."""
    eng = engines[name]
    n = 25 * 16000 + 77
    x = torch.from_numpy((0.1 * np.random.default_rng(9).standard_normal(n)).astype(np.float32)).to(gpu)
    for gemm in ("bf16x3", "f16x2"):
        eng.handle.set_gemm_mode(gemm)
        one = eng.forward(x[None], torch.tensor([n], device=gpu), want_logp=True)
        r = eng.forward_long(x, chunk_frames=256, rows_per_pass=2, want_logp=True)
        assert torch.equal(r["pred"], one["pred"]), (name, gemm)
        if gemm == "bf16x3":
            assert torch.equal(r["logp"], one["logp"]), name
    eng.handle.set_gemm_mode("f16x2")


# ---------------------------------------------------------------------------------------------------------------------------
# The grouped split GEMM against the block-diagonal form (VASR_NO_GROUPED=1, devtools library): every grouped layer of the
# fixtures is at least 64 channels wide per group, a multiple of 16, so the two reductions add the same products in the same
# order -- the floats must be equal.

_DIAG_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_groups as T
from viet_asr_amd.engine import QuartzNetCTC
gpu = torch.device("cuda:0")
out = {{}}
for name in T.FIXTURES:
    g, cfg, jas, enc_sd, dec_sd, rows, lens = T._case(name)
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    for gemm in ("f16x2", "bf16x3"):
        eng.handle.set_gemm_mode(gemm)
        for order in ([0], [0, 1, 2], [k % 3 for k in range(64)]):
            w, l = T._batch(rows, order, gpu)
            out[f"{{name}}/{{gemm}}/{{len(order)}}"] = eng.forward(w, l, want_logp=True)["logp"].cpu().numpy()
    eng.handle.profile_begin()
    eng.forward(w, l)
    torch.cuda.synchronize()
    out[f"{{name}}/pointwise_flops"] = np.array(eng.handle.profile_end()["pointwise"]["flops"])
    del eng
torch.cuda.synchronize()
np.savez({path!r}, **out)
print("DIAG_OK")
"""


def test_grouped_gemm_equals_the_block_diagonal_form(gpu, tmp_path):
    from viet_asr_amd import _lib
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    got = {}
    for flag in ("0", "1"):
        path = str(tmp_path / f"diag{flag}.npz")
        code = _DIAG_SNIPPET.format(tests=HERE, root=os.path.dirname(HERE), path=path)
        out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "VASR_LIB_PATH": dev, "VASR_NO_GROUPED": flag},
                             capture_output=True, text=True, timeout=300)
        assert "DIAG_OK" in out.stdout, (flag, out.stdout[-2000:], out.stderr[-2000:])
        got[flag] = dict(np.load(path))
    assert sorted(got["0"]) == sorted(got["1"])
    for name in FIXTURES:
        # the grouped GEMM did run: its matrix work is 1/G of the block-diagonal form's on every grouped layer it covers
        fg, fd = float(got["0"].pop(f"{name}/pointwise_flops")), float(got["1"].pop(f"{name}/pointwise_flops"))
        _record("groups_vs_block_diagonal", case=name, pointwise_flops=fg, block_diagonal_flops=fd)
        assert fg < fd, (name, fg, fd)
    for key in got["0"]:
        same = np.array_equal(got["0"][key].view(np.uint32), got["1"][key].view(np.uint32))
        _record("groups_vs_block_diagonal", case=key, same_bits=same)
        assert same, key


# ---------------------------------------------------------------------------------------------------------------------------
# One grouped layer (a block of one grouped conv + BN + shuffle + ReLU, module path) against float64, at the tiles the product
# picks for its per-group rows: batch 1 / 2 / 8 / 12 / 16 of 1024 frames reach 64x32, 128x64, 256x128, 256x64 and 512x128.

SPLIT_TILES = {1: (512, 128), 2: (256, 128), 3: (128, 64), 4: (64, 32), 5: (256, 64)}


def split_tile(M, groups, cols, batch, cus):
    """launch_pointwise_split's tile for a grouped GEMM of M rows (encoder_pw_split.hip), restated: the divisibility tests use
    the rows per group, the workgroup counts the layer's rows."""
    mg = M // groups
    blocks = lambda bm, bn: (M // bm) * (-(-cols // bn)) * batch   # noqa: E731
    tile = 4
    if mg % 512 == 0 and blocks(512, 128) >= 192:
        tile = 1
    elif mg % 256 == 0 and blocks(256, 128) >= 192:
        tile = 2
    elif mg % 128 == 0 and blocks(128, 64) >= 192:
        tile = 3
    if tile == 2 and mg == 256 and blocks(256, 64) >= 384:
        tile = 5
    if tile == 1:
        n1 = blocks(512, 128)
        rounds = -(-n1 // cus)
        if n1 < 0.85 * rounds * cus:
            tile = 5
    return tile


# (id, C_in, C_out, K, groups, residual); G = 3 is an odd group count, pw_g4_narrow has 32 inputs per group (block-diagonal)
LAYERS = [("pw_g2", 512, 1024, 1, 2, False), ("conv_k3_g4", 512, 1024, 3, 4, False), ("pw_g8_res", 512, 512, 1, 8, True),
          ("pw_g3", 192, 384, 1, 3, False), ("pw_g4_narrow", 128, 512, 1, 4, False)]


def takes_grouped_gemm(cin, cout, G):
    """grouped_split_supported (encoder_pw_split.hip), restated: per-group widths multiples of 64, C_out of 128."""
    return G > 1 and cout % 128 == 0 and (cin // G) % 64 == 0 and (cout // G) % 64 == 0


def _layer64(x, lens, sd, cin, cout, k, G, res):
    t = torch.arange(x.shape[2])
    xm = x.masked_fill(t[None, None, :] >= lens[:, None, None], 0.0)
    y = F.conv1d(xm, torch.as_tensor(sd["encoder.0.mconv.0.conv.weight"]).double(), padding=k // 2, groups=G)

    def bn(z, p):
        g, b, m, v = (torch.as_tensor(sd[f"{p}.{n}"]).double() for n in ("weight", "bias", "running_mean", "running_var"))
        return (z - m[:, None]) / torch.sqrt(v[:, None] + 1e-3) * g[:, None] + b[:, None]
    y = bn(y, "encoder.0.mconv.1")
    B, C, T = y.shape
    y = y.reshape(B, G, C // G, T).transpose(1, 2).reshape(B, C, T)
    if res:
        y = y + bn(F.conv1d(xm, torch.as_tensor(sd["encoder.0.res.0.0.conv.weight"]).double()), "encoder.0.res.0.1")
    return torch.relu(y)


@pytest.mark.parametrize("layer", LAYERS, ids=[c[0] for c in LAYERS])
def test_grouped_layer_against_float64_at_every_tile(gpu, layer):
    from viet_asr_amd import asr, configs, synth
    lid, cin, cout, k, G, res = layer
    jas = [dict(filters=cout, repeat=1, kernel=[k], stride=[1], dilation=[1], dropout=0.0, residual=res, groups=G)]
    sd = synth.encoder_state_dict(jas, cin, 21)
    enc = asr.JasperEncoder(feat_in=cin, **configs.jasper_definition(jas)["JasperEncoder"])
    enc.load_state_dict({kk: torch.as_tensor(v) for kk, v in sd.items()})
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    T = 1024
    rng = np.random.default_rng(21)
    grouped = takes_grouped_gemm(cin, cout, G)
    assert grouped == (lid != "pw_g4_narrow")
    for batch in (1, 2, 8, 12, 16):
        x = np.maximum(rng.standard_normal((batch, cin, T)), 0.0).astype(np.float32)   # after a ReLU, like a block input
        lens = np.array([T - 37 * b for b in range(batch)], dtype=np.int64)
        want = _layer64(torch.from_numpy(x).double(), torch.from_numpy(lens), sd, cin, cout, k, G, res)
        scale = float(want.abs().max())
        tile = split_tile(cout, G, T, batch, cus)
        for gemm in ("f16x2", "bf16x3", "fp32"):
            h = enc._get_handle()
            h.set_gemm_mode(gemm)
            h.profile_begin()
            y, yl = enc.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu))
            torch.cuda.synchronize()
            flops = h.profile_end()["pointwise"]["flops"]
            # which form ran: the grouped GEMM reduces over C_in / G per output (1/G of the block-diagonal form's matrix
            # work); the fp32 mode and narrow groups run the block-diagonal form over all C_in
            k_red = k * (cin // G if grouped and gemm != "fp32" else cin)
            assert flops == 2.0 * k_red * cout * T * batch + (2.0 * cin * cout * T * batch if res else 0.0), (lid, gemm, flops)
            err = float((y.cpu().double() - want).abs().max())
            _record("groups_layer_f64", case=lid, batch=batch, tile="%dx%d" % SPLIT_TILES[tile], gemm=gemm, err=err, scale=scale)
            assert err <= 2e-5 * scale, (lid, batch, gemm, err, scale)
