"""-m gpu: Jasper layouts -- non-separable K-tap convolutions (implicit GEMM, csrc/encoder_pw_split.hip and encoder_pw.hip
CONV) and dense residuals -- against the imported reference's own outputs (tests/golden/make_golden_jasper.py) and the
oracle's non-separable restatement.

Per fixture and arithmetic (f16x2, bf16x3, fp32), through the fused path (QuartzNetCTC.forward) and the module path
(asr.JasperEncoder -> vasr_encoder_f32 on the reference's mel, then the CTC head): log-probs within max(5e-4, 2e-5 |log-prob|),
equal encoded lengths, equal predictions except frames whose FLOAT64 top-2 margin lies inside that tolerance (counted and
asserted exactly: the fixtures have none), equal transcripts.
"""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOGP_REL = 2e-5
LOGP_ABS = 5e-4
ARITHMETICS = ("f16x2", "bf16x3", "fp32")
FIXTURES = ("jasper_10x5dr_b2_ragged", "jasper_dr3_from_mel_b3", "jasper_k11_s2_b3", "jasper_k29_d2_b3",
            "jasper_dense_then_plain_b3")
EXPECTED_NEAR_TIES = {f: 0 for f in FIXTURES}      # frames whose float64 margin lies inside the tolerance


def _tol(logp):
    return max(LOGP_ABS, LOGP_REL * float(np.abs(np.asarray(logp)).max()))


_CACHE = {}


def _case(name):
    """(golden, definition, jasper list, encoder sd, decoder sd, signal, lengths), weights generated once per module."""
    if name not in _CACHE:
        from viet_asr_amd import configs, synth
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        src = json.loads(str(g["definition"]))
        cfg = configs.builtin(src) if isinstance(src, str) else configs.jasper_definition(src)
        jas = cfg["JasperEncoder"]["jasper"]
        seed = int(g["seed"])
        enc_sd = synth.encoder_state_dict(jas, 64, seed)
        dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, seed)
        sig, lens = synth.audio_batch(int(g["batch"]), int(g["samples"]), seed, bool(g["ragged"]))
        assert np.array_equal(lens, g["lens"])
        _CACHE[name] = (g, cfg, jas, enc_sd, dec_sd, sig, lens)
    return _CACHE[name]


def _check(tag, g, logp, pred, enc_len, hyp=None):
    logp, pred = np.asarray(logp), np.asarray(pred)
    assert logp.shape == g["logp"].shape, tag
    tol = _tol(g["logp"])
    err = float(np.abs(logp - g["logp"]).max())
    _record("jasper_fixture", case=tag[0], gemm=tag[1], path=tag[2], err=err, tol=tol, flips=int((pred != g["pred"]).sum()))
    assert err <= tol, (tag, err, tol)
    assert np.array_equal(np.asarray(enc_len, dtype=np.float32), g["enc_len"].astype(np.float32)), tag
    near = g["margin64"] < tol
    flips = pred != g["pred"]
    assert not (flips & ~near).any(), (tag, np.argwhere(flips & ~near)[:5])
    assert int(near.sum()) == EXPECTED_NEAR_TIES[tag[0]], tag
    if hyp is not None and not flips.any():
        assert list(hyp) == [str(h) for h in g["hyp"]], tag
    return err


@pytest.fixture(scope="module")
def engines(gpu):
    """One QuartzNetCTC per fixture (the arithmetic is switched on its handle)."""
    from viet_asr_amd.engine import QuartzNetCTC
    out = {}
    for name in FIXTURES:
        g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
        out[name] = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    yield out
    out.clear()


@pytest.mark.parametrize("name", FIXTURES)
def test_fused_path_matches_reference(gpu, engines, name):
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    eng = engines[name]
    for gemm in ARITHMETICS:
        eng.handle.set_gemm_mode(gemm)
        r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
        hyp = eng.texts(r["ids"], r["id_len"])
        _check((name, gemm, "fused"), g, r["logp"].cpu(), r["pred"].cpu(), r["enc_len"].cpu(), hyp)
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("name", FIXTURES)
def test_module_path_matches_reference(gpu, name):
    """asr.JasperEncoder on the reference's own mel features (vasr_encoder_f32), then asr.JasperDecoderForCTC."""
    from viet_asr_amd import asr
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec = asr.JasperDecoderForCTC(feat_in=jas[-1]["filters"], num_classes=len(cfg["labels"]))
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    mel = torch.from_numpy(g["mel"]).to(gpu)
    seq = torch.from_numpy(np.ceil(lens / 160).astype(np.int64)).to(gpu)    # get_seq_len (features.py:238-239)
    for gemm in ARITHMETICS:
        enc._get_handle().set_gemm_mode(gemm)
        dec._get_handle().set_gemm_mode(gemm)
        e, el = enc.forward(mel, seq)
        logp = dec.forward(e)
        _check((name, gemm, "module"), g, logp.cpu(), logp.argmax(-1).cpu(), el.cpu())


@pytest.mark.parametrize("name", FIXTURES)
def test_reduced_bf16x2_mode_stays_inside_ten_times_the_tolerance(gpu, engines, name):
    """The opt-in reduced arithmetic gets the check the QuartzNet fixtures apply to it (test_gpu_parity.py)."""
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    eng = engines[name]
    eng.handle.set_gemm_mode("bf16x2")
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
    eng.handle.set_gemm_mode("f16x2")
    assert np.abs(r["logp"].cpu().numpy() - g["logp"]).max() <= 10 * _tol(g["logp"])
    assert (r["pred"].cpu().numpy() == g["pred"]).all()


SHAPES = [  # (C_in, C_out, K, stride, dilation, repeat, residual)
    (64, 256, 11, 2, 1, 1, False), (256, 256, 3, 1, 1, 2, True), (384, 512, 17, 1, 1, 1, False),
    (768, 896, 29, 1, 2, 1, False), (256, 384, 13, 2, 1, 1, False), (64, 128, 5, 1, 2, 3, True)]


@pytest.mark.parametrize("shape", SHAPES)
def test_single_block_shapes_match_the_oracle(gpu, shape):
    """One non-separable block, ragged lengths, against oracle.quartznet_oracle's restatement (float32), every arithmetic."""
    from viet_asr_amd import asr, synth
    from oracle import quartznet_oracle as O
    cin, cout, k, stride, dil, rep, res = shape
    jas = [dict(filters=cout, repeat=rep, kernel=[k], stride=[stride], dilation=[dil], dropout=0.0, residual=res)]
    sd = synth.encoder_state_dict(jas, cin, 40 + k)
    enc = asr.JasperEncoder(jasper=jas, activation="relu", feat_in=cin)
    enc.load_state_dict({kk: torch.as_tensor(v) for kk, v in sd.items()})
    rng = np.random.default_rng(k)
    lens = np.array([333, 190, 97, 301], dtype=np.int64)
    x = np.zeros((4, cin, 333), dtype=np.float32)
    for b, n in enumerate(lens):
        x[b, :, :n] = rng.standard_normal((cin, n))
    want, wlen = O.encoder_forward(x, torch.from_numpy(lens), sd, jas)
    scale = float(want.abs().max())
    for gemm in ARITHMETICS:
        enc._get_handle().set_gemm_mode(gemm)
        y, yl = enc.forward(torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu))
        assert tuple(y.shape) == tuple(want.shape)
        assert np.array_equal(yl.cpu().numpy().astype(np.float32), wlen.numpy().astype(np.float32))
        err = float((y.cpu() - want).abs().max())     # (padded frames too: the reference computes them from masked inputs)
        _record("jasper_single_block", shape=list(shape), gemm=gemm, err=err, scale=scale)
        assert err <= 1e-4 * scale, (shape, gemm, err, scale)


@pytest.mark.parametrize("gemm", ["f16x2", "fp32"])
def test_row_independent_rows_are_bit_identical_across_batches(gpu, engines, gemm):
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case("jasper_dr3_from_mel_b3")
    eng = engines["jasper_dr3_from_mel_b3"]
    eng.handle.set_gemm_mode(gemm)
    full = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True, row_independent=True)
    rev = eng.forward(torch.from_numpy(sig[::-1].copy()).to(gpu), torch.from_numpy(lens[::-1].copy()).to(gpu),
                      want_logp=True, row_independent=True)
    for b in range(len(lens)):
        n = int(lens[b])
        one = eng.forward(torch.from_numpy(sig[b:b + 1, :n].copy()).to(gpu), torch.from_numpy(lens[b:b + 1]).to(gpu),
                          want_logp=True, row_independent=True)
        f = one["logp"].shape[1]
        assert torch.equal(full["logp"][b, :f], one["logp"][0]), (gemm, b)
        assert torch.equal(rev["logp"][len(lens) - 1 - b, :f], one["logp"][0]), (gemm, b)
    eng.handle.set_gemm_mode("f16x2")


def test_forward_long_equals_the_one_pass_result_in_fp32(gpu, engines):
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case("jasper_dr3_from_mel_b3")
    eng = engines["jasper_dr3_from_mel_b3"]
    eng.handle.set_gemm_mode("fp32")
    n = 40 * 16000 + 77
    x = torch.from_numpy((0.1 * np.random.default_rng(8).standard_normal(n)).astype(np.float32)).to(gpu)
    one = eng.forward(x[None], torch.tensor([n], device=gpu), want_logp=True)
    r = eng.forward_long(x, chunk_frames=1024, rows_per_pass=2, want_logp=True)
    eng.handle.set_gemm_mode("f16x2")
    assert eng.halo_mel_frames() == 36            # (5 + 6 + 7) taps either side, twice per block
    assert torch.equal(r["pred"], one["pred"])
    assert torch.equal(r["logp"], one["logp"])


# ---------------------------------------------------------------------------------------------------------------------------
# The implicit-GEMM convolution (CONV form of encoder_pw_split.hip / encoder_pw.hip) against float64, at every split tile.

SPLIT_TILES = {1: (512, 128), 2: (256, 128), 3: (128, 64), 4: (64, 32), 5: (256, 64)}    # VASR_PW3_TILE -> (rows, columns)


def split_tile(M, cols, batch, cus):
    """The tile launch_pointwise_split (encoder_pw_split.hip) picks for an M-row GEMM (M = C_out padded to 128) over `cols`
    output columns (a CONV layer's padded output frame count) of `batch` utterances, restated from its thresholds."""
    blocks = lambda bm, bn: (M // bm) * (-(-cols // bn)) * batch
    tile = 4
    if M % 512 == 0 and blocks(512, 128) >= 192:
        tile = 1
    elif M % 256 == 0 and blocks(256, 128) >= 192:
        tile = 2
    elif M % 128 == 0 and blocks(128, 64) >= 192:
        tile = 3
    if tile == 2 and M == 256 and blocks(256, 64) >= 384:
        tile = 5
    if tile == 1:
        n1 = blocks(512, 128)
        rounds = -(-n1 // cus)
        if n1 < 0.85 * rounds * cus:
            tile = 5
    return tile


def _conv_out(T, k, stride, dil):
    from oracle import quartznet_oracle as O
    pad = O.get_same_padding(k, stride, dil)
    return (T + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _edge_lengths(T, stride, k, dil):
    """Input lengths at the edges of the CONV kernel's tiles: rows of 1-3 frames (shorter than the kernel's reach), output
    lengths at and one past multiples of 32 / 64 / 128 columns -- for stride 2 also the even and odd input lengths behind
    them, where the output tile starting at ceil(L / 2) still reads valid inputs through the padding (the zero_from rule) --
    and the full width."""
    out = [1, 2, 3]
    for bn in (32, 64, 128):
        for t_out in (bn, bn + 1):
            out += [t_out] if stride == 1 else [2 * t_out - 1, 2 * t_out]
    return [n for n in out if n < T] + [T]


# (id, C_in, C_out, K, stride, dilation, residual, batch, T (input frames), input kind, tile the product picks)
# (C_out is a multiple of 128: vasr_create refuses other encoder widths, so a block's GEMM rows are never padded)
CONV_CASES = [
    ("t1_k1s2", 64, 512, 1, 2, 1, False, 128, 500, "relu", 1),
    ("t1_res", 64, 512, 3, 1, 1, True, 256, 128, "gauss", 1),
    ("t2_res", 128, 768, 5, 1, 1, True, 32, 250, "wide", 2),
    ("t2", 64, 768, 7, 2, 1, False, 32, 500, "gauss", 2),
    ("t5_m256", 64, 256, 11, 1, 1, False, 48, 500, "gauss", 5),
    ("t5_m256_res", 64, 256, 3, 1, 1, True, 48, 500, "relu", 5),
    ("t5_fill", 64, 512, 7, 2, 1, False, 40, 1200, "wide", 5),
    ("t3_d2_res", 128, 384, 13, 1, 2, True, 16, 250, "relu", 3),
    ("t3_s2", 256, 384, 11, 2, 1, False, 16, 500, "gauss", 3),
    ("t4_k29d2", 768, 512, 29, 1, 2, False, 11, 250, "gauss", 4),
    ("t4_s2", 384, 256, 17, 2, 1, False, 16, 500, "wide", 4),
    ("t4_res", 256, 256, 11, 1, 1, True, 16, 250, "relu", 4),
    ("t4_k3_res", 768, 384, 3, 1, 1, True, 12, 140, "wide", 4),
]
CONV_GEMMS = ("f16x2", "bf16x3", "bf16x2", "fp32")


def _conv_input(cid, cin, B, T, stride, k, dil, kind):
    """Rows at the edge lengths, the others at random lengths in [T/2, T]; Gaussian / ReLU'd Gaussian / "wide" (magnitudes
    2^-24 ... 2^6 inside one utterance); utterance 1 scaled by 37.5; the padding past each row's length is NOT zero (the
    kernel's length mask must hide it)."""
    rng = np.random.default_rng(sum(map(ord, cid)))
    edges = _edge_lengths(T, stride, k, dil)
    lens = np.concatenate([edges, rng.integers(T // 2, T + 1, max(0, B - len(edges)))])[:B].astype(np.int64)
    lens[rng.integers(len(edges), B) if B > len(edges) else -1] = T
    rng.shuffle(lens)
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    if kind == "relu":
        x = np.maximum(x, 0)
    if kind == "wide":
        x = x * np.exp2(rng.integers(-24, 7, x.shape)).astype(np.float32)
    x[1] *= 37.5
    return x, lens


_CONV_CACHE = {}


def _conv_case(cid):
    """(case tuple, jasper list, state dict, input, lengths, float64 reference output [B, C_out, T'] -- padded frames
    included --, reference lengths)."""
    if cid not in _CONV_CACHE:
        from viet_asr_amd import synth
        from oracle import quartznet_oracle as O
        case = next(c for c in CONV_CASES + FORCED_CASES if c[0] == cid)
        _, cin, cout, k, stride, dil, res, B, T, kind = case[:10]
        jas = [dict(filters=cout, repeat=1, kernel=[k], stride=[stride], dilation=[dil], dropout=0.0, residual=res)]
        sd = synth.encoder_state_dict(jas, cin, 70 + k)
        x, lens = _conv_input(cid, cin, B, T, stride, k, dil, kind)
        want, wlen = O.encoder_forward(x, torch.from_numpy(lens), sd, jas, dtype=torch.float64)
        _CONV_CACHE[cid] = (case, jas, sd, x, lens, want, wlen)
    return _CONV_CACHE[cid]


def _run_conv_block(gpu, jas, sd, cin, x, lens, gemms):
    """The block through asr.JasperEncoder (vasr_encoder_f32) in each arithmetic -> {gemm: (output, lengths)} on the host."""
    from viet_asr_amd import asr
    enc = asr.JasperEncoder(jasper=jas, activation="relu", feat_in=cin)
    enc.load_state_dict({kk: torch.as_tensor(v) for kk, v in sd.items()})
    xd, ld = torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu)
    out = {}
    for gemm in gemms:
        enc._get_handle().set_gemm_mode(gemm)
        y, yl = enc.forward(xd, ld)
        out[gemm] = (y.cpu(), yl.cpu())
    return out


def _check_conv_accuracy(cid, want, wlen, got, k, cin):
    """Per utterance, every frame (padded ones too -- the reference computes them from the masked inputs): the split
    arithmetics no less accurate than the fp32 MFMA chain, which stays inside fp32 round-off of a K * C_in reduction."""
    B = want.shape[0]
    errs = {}
    for gemm in ("f16x2", "bf16x3", "fp32"):
        y, yl = got[gemm]
        assert tuple(y.shape) == tuple(want.shape), (cid, gemm)
        assert np.array_equal(yl.numpy().astype(np.float32), wlen.numpy().astype(np.float32)), (cid, gemm)
        assert bool(torch.isfinite(y).all()), (cid, gemm)
        errs[gemm] = [float((y[b].double() - want[b]).abs().max()) for b in range(B)]
    top = [float(want[b].abs().max()) for b in range(B)]
    bound = lambda b: 2e-6 * (k * cin / 1024) ** 0.5 * max(1.0, top[b])
    _record("jasper_conv_f64", case=cid, **{g: max(e / bound(b) for b, e in enumerate(errs[g])) for g in errs},
            worst_f32=max(errs["fp32"]), scale=max(top))
    # The split arithmetics against the fp32 chain: over the batch, the worst error at most 1.5 x the fp32 one (+ 1e-7 of the
    # largest output).  Per utterance that rule is a comparison of two noisy maxima: on a 256-row batch of K * C_in = 192
    # (t1_res) one row measured 5.9e-6 for bf16x3 against 2.7e-6 for fp32 at magnitude 7 -- seven fp32 ulps of a
    # 256-term sum, where the three dropped bf16 cross products cost about as much as fp32 accumulation.  So per utterance
    # every arithmetic is held to the fp32 round-off bound itself.
    for gemm in ("f16x2", "bf16x3"):
        assert max(errs[gemm]) <= 1.5 * max(errs["fp32"]) + 1e-7 * max(top), (cid, gemm, max(errs["fp32"]), max(errs[gemm]))
    for b in range(B):
        for gemm in ("f16x2", "bf16x3", "fp32"):
            assert errs[gemm][b] <= bound(b), (cid, gemm, b, errs[gemm][b], bound(b))


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_gemm_against_float64_at_the_tile_the_product_picks(gpu, case):
    """One non-separable block (the CONV GEMM, with and without its residual epilogue) at batch sizes that make the PRODUCT
    pick each split tile -- 512x128, 256x128, 256x64 (both ways: 256-row layers, and 512-row ones that would not fill the
    chip's rounds), 128x64, 64x32 --, against oracle.encoder_forward in float64."""
    cid, cin, cout, k, stride, dil, res, B, T, kind, tile = case
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    m_pad = -(-cout // 128) * 128
    cols = -(-_conv_out(T, k, stride, dil) // 128) * 128          # pad_frames of the output frames
    assert split_tile(m_pad, cols, B, cus) == tile, (cid, split_tile(m_pad, cols, B, cus))
    _, jas, sd, x, lens, want, wlen = _conv_case(cid)
    got = _run_conv_block(gpu, jas, sd, cin, x, lens, CONV_GEMMS)
    _record("jasper_conv_tile", case=cid, tile=f"{SPLIT_TILES[tile][0]}x{SPLIT_TILES[tile][1]}", forced=False, batch=B)
    _check_conv_accuracy(cid, want, wlen, got, k, cin)
    # the reduced opt-in arithmetic: its own (bf16-level) bound, padded frames included
    err2 = max(float((got["bf16x2"][0][b].double() - want[b]).abs().max()) / max(1.0, float(want[b].abs().max()))
               for b in range(B))
    assert err2 <= 2e-3, (cid, err2)


# Small batches with C_out padded to 512 or 1024 rows: every VASR_PW3_TILE value applies (M % 512 == 0)
FORCED_CASES = [
    ("f_k25", 640, 512, 25, 1, 1, False, 11, 250, "wide"),
    ("f_k11s2", 64, 512, 11, 2, 1, False, 14, 300, "relu"),
    ("f_k5_res", 384, 1024, 5, 1, 1, True, 13, 140, "gauss"),
]

_FORCED_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_jasper as T
out = {{}}
for c in T.FORCED_CASES:
    _, jas, sd, x, lens, _w, _l = T._conv_case(c[0])
    got = T._run_conv_block(torch.device("cuda:0"), jas, sd, c[1], x, lens, ("f16x2", "bf16x3", "bf16x2"))
    for g, (y, yl) in got.items():
        out[c[0] + "/" + g] = y.numpy()
torch.cuda.synchronize()
np.savez({path!r}, **out)
print("FORCED_OK")
"""


def test_conv_gemm_forced_tiles_equal_the_products_choice(gpu, tmp_path):
    """Every split tile forced (VASR_PW3_TILE=1..5, read by the DEVTOOLS build only, once per process: one child process per
    tile) on small ragged batches gives the same bits as the tile the product picks, in f16x2, bf16x3 and bf16x2 -- the
    reduction order does not depend on the tile --, and the product's choice is checked against float64 here."""
    import subprocess
    import sys
    from viet_asr_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    base = {}
    for c in FORCED_CASES:
        cid, cin, cout, k, stride, dil, res, B, T, kind = c
        case, jas, sd, x, lens, want, wlen = _conv_case(cid)
        got = _run_conv_block(gpu, jas, sd, cin, x, lens, CONV_GEMMS)
        _check_conv_accuracy(cid, want, wlen, got, k, cin)
        cols = -(-_conv_out(T, k, stride, dil) // 128) * 128
        _record("jasper_conv_tile", case=cid, tile="%dx%d" % SPLIT_TILES[split_tile(-(-cout // 128) * 128, cols, B, cus)],
                forced=False, batch=B)
        for g in ("f16x2", "bf16x3", "bf16x2"):
            base[cid + "/" + g] = got[g][0].numpy()
    for tile in sorted(SPLIT_TILES):
        path = str(tmp_path / f"tile{tile}.npz")
        code = _FORCED_SNIPPET.format(tests=here, root=os.path.dirname(here), path=path)
        out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "VASR_LIB_PATH": dev, "VASR_PW3_TILE": str(tile)},
                             capture_output=True, text=True, timeout=600)
        assert "FORCED_OK" in out.stdout, (tile, out.stdout[-2000:], out.stderr[-2000:])
        forced = dict(np.load(path))
        for key, y in base.items():
            _record("jasper_conv_tile", case=key, tile="%dx%d" % SPLIT_TILES[tile], forced=True,
                    same_bits=bool(np.array_equal(forced[key], y)))
            assert np.array_equal(forced[key].view(np.uint32), y.view(np.uint32)), (tile, key)


# ---------------------------------------------------------------------------------------------------------------------------
# Jasper10x5DR at the production batch size (64 x 10 s): the 256-channel layers take 256x64 tiles, 384 / 640 / 896 128x64,
# 512 512x128 and 768 256x128 -- where a batch-1 call takes 64x32 everywhere.

B64_SAMPLES = 160000
B64_ORACLE_ROWS = 5                     # sampled rows checked against the oracle: the shortest, the longest and three others
EXPECTED_B64_NEAR_TIES = 0              # their frames whose float64 margin lies inside the tolerance (oracle only: measured)


@pytest.fixture(scope="module")
def jasper_b64(gpu):
    from viet_asr_amd import configs, synth
    from viet_asr_amd.engine import QuartzNetCTC
    cfg = configs.builtin("jasper10x5dr")
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd = synth.encoder_state_dict(jas, 64, 64)
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, 64)
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    yield cfg, jas, enc_sd, dec_sd, eng
    eng.handle.set_gemm_mode("f16x2")


def _one_row(eng, gpu, sig, n, row_independent):
    return eng.forward(torch.from_numpy(np.ascontiguousarray(sig[:n])[None]).to(gpu), torch.tensor([n], device=gpu),
                       want_logp=True, row_independent=row_independent)


@pytest.mark.parametrize("gemm", ARITHMETICS)
def test_jasper10x5dr_b64_equal_length_rows_equal_batch_1_calls(gpu, jasper_b64, gemm):
    """64 equal-length 10 s clips (the benchmark's shape: every tile but 64x32) -- each row bit-identical to the clip run
    alone (64x32 tiles everywhere): no reduction order depends on the tile or on the batch."""
    from viet_asr_amd import synth
    cfg, jas, enc_sd, dec_sd, eng = jasper_b64
    sig, lens = synth.audio_batch(64, B64_SAMPLES, 65, ragged=False)
    sig[7] *= 1e-3                                     # rows at very different levels: the fp16 split scales per utterance
    sig[40] *= 30.0
    eng.handle.set_gemm_mode(gemm)
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
    same = 0
    for b in range(64):
        one = _one_row(eng, gpu, sig[b], int(lens[b]), False)
        assert torch.equal(r["logp"][b], one["logp"][0]), (gemm, b)
        assert torch.equal(r["pred"][b], one["pred"][0]), (gemm, b)
        same += 1
    _record("jasper_b64_bits", gemm=gemm, ragged=False, rows_bit_identical=same)


_B64_ORACLE = {}


def _b64_oracle(jasper_b64):
    """Ragged 64 x 10 s batch and the oracle (float32, and float64 margins) on the sampled rows, each computed on the row
    alone -- what row-independent mode promises a row of any batch."""
    if not _B64_ORACLE:
        from viet_asr_amd import synth
        from oracle import quartznet_oracle as O
        cfg, jas, enc_sd, dec_sd, eng = jasper_b64
        sig, lens = synth.audio_batch(64, B64_SAMPLES, 66, ragged=True)
        lens[11] = 4000                                            # a row far shorter than the batch (24 mel frames)
        for b in range(64):
            sig[b, lens[b]:] = 0
        rows = sorted({int(np.argmin(lens)), int(np.argmax(lens)), 5, 30, 57})
        refs = {}
        for b in rows:
            n = int(lens[b])
            ref = O.forward_all(sig[b:b + 1, :n], lens[b:b + 1], enc_sd, dec_sd, jas)
            e64, _ = O.encoder_forward(ref["mel"], ref["seq"], enc_sd, jas, dtype=torch.float64)
            top2 = torch.topk(O.decoder_forward(e64, dec_sd), 2, dim=-1).values
            refs[b] = (ref, (top2[..., 0] - top2[..., 1]).numpy())
        _B64_ORACLE.update(sig=sig, lens=lens, refs=refs)
    return _B64_ORACLE["sig"], _B64_ORACLE["lens"], _B64_ORACLE["refs"]


@pytest.mark.parametrize("gemm", ARITHMETICS)
def test_jasper10x5dr_b64_ragged_rows_match_the_oracle(gpu, jasper_b64, gemm):
    """Ragged 64 x 10 s in row-independent mode: sampled rows (the shortest among them) against the dense-capable oracle --
    log-probs within the fixtures' tolerance, equal encoded lengths, equal predictions except frames whose float64 margin
    lies inside the tolerance (counted and asserted)."""
    cfg, jas, enc_sd, dec_sd, eng = jasper_b64
    sig, lens, refs = _b64_oracle(jasper_b64)
    eng.handle.set_gemm_mode(gemm)
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True, row_independent=True)
    near_total, worst = 0, 0.0
    for b, (ref, margin64) in refs.items():
        want = ref["logp"][0].numpy()
        f = want.shape[0]
        got = r["logp"][b, :f].cpu().numpy()
        tol = _tol(want)
        err = float(np.abs(got - want).max())
        worst = max(worst, err / tol)
        assert err <= tol, (gemm, b, err, tol)
        assert float(r["enc_len"][b]) == float(ref["enc_len"][0]), (gemm, b)
        near = margin64[0] < tol
        flips = r["pred"][b, :f].cpu().numpy() != ref["pred"][0].numpy()
        assert not (flips & ~near).any(), (gemm, b, np.argwhere(flips & ~near)[:5])
        near_total += int(near.sum())
    _record("jasper_b64_oracle", gemm=gemm, rows=sorted(refs), worst_err_over_tol=worst, near_ties=near_total)
    assert near_total == EXPECTED_B64_NEAR_TIES


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3"])
def test_jasper10x5dr_b64_ragged_rows_equal_batch_1_calls(gpu, jasper_b64, gemm):
    """Every row of the ragged 64 x 10 s batch in row-independent mode equals its batch-1 call bit for bit (the pane buffer,
    the dense-residual GEMMs and every CONV tile included)."""
    cfg, jas, enc_sd, dec_sd, eng = jasper_b64
    sig, lens, _ = _b64_oracle(jasper_b64)
    eng.handle.set_gemm_mode(gemm)
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True, row_independent=True)
    for b in range(64):
        one = _one_row(eng, gpu, sig[b], int(lens[b]), True)
        f = one["logp"].shape[1]
        assert torch.equal(r["logp"][b, :f], one["logp"][0]), (gemm, b)
        assert torch.equal(r["ids"][b, : int(one["id_len"][0])], one["ids"][0, : int(one["id_len"][0])]), (gemm, b)
    _record("jasper_b64_bits", gemm=gemm, ragged=True, rows_bit_identical=64)


@pytest.mark.parametrize("gemm", ["fp32", "bf16x3"])
def test_forward_long_on_a_strided_prologue_equals_the_one_pass_result(gpu, jasper_b64, gemm):
    """Jasper10x5DR's prologue has stride 2: forward_long's windows must start on the stride grid.  A recording with an
    odd number of mel frames (4001), windows of 512 output frames, three per pass: bit for bit the one-pass result."""
    cfg, jas, enc_sd, dec_sd, eng = jasper_b64
    eng.handle.set_gemm_mode(gemm)
    n = 40 * 16000 + 77
    assert (1 + n // 160) % 2 == 1
    x = torch.from_numpy((0.1 * np.random.default_rng(9).standard_normal(n)).astype(np.float32)).to(gpu)
    one = eng.forward(x[None], torch.tensor([n], device=gpu), want_logp=True)
    r = eng.forward_long(x, chunk_frames=512, rows_per_pass=3, want_logp=True)
    assert torch.equal(r["pred"], one["pred"])
    assert torch.equal(r["logp"], one["logp"])
    assert torch.equal(r["enc_len"], one["enc_len"])


_JASPER_ALT_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
from viet_asr_amd import configs, synth
from viet_asr_amd.engine import QuartzNetCTC
cfg = configs.builtin("jasper10x5dr")
jas = cfg["JasperEncoder"]["jasper"]
eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 67), synth.decoder_state_dict(jas[-1]["filters"], 29, 67))
sig, lens = synth.audio_batch(16, 48000, 67, ragged=True)
out = {{}}
for gemm in ("f16x2", "bf16x3", "fp32"):
    eng.handle.set_gemm_mode(gemm)
    r = eng.forward(torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda(), want_logp=True)
    out[gemm] = r["logp"].cpu().numpy()
torch.cuda.synchronize()
np.savez({path!r}, **out)
print("JASPER_ALT_OK")
"""


@pytest.mark.parametrize("env", [{}, {"VASR_SLICES": "2"}, {"VASR_NO_FUSED_RESIDUAL": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "devtools")
def test_alternate_paths_on_jasper_are_bit_identical(gpu, tmp_path, env):
    """Batch slices (16 rows: two slices of 8, each planning its own pane buffer) and the two-GEMM residual, on the DEVTOOLS
    build in a child process: the log-probs of a ragged Jasper10x5DR batch equal the product library's bit for bit."""
    import subprocess
    import sys
    from viet_asr_amd import _lib, configs, synth
    from viet_asr_amd.engine import QuartzNetCTC
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "alt.npz")
    code = _JASPER_ALT_SNIPPET.format(tests=here, root=os.path.dirname(here), path=path)
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "VASR_LIB_PATH": dev, **env}, capture_output=True,
                         text=True, timeout=600)
    assert "JASPER_ALT_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    alt = dict(np.load(path))
    cfg = configs.builtin("jasper10x5dr")
    jas = cfg["JasperEncoder"]["jasper"]
    eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 67), synth.decoder_state_dict(jas[-1]["filters"], 29, 67), device=gpu)
    sig, lens = synth.audio_batch(16, 48000, 67, ragged=True)
    for gemm in ("f16x2", "bf16x3", "fp32"):
        eng.handle.set_gemm_mode(gemm)
        r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
        assert np.array_equal(r["logp"].cpu().numpy().view(np.uint32), alt[gemm].view(np.uint32)), (env, gemm)


def test_random_jasper_layouts_in_batches_of_every_size_class(gpu):
    """Thirty cases of tests/devtools/fuzz_jasper.py: random Jasper layouts (strided or unstrided prologue, one dense run of
    1-4 blocks, optionally a plain residual block after it, filters 128-384, K 1-29, dilation 1-2, repeat 1-3) in ragged
    batches of 1-5 / 6-20 / 21-72 rows with one very short row, in a random arithmetic, against the dense-capable oracle."""
    import sys
    sys.path.insert(0, os.path.join(HERE, "devtools"))
    import fuzz_jasper
    bad = [m for m in (fuzz_jasper.jasper_case(c) for c in range(30)) if m]
    _record("jasper_fuzz", **{k: (v if not isinstance(v, list) else str(v)) for k, v in fuzz_jasper.STATS.items()})
    assert not bad, bad
    assert min(fuzz_jasper.STATS["by_batch_class"]) > 0
