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
