"""-m gpu: squeeze-and-excitation JasperBlocks (csrc/encoder_se.hip; vasr_set_block_se) against the imported reference's
own batch-1 outputs (tests/golden/make_golden_se.py).

Per fixture row and arithmetic (f16x2, bf16x3, fp32), through the fused path (QuartzNetCTC.forward) and the module path
(asr.JasperEncoder -> vasr_encoder_f32 on the reference's mel, then the CTC head): log-probs within max(5e-4, 2e-5 |log-prob|),
equal encoded lengths, equal predictions except frames whose FLOAT64 top-2 margin lies inside that tolerance (counted and
asserted exactly: the fixtures have none), equal transcripts.  Then: rows of different lengths batched together in
row-independent mode against each row's own batch-1 fixture; that mode's bit-identical rows across batch compositions and
slicings; run-to-run bit equality; NaN in the padding of the encoder input reaching neither the pooled means nor any valid frame.
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
FIXTURES = ("se_15x5_rows3", "se_dense_rows3", "se_nores_k11s2_rows3")
EXPECTED_NEAR_TIES = {f: [0, 0, 0] for f in FIXTURES}      # per row: frames whose float64 margin lies inside the tolerance
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
    """Row i of fixture g against logp [T, V] / pred [T] of the same row (frames past the row's own output cut off)."""
    want = g[f"logp_{i}"][0]
    logp, pred = np.asarray(logp)[: want.shape[0]], np.asarray(pred)[: want.shape[0]]
    assert logp.shape == want.shape, (tag, logp.shape, want.shape)
    tol = _tol(want)
    err = float(np.abs(logp - want).max())
    flips = pred != g[f"pred_{i}"][0]
    _record("se_fixture", case=tag[0], gemm=tag[1], path=tag[2], row=i, err=err, tol=tol, flips=int(flips.sum()))
    assert err <= tol, (tag, i, err, tol)
    if enc_len is not None:
        assert np.float32(enc_len) == np.float32(g[f"enc_len_{i}"][0]), (tag, i)
    near = g[f"margin64_{i}"][0] < tol
    assert not (flips & ~near).any(), (tag, i, np.argwhere(flips & ~near)[:5])
    assert int(near.sum()) == EXPECTED_NEAR_TIES[tag[0]][i], (tag, i)
    if hyp is not None and not flips.any():
        assert hyp == str(g[f"hyp_{i}"][0]), (tag, i)
    return err


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
        for i, row in enumerate(rows):
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
    """Rows of different lengths in ONE call (row-independent mode: every row as its own unbatched call) against each row's
    batch-1 reference output: the time means are over each row's own frames."""
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


@pytest.mark.parametrize("gemm", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_row_independent_rows_are_bit_identical_across_batches(gpu, engines, name, gemm):
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    eng.handle.set_gemm_mode(gemm)
    one = []
    for i in range(len(rows)):
        w, l = _batch(rows, [i], gpu)
        one.append(eng.forward(w, l, want_logp=True, row_independent=True)["logp"][0])
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0, 0, 2, 1, 1, 0, 2, 2, 0, 1]):
        w, l = _batch(rows, order, gpu)
        r = eng.forward(w, l, want_logp=True, row_independent=True)
        for k, i in enumerate(order):
            f = one[i].shape[0]
            assert torch.equal(r["logp"][k, :f], one[i]), (name, gemm, order, k)
    # sliced execution (vasr_set_slices) gives the same rows
    eng.handle.set_slices(2)
    try:
        w, l = _batch(rows, [0, 1, 2, 1], gpu)
        r = eng.forward(w, l, want_logp=True, row_independent=True)
    finally:
        eng.handle.set_slices(1)
    for k, i in enumerate([0, 1, 2, 1]):
        assert torch.equal(r["logp"][k, :one[i].shape[0]], one[i]), (name, gemm, "slices", k)
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("name", FIXTURES)
def test_runs_are_bit_identical(gpu, engines, name):
    """Deterministic reductions (no float atomics): the same call twice gives the same bits, default mode, 64 rows (the
    256-channel sub-blocks not followed by an SE may take the fused kernel here)."""
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    w, l = _batch(rows, [k % 3 for k in range(64)], gpu)
    a = eng.forward(w, l, want_logp=True)["logp"].clone()
    b = eng.forward(w, l, want_logp=True)["logp"]
    assert torch.equal(a, b)


@pytest.mark.parametrize("gemm", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_nan_padding_reaches_no_pooled_mean(gpu, name, gemm):
    """Module path, three rows batched: NaN in every column past a row's length of the mel input gives the same valid
    frames, bit for bit, as zero padding -- the pooled sums read t < len only."""
    from viet_asr_amd import asr
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    enc._get_handle().set_gemm_mode(gemm)
    T = max(g[f"mel_{i}"].shape[2] for i in range(3))
    mel = np.zeros((3, 64, T), dtype=np.float32)
    seq = np.zeros(3, dtype=np.int64)
    for i in range(3):
        m = g[f"mel_{i}"][0]
        mel[i, :, : m.shape[1]] = m
        seq[i] = m.shape[1]
    poisoned = mel.copy()
    for i in range(3):
        poisoned[i, :, seq[i]:] = np.nan
    s = torch.from_numpy(seq).to(gpu)
    clean, cl = enc.forward(torch.from_numpy(mel).to(gpu), s)
    clean = clean.clone()
    dirty, dl = enc.forward(torch.from_numpy(poisoned).to(gpu), s)
    for i in range(3):
        f = int(cl[i])
        assert torch.isfinite(dirty[i, :, :f]).all(), (name, gemm, i)
        assert torch.equal(dirty[i, :, :f], clean[i, :, :f]), (name, gemm, i)
