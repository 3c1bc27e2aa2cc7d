"""-m gpu: GroupNorm JasperEncoders (csrc/encoder_norm.hip; vasr_set_block_norm) against the imported reference's own
batch-1 outputs (tests/golden/make_golden_norm.py), and the two device passes in isolation against float64.

Per fixture row and arithmetic (f16x2, bf16x3, fp32), through the fused path (QuartzNetCTC.forward) and the module path
(asr.JasperEncoder -> vasr_encoder_f32 on the reference's mel, then the CTC head): log-probs within max(5e-4, 2e-5 |log-prob|),
equal encoded lengths, equal predictions except frames whose FLOAT64 top-2 margin lies inside that tolerance, equal
transcripts.  Then: rows of different lengths batched together in row-independent mode against each row's own batch-1
fixture; that mode's bit-identical rows across batch compositions and slicings; run-to-run bit equality; NaN in the padding of
the encoder input reaching no statistic.  vasr_bench_groupnorm (devtools): row lengths 0 / 1 / 63 / 64 / 65 / 3001, 64 to 1024
channels, 1 group, one per channel and in between, with and without a channel shuffle, and a mean / std ratio of 1e3.
"""
import ctypes as C
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
FIXTURES = ("norm_15x5_group32_rows3", "norm_dense_layer_rows3", "norm_se_instance_rows3", "norm_groups_group8_rows3")
HOP = 160

_CACHE = {}


def _tol(logp):
    return max(LOGP_ABS, LOGP_REL * float(np.abs(np.asarray(logp)).max()))


def _case(name):
    """(golden, definition, jasper list, encoder sd, decoder sd, [row signals], lengths)."""
    if name not in _CACHE:
        from viet_asr_amd import configs, engine, synth
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        jas = json.loads(str(g["definition"]))
        cfg = configs.jasper_definition(jas)
        cfg["JasperEncoder"].update(normalization_mode=str(g["normalization_mode"]), norm_groups=int(g["norm_groups"]))
        seed = int(g["seed"])
        lens = g["lens"].astype(np.int64)
        enc_sd = synth.encoder_state_dict(jas, 64, seed, norm=engine.norm_from_config(cfg["JasperEncoder"], jas))
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
    _record("norm_fixture", case=tag[0], gemm=tag[1], path=tag[2], row=i, err=err, tol=tol, flips=int(flips.sum()))
    assert err <= tol, (tag, i, err, tol)
    if enc_len is not None:
        assert np.float32(enc_len) == np.float32(g[f"enc_len_{i}"][0]), (tag, i)
    near = g[f"margin64_{i}"][0] < tol
    assert not (flips & ~near).any(), (tag, i, np.argwhere(flips & ~near)[:5])
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
    """Rows of different lengths in ONE call (row-independent mode) against each row's batch-1 reference output: the
    statistics are over each row's own frames."""
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
    """Deterministic reductions (no atomics): the same call twice gives the same bits, default mode, 64 rows."""
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    w, l = _batch(rows, [k % 3 for k in range(64)], gpu)
    a = eng.forward(w, l, want_logp=True)["logp"].clone()
    b = eng.forward(w, l, want_logp=True)["logp"]
    assert torch.equal(a, b)


@pytest.mark.parametrize("gemm", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", FIXTURES)
def test_nan_padding_reaches_no_statistic(gpu, name, gemm):
    """Module path, three rows batched: NaN in every column past a row's length of the mel input gives the same valid
    frames, bit for bit, as zero padding -- the statistics read t < len only."""
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


# ---- the two passes in isolation (vasr_bench_groupnorm) against float64 --------------------------------------------------

LENS = [0, 1, 63, 64, 65, 3001]


def _groupnorm64(x, lens, G, shuffle, gamma, beta, relu):
    """float64: x [B][C][T] stored AFTER a GroupShuffle(shuffle); statistics per pre-shuffle group over t < lens[b]."""
    B, Cn, T = x.shape
    mg = Cn // shuffle
    perm = np.array([(p % mg) * shuffle + p // mg for p in range(Cn)])    # pre-shuffle channel p is stored at perm[p]
    y = np.zeros_like(x, dtype=np.float64)
    for b in range(B):
        n = min(int(lens[b]), T)
        if n == 0:
            continue
        pre = x[b, perm, :n].astype(np.float64).reshape(G, Cn // G, n)
        mean = pre.mean(axis=(1, 2), keepdims=True)
        var = ((pre - mean) ** 2).mean(axis=(1, 2), keepdims=True)
        v = ((pre - mean) / np.sqrt(var + 1e-5)).reshape(Cn, n) * gamma[:, None] + beta[:, None]
        if relu:
            v = np.maximum(v, 0.0)
        y[b, perm, :n] = v
    return y


def _bench(gpu, x, lens, G, shuffle, gamma, beta, relu):
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    B, Cn, T = x.shape
    ld = (T + 127) // 128 * 128
    xd = torch.full((B, Cn, ld), float("nan"), dtype=torch.float32, device=gpu)
    xd[:, :, :T] = torch.from_numpy(x).to(gpu)
    for b in range(B):
        xd[b, :, int(lens[b]):] = float("nan")          # no statistic may read past a row's length
    yd = torch.full_like(xd, float("nan"))
    ld_t = torch.tensor(np.minimum(lens, T), dtype=torch.int32, device=gpu)
    g32, b32 = np.ascontiguousarray(gamma, np.float32), np.ascontiguousarray(beta, np.float32)
    st = torch.cuda.current_stream().cuda_stream
    rc = L.vasr_bench_groupnorm(C.c_void_p(xd.data_ptr()), C.c_void_p(ld_t.data_ptr()), B, Cn, T, G, shuffle,
                                g32.ctypes.data_as(C.c_void_p), b32.ctypes.data_as(C.c_void_p), int(relu),
                                C.c_void_p(yd.data_ptr()), C.c_void_p(st))
    _lib.check(rc, L)
    return yd.cpu().numpy()


@pytest.mark.parametrize("C_,G,shuffle", [(64, 1, 1), (64, 64, 1), (256, 8, 4), (256, 32, 1), (512, 1, 4), (512, 512, 2),
                                          (1024, 32, 8), (1024, 1024, 1), (1024, 16, 1)])
def test_isolated_passes_match_float64(gpu, C_, G, shuffle):
    rng = np.random.default_rng(C_ * 7 + G)
    T = max(LENS)
    lens = np.array(LENS, dtype=np.int64)
    x = (rng.normal(0, 2.0, size=(len(LENS), C_, T)) + rng.normal(0, 3.0, size=(1, C_, 1))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, size=C_)
    beta = rng.normal(0, 0.3, size=C_)
    for relu in (0, 1):
        y = _bench(gpu, x, lens, G, shuffle, gamma, beta, relu)
        want = _groupnorm64(x, lens, G, shuffle, gamma.astype(np.float32), beta.astype(np.float32), relu)
        for b, n in enumerate(LENS):
            assert np.isfinite(y[b]).all(), (C_, G, shuffle, n)
            assert (y[b, :, n:] == 0).all(), (C_, G, shuffle, n)          # zero past the row, zeros for an empty row
            err = float(np.abs(y[b, :, :n] - want[b, :, :n]).max()) if n else 0.0
            assert err <= 2e-5 * max(1.0, float(np.abs(want[b]).max())) * 8, (C_, G, shuffle, n, err)


def test_isolated_passes_are_centred(gpu):
    """Mean / std of 1e3: E[x^2] - E[x]^2 in fp32 loses the variance entirely (O(1) error after normalization); the
    two-pass form and the centred merge stay within 1e-2 (in fact near fp32 round-off of the mean)."""
    rng = np.random.default_rng(5)
    Cn, G = 256, 8
    lens = np.array([3001, 777], dtype=np.int64)
    x = (1000.0 + rng.normal(0, 1.0, size=(2, Cn, 3001))).astype(np.float32)
    gamma, beta = np.ones(Cn), np.zeros(Cn)
    y = _bench(gpu, x, lens, G, 4, gamma, beta, 0)
    want = _groupnorm64(x, lens, G, 4, gamma, beta, 0)
    for b, n in enumerate(lens):
        err = float(np.abs(y[b, :, :n] - want[b, :, :n]).max())
        assert err < 1e-2, (b, err)
