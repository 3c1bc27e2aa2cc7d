"""-m gpu: JasperEncoders with a hardtanh or SELU activation and / or residual_mode "max" (vasr_set_activation) against the
imported reference's own batch-1 outputs (tests/golden/make_golden_act.py).

Per fixture row and arithmetic (f16x2, bf16x3, fp32), through the fused path (QuartzNetCTC.forward) and the module path
(asr.JasperEncoder -> vasr_encoder_f32 on the reference's mel, then the CTC head): log-probs within max(5e-4, 2e-5 |log-prob|),
equal encoded lengths, equal predictions except frames whose FLOAT64 top-2 margin lies inside that tolerance, equal
transcripts.  Then: rows of different lengths batched together in row-independent mode against each row's own batch-1
fixture; that mode's bit-identical rows across batch compositions; run-to-run bit equality; NaN in the padding of the encoder
input reaching no output under a max residual (fmaxf and torch.max treat NaN differently); QuartzNet15x5 at 64 x 10 s with
hardtanh and SELU on the fused depthwise + pointwise kernel against batch-1 calls and against the two-kernel form
(VASR_FUSED=0, devtools build); forward_long against the one-pass result on a SELU + max model.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOGP_REL = 2e-5
LOGP_ABS = 5e-4
ARITHMETICS = ("f16x2", "bf16x3", "fp32")
FIXTURES = ("act_15x5_selu_add_rows3", "act_15x5_hardtanh_max_rows3", "act_dense_selu_max_rows3",
            "act_dense_se_relu_max_rows3", "act_conv_selu_add_rows3", "act_groups_se_hardtanh_group_rows3")
MAX_FIXTURES = tuple(n for n in FIXTURES if "_max_" in n)
HOP = 160

_CACHE = {}


def _tol(logp):
    return max(LOGP_ABS, LOGP_REL * float(np.abs(np.asarray(logp)).max()))


def _definition(jas, activation, residual_mode, mode="batch", norm_groups=-1):
    from viet_asr_amd import configs
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(activation=activation, residual_mode=residual_mode, normalization_mode=mode,
                                norm_groups=norm_groups)
    return cfg


def _case(name):
    """(golden, definition, jasper list, encoder sd, decoder sd, [row signals], lengths)."""
    if name not in _CACHE:
        from viet_asr_amd import engine, synth
        g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
        jas = json.loads(str(g["definition"]))
        cfg = _definition(jas, str(g["activation"]), str(g["residual_mode"]), str(g["normalization_mode"]),
                          int(g["norm_groups"]))
        seed = int(g["seed"])
        lens = g["lens"].astype(np.int64)
        enc_sd = synth.scale_conv_weights(
            synth.encoder_state_dict(jas, 64, seed, norm=engine.norm_from_config(cfg["JasperEncoder"], jas)), float(g["gain"]))
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
    _record("act_fixture", case=tag[0], gemm=tag[1], path=tag[2], row=i, err=err, tol=tol, flips=int(flips.sum()))
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
    """Rows of different lengths in ONE call (row-independent mode) against each row's batch-1 reference output."""
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


@pytest.mark.parametrize("gemm", ["f16x2", "fp32"])
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
    eng.handle.set_gemm_mode("f16x2")


@pytest.mark.parametrize("name", FIXTURES)
def test_runs_are_bit_identical(gpu, engines, name):
    """The same call twice gives the same bits, default mode, 64 rows."""
    g, cfg, jas, enc_sd, dec_sd, rows, lens = _case(name)
    eng = engines[name]
    w, l = _batch(rows, [k % 3 for k in range(64)], gpu)
    a = eng.forward(w, l, want_logp=True)["logp"].clone()
    b = eng.forward(w, l, want_logp=True)["logp"]
    assert torch.equal(a, b)


@pytest.mark.parametrize("gemm", ["f16x2", "fp32"])
@pytest.mark.parametrize("name", MAX_FIXTURES)
def test_nan_padding_reaches_no_output_under_max(gpu, name, gemm):
    """Module path, three rows batched: NaN in every column past a row's length of the mel input gives the same valid
    frames, bit for bit, as zero padding.  fmaxf(NaN, x) = x while torch.max propagates NaN, so a poisoned pane that reached
    the max would show up here as a difference (or as NaN), not be hidden by either convention."""
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


# ---- QuartzNet15x5 at 64 x 10 s: the fused depthwise + pointwise kernel with a non-ReLU activation -----------------------

_B64 = {}
# conv weight gains that keep the 54-layer model contracting under each activation (make_golden_act.py's 15x5 cases)
B64_GAIN = {"hardtanh": 0.85, "selu": 0.8}


def _b64_model(gpu, activation):
    if activation not in _B64:
        from viet_asr_amd import configs, synth
        from viet_asr_amd.engine import QuartzNetCTC
        jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
        cfg = _definition(jas, activation, "add")
        enc_sd = synth.scale_conv_weights(synth.encoder_state_dict(jas, 64, 81), B64_GAIN[activation])
        dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, 81)
        _B64[activation] = (QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu), cfg, enc_sd, dec_sd)
    return _B64[activation]


_FUSED_OFF_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
from viet_asr_amd import configs, synth
from viet_asr_amd.engine import QuartzNetCTC
import test_gpu_act as T
gpu = torch.device("cuda:0")
jas = configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]
cfg = T._definition(jas, {act!r}, "add")
enc_sd = synth.scale_conv_weights(synth.encoder_state_dict(jas, 64, 81), T.B64_GAIN[{act!r}])
eng = QuartzNetCTC(cfg, enc_sd, synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, 81), device=gpu)
sig, lens = synth.audio_batch(64, 160000, 82, ragged=False)
eng.handle.profile_begin()
r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
torch.cuda.synchronize()
fused = eng.handle.profile_end()["fused"]["launches"]
np.savez({path!r}, logp=r["logp"].cpu().numpy(), fused=np.array(fused))
print("FUSED_OFF_OK")
"""


@pytest.mark.parametrize("activation", ["hardtanh", "selu"])
def test_15x5_b64_runs_the_fused_kernel_and_matches_batch1_and_two_kernels(gpu, tmp_path, activation):
    from viet_asr_amd import _lib, synth
    eng, cfg, enc_sd, dec_sd = _b64_model(gpu, activation)
    sig, lens = synth.audio_batch(64, 160000, 82, ragged=False)
    eng.handle.profile_begin()
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
    torch.cuda.synchronize()
    fused = int(eng.handle.profile_end()["fused"]["launches"])
    assert fused > 0, activation                               # 64 x 10 s: the 256-channel sub-blocks take the fused kernel
    logp = r["logp"].cpu().numpy()
    worst = 0.0
    for b in range(64):
        one = eng.forward(torch.from_numpy(sig[b:b + 1]).to(gpu), torch.from_numpy(lens[b:b + 1]).to(gpu), want_logp=True)
        want = one["logp"][0].cpu().numpy()
        tol = _tol(want)
        err = float(np.abs(logp[b] - want).max())
        worst = max(worst, err / tol)
        assert err <= tol, (activation, b, err, tol)
    _record("act_b64_vs_batch1", activation=activation, fused_launches=fused, worst_err_over_tol=worst)
    # the two-kernel form of the same batch (devtools build, VASR_FUSED=0)
    path = str(tmp_path / "fused_off.npz")
    code = _FUSED_OFF_SNIPPET.format(tests=HERE, root=os.path.dirname(HERE), path=path, act=activation)
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "VASR_LIB_PATH": dev, "VASR_FUSED": "0"},
                         capture_output=True, text=True, timeout=600)
    assert "FUSED_OFF_OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    alt = dict(np.load(path))
    assert int(alt["fused"]) == 0
    err = float(np.abs(alt["logp"] - logp).max())
    tol = _tol(logp)
    _record("act_b64_vs_two_kernels", activation=activation, err=err, tol=tol)
    assert err <= tol, (activation, err, tol)


def test_forward_long_equals_the_one_pass_result_in_fp32(gpu, engines):
    """A SELU + max dense-residual model is local in time: forward_long's windows give the one-pass log-probs bit for bit in
    fp32."""
    eng = engines["act_dense_selu_max_rows3"]
    n = 25 * 16000 + 77
    x = torch.from_numpy((0.1 * np.random.default_rng(9).standard_normal(n)).astype(np.float32)).to(gpu)
    eng.handle.set_gemm_mode("fp32")
    try:
        one = eng.forward(x[None], torch.tensor([n], device=gpu), want_logp=True)
        r = eng.forward_long(x, chunk_frames=256, rows_per_pass=2, want_logp=True)
    finally:
        eng.handle.set_gemm_mode("f16x2")
    assert torch.equal(r["pred"], one["pred"])
    assert torch.equal(r["logp"], one["logp"])
