"""The speech-classification path on the device (classify.hip): every fixture of tests/golden/make_golden_cls.py -- the imported
reference's own batched runs -- through the fused call (engine.QuartzNetClassifier) and the module path (asr.*) in the three
arithmetics; the pool + linear (+ softmax) kernels alone against float64 with a derived bound; the crop / pad kernel alone,
bit-equal to the torch expression of the reference; and row independence."""
import numpy as np
import pytest
import torch

import cls_reference as CR

pytestmark = pytest.mark.gpu
ARITHMETICS = ("f16x2", "bf16x3", "fp32")
EPS = 2.0 ** -24
MEL_TOL = 2e-4          # the front end's tolerance on the mel (tests/test_gpu_parity.py)


def _check(tag, g, got):
    got = got.double().cpu().numpy()
    tol = CR.tolerance(g["out64"])
    err = np.abs(got - g["out64"]).max()
    print(tag, f"max |out - out64| = {err:.3e} (tolerance {tol:.1e}), classes {got.argmax(-1).tolist()}")
    assert err <= tol, (tag, err, tol)
    assert np.abs(got - g["out"]).max() <= tol, tag
    assert np.array_equal(got.argmax(-1), g["pred64"]), tag        # every row: no row is excused


def _case(name):
    g, cfg, jas = CR.load(name)
    enc_sd, dec_sd = CR.fixture_weights(g, jas)
    sig, lens = CR.signals(g["lens"], int(g["seed"]))
    return g, cfg, jas, enc_sd, dec_sd, sig, lens


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_fused_path_matches_the_reference(gpu, name):
    from viet_asr_amd.engine import QuartzNetClassifier
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    eng = QuartzNetClassifier(cfg, enc_sd, dec_sd, int(g["audio_length"]), pooling_type=str(g["pooling_type"]))
    w, l = torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu)
    crops = g["mel_raw"].shape[-1] > int(g["audio_length"])
    for gemm in ARITHMETICS:
        eng.handle.set_gemm_mode(gemm)
        torch.manual_seed(int(g["seed"]))            # offsets=None: the reference's draw on the CPU generator
        out, mel = eng.forward(w, l, softmax=not bool(g["return_logits"]), want_mel=True)
        # the pads are exact zeros
        assert np.abs(mel.cpu().numpy() - g["mel"]).max() <= MEL_TOL, (name, gemm)
        left, right = CR.pad_split(int(g["audio_length"]), min(int(g["audio_length"]), g["mel_raw"].shape[-1]))
        assert not mel[:, :, :left].any() and not mel[:, :, mel.shape[2] - right:].any()
        _check((name, gemm, "fused"), g, out)
        if crops:                                    # an explicit array crops at the same place without the generator
            again = eng.forward(w, l, offsets=g["offsets"], softmax=not bool(g["return_logits"]))
            assert torch.equal(again, out)
    idx = eng.classify([sig[b, : lens[b]] for b in range(3)], offsets=g["offsets"] if crops else None)
    assert idx == g["pred64"].tolist()
    eng.labels = [f"c{k}" for k in range(eng.num_classes)]
    assert eng.classify([sig[b, : lens[b]] for b in range(3)], offsets=g["offsets"] if crops else None) == [f"c{k}" for k in idx]


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_module_path_matches_the_reference(gpu, name):
    """preprocessor -> crop / pad -> encoder -> decoder modules, restored from state_dicts under the reference's keys."""
    from viet_asr_amd import asr
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    pre = asr.AudioToMelSpectrogramPreprocessor(**dict(cfg["AudioToMelSpectrogramPreprocessor"], dither=0, pad_to=0))
    crop = asr.CropOrPadSpectrogramAugmentation(audio_length=int(g["audio_length"]))
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec = asr.JasperDecoderForClassification(feat_in=jas[-1]["filters"], num_classes=int(g["num_classes"]),
                                             return_logits=bool(g["return_logits"]), pooling_type=str(g["pooling_type"]))
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    mel_raw, seq = pre.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu))
    assert np.array_equal(seq.cpu().numpy(), g["seq"])
    torch.manual_seed(int(g["seed"]))
    mel, length = crop.forward(mel_raw, seq)
    # a copy with zero pads: bit-equal to the input it was cut from
    assert np.array_equal(mel.cpu().numpy(), CR.crop_or_pad(mel_raw.cpu().numpy(), int(g["audio_length"]), g["offsets"]))
    assert length.dtype == torch.int64 and length.tolist() == [int(g["audio_length"])] * 3
    assert np.abs(mel.cpu().numpy() - g["mel"]).max() <= MEL_TOL
    for gemm in ARITHMETICS:
        enc._get_handle().set_gemm_mode(gemm)
        e, _ = enc.forward(mel, length)
        _check((name, gemm, "module"), g, dec.forward(e))
    # the decoder module alone on the reference's own encoder output
    _check((name, "reference enc", "decoder"), g, dec.forward(torch.from_numpy(g["enc"]).to(gpu)))


# ---- pool + linear (+ softmax) alone against float64 ------------------------------------------------------------------------
T_GRID, K_GRID, B_GRID = (1, 2, 63, 64, 127, 128, 129, 257), (1, 2, 35, 64, 65, 130), (1, 3, 65)
_inputs = {}


def _input(C):
    """One [65][C][257] draw per width, mean -1 (an all-negative channel catches a zero-initialised maximum), shared by
    every case and never modified; the weights of the widest head, of which a head of K classes takes the first K rows."""
    if C not in _inputs:
        r = np.random.default_rng(1000 + C)
        x = (r.standard_normal((max(B_GRID), C, max(T_GRID))) - 1.0).astype(np.float32)
        x[:, ::7] = -np.abs(x[:, ::7]) - 0.5                  # every seventh channel: negative on every frame
        w = (r.standard_normal((max(K_GRID), C)) / np.sqrt(C)).astype(np.float32)
        b = r.standard_normal(max(K_GRID)).astype(np.float32)
        _inputs[C] = (x, w, b, {})
    return _inputs[C]


def _pooled64(C, T, pooling):
    """(pooled, P) in float64 at B = 65: the pool, and the magnitude the bound is built from -- the mean of |x| for avg,
    |max x| for max."""
    x, _, _, cache = _input(C)
    if (T, pooling) not in cache:
        v = x[:, :, :T].astype(np.float64)
        cache[(T, pooling)] = (v.mean(-1), np.abs(v).mean(-1)) if pooling == "avg" else (v.max(-1), np.abs(v.max(-1)))
    return cache[(T, pooling)]


@pytest.mark.parametrize("pooling", ["avg", "max"])
@pytest.mark.parametrize("C", [128, 1024])
def test_classifier_kernels_against_float64(gpu, C, pooling):
    """First-order worst case of ANY fp32 summation order: with S_k = |b_k| + sum_c |W_kc| P_c, |err_k| <= (T' + C + 8) eps S_k
    for avg and (C + 8) eps S_k for max (the pooled maximum is exact), eps = 2^-24, 8 for the division, bias, fused multiply
    and second-order terms; softmax within 2 max_k(bound_k) + 8 eps of the float64 softmax of the float64 logits."""
    from viet_asr_amd import _lib, stages
    x, w, b, _ = _input(C)
    xd = torch.from_numpy(x).to(gpu)
    worst = 0.0
    for K in K_GRID:
        h = _lib.Handle(classifier=(C, K, 0 if pooling == "avg" else 1))
        h.load_state_dict({"decoder_layers.0.weight": w[:K], "decoder_layers.0.bias": b[:K]})
        h.finalize()
        w64, b64 = w[:K].astype(np.float64), b[:K].astype(np.float64)
        for T in T_GRID:
            pooled, P = _pooled64(C, T, pooling)
            logits64 = pooled @ w64.T + b64
            S = np.abs(b64) + P @ np.abs(w64).T
            bound = ((T + C + 8) if pooling == "avg" else (C + 8)) * EPS * S
            e = np.exp(logits64 - logits64.max(-1, keepdims=True))
            prob64 = e / e.sum(-1, keepdims=True)
            if pooling == "max":
                assert (pooled[:, ::7] < 0).all()
            for B in B_GRID:
                xin = xd[:B, :, :T].contiguous()
                got = stages.classifier(h, xin, softmax=False).double().cpu().numpy()
                err = np.abs(got - logits64[:B])
                worst = max(worst, float((err / bound[:B]).max()))
                assert (err <= bound[:B]).all(), (C, pooling, K, T, B, float((err / bound[:B]).max()))
                gotp = stages.classifier(h, xin, softmax=True).double().cpu().numpy()
                pb = 2 * bound[:B].max(-1, keepdims=True) + 8 * EPS
                assert (np.abs(gotp - prob64[:B]) <= pb).all(), (C, pooling, K, T, B, float(np.abs(gotp - prob64[:B]).max()))
        h.close()
    print(f"C={C} {pooling}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("pooling", ["avg", "max"])
def test_classifier_rows_do_not_depend_on_the_batch(gpu, pooling):
    """A row's logits (and probabilities) are bit-equal at B = 1, B = 3 and inside B = 65, and from one call to the next."""
    from viet_asr_amd import _lib, stages
    C, K = 1024, 130
    x, w, b, _ = _input(C)
    h = _lib.Handle(classifier=(C, K, 0 if pooling == "avg" else 1))
    h.load_state_dict({"decoder_layers.0.weight": w[:K], "decoder_layers.0.bias": b[:K]})
    h.finalize()
    xd = torch.from_numpy(x).to(gpu)
    for T in (1, 63, 129, 257):
        for softmax in (False, True):
            full = stages.classifier(h, xd[:, :, :T].contiguous(), softmax=softmax).clone()
            assert torch.equal(full, stages.classifier(h, xd[:, :, :T].contiguous(), softmax=softmax))
            for rows in ([0], [64], [17], [5, 64, 0]):
                part = stages.classifier(h, xd[rows][:, :, :T].contiguous(), softmax=softmax)
                assert torch.equal(part, full[rows]), (pooling, T, softmax, rows)
    h.close()


# ---- crop / pad alone -------------------------------------------------------------------------------------------------------
def _reference_crop_or_pad(image, audio_length, offset):
    """The reference's forward (audio_preprocessing.py:681-712) in torch, with the offsets handed in."""
    image_len = image.shape[-1]
    if image_len > audio_length:
        return torch.cat([image[i : i + 1, :, o : o + audio_length] for i, o in enumerate(offset.tolist())], dim=0)
    pad_left = pad_right = (audio_length - image_len) // 2
    if (audio_length - image_len) % 2 == 1:
        pad_right += 1
    return torch.nn.functional.pad(image, [pad_left, pad_right], mode="constant", value=0)


@pytest.mark.parametrize("F", [64, 192])
def test_crop_or_pad_kernel_is_bit_equal_to_the_reference_expression(gpu, F):
    from viet_asr_amd import stages
    B = 3
    r = np.random.default_rng(F)
    for T in (1, 127, 128, 129, 300):
        x = torch.from_numpy(r.standard_normal((B, F, T)).astype(np.float32))
        xd = x.to(gpu)
        for A in (1, 128):
            hi = T - A
            cases = [None] if hi <= 0 else [torch.zeros(B, dtype=torch.int64), torch.full((B,), hi, dtype=torch.int64),
                                            torch.tensor([hi // 3, hi, 0], dtype=torch.int64)]
            for off in cases:
                got, length = stages.crop_or_pad(xd, A, off)
                assert got.shape == (B, F, A) and length.tolist() == [A] * B and length.dtype == torch.int64
                assert torch.equal(got.cpu(), _reference_crop_or_pad(x, A, off)), (F, T, A, off)
    with pytest.raises(ValueError):
        stages.crop_or_pad(torch.zeros((2, F, 9), device=gpu), 4)        # a crop without offsets


def test_crop_module_draws_like_the_reference(gpu):
    """After the same torch.manual_seed the module crops where the reference's expression crops."""
    from viet_asr_amd import asr
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((5, 64, 301)).astype(np.float32))
    crop = asr.CropOrPadSpectrogramAugmentation(audio_length=128)
    torch.manual_seed(77)
    got, length = crop.forward(x.to(gpu), torch.tensor([301, 200, 250, 13, 301], device=gpu))
    torch.manual_seed(77)
    off = torch.randint(low=0, high=301 - 128 + 1, size=[5])
    assert torch.equal(got.cpu(), _reference_crop_or_pad(x, 128, off)) and length.tolist() == [128] * 5


# ---- row independence of the fused path --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cls_pad_avg_rows3", "cls_crop_max_selu_rows3"])
def test_fused_rows_do_not_depend_on_the_batch(gpu, name):
    """row_independent=True: a row's output is bit-equal alone and in a ragged batch, in the arithmetics in which
    QuartzNetCTC promises the same (f16x2 and fp32); each row is cut or centred on its OWN width."""
    from viet_asr_amd.engine import QuartzNetClassifier
    g, cfg, jas, enc_sd, dec_sd, sig, lens = _case(name)
    A = int(g["audio_length"])
    eng = QuartzNetClassifier(cfg, enc_sd, dec_sd, A, pooling_type=str(g["pooling_type"]))
    off = [max(0, min(o, 1 + int(n) // 160 - A)) for o, n in zip((1, 3, 19), lens)]     # valid inside each row's own width
    for gemm in ("f16x2", "fp32"):
        eng.handle.set_gemm_mode(gemm)
        one = []
        for b in range(3):
            w = torch.from_numpy(sig[b : b + 1, : lens[b]].copy()).to(gpu)
            out, mel = eng.forward(w, torch.tensor([lens[b]], device=gpu), offsets=[off[b]], row_independent=True, want_mel=True)
            one.append((out[0].clone(), mel[0].clone()))
        for order in ([0, 1, 2], [2, 1, 0, 0, 1]):
            L = max(int(lens[i]) for i in order)
            w = np.zeros((len(order), L), dtype=np.float32)
            for k, i in enumerate(order):
                w[k, : lens[i]] = sig[i, : lens[i]]
            out, mel = eng.forward(torch.from_numpy(w).to(gpu), torch.tensor([int(lens[i]) for i in order], device=gpu),
                                   offsets=[off[i] for i in order], row_independent=True, want_mel=True)
            for k, i in enumerate(order):
                assert torch.equal(mel[k], one[i][1]), (name, gemm, order, k)
                assert torch.equal(out[k], one[i][0]), (name, gemm, order, k)
