"""CPU checks of the speech-classification path: JasperDecoderForClassification and CropOrPadSpectrogramAugmentation (ports,
state_dict layout against the reference's own -- tests/golden/cls_*_state_dict_keys.json, written by make_golden_cls.py --,
the reference's ValueError, the offsets drawn after torch.manual_seed, the pad split), the vasr_set_classifier / vasr_finalize
refusals before anything touches a device, the exported symbols and the ABI version, and the float64 restatement of
crop / pad + pool + linear + softmax (tests/cls_reference.py) against every fixture's float64 output."""
import json
import os

import numpy as np
import pytest

import cls_reference as CR

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_SYMBOLS = ("vasr_set_classifier", "vasr_crop_or_pad_f32", "vasr_classifier_f32", "vasr_classify_f32",
               "vasr_classify_workspace_bytes")
_JAS = [dict(filters=256, repeat=1, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True),
        dict(filters=128, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]


def _decoder(g, **over):
    from viet_asr_amd import asr
    kw = dict(feat_in=int(g["enc"].shape[1]), num_classes=int(g["num_classes"]), return_logits=bool(g["return_logits"]),
              pooling_type=str(g["pooling_type"]))
    kw.update(over)
    return asr.JasperDecoderForClassification(**kw)


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_state_dict_keys_equal_the_reference_layout(name):
    from viet_asr_amd import asr
    g, cfg, jas = CR.load(name)
    with open(os.path.join(HERE, "golden", name.replace("_rows3", "") + "_state_dict_keys.json")) as f:
        want = json.load(f)
    dec = _decoder(g)
    assert {k: list(v.shape) for k, v in dec.state_dict().items()} == want["decoder"]
    assert list(dec.state_dict()) == ["decoder_layers.0.weight", "decoder_layers.0.bias"] and dec.state_dict()["decoder_layers.0.weight"].dim() == 2
    enc = asr.JasperEncoder(feat_in=64, **cfg["JasperEncoder"])
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == want["encoder"]
    enc_sd, dec_sd = CR.fixture_weights(g, jas)
    assert {k: list(np.shape(v)) for k, v in dec_sd.items()} == want["decoder"]
    assert {k: list(np.shape(v)) for k, v in enc_sd.items()} == want["encoder"]


def test_ports_are_the_references():
    from viet_asr_amd import asr, core
    dec = asr.JasperDecoderForClassification(feat_in=128, num_classes=5)
    assert list(dec.input_ports) == ["encoder_output"] and list(dec.output_ports) == ["logits"]
    assert dec.input_ports["encoder_output"].axes == ("B", "D", "T")
    assert isinstance(dec.input_ports["encoder_output"].elements_type, core.AcousticEncodedRepresentation)
    assert dec.output_ports["logits"].axes == ("B", "D") and isinstance(dec.output_ports["logits"].elements_type, core.LogitsType)
    crop = asr.CropOrPadSpectrogramAugmentation(audio_length=128)
    assert list(crop.input_ports) == ["input_signal", "length"] and list(crop.output_ports) == ["processed_signal", "processed_length"]
    for ports, sig, ln in ((crop.input_ports, "input_signal", "length"), (crop.output_ports, "processed_signal", "processed_length")):
        assert ports[sig].axes == ("B", "D", "T") and type(ports[sig].elements_type) is core.SpectrogramType
        assert ports[ln].axes == ("B",) and isinstance(ports[ln].elements_type, core.LengthsType)
    assert {"JasperDecoderForClassification", "CropOrPadSpectrogramAugmentation"} <= set(asr.__all__)


def test_bad_pooling_type_raises_the_references_error():
    from viet_asr_amd import asr
    with pytest.raises(ValueError) as e:
        asr.JasperDecoderForClassification(feat_in=128, num_classes=5, pooling_type="sum")
    assert str(e.value) == "Pooling type chosen is not valid. Must be either `avg` or `max`"
    for p in ("avg", "max"):
        asr.JasperDecoderForClassification(feat_in=128, num_classes=5, pooling_type=p)
    with pytest.raises(TypeError):
        asr.JasperDecoderForClassification(128, 5)      # keyword-only, as in the reference


def test_forward_on_cpu_tensors_raises():
    import torch
    from viet_asr_amd import _lib, asr
    # CPU tensors are refused whether or not a device is present: there is no CPU fallback
    with pytest.raises(_lib.VasrError):
        asr.JasperDecoderForClassification(feat_in=128, num_classes=5).forward(torch.zeros(1, 128, 4))
    with pytest.raises(_lib.VasrError):
        asr.CropOrPadSpectrogramAugmentation(8).forward(torch.zeros(1, 64, 4), torch.tensor([4]))


def test_offsets_are_the_references_draw():
    """After the same torch.manual_seed the module draws the offsets the reference drew (stored in the crop fixture)."""
    import torch
    from viet_asr_amd import asr
    g, _, _ = CR.load("cls_crop_max_selu_rows3")
    crop = asr.CropOrPadSpectrogramAugmentation(audio_length=int(g["audio_length"]))
    torch.manual_seed(int(g["seed"]))
    off = crop.draw_offsets(len(g["lens"]), g["mel_raw"].shape[-1])
    assert off.dtype == torch.int64 and off.tolist() == g["offsets"].tolist()
    hi = g["mel_raw"].shape[-1] - int(g["audio_length"])
    assert len(set(off.tolist())) > 1 and any(0 < o < hi for o in off.tolist())
    # no draw (the generator is left alone) when nothing is cropped
    state = torch.get_rng_state()
    assert crop.draw_offsets(3, int(g["audio_length"])) is None and crop.draw_offsets(3, 5) is None
    assert torch.equal(state, torch.get_rng_state())


def test_pad_split_puts_the_odd_frame_right():
    from viet_asr_amd import asr
    for a, t in ((128, 101), (128, 100), (128, 128), (128, 127), (1, 1), (7, 2), (6, 2)):
        d = a - t
        assert asr.crop_or_pad_split(a, t) == (d // 2, d - d // 2) == CR.pad_split(a, t)
        left, right = asr.crop_or_pad_split(a, t)
        assert left + right + t == a and right - left == d % 2
    with pytest.raises(ValueError):
        asr.crop_or_pad_split(4, 5)


def test_set_classifier_and_finalize_refusals():
    """Raised with no device present: VASR_ERR_INVALID (-1) for a CTC head on the same handle, a pooling code out of range,
    feat_in or num_classes <= 0 and a weight of the wrong shape; VASR_ERR_STATE (-2) for a missing weight at finalize;
    VASR_ERR_UNSUPPORTED (-5) for feat_in > 1024."""
    from viet_asr_amd import _lib, engine, synth
    L = _lib.lib()
    h = _lib.Handle(dec_feat_in=128, num_classes=5)
    assert L.vasr_set_classifier(h.h, 128, 5, 0) == -1 and "CTC head" in L.vasr_last_error().decode()
    h.close()
    h = _lib.Handle()
    for args in ((128, 5, 2), (128, 5, -1), (0, 5, 0), (-3, 5, 0), (128, 0, 0), (128, -1, 1)):
        assert L.vasr_set_classifier(h.h, *args) == -1, args
    assert L.vasr_set_classifier(h.h, 1025, 5, 0) == -5
    for pool in (0, 1):
        assert L.vasr_set_classifier(h.h, 1024, 2048, pool) == 0
    h.close()
    with pytest.raises(ValueError):
        _lib.Handle(classifier=(128, 5, 7))
    with pytest.raises(NotImplementedError):
        _lib.Handle(classifier=(2048, 5, 0))
    sd = synth.classifier_state_dict(128, 5, 1)
    # missing weights: STATE
    for drop in ("decoder_layers.0.weight", "decoder_layers.0.bias"):
        h = _lib.Handle(classifier=(128, 5, 0))
        h.load_state_dict({k: v for k, v in sd.items() if k != drop})
        assert L.vasr_finalize(h.h) == -2 and drop in L.vasr_last_error().decode()
        h.close()
    # wrong shapes: INVALID -- a transposed weight, a Conv1d's 3-D weight (the CTC head's layout), another class count
    w, b = sd["decoder_layers.0.weight"], sd["decoder_layers.0.bias"]
    for bad in ({"decoder_layers.0.weight": np.ascontiguousarray(w.T)}, {"decoder_layers.0.weight": w[:, :, None]},
                {"decoder_layers.0.weight": w[:4]}, {"decoder_layers.0.bias": b[:4]}, {"decoder_layers.0.bias": b[None]}):
        h = _lib.Handle(classifier=(128, 5, 1))
        h.load_state_dict({**sd, **bad})
        assert L.vasr_finalize(h.h) == -1, {k: v.shape for k, v in bad.items()}
        h.close()
    # a classifier that does not read what the encoder writes: INVALID
    h = _lib.Handle(feat_in=64, blocks=engine.blocks_from_config(_JAS), classifier=(256, 5, 0))
    h.load_state_dict(synth.encoder_state_dict(_JAS, 64, 1))
    h.load_state_dict(synth.classifier_state_dict(256, 5, 1))
    assert L.vasr_finalize(h.h) == -1 and "filters" in L.vasr_last_error().decode()
    h.close()
    # compute entry points refuse a handle that was never finalized, and the workspace query answers 0
    h = _lib.Handle(classifier=(128, 5, 0))
    assert L.vasr_classifier_f32(h.h, None, 1, 4, 0, None, None, 0, None) == -2
    assert L.vasr_classify_f32(h.h, None, None, 1, 16000, 128, None, 0, None, None, None, 0, None) == -2
    assert L.vasr_classify_workspace_bytes(h.h, 1, 16000, 128) == 0
    h.close()
    assert L.vasr_crop_or_pad_f32(None, 1, 64, 4, 8, None, None, None, None) == -1


def test_new_symbols_are_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(HERE, "..", "include", "vasr.h")).read()
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header, n
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_fixture_conditions_hold(name):
    """What make_golden_cls.py asserted when it wrote the fixture, re-read from the file."""
    g, _, _ = CR.load(name)
    tol = CR.tolerance(g["out64"])
    assert g["mel"].shape == (3, 64, int(g["audio_length"])) and g["out"].shape == g["out64"].shape == (3, int(g["num_classes"]))
    assert (g["margin64"] > 2 * tol).all() and len(set(g["pred64"].tolist())) > 1
    assert np.array_equal(g["out64"].argmax(-1), g["pred64"]) and np.array_equal(g["out"].argmax(-1), g["pred64"])
    assert np.abs(g["out"].astype(np.float64) - g["out64"]).max() <= tol / 4
    if not bool(g["return_logits"]):
        assert np.allclose(g["out64"].sum(-1), 1.0, atol=1e-12)
    if "crop" in name:
        assert g["mel_raw"].shape[-1] > int(g["audio_length"]) and float(g["negative_pooled_max_share"]) > 0
        assert (g["enc"].max(-1) < 0).any()


@pytest.mark.parametrize("name", CR.FIXTURES)
def test_float64_restatement_reproduces_the_fixtures(name):
    """crop / pad: bit-equal to the reference's mel.  pool + linear (+ softmax) from the fixture's float32 encoder output,
    and -- for the ReLU encoders the oracle covers -- from the restated crop / pad through the oracle encoder in float64:
    the reference's float64 output within the oracle's log-prob tolerance (tests/test_oracle_golden.py: 2e-4)."""
    from oracle import quartznet_oracle as O
    g, cfg, jas = CR.load(name)
    A = int(g["audio_length"])
    mel = CR.crop_or_pad(g["mel_raw"], A, g["offsets"])
    assert mel.dtype == np.float32 and np.array_equal(mel, g["mel"])
    left, right = CR.pad_split(A, min(A, g["mel_raw"].shape[-1]))
    assert not mel[:, :, :left].any() and not mel[:, :, A - right:].any()
    enc_sd, dec_sd = CR.fixture_weights(g, jas)
    w, b = dec_sd["decoder_layers.0.weight"], dec_sd["decoder_layers.0.bias"]
    softmax = not bool(g["return_logits"])
    out, _ = CR.classifier(g["enc"], w, b, str(g["pooling_type"]), softmax)
    assert np.abs(out - g["out64"]).max() <= 2e-4
    assert np.array_equal(out.argmax(-1), g["pred64"])
    if str(g["activation"]) == "relu":
        e64, _ = O.encoder_forward(mel.astype(np.float64), np.full(3, A, dtype=np.int64), enc_sd, jas, dtype=__import__("torch").float64)
        out, _ = CR.classifier(e64.numpy(), w, b, str(g["pooling_type"]), softmax)
        assert np.abs(out - g["out64"]).max() <= 2e-4
        assert np.array_equal(out.argmax(-1), g["pred64"])
