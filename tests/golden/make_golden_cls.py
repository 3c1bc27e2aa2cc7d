#!/usr/bin/env python3
"""Generate tests/golden/cls_*.npz / cls_*_state_dict_keys.json by running the REAL reference speech-classification path on the
CPU: AudioToMelSpectrogramPreprocessor (dither 0, pad_to 0) -> CropOrPadSpectrogramAugmentation -> JasperEncoder ->
JasperDecoderForClassification (audio_preprocessing.py:666-738, jasper.py:257-319) -- dev container only; shims and module
construction from make_golden.py.

    python tests/golden/make_golden_cls.py [case ...]     # needs the reference checkout

Each fixture is ONE batched run of three ragged rows (the crop acts on the batch tensor's width).  Inputs and weights are NOT
stored -- they are regenerated from viet-asr_amd/synth.py seeds by tests/cls_reference.py (``signals``, ``state_dicts``).  Stored: the block list and options, lens, seed, the drawn
offsets, the mel before and after crop / pad, the float32 encoder output and logits (or probabilities), and from the same
modules after ``.double()`` the float64 output, its arg-max and each row's top-2 margin.

The conditions the tests rest on are asserted here (TOL = the tests' tolerance max(5e-4, 2e-5 |x|)): every row's float64 top-2
margin exceeds 2 TOL (no row is ever excused from the arg-max comparison); the three rows do not all have the same class; in
the crop case the offsets are not all equal and one is neither 0 nor the maximum, and a non-zero share of the pooled maxima
is negative; the reference's own float32 output is within TOL / 4 of its float64 output."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import cls_reference as CR  # noqa: E402  (tests/cls_reference.py: the regenerated inputs and weights, the tolerance)


def _b(filters, repeat, kernel, stride=1, dilation=1, residual=False, separable=True):
    return dict(filters=filters, repeat=repeat, kernel=[kernel], stride=[stride], dilation=[dilation], dropout=0.0,
                residual=residual, separable=separable)


# separable blocks, ReLU: the pad branch with an odd remainder (101 frames -> 128: 13 left, 14 right)
_PAD = [_b(256, 1, 11), _b(256, 2, 13, residual=True), _b(128, 1, 15)]
# a stride-2 first block (T' = 64) and SELU, so that negative values reach the max pool
_CROP = [_b(256, 1, 11, stride=2), _b(256, 2, 13, residual=True), _b(128, 1, 15)]
# a dilated non-separable block; mel width exactly audio_length: the pad branch with zero pads
_EXACT = [_b(128, 1, 11), _b(128, 1, 7, dilation=2, residual=True, separable=False), _b(128, 1, 13)]

AUDIO_LENGTH = 128
# (name, blocks, activation, pooling, return_logits, classes, row lengths in samples, seed, neg_shift of cls_reference.state_dicts)
CASES = [
    ("cls_pad_avg_rows3", _PAD, "relu", "avg", True, 35, [16_000, 9_011, 12_503], 81, 0.0),
    ("cls_crop_max_selu_rows3", _CROP, "selu", "max", True, 12, [32_000, 21_013, 26_777], 82, 6.0),
    ("cls_exact_softmax_rows3", _EXACT, "relu", "avg", False, 2, [20_400, 11_111, 16_013], 83, 0.0),
]


def definition(blocks, activation):
    from viet_asr_amd import configs
    cfg = configs.jasper_definition(json.loads(json.dumps(blocks)))
    cfg["JasperEncoder"].update(activation=activation)
    return cfg


def run_case(name, blocks, activation, pooling, return_logits, classes, lens, seed, neg_shift):
    pkg = MG._load_pkg()
    synth = pkg.synth
    import nemo.collections.asr as nemo_asr
    cfg = definition(blocks, activation)
    nf, pre, enc, _, _ = MG.build_reference(cfg, cfg["labels"])
    crop = nemo_asr.CropOrPadSpectrogramAugmentation(audio_length=AUDIO_LENGTH)
    jas = cfg["JasperEncoder"]["jasper"]
    dec = nemo_asr.JasperDecoderForClassification(feat_in=jas[-1]["filters"], num_classes=classes, return_logits=return_logits,
                                                  pooling_type=pooling)
    enc_sd, dec_sd = CR.state_dicts(jas, classes, seed, seed, neg_shift)
    head_seed = seed
    enc_keys = {k: list(v.shape) for k, v in enc.state_dict().items()}
    dec_keys = {k: list(v.shape) for k, v in dec.state_dict().items()}
    assert not set(enc_keys) ^ set(enc_sd) and not set(dec_keys) ^ set(dec_sd)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    enc.eval(); dec.eval()
    sig, ln = CR.signals(lens, seed)
    with torch.no_grad():
        mel_raw, seq = pre(force_pt=True, input_signal=torch.as_tensor(sig), length=torch.as_tensor(ln))
        T = mel_raw.shape[-1]
        torch.manual_seed(seed)
        mel, length = crop(force_pt=True, input_signal=mel_raw, length=seq)
        # the draw the module made, repeated: the same call on the same generator state
        torch.manual_seed(seed)
        offsets = torch.randint(low=0, high=T - AUDIO_LENGTH + 1, size=[len(lens)]).numpy() if T > AUDIO_LENGTH \
            else np.zeros(0, dtype=np.int64)
        for b, o in enumerate(offsets):
            assert torch.equal(mel[b], mel_raw[b, :, o : o + AUDIO_LENGTH])
        e, _ = enc(force_pt=True, audio_signal=mel, length=length)
        enc.double(); dec.double()
        e64, _ = enc(force_pt=True, audio_signal=mel.double(), length=length)
        # The pooled vectors of the three rows share a large common component, and most random heads put all of them into one
        # class: the head's seed is the first one from the case's seed on whose float64 classes differ with clear margins.
        # Only the choice of test data looks at the reference's output; the weights stay synth.classifier_state_dict(head_seed).
        pooled64 = (e64.mean(-1) if pooling == "avg" else e64.max(-1).values).numpy()
        for head_seed in range(seed, seed + 500):
            dec_sd = CR.state_dicts(jas, classes, seed, head_seed, neg_shift)[1]
            lg = pooled64 @ dec_sd["decoder_layers.0.weight"].astype(np.float64).T + dec_sd["decoder_layers.0.bias"]
            top = np.sort(lg, axis=-1)
            if classes == 1 or (len(set(lg.argmax(-1).tolist())) > 1 and (top[:, -1] - top[:, -2]).min() > 0.05):
                break
        dec.load_state_dict({k: torch.as_tensor(v).double() for k, v in dec_sd.items()})
        out64 = dec(force_pt=True, encoder_output=e64)
        dec.float()
        out = dec(force_pt=True, encoder_output=e)
        enc.float(); dec.float()
    assert mel.shape == (len(lens), 64, AUDIO_LENGTH) and (length == AUDIO_LENGTH).all()
    tol = CR.tolerance(out64.numpy())
    if classes > 1:
        top2 = torch.topk(out64, 2, dim=-1).values
        margin = (top2[:, 0] - top2[:, 1]).numpy()
        assert (margin > 2 * tol).all(), (name, margin, tol)       # no row excused: the cap on excluded rows is 0
        assert len(set(out64.argmax(-1).tolist())) > 1, (name, out64.argmax(-1).tolist())
    else:
        margin = np.full(len(lens), np.inf)
    self_err = float((out.double() - out64).abs().max())
    assert self_err <= tol / 4, (name, self_err, tol)
    neg_share = float((e.max(dim=-1).values < 0).float().mean())
    if T > AUDIO_LENGTH:
        hi = T - AUDIO_LENGTH
        assert len(set(offsets.tolist())) > 1 and any(0 < o < hi for o in offsets), offsets
        if pooling == "max":
            assert neg_share > 0, name
    d = AUDIO_LENGTH - T
    fixture = dict(definition=json.dumps(jas, sort_keys=True), activation=activation, pooling_type=pooling,
                   return_logits=return_logits, num_classes=classes, audio_length=AUDIO_LENGTH, seed=seed, head_seed=head_seed, neg_shift=neg_shift,
                   lens=ln, seq=seq.numpy(), offsets=offsets.astype(np.int64), mel_raw=mel_raw.numpy(), mel=mel.numpy(),
                   enc=e.numpy(), out=out.numpy(), out64=out64.numpy(), pred64=out64.argmax(-1).numpy(), margin64=margin,
                   negative_pooled_max_share=neg_share)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **fixture)
    print(f"{name}: mel_raw{tuple(mel_raw.shape)} -> mel{tuple(mel.shape)} (d={d}) enc{tuple(e.shape)} offsets={offsets.tolist()} "
          f"head_seed={head_seed} classes={out64.argmax(-1).tolist()} min_margin64={margin.min():.3e} tol={tol:.1e} |f32-f64|={self_err:.2e} "
          f"negative pooled maxima {neg_share:.3f} enc range [{float(e.min()):.2f}, {float(e.max()):.2f}] "
          f"bytes={os.path.getsize(path)}")
    assert os.path.getsize(path) < 1 << 20
    return dict(encoder=enc_keys, decoder=dec_keys)


def main():
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    only = set(sys.argv[1:])
    for case in CASES:
        if only and case[0] not in only:
            continue
        keys = run_case(*case)
        with open(os.path.join(HERE, case[0].replace("_rows3", "") + "_state_dict_keys.json"), "w", encoding="utf-8") as f:
            json.dump(keys, f, indent=0, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
