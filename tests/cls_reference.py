"""What the classification tests and tests/golden/make_golden_cls.py share: the fixtures' regenerated inputs and weights, the
tolerance, and a plain float64 restatement of the stages the oracle does not cover -- CropOrPadSpectrogramAugmentation
(reference audio_preprocessing.py:666-738) and JasperDecoderForClassification (jasper.py:257-319): crop / pad, pool over
time, Linear, softmax."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("cls_pad_avg_rows3", "cls_crop_max_selu_rows3", "cls_exact_softmax_rows3")


def tolerance(x):
    """The project's parity tolerance on logits and probabilities: max(5e-4, 2e-5 |x|) (README: the log-prob tolerance)."""
    return max(5e-4, 2e-5 * float(np.abs(np.asarray(x)).max()))


def signals(lens, seed):
    """[rows][max(lens)] f32 zero padded past each length, and the lengths.  The rows of synth.audio_batch are statistically
    alike and, after the per-feature normalization, would all fall into one class: row 1 is gated into bursts of 2000
    samples, row 2 fades in quadratically -- elementwise float32 arithmetic, the same bits on every host."""
    from viet_asr_amd import synth
    sig, _ = synth.audio_batch(len(lens), int(max(lens)), int(seed))
    n = np.arange(sig.shape[1])
    sig[1] *= (n // 2000 % 2).astype(np.float32)
    ramp = n.astype(np.float32) / np.float32(sig.shape[1])
    sig[2] *= ramp * ramp
    for b, m in enumerate(lens):
        sig[b, int(m):] = 0.0
    return sig, np.asarray(lens, dtype=np.int64)


def state_dicts(jas, num_classes, seed, head_seed, neg_shift=0.0):
    """(encoder state_dict, classifier state_dict) of a fixture.  neg_shift > 0 lowers the bias of the encoder's LAST
    normalization on every fourth channel by that much: under SELU those channels stay negative on every frame, so that
    negative values reach a max pool (a zero-initialised maximum, or one that reads zero padding, then shows)."""
    from viet_asr_amd import synth
    enc_sd = synth.encoder_state_dict(jas, 64, int(seed))
    if neg_shift:
        last = len(jas) - 1
        idx = max(int(k.split(".")[3]) for k in enc_sd if k.startswith(f"encoder.{last}.mconv.") and k.endswith(".running_var"))
        key = f"encoder.{last}.mconv.{idx}.bias"
        b = enc_sd[key].copy()
        b[::4] -= np.float32(neg_shift)
        enc_sd[key] = b
    return enc_sd, synth.classifier_state_dict(jas[-1]["filters"], int(num_classes), int(head_seed))


def load(name):
    """(fixture dict, model definition, block list) of tests/golden/<name>.npz."""
    from viet_asr_amd import configs
    g = dict(np.load(os.path.join(HERE, "golden", name + ".npz")))
    jas = json.loads(str(g["definition"]))
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(activation=str(g["activation"]))
    return g, cfg, jas


def fixture_weights(g, jas):
    return state_dicts(jas, int(g["num_classes"]), int(g["seed"]), int(g["head_seed"]), float(g["neg_shift"]))


def pad_split(audio_length, image_len):
    """(left, right) zero frames of the pad branch: the odd frame goes on the right (:700-707)."""
    d = int(audio_length) - int(image_len)
    return d // 2, d - d // 2


def crop_or_pad(image, audio_length, offsets=None):
    """CropOrPadSpectrogramAugmentation.forward on a numpy [B][F][T] array (any dtype): rows cut at offsets[b] when
    T > audio_length, else zero padded by pad_split (T == audio_length: zero pads)."""
    image = np.asarray(image)
    B, F, T = image.shape
    out = np.zeros((B, F, audio_length), dtype=image.dtype)
    if T > audio_length:
        for b in range(B):
            o = int(offsets[b])
            out[b] = image[b, :, o : o + audio_length]
        return out
    left, _ = pad_split(audio_length, T)
    out[:, :, left : left + T] = image
    return out


def classifier(enc, weight, bias, pooling, softmax):
    """JasperDecoderForClassification.forward in float64: pool every channel over ALL frames of enc [B][C][T'] (mean or max),
    logits[k] = bias[k] + sum_c W[k][c] pooled[c], optionally softmax over the classes.  Returns (output, logits)."""
    x = np.asarray(enc, dtype=np.float64)
    pooled = x.mean(-1) if pooling == "avg" else x.max(-1)
    logits = pooled @ np.asarray(weight, dtype=np.float64).T + np.asarray(bias, dtype=np.float64)
    if not softmax:
        return logits, logits
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True), logits
