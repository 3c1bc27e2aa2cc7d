#!/usr/bin/env python3
"""Generate tests/golden/se_*.npz / se_state_dict_keys.json by running the REAL reference JasperEncoder +
JasperDecoderForCTC with squeeze-and-excitation blocks (``se`` / ``se_reduction_ratio``, jasper.py:162-182,
parts/jasper.py:152-168, :223-253) -- dev container only; shims and module construction from make_golden.py.

    python tests/golden/make_golden_se.py [case ...]     # needs the reference checkout

Every row of a fixture is run by the reference ALONE (batch 1, pad_to = 0: the reference's own serving shape, infer.py), on
a length that is not a multiple of the hop, so that the mel tensor is exactly as wide as the row's length at every layer.
There the library's masked time mean (over each row's own frames) and the reference's AdaptiveAvgPool1d (over the tensor
width) are the same computation.  The GPU tests batch rows of different lengths and compare each with its own batch-1 output.
Inputs and weights are NOT stored -- they are regenerated from viet-asr_amd/synth.py seeds (``audio_batch(rows, max(lens),
seed)``, row b cut to ``lens[b]``); stored per row i are the float32 outputs (mel_i, enc_len_i, logp_i, pred_i, hyp_i) and,
from the same modules after ``.double()``, the float64 argmax and top-2 margin of every frame (margin64_i).
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def _with_se(blocks, **se):
    out = copy.deepcopy(blocks)
    for b in out:
        b.update(se)
    return out


# a dense run with SE on every pane (three panes reach block 2), ratios with odd / non-power-of-two hidden widths
_DENSE_SE = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                  se=True, se_reduction_ratio=48),
             dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                  se=True, se_reduction_ratio=48),
             dict(filters=384, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                  se=True, se_reduction_ratio=48),
             dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False, se=True)]
# SE after every sub-layer (no residual): a non-separable K = 11 stride-2 block of two sub-layers (256 // 48 = 5 hidden
# units), a separable 256-channel block of three, a 1x1 block with 384 // 5 = 76 hidden units
_NORES_SE = [dict(filters=256, repeat=2, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False,
                  se=True, se_reduction_ratio=48),
             dict(filters=256, repeat=3, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
                  se=True),
             dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False,
                  se=True, se_reduction_ratio=5)]

# (name, model definition source, row lengths in samples, seed): source "quartznet15x5" = the builtin layout, se on every block
CASES = [
    ("se_15x5_rows3", "quartznet15x5", [159_963, 47_981, 101_117], 41),
    ("se_dense_rows3", _DENSE_SE, [40_013, 23_111, 31_337], 42),
    ("se_nores_k11s2_rows3", _NORES_SE, [40_017, 17_203, 29_999], 43),
]


def definition(src):
    """Model definition dict of a case (the tests rebuild it the same way)."""
    from viet_asr_amd import configs
    if isinstance(src, str):
        return configs.jasper_definition(_with_se(configs.builtin(src)["JasperEncoder"]["jasper"], se=True))
    return configs.jasper_definition(src)


def signals(lens, seed):
    """Row b: the first lens[b] samples of row b of synth.audio_batch(len(lens), max(lens), seed)."""
    from viet_asr_amd import synth
    sig, _ = synth.audio_batch(len(lens), max(lens), seed, ragged=False)
    return [sig[b, :n].copy() for b, n in enumerate(lens)]


def run_case(name, src, lens, seed):
    pkg = MG._load_pkg()
    synth = pkg.synth
    from nemo.collections.asr.helpers import post_process_predictions
    cfg = definition(src)
    labels = cfg["labels"]
    nf, pre, enc, dec, greedy = MG.build_reference(cfg, labels)
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd = synth.encoder_state_dict(jas, 64, seed)
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(labels) + 1, seed)
    ref_keys = {k: list(v.shape) for k, v in enc.state_dict().items()}
    missing = set(ref_keys) ^ set(enc_sd)
    assert not missing, sorted(missing)[:8]
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    enc.eval(); dec.eval(); greedy.eval()
    out = dict(definition=json.dumps(jas, sort_keys=True), seed=seed, lens=np.asarray(lens, dtype=np.int64))
    for i, sig in enumerate(signals(lens, seed)):
        assert len(sig) % 160, "a row length that is a multiple of the hop leaves one frame past the mask"
        enc.float(); dec.float()
        with torch.no_grad():
            mel, seq = pre(force_pt=True, input_signal=torch.as_tensor(sig[None]), length=torch.as_tensor([len(sig)]))
            assert mel.shape[2] == int(seq[0]), (mel.shape, seq)
            e, elen = enc(force_pt=True, audio_signal=mel, length=seq)
            logp = dec(force_pt=True, encoder_output=e)
            pred = greedy(force_pt=True, log_probs=logp)
            enc.double(); dec.double()
            e64, _ = enc(force_pt=True, audio_signal=mel.double(), length=seq)
            logp64 = dec(force_pt=True, encoder_output=e64)
        hyp = post_process_predictions([pred], labels)
        top2 = torch.topk(logp64, 2, dim=-1).values
        out.update({f"mel_{i}": mel.numpy(), f"enc_len_{i}": elen.numpy(), f"logp_{i}": logp.numpy(),
                    f"pred_{i}": pred.numpy(), f"pred64_{i}": logp64.argmax(-1).numpy(),
                    f"margin64_{i}": (top2[..., 0] - top2[..., 1]).numpy(), f"hyp_{i}": np.array(hyp, dtype=object).astype("U")})
        print(f"{name} row {i}: mel{tuple(mel.shape)} enc{tuple(e.shape)} enc_len={elen.tolist()} "
              f"min_margin64={float((top2[..., 0] - top2[..., 1]).min()):.3e} |logp|max={float(logp.abs().max()):.1f}")
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: bytes={os.path.getsize(path)}")
    return ref_keys


def main():
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    only = set(sys.argv[1:])             # case names to (re)generate; none: all
    for name, src, lens, seed in CASES:
        if only and name not in only:
            continue
        keys = run_case(name, src, lens, seed)
        if name in ("se_dense_rows3", "se_nores_k11s2_rows3"):   # the reference's state_dict layouts with SE
            path = os.path.join(HERE, name.replace("_rows3", "") + "_state_dict_keys.json")
            with open(path, "w", encoding="utf-8") as f:
                f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(keys.items())) + "\n}\n")


if __name__ == "__main__":
    main()
