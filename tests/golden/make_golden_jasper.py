#!/usr/bin/env python3
"""Generate tests/golden/jasper_*.npz / .json by running the REAL reference JasperEncoder + JasperDecoderForCTC (dev
container only; shims and module construction from make_golden.py).

    python tests/golden/make_golden_jasper.py [case ...]     # needs /root/reference

Jasper layouts: non-separable K-tap convolutions (stride 2, dilation 2) and dense residuals (JasperEncoder's
residual_dense, jasper.py:152-161, parts/jasper.py:264-288, :408-448).  Inputs and
weights are NOT stored -- they are regenerated from viet-asr_amd/synth.py seeds; stored are the outputs of the float32
reference (mel, enc_len, log-probs, predictions, transcripts) and, from the same modules after ``.double()``, the float64
top-2 margin of every frame (a frame whose margin lies inside float32 round-off may legitimately decode either way).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

# (name, model definition source, batch, samples, seed, ragged)
#   jasper10x5dr: the builtin layout (53 conv layers, 10 dense blocks in one run from block 1 on)
#   dr3_from_mel: a dense run that starts at block 0 -- the mel features are pane 0 of every block's residual
#   k11_s2 / k29_d2: single non-dense, non-separable blocks from 64 channels (the prologue / epilogue shapes)
#   dense_then_plain: a residual block that is not dense right after a dense run (its residual source is the run's input)
_DR3 = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True),
        dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True),
        dict(filters=384, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True),
        dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# a plain residual block right after a dense run: JasperBlock.forward takes its residual from xs[0], the RUN's input
_DENSE_THEN_PLAIN = [
    dict(filters=256, repeat=1, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=False),
    dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True),
    dict(filters=256, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True),
    dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True),
    dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
_K11_S2 = [dict(filters=256, repeat=1, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False)]
_K29_D2 = [dict(filters=256, repeat=1, kernel=[29], stride=[1], dilation=[2], dropout=0.0, residual=False)]
CASES = [
    ("jasper_10x5dr_b2_ragged", "jasper10x5dr", 2, 48000, 31, True),
    ("jasper_dr3_from_mel_b3", _DR3, 3, 40000, 32, True),
    ("jasper_k11_s2_b3", _K11_S2, 3, 32000, 33, True),
    ("jasper_dense_then_plain_b3", _DENSE_THEN_PLAIN, 3, 40000, 35, True),
    ("jasper_k29_d2_b3", _K29_D2, 3, 32000, 34, True),
]


def definition(src):
    """Model definition dict of a case (the GPU tests rebuild it the same way: configs.builtin / jasper_definition)."""
    from viet_asr_amd import configs
    if isinstance(src, str):
        return configs.builtin(src)
    return configs.jasper_definition(src)


def run_case(name, src, batch, samples, seed, ragged):
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
    sig, lens = synth.audio_batch(batch, samples, seed, ragged)
    enc.eval(); dec.eval(); greedy.eval()
    with torch.no_grad():
        mel, seq = pre(force_pt=True, input_signal=torch.as_tensor(sig), length=torch.as_tensor(lens))
        e, elen = enc(force_pt=True, audio_signal=mel, length=seq)
        logp = dec(force_pt=True, encoder_output=e)
        pred = greedy(force_pt=True, log_probs=logp)
        enc.double(); dec.double()
        e64, _ = enc(force_pt=True, audio_signal=mel.double(), length=seq)
        logp64 = dec(force_pt=True, encoder_output=e64)
    hyp = post_process_predictions([pred], labels)
    top2 = torch.topk(logp64, 2, dim=-1).values
    margin64 = (top2[..., 0] - top2[..., 1]).numpy()
    out = dict(definition=json.dumps(src if isinstance(src, str) else jas, sort_keys=True),
               batch=batch, samples=samples, seed=seed, ragged=ragged, lens=lens,
               mel=mel.numpy(), enc_len=elen.numpy(), enc_sum=np.float64(e.double().sum().item()),
               logp=logp.numpy(), pred=pred.numpy(), pred64=logp64.argmax(-1).numpy(), margin64=margin64,
               hyp=np.array(hyp, dtype=object).astype("U"))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: mel{tuple(mel.shape)} enc{tuple(e.shape)} enc_len={elen.tolist()} "
          f"min_margin64={margin64.min():.3e} |logp|max={float(logp.abs().max()):.1f} bytes={os.path.getsize(path)}")
    print("   hyp[0][:60] =", repr(hyp[0][:60]))
    return ref_keys


def main():
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    only = set(sys.argv[1:])             # case names to (re)generate; none: all
    for name, src, batch, samples, seed, ragged in CASES:
        if only and name not in only:
            continue
        keys = run_case(name, src, batch, samples, seed, ragged)
        if src == "jasper10x5dr":   # (d) the reference's state_dict layout of the builtin model
            with open(os.path.join(HERE, "jasper10x5dr_state_dict_keys.json"), "w", encoding="utf-8") as f:
                f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(keys.items())) + "\n}\n")


if __name__ == "__main__":
    main()
