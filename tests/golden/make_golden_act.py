#!/usr/bin/env python3
"""Generate tests/golden/act_*.npz / act_*_state_dict_keys.json by running the REAL reference JasperEncoder +
JasperDecoderForCTC with a non-ReLU ``activation`` ("hardtanh", "selu") and / or ``residual_mode`` "max" (jasper.py:136-190,
parts/jasper.py:21-25, :428-448) -- dev container only; shims and module construction from make_golden.py, the row layout of
make_golden_norm.py.

    python tests/golden/make_golden_act.py [case ...]     # needs the reference checkout

Every row of a fixture is run by the reference ALONE (batch 1, pad_to = 0).  Inputs and weights are NOT stored -- they are
regenerated from viet-asr_amd/synth.py seeds (``audio_batch(rows, max(lens), seed)``, row b cut to ``lens[b]``;
``scale_conv_weights(encoder_state_dict(..., norm=engine.norm_from_config(...)), gain)``); stored per row i are the float32
outputs (mel_i, enc_len_i, logp_i, pred_i, hyp_i) and, from the same modules after ``.double()``, the float64 argmax and top-2
margin of every frame (margin64_i), beside the block list, activation, residual_mode, normalization_mode, norm_groups and gain.

Each fixture must be worth having: the same weights run with activation="relu", residual_mode="add" must differ from it far
beyond the tests' tolerance and in the argmax of some frames (asserted here).  The fraction of pre-activations on which
the activation differs from ReLU's behaviour -- inside (-1, 1) for hardtanh, below 0 for selu -- is printed.
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
import make_golden_se as MS  # noqa: E402

# dense-residual run (three panes reach block 2), then a plain 1x1 block
_DENSE = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=384, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# the same run with SE on every block (one SE per residual pane, combined by max)
_DENSE_SE = [dict(b, se=True, se_reduction_ratio=8) if b["residual"] else dict(b) for b in _DENSE]
# the implicit-GEMM CONV epilogue: a K = 11 stride-2 non-separable prologue, a dilation-2 non-separable residual block
_CONV = [dict(filters=256, repeat=1, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False),
         dict(filters=256, repeat=2, kernel=[7], stride=[1], dilation=[2], dropout=0.0, residual=True),
         dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True),
         dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# grouped blocks with SE and no residual, GroupNorm: the norm apply pass and the SE rescale apply the activation
_GROUPED_SE = [dict(filters=256, repeat=1, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, groups=4),
               dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
                    groups=4, se=True, se_reduction_ratio=8),
               dict(filters=512, repeat=2, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=True, groups=4),
               dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]

# (name, block list source, activation, residual_mode, normalization_mode, norm_groups, row lengths in samples, seed, conv
# weight gain): "15x5" = the builtin layout.  The gain (synth.scale_conv_weights) keeps the 54-layer 15x5 contracting under
# an activation that passes negative values: at gain 1 a relative input perturbation of 1e-7 moves the reference's own
# log-probs by 1e-2 (hardtanh / max) and 8e-2 (SELU), far past the tolerance; at these gains by < 5e-5, with 5 and 17
# distinct argmax classes per row.
CASES = [
    ("act_15x5_selu_add_rows3", "15x5", "selu", "add", "batch", -1, [96_013, 47_981, 70_117], 71, 0.8),
    ("act_15x5_hardtanh_max_rows3", "15x5", "hardtanh", "max", "batch", -1, [80_011, 41_117, 63_331], 72, 0.85),
    ("act_dense_selu_max_rows3", _DENSE, "selu", "max", "batch", -1, [40_013, 23_111, 31_337], 73, 1.0),
    ("act_dense_se_relu_max_rows3", _DENSE_SE, "relu", "max", "batch", -1, [40_017, 17_203, 29_999], 74, 1.0),
    ("act_conv_selu_add_rows3", _CONV, "selu", "add", "batch", -1, [36_011, 19_999, 27_123], 75, 1.0),
    ("act_groups_se_hardtanh_group_rows3", _GROUPED_SE, "hardtanh", "add", "group", 8, [36_017, 21_001, 28_337], 76, 1.0),
]


def definition(src, activation, residual_mode, mode, norm_groups):
    """Model definition dict of a case (the tests rebuild it from the stored block list and options)."""
    from viet_asr_amd import configs
    jas = copy.deepcopy(configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]) if src == "15x5" else copy.deepcopy(src)
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(activation=activation, residual_mode=residual_mode, normalization_mode=mode,
                                norm_groups=norm_groups)
    return cfg


def _pre_activation_fraction(enc, activation, mel, seq):
    """Fraction of the encoder activation's inputs inside (-1, 1) (hardtanh) or below 0 (selu)."""
    seen = []

    def hook(_m, inp, _out):
        x = inp[0].detach()
        seen.append((float(((x > -1) & (x < 1)).sum() if activation == "hardtanh" else (x < 0).sum()), x.numel()))
    hs = [m.register_forward_hook(hook) for m in enc.modules() if isinstance(m, (torch.nn.Hardtanh, torch.nn.SELU))]
    with torch.no_grad():
        enc(force_pt=True, audio_signal=mel, length=seq)
    for h in hs:
        h.remove()
    return sum(a for a, _ in seen) / max(1, sum(n for _, n in seen))


def run_case(name, src, activation, residual_mode, mode, norm_groups, lens, seed, gain):
    pkg = MG._load_pkg()
    synth = pkg.synth
    from viet_asr_amd import engine
    from nemo.collections.asr.helpers import post_process_predictions
    cfg = definition(src, activation, residual_mode, mode, norm_groups)
    labels = cfg["labels"]
    nf, pre, enc, dec, greedy = MG.build_reference(cfg, labels)
    base_cfg = definition(src, "relu", "add", mode, norm_groups)
    _, _, enc_base, _, _ = MG.build_reference(base_cfg, labels)
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd = synth.scale_conv_weights(
        synth.encoder_state_dict(jas, 64, seed, norm=engine.norm_from_config(cfg["JasperEncoder"], jas)), gain)
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(labels) + 1, seed)
    ref_keys = {k: list(v.shape) for k, v in enc.state_dict().items()}
    missing = set(ref_keys) ^ set(enc_sd)
    assert not missing, sorted(missing)[:8]
    for e_ in (enc, enc_base):
        e_.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
        e_.eval()
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    dec.eval(); greedy.eval()
    out = dict(definition=json.dumps(jas, sort_keys=True), activation=activation, residual_mode=residual_mode,
               normalization_mode=mode, norm_groups=norm_groups, seed=seed, gain=gain, lens=np.asarray(lens, dtype=np.int64))
    worst_diff, frames_differ = np.inf, 0
    for i, sig in enumerate(MS.signals(lens, seed)):
        enc.float(); dec.float()
        with torch.no_grad():
            mel, seq = pre(force_pt=True, input_signal=torch.as_tensor(sig[None]), length=torch.as_tensor([len(sig)]))
            e, elen = enc(force_pt=True, audio_signal=mel, length=seq)
            logp = dec(force_pt=True, encoder_output=e)
            pred = greedy(force_pt=True, log_probs=logp)
            eb, _ = enc_base(force_pt=True, audio_signal=mel, length=seq)
            logp_base = dec(force_pt=True, encoder_output=eb)
            enc.double(); dec.double()
            e64, _ = enc(force_pt=True, audio_signal=mel.double(), length=seq)
            logp64 = dec(force_pt=True, encoder_output=e64)
            enc.float(); dec.float()
        frac = _pre_activation_fraction(enc, activation, mel, seq) if activation != "relu" else float("nan")
        hyp = post_process_predictions([pred], labels)
        top2 = torch.topk(logp64, 2, dim=-1).values
        diff = float((logp - logp_base).abs().max())
        tol = 5e-4 + 2e-5 * float(logp.abs().max())
        worst_diff = min(worst_diff, diff / tol)
        frames_differ += int((logp.argmax(-1) != logp_base.argmax(-1)).sum())
        out.update({f"mel_{i}": mel.numpy(), f"enc_len_{i}": elen.numpy(), f"logp_{i}": logp.numpy(),
                    f"pred_{i}": pred.numpy(), f"pred64_{i}": logp64.argmax(-1).numpy(),
                    f"margin64_{i}": (top2[..., 0] - top2[..., 1]).numpy(), f"hyp_{i}": np.array(hyp, dtype=object).astype("U")})
        print(f"{name} row {i}: mel{tuple(mel.shape)} enc{tuple(e.shape)} enc_len={elen.tolist()} "
              f"min_margin64={float((top2[..., 0] - top2[..., 1]).min()):.3e} |logp|max={float(logp.abs().max()):.1f} "
              f"enc range [{float(e.min()):.2f}, {float(e.max()):.2f}] pre-activation fraction {frac:.3f} "
              f"vs relu/add: max|dlogp| {diff:.3e} = {diff / tol:.0f} x tol, argmax differs on "
              f"{int((logp.argmax(-1) != logp_base.argmax(-1)).sum())} of {logp.shape[1]} frames")
    assert worst_diff > 100, f"{name}: relu/add is within {worst_diff:.1f} x the tolerance of the fixture"
    assert frames_differ > 0, f"{name}: relu/add decodes every frame the same"
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: bytes={os.path.getsize(path)}")
    return ref_keys


def main():
    MG.install_shims()
    sys.path.insert(0, MG.REF)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    only = set(sys.argv[1:])             # case names to (re)generate; none: all
    for name, src, act, rmode, mode, ng, lens, seed, gain in CASES:
        if only and name not in only:
            continue
        keys = run_case(name, src, act, rmode, mode, ng, lens, seed, gain)
        path = os.path.join(HERE, name.replace("_rows3", "") + "_state_dict_keys.json")
        with open(path, "w", encoding="utf-8") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(keys.items())) + "\n}\n")


if __name__ == "__main__":
    main()
