#!/usr/bin/env python3
"""Generate tests/golden/norm_*.npz / norm_*_state_dict_keys.json by running the REAL reference JasperEncoder +
JasperDecoderForCTC with GroupNorm (``normalization_mode`` "group" / "instance" / "layer", ``norm_groups``; jasper.py:136-186,
parts/jasper.py:342-393) -- dev container only; shims and module construction from make_golden.py, the row layout of
make_golden_se.py.

    python tests/golden/make_golden_norm.py [case ...]     # needs the reference checkout

Every row of a fixture is run by the reference ALONE (batch 1, pad_to = 0), on a length that is not a multiple of the hop, so
that the tensor is exactly as wide as the row's length at every layer: there the library's statistics over each row's own
frames and nn.GroupNorm's over the tensor width are the same computation.  Inputs and weights are NOT stored -- they are
regenerated from viet-asr_amd/synth.py seeds (``audio_batch(rows, max(lens), seed)``, row b cut to ``lens[b]``;
``encoder_state_dict(..., norm=engine.norm_from_config(...))``); stored per row i are the float32 outputs (mel_i, enc_len_i,
logp_i, pred_i, hyp_i) and, from the same modules after ``.double()``, the float64 argmax and top-2 margin of every frame
(margin64_i), beside the block list, normalization_mode and norm_groups.
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

# dense-residual run (three panes reach block 2, each normalized on its own), then a plain 1x1 block
_DENSE = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=384, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
               separable=True),
          dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# SE without residual (after every sub-layer's norm and activation): a non-separable K = 11 stride-2 block, a separable block,
# a 1x1 block
_SE_NORES = [dict(filters=256, repeat=2, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False,
                  se=True, se_reduction_ratio=8),
             dict(filters=256, repeat=3, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
                  se=True),
             dict(filters=384, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# grouped blocks at norm_groups = 8 != groups = 4: a block reading the 64 mel features at G = 4 (16 per group: the narrow
# block-diagonal form), grouped separable blocks with and without residual, a grouped 1x1 residual block
_GROUPED = [dict(filters=256, repeat=1, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, groups=4),
            dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                 groups=4),
            dict(filters=512, repeat=2, kernel=[7], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
                 groups=4),
            dict(filters=512, repeat=2, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=True, groups=4),
            dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]

# (name, block list source, normalization_mode, norm_groups, row lengths in samples, seed): "15x5" = the builtin layout
CASES = [
    ("norm_15x5_group32_rows3", "15x5", "group", 32, [96_013, 47_981, 70_117], 61),
    ("norm_dense_layer_rows3", _DENSE, "layer", -1, [40_013, 23_111, 31_337], 62),
    ("norm_se_instance_rows3", _SE_NORES, "instance", -1, [40_017, 17_203, 29_999], 63),
    ("norm_groups_group8_rows3", _GROUPED, "group", 8, [36_011, 19_999, 27_123], 64),
]


def definition(src, mode, norm_groups):
    """Model definition dict of a case (the tests rebuild it from the stored block list, mode and norm_groups)."""
    from viet_asr_amd import configs
    jas = copy.deepcopy(configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"]) if src == "15x5" else src
    cfg = configs.jasper_definition(jas)
    cfg["JasperEncoder"].update(normalization_mode=mode, norm_groups=norm_groups)
    return cfg


def run_case(name, src, mode, norm_groups, lens, seed):
    pkg = MG._load_pkg()
    synth = pkg.synth
    from viet_asr_amd import engine
    from nemo.collections.asr.helpers import post_process_predictions
    cfg = definition(src, mode, norm_groups)
    labels = cfg["labels"]
    nf, pre, enc, dec, greedy = MG.build_reference(cfg, labels)
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd = synth.encoder_state_dict(jas, 64, seed, norm=engine.norm_from_config(cfg["JasperEncoder"], jas))
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(labels) + 1, seed)
    ref_keys = {k: list(v.shape) for k, v in enc.state_dict().items()}
    missing = set(ref_keys) ^ set(enc_sd)
    assert not missing, sorted(missing)[:8]
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in enc_sd.items()})
    dec.load_state_dict({k: torch.as_tensor(v) for k, v in dec_sd.items()})
    enc.eval(); dec.eval(); greedy.eval()
    out = dict(definition=json.dumps(jas, sort_keys=True), normalization_mode=mode, norm_groups=norm_groups, seed=seed,
               lens=np.asarray(lens, dtype=np.int64))
    for i, sig in enumerate(MS.signals(lens, seed)):
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
    for name, src, mode, ng, lens, seed in CASES:
        if only and name not in only:
            continue
        keys = run_case(name, src, mode, ng, lens, seed)
        path = os.path.join(HERE, name.replace("_rows3", "") + "_state_dict_keys.json")
        with open(path, "w", encoding="utf-8") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(keys.items())) + "\n}\n")


if __name__ == "__main__":
    main()
