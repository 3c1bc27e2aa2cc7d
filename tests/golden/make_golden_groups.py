#!/usr/bin/env python3
"""Generate tests/golden/groups_*.npz / groups_*_state_dict_keys.json by running the REAL reference JasperEncoder +
JasperDecoderForCTC with grouped blocks (``groups``: grouped main-branch convs, each followed by a GroupShuffle), shared
depthwise weights (``heads``) and scaled kernels (``kernel_size_factor``) -- jasper.py:162-189, parts/jasper.py:52-57, :70-150,
:329-400 -- dev container only; shims, module construction and the row layout of make_golden_se.py.

    python tests/golden/make_golden_groups.py [case ...]     # needs the reference checkout

Every row of a fixture is run by the reference ALONE (batch 1, pad_to = 0), on a length that is not a multiple of the hop.
Inputs and weights are NOT stored -- they are regenerated from viet-asr_amd/synth.py seeds (``audio_batch(rows, max(lens),
seed)``, row b cut to ``lens[b]``); stored per row i are the float32 outputs (mel_i, enc_len_i, logp_i, pred_i, hyp_i) and,
from the same modules after ``.double()``, the float64 argmax and top-2 margin of every frame (margin64_i).
"""
import copy
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_se as MS  # noqa: E402


def _grouped_15x5():
    """QuartzNet15x5 with groups = 4 on every block: block 0 reads the 64 mel features (16 per group: the block-diagonal
    fallback), block 17 is the grouped 512 -> 1024 1x1.  heads on blocks 1-3 (16 rows) and 9 (64 rows), kernel_size_factor 0.5
    on block 4 (39 -> 19 taps)."""
    from viet_asr_amd import configs
    out = copy.deepcopy(configs.builtin("quartznet15x5")["JasperEncoder"]["jasper"])
    for i, b in enumerate(out):
        b["groups"] = 4
        if i in (1, 2, 3):
            b["heads"] = 16
        if i == 9:
            b["heads"] = 64
        if i == 4:
            b["kernel_size_factor"] = 0.5
    return out


# non-separable grouped K = 11 stride-2 conv (128 per group: the grouped implicit GEMM), a grouped separable residual block
# (64 per group), G = 8 on 512 channels (first sub-layer 32 inputs per group: fallback; second 64: grouped), a grouped
# non-separable 1x1 residual block
_JASPER_G = [dict(filters=256, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False),
             dict(filters=256, repeat=1, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, groups=2),
             dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                  groups=4),
             dict(filters=512, repeat=2, kernel=[7], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
                  groups=8),
             dict(filters=512, repeat=2, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=True, groups=2)]
# a dense-residual run with grouped blocks (the panes' 1x1 convs are not grouped); 384 channels at G = 2: 192 rows per group,
# only the 64-row tile divides them
_DENSE_G = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                 separable=True, groups=2),
            dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                 separable=True, groups=4),
            dict(filters=384, repeat=2, kernel=[15], stride=[1], dilation=[1], dropout=0.0, residual=True, residual_dense=True,
                 separable=True, groups=2),
            dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]
# groups with squeeze-and-excitation: without residual (the SE follows the shuffle of every sub-layer), with residual (the SE
# sits on the ungrouped residual branch)
_SE_G = [dict(filters=256, repeat=2, kernel=[11], stride=[1], dilation=[1], dropout=0.0, residual=False, separable=True,
              groups=4, se=True, se_reduction_ratio=8),
         dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
              groups=2, se=True),
         dict(filters=512, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=False)]

# state-dict keys only: heads on blocks that are not separable -- the reference never hands heads to their convs
# (_get_conv_bn_layer passes it to the depthwise conv of a separable block alone), so they keep the plain keys and shapes
_HEADS_NONSEP = [dict(filters=256, repeat=2, kernel=[11], stride=[2], dilation=[1], dropout=0.0, residual=False, groups=2,
                      heads=4),
                 dict(filters=256, repeat=1, kernel=[1], stride=[1], dilation=[1], dropout=0.0, residual=True, heads=8),
                 dict(filters=256, repeat=2, kernel=[13], stride=[1], dilation=[1], dropout=0.0, residual=True, separable=True,
                      heads=16)]
KEY_CASES = [("groups_heads_nonsep", _HEADS_NONSEP)]

# (name, block list, row lengths in samples, seed)
CASES = [
    ("groups_15x5_rows3", "15x5", [96_013, 47_981, 70_117], 51),
    ("groups_jasper_rows3", _JASPER_G, [40_017, 17_203, 29_999], 52),
    ("groups_dense_rows3", _DENSE_G, [40_013, 23_111, 31_337], 53),
    ("groups_se_rows3", _SE_G, [36_011, 19_999, 27_123], 54),
]


def definition(src):
    """Model definition dict of a case (the tests rebuild it from the stored block list)."""
    from viet_asr_amd import configs
    return configs.jasper_definition(_grouped_15x5() if src == "15x5" else src)


def main():
    MS.MG.install_shims()
    sys.path.insert(0, MS.MG.REF)
    import torch
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    MS.definition = definition          # run_case builds the case's model definition through this name
    only = set(sys.argv[1:])
    for name, src in KEY_CASES:
        if only and name not in only:
            continue
        cfg = definition(src)
        _nf, _pre, enc, _dec, _greedy = MS.MG.build_reference(cfg, cfg["labels"])
        _write_keys(name, {k: list(v.shape) for k, v in enc.state_dict().items()})
    for name, src, lens, seed in CASES:
        if only and name not in only:
            continue
        _write_keys(name.replace("_rows3", ""), MS.run_case(name, src, lens, seed))


def _write_keys(stem, keys):
    with open(os.path.join(HERE, stem + "_state_dict_keys.json"), "w", encoding="utf-8") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(keys.items())) + "\n}\n")


if __name__ == "__main__":
    main()
