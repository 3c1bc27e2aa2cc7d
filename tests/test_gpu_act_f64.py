"""-m gpu: the hardtanh and SELU activations and the max residual (vasr_set_activation: Epilogue<1> and Epilogue<2> of every GEMM
and of the fused depthwise + pointwise kernel) against float64, element by element, in every kernel form the product picks
(tests/sep_reference.py: ACT_CASES, PROBES, the chain's bound with the activation's and the max's terms, the restated choice
under a max residual).  tests/test_gpu_act.py holds whole models to the reference's float32 log-probs at 5e-4; this file holds
each epilogue instantiation to the float64 value of its own output.

Per ACT_CASE, per identity probe and per arithmetic (f16x2, bf16x3, fp32), as tests/test_gpu_sep.py does for ReLU / add: the
launch counts equal the restated plan for the device's compute-unit count, every stored element inside the bound (the columns
past a row's length too: selu(shift (+ residual shift)), max(shift, residual shift)), equal encoded lengths, sampled rows
bit-equal to the same rows run as a small batch.  Then, on the devtools build through sep_child.py: every forced split tile and
the chunked kernel give the product's bits on four small cases (SELU / add, hardtanh / max, SELU / max, ReLU / max), the fused
kernel's 64- and 128-frame tiles give equal bits under hardtanh and under SELU, and the fused kernel and the two-kernel form
(VASR_FUSED=0) both lie inside their bounds.

THE IDENTITY PROBES (SEP._probe) put the activation behind nothing: a first block whose 1x1 conv is the identity, so that the
pre-activation is the input, a sweep of both signs from 2^-24 to 2^6 with exact +-1, +-0, +-(1 +- 2^-23) and values below
-88.  The probe's bound is ~ 12 u |act(x)| (one non-zero product a row, the affine's 7 u, SELU's own 4 u); float32 exp(x) - 1
in place of expm1f leaves it by 2e5 (test_sep_host.py), where a table case's bound can hide it by 5 ... 20.  A first block's
source has no published maxima, so the probe's own GEMM runs 3 x bf16 in f16x2 mode (the product's amax logic forces it: only
a block behind another one sees maxima, and that other block would apply the activation first).  A LIMITATION to keep in mind
when reading the table below: the fp16-split and latency instantiations of Epilogue<1> / <2> never meet the sweep itself.  They
meet act(x) one block later, in the trailing identity blocks of the interior probes, which apply the activation once more --
under SELU values in (-1.76, 67], so nothing below -10 or -88 -- and there the bound carries the fp16 split's floor
(2^-39 of the row's maximum), not the probe's 12 u alone: exp(x) - 1 leaves that bound by 30, not by 2e5.  Deeply negative
pre-activations reach those instantiations in the table cases, at the table's looser bound.

PUBLISHED MAXIMA.  Every interior SELU case here is followed by a block that consumes, in f16x2 mode, the per-utterance maxima
the SELU layer published over outputs half of which are negative: the trailing block's GEMM (one product a row: the table's
halves and lifts, a probe's is the identity) scales its fp16 split by them, and the judged chain includes that block (its
bound takes M_x = max(|v| + E) of the SELU output).  Inside a block the second sub-layer's Toeplitz depthwise or fused kernel
consumes the first sub-layer's maxima the same way.  No separate probe of the table is needed: a maximum published too small
saturates the consumer's fp16 split and leaves the bound there.

NOT COVERED here (passes of their own, encoder_se.hip accumulate == 2 and encoder_norm.hip activate, with float64 suites of
their own to extend): SE blocks, GroupNorm, grouped convolutions and K-tap (implicit-GEMM) convolutions under the new
activations; the dense-residual max over several residual GEMMs (the in-place gemm_max chain).  With them, the relu-flag-clear
case of Epilogue<1> (bounds -inf, +inf): it needs a launch that takes a max with the flag clear, i.e. the last sub-layer before
an SE or a gemm_max pane.  A plain max block's own residual GEMM is built from pw_args' defaults and runs Epilogue<0> with the
flag clear under every activation (SEP.act_forms; test_sep_host.py reads the launchers' call sites), so the chain cannot reach
that case, and the host defect clamp_without_relu_flag models a clamp in that Epilogue<0> GEMM.

Largest |y - ref| / bound seen on an MI355X (256 compute units; all elements | frames below the row lengths only), by the
tile, form, EPI and residual mode of the launch that ends the block under test (its first sub-layer's plain GEMM and, under max,
its residual's masked Epilogue<0> GEMM on the same tile lie inside each figure; where the form is not ":port" a trailing block
follows and the figure is of the chain's output; the columns are the arithmetic MODES: in f16x2 mode a first block's GEMM, so
every probe's own, runs 3 x bf16 -- a probe row's f16x2 column is that 3 x bf16 launch followed, where a trailing block
exists, by an fp16-split GEMM on act(x), see the limitation above):
    cases  tile       form         EPI mode  f16x2              bf16x3             fp32
    table  512x128    RES          2   max   0.123 | 1.2e-01    0.124 | 1.2e-01
    table  512x128    RES:port     1   max   0.110 | 1.8e-03    0.110 | 1.8e-03
    table  256x128    RES          2   max   0.090 | 9.0e-02    0.095 | 9.5e-02
    table  256x128    RES:port     1   max   0.121 | 3.3e-03    0.121 | 3.4e-03
    table  256x64     DUAL         1   add                      0.115 | 1.2e-01
    table  256x64     DUAL         2   add                      0.125 | 1.3e-01
    table  256x64     RES          2   max   0.128 | 1.3e-01    0.130 | 1.3e-01
    table  256x64     RES:port     1   max   0.125 | 2.4e-03    0.125 | 2.5e-03
    table  128x64     DUAL         1   add   0.080 | 8.0e-02    0.102 | 1.0e-01
    table  128x64     DUAL         2   add                      0.137 | 1.4e-01
    table  128x64     RES          1   max   0.032 | 3.2e-02    0.034 | 3.4e-02
    table  128x64     RES:port     2   max   0.300 | 3.0e-01    0.300 | 3.0e-01
    table  64x32      DUAL:port    2   add                      0.274 | 2.7e-01
    table  64x32      RES          1   max   0.010 | 9.9e-03    0.057 | 5.7e-02
    table  64x32      RES          2   max   0.071 | 7.1e-02    0.074 | 7.4e-02
    table  64x32      RES:port     1   max                      0.001 | 6.9e-04
    table  64x32      RES:port     2   max                      0.317 | 2.8e-01
    table  64x32      masked:port  2   add                      0.314 | 3.1e-01
    table  latency    DUAL:port    2   add   0.273 | 2.7e-01
    table  latency    RES          1   max   0.057 | 5.7e-02
    table  latency    RES:port     1   max   0.001 | 7.1e-04
    table  latency    RES:port     2   max   0.317 | 2.8e-01
    table  latency    masked:port  2   add   0.314 | 3.1e-01
    table  fused 64, folded residual    1   add   0.099 | 9.9e-02
    table  fused 64, folded residual    2   add   0.133 | 1.3e-01
    table  fused 128, folded residual   1   add   0.113 | 1.1e-01
    table  fused 128, folded residual   2   add   0.123 | 1.2e-01
    table  the same two-kernel, DUAL    1   add   0.086 | 8.6e-02
    table  the same two-kernel, DUAL    2   add   0.131 | 1.3e-01
    table  fp32       DUAL         1   add                                         0.115 | 1.2e-01
    table  fp32       DUAL         2   add                                         0.137 | 1.4e-01
    table  fp32       DUAL:port    2   add                                         0.275 | 2.7e-01
    table  fp32       RES          1   max                                         0.058 | 5.8e-02
    table  fp32       RES          2   max                                         0.130 | 1.3e-01
    table  fp32       RES:port     1   max                                         0.125 | 5.1e-03
    table  fp32       RES:port     2   max                                         0.317 | 3.0e-01
    table  fp32       masked:port  2   add                                         0.314 | 3.1e-01
    probe  256x128    RES          2   max   0.322 | 3.2e-01    0.079 | 7.9e-02
    probe  256x128    RES:port     1   max   0.011 | 1.1e-02    0.011 | 1.1e-02
    probe  256x128    masked       1   add   0.008 | 7.5e-03    0.011 | 1.1e-02
    probe  256x128    masked:port  2   add   0.264 | 2.6e-01    0.264 | 2.6e-01
    probe  256x64     RES:port     1   max   0.011 | 1.1e-02    0.011 | 1.1e-02
    probe  256x64     RES:port     2   max   0.088 | 8.8e-02    0.088 | 8.8e-02
    probe  256x64     masked       2   add   0.127 | 1.3e-01    0.118 | 1.2e-01
    probe  128x64     RES          1   max   0.008 | 7.5e-03    0.011 | 1.1e-02
    probe  128x64     masked       2   add   0.110 | 1.1e-01    0.144 | 1.4e-01
    probe  128x64     masked:port  1   add   0.011 | 1.1e-02    0.011 | 1.1e-02
    probe  64x32      RES          1   max   0.254 | 2.5e-01    0.011 | 1.1e-02
    probe  64x32      RES:port     2   max   0.088 | 8.8e-02    0.088 | 8.8e-02
    probe  64x32      masked       1   add   0.015 | 1.5e-02    0.011 | 1.1e-02
    probe  64x32      masked       2   add   0.127 | 1.3e-01    0.118 | 1.2e-01
    probe  64x32      masked:port  2   add   0.264 | 2.6e-01    0.264 | 2.6e-01
    probe  fp32       RES          1   max                                         0.013 | 1.3e-02
    probe  fp32       RES          2   max                                         0.093 | 9.3e-02
    probe  fp32       RES:port     1   max                                         0.014 | 1.4e-02
    probe  fp32       RES:port     2   max                                         0.103 | 1.0e-01
    probe  fp32       masked       1   add                                         0.013 | 1.3e-02
    probe  fp32       masked       2   add                                         0.159 | 1.6e-01
    probe  fp32       masked:port  1   add                                         0.014 | 1.4e-02
    probe  fp32       masked:port  2   add                                         0.265 | 2.6e-01
The probes' SELU figures, 0.26 of a bound of ~ 12 u: about 3 u on |selu(x)|, inside S = 4 with the affine's unused 7 u to spare;
under hardtanh and ReLU the probes are exact up to the trailing block's fp16 split.  All 121 bit comparisons (rows alone, forced
tiles, the chunked kernel, fused widths) held.  The bound comes from the derivation in tests/sep_reference.py, not from these.
"""
import numpy as np
import pytest
import torch

import sep_reference as SEP
import test_sep_host as HOST
from test_gpu_parity import _record
from test_gpu_sep import _child, _cus, _same_bits

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("case", SEP.ACT_CASES + SEP.PROBES, ids=repr)
def test_block_against_float64_in_the_form_the_product_picks(gpu, case):
    cus = _cus(gpu)
    got = SEP.device_outputs(case, gpu)
    r = SEP.check_case(case, got, cus)
    for a in SEP.ARITHS:
        last = SEP.act_forms(case, a, cus)[-1]
        print(f"{case} {a} {' '.join(r['forms'][a])}: worst |y - ref| / bound = {r['ratios'][a]:.4f} "
              f"(frames below the lengths: {r['valid'].get(a, float('nan')):.4f})")
        _record("act_block_f64", case=case.name, gemm=a, forms=" ".join(r["forms"][a]), tile=last[0], form=last[1], epi=last[2],
                activation=case.activation, residual_mode=case.residual_mode, arith=last[4], port=last[5], ratio=r["ratios"][a],
                ratio_valid=r["valid"].get(a))
    assert not r["failures"], r["failures"]
    # the same rows as a small batch of their own (the 64 x 32 tile or the latency kernel): the same bits, see test_gpu_sep.py
    rows = SEP.sampled_rows(case)
    if case.B > len(rows):
        small = case.small(len(rows))
        fused = lambda c, a: any(l["kind"] == "fused" for L in SEP.plan(c, a, cus) for l in L)
        ariths = [a for a in ("f16x2", "bf16x3") if not fused(case, a) and not fused(small, a)]
        alone = SEP.device_rows(case, gpu, rows, ariths)
        for a in ariths:
            same = bool(np.array_equal(alone[a].numpy().view(np.uint32), got[a]["y"][rows].numpy().view(np.uint32)))
            _record("act_block_bits", case=case.name, what=f"{a}: rows {rows} alone", same=same)
            assert same, (case.name, a, rows)


def test_act_table_reaches_every_form_on_this_device(gpu):
    """The coverage test_sep_host.py computes for 256 compute units (test_the_act_table_meets_every_form), on the count of the
    device the cases really ran on."""
    cus = _cus(gpu)
    missing, seen = HOST.act_coverage(cus)
    _record("act_block_forms", cus=cus, forms=sorted(str(f) for f in seen["f16x2"]), missing=[str(m) for m in missing])
    assert not missing, (cus, missing)


_BASE = {}


@pytest.mark.parametrize("env", [{"VASR_PW3_TILE": str(t)} for t in sorted(SEP.SPLIT_TILES)] + [{"VASR_PW_LAT": "0"}],
                         ids=lambda env: "_".join(f"{k}{v}" for k, v in env.items()))
def test_forced_split_tiles_and_the_chunked_kernel_give_the_products_bits(gpu, tmp_path, env):
    """VASR_PW3_TILE=1..5 and VASR_PW_LAT=0 (devtools build, one child process per setting) on four small cases, one each of
    SELU / add, hardtanh / max, SELU / max and ReLU / max: the bits of the product's choice in f16x2 and bf16x3 -- every tile's
    Epilogue<1> and Epilogue<2>, plain, DUAL and RES with max, computes what the tile the product picked computes (which the
    parametrised test above judges against float64)."""
    if not _BASE:       # the product's own outputs, once for the six settings
        for n in SEP.ACT_FORCED:
            got = SEP.device_outputs(SEP.BY_NAME[n], gpu, ("f16x2", "bf16x3"), profile=False)
            for a, g in got.items():
                _BASE[f"{n}/{a}"] = g["y"].numpy()
    tag = "_".join(f"{k}{v}" for k, v in env.items())
    forced = _child(tmp_path, tag, env, SEP.ACT_FORCED)
    for key, y in _BASE.items():
        same = _same_bits(forced[key], y)
        _record("act_block_bits", case=key, what=tag, same=same)
        assert same, (env, key)


def test_fused_tile_widths_give_the_same_bits(gpu, tmp_path):
    """Under hardtanh and under SELU (add mode, the residual folded): 64- and 128-frame tiles of the fused kernel forced
    (VASR_FUSED_MIN_TILES=1, VASR_FUSED_TILE; devtools build, one child process each) give the same bits, the product's own
    where its choice is a fused form, inside the bound."""
    cus = _cus(gpu)
    outs = {t: _child(tmp_path, f"fused{t}", {"VASR_FUSED_MIN_TILES": "1", "VASR_FUSED_TILE": t}, SEP.ACT_FUSED)
            for t in ("64", "128")}
    for n in SEP.ACT_FUSED:
        case = SEP.BY_NAME[n]
        for t in ("64", "128"):
            assert int(outs[t][f"{n}/f16x2/counts"][0]) == case.blocks[case.under]["repeat"], (n, t)
        assert _same_bits(outs["64"][f"{n}/f16x2"], outs["128"][f"{n}/f16x2"]), n
        got = SEP.device_outputs(case, gpu, ("f16x2",))
        r = SEP.check_case(case, got, cus, ("f16x2",))
        assert not r["failures"], r["failures"]
        if any(f.startswith("fused") for f in r["forms"]["f16x2"]):
            assert _same_bits(got["f16x2"]["y"].numpy(), outs["64"][f"{n}/f16x2"]), n
        _record("act_block_bits", case=n, what="fused 64 == 128", same=True)


def test_fused_kernel_and_two_kernel_form_both_inside_the_bound(gpu, tmp_path):
    """The same two blocks with the fused kernel switched off (VASR_FUSED=0: Toeplitz depthwise, then a split tile, the last
    sub-layer with the DUAL epilogue): no fused launch, and every element inside the bound of the plan without the fused
    kernel, as the product's fused form is inside the bound of its own (the two round differently: no bit equality)."""
    cus = _cus(gpu)
    off = _child(tmp_path, "fused_off", {"VASR_FUSED": "0"}, SEP.ACT_FUSED)
    for n in SEP.ACT_FUSED:
        case = SEP.BY_NAME[n]
        got = SEP.device_outputs(case, gpu, ("f16x2",))
        r = SEP.check_case(case, got, cus, ("f16x2",))
        assert not r["failures"], r["failures"]
        # the two-kernel form: the same leading output (its GEMM does not depend on the switch), the plan without the fused kernel
        assert int(off[f"{n}/f16x2/counts"][0]) == 0, n
        two = {"f16x2": dict(got["f16x2"], y=torch.from_numpy(off[f"{n}/f16x2"]),
                             counts=tuple(int(v) for v in off[f"{n}/f16x2/counts"]))}
        r2 = SEP.check_case(case, two, cus, ("f16x2",), fused=False)
        assert not r2["failures"], r2["failures"]
        _record("act_block_f64", case=n, gemm="f16x2", forms=" ".join(r2["forms"]["f16x2"]), tile="two-kernel", form="DUAL",
                epi=SEP.epilogue_kind(1, case.activation, False), activation=case.activation, residual_mode="add", arith="f16x2",
                port=False, ratio=r2["ratios"]["f16x2"], ratio_valid=r2["valid"].get("f16x2"))
