"""-m gpu: QuartzNet's separable block (depthwise K-tap conv -> 1x1 conv + BN -> residual -> ReLU) against float64 in every
kernel form the product picks for it (tests/sep_reference.py: reference, elementwise bound, the restated kernel choice, the
case table).  Per case and arithmetic (f16x2, bf16x3, fp32): the encoder of the case through asr.JasperEncoder
(vasr_encoder_f32), the launch counts of the fused / depthwise / pointwise profile classes equal to what the restated choice
predicts for the device's compute-unit count, every stored element inside the bound of the judged chain evaluated on the
device's own leading-block output, equal encoded lengths, and sampled rows bit-equal to the same rows run as a small batch
(the tile of the large batch against the 64 x 32 tile / latency kernel).  Then the bit equalities the other files assert end
to end, per block: 64- and 128-frame fused tiles, every forced split tile, the latency kernel against the chunked kernel.

Largest |y - ref| / bound seen on an MI355X (256 compute units; all elements | frames below the row lengths only), by the tile
and form of the launch that ends the block under test (the first sub-layer's plain GEMM on the same tile, or its fused kernel,
lies inside each figure; the fp32 arithmetic has one tile):
    tile      form      f16x2              bf16x3             fp32
    512x128   masked    0.277 | 9.5e-3     0.279 | 1.4e-2
    512x128   RES       0.214 | 3.1e-3     0.214 | 3.2e-3
    512x128   DUAL      0.203 | 1.4e-3     0.203 | 2.1e-3
    256x128   RES       0.289 | 1.1e-2     0.289 | 1.2e-2
    256x128   DUAL      0.228 | 1.7e-3     0.228 | 2.8e-3
    256x64    plain     0.371 | 6.0e-4     0.371 | 6.2e-4
    256x64    RES       0.238 | 3.7e-3     0.238 | 3.7e-3
    256x64    DUAL      0.267 | 2.3e-3     0.276 | 2.4e-3
    128x64    plain     0.338 | 7.4e-4     0.338 | 8.3e-4
    128x64    RES       0.189 | 4.2e-3     0.189 | 4.2e-3
    128x64    DUAL      0.254 | 1.4e-3     0.255 | 2.4e-3
    64x32     plain     0.265 | 1.9e-2     0.290 | 1.4e-2
    64x32     masked                       0.389 | 1.0e-2
    64x32     RES                          0.263 | 8.7e-3
    64x32     DUAL      0.217 | 1.6e-3     0.218 | 3.5e-3
    latency   plain     0.290 | 5.2e-4
    latency   masked    0.376 | 8.5e-3
    latency   RES       0.263 | 8.6e-3
    latency   DUAL      0.218 | 2.5e-3
    fused, 64 frames, folded residual     0.003 | 2.6e-3
    fused, 128 frames, folded residual    0.002 | 1.5e-3
    fp32      plain                                           0.371 | 2.2e-2
    fp32      masked                                          0.389 | 1.1e-2
    fp32      RES                                             0.289 | 1.1e-2
    fp32      DUAL                                            0.276 | 3.3e-3
(The fused kernel without a folded residual is a block's first sub-layer here, under the plain rows; a block that ends in the
fused kernel is followed by the identity trailing block, whose output has no column of the kind described next.)
The maximum over all elements sits in every arithmetic on the SAME element of a case: a column past the row's length of a block
that writes the encoder's output, where the output is relu(shift (+ residual shift)) and the error is the float32 rounding of
the BN affine itself (bound 7 u, no slack to average into).  Below the lengths the worst-case n u accumulation term and the
propagation of the first sub-layer's bound through |w_dw| and |W| of the second leave the bound 10^2 ... 10^3 above what the
kernels do: it catches what is structurally wrong (test_sep_host.py: masks, lengths, padding, a dropped chunk, a missing
shift -- each at 13 times the bound or more on every case it can occur in), not a lost low-order product at K = 512 -- that
is what the bit equalities are for.  The opt-in bf16x2 arithmetic: 9.2e-6 of the utterance's largest output on its one case
(allowed: 2e-3).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sep_reference as SEP
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.mark.parametrize("case", SEP.CASES, ids=repr)
def test_block_against_float64_in_the_form_the_product_picks(gpu, case):
    got = SEP.device_outputs(case, gpu)
    r = SEP.check_case(case, got, _cus(gpu))
    for a in SEP.ARITHS:
        print(f"{case} {a} {' '.join(r['forms'][a])}: worst |y - ref| / bound = {r['ratios'][a]:.4f} "
              f"(frames below the lengths: {r['valid'].get(a, float('nan')):.4f})")
        _record("sep_block_f64", case=case.name, gemm=a, forms=" ".join(r["forms"][a]), ratio=r["ratios"][a],
                ratio_valid=r["valid"].get(a))
    assert not r["failures"], r["failures"]
    # The same rows as a small batch of their own take the 64 x 32 tile or the latency kernel: no reduction order depends on
    # the tile or on the batch, so the tile the product picked for the whole batch must give those rows the same BITS -- a
    # low product dropped in one tile shape, which the worst-case bound above would let through at K = 512, shows here.  (Not
    # across the fused kernel and the two-kernel form, which round differently, nor in fp32, which has tiles of its own.)
    rows = SEP.sampled_rows(case)
    if case.B > len(rows):
        small = SEP.Case(case.name, case.feat_in, case.blocks, case.under, len(rows), case.T, case.kind)
        fused = lambda c, a: any(l["kind"] == "fused" for L in SEP.plan(c, a, _cus(gpu)) for l in L)
        ariths = [a for a in ("f16x2", "bf16x3") if not fused(case, a) and not fused(small, a)]
        alone = SEP.device_rows(case, gpu, rows, ariths)
        for a in ariths:
            same = bool(np.array_equal(alone[a].numpy().view(np.uint32), got[a]["y"][rows].numpy().view(np.uint32)))
            _record("sep_block_bits", case=case.name, what=f"{a}: rows {rows} alone", same=same)
            assert same, (case.name, a, rows)


def test_table_reaches_every_form_on_this_device(gpu):
    """The coverage test_sep_host.py computes for 256 compute units, on the count of the device the cases really ran on:
    the fused kernel in both widths with and without the folded residual, and every split tile."""
    cus = _cus(gpu)
    seen = set()
    for c in SEP.CASES:
        seen.update(SEP.form_names(SEP.plan(c, "f16x2", cus)[c.under]))
    _record("sep_block_forms", cus=cus, forms=sorted(seen))
    assert {"fused64", "fused64+res", "fused128", "fused128+res"} <= seen, (cus, sorted(seen))
    for t in ("512x128", "256x128", "128x64", "256x64", "lat"):
        assert any(n.startswith(t + ":") for n in seen), (cus, t)


def test_reduced_bf16x2_mode_on_one_block(gpu):
    """The opt-in reduced arithmetic, held to the bf16-level bound test_gpu_jasper.py applies to it: 2e-3 of the utterance's
    largest output (or of 1), padded frames included."""
    case = SEP.BY_NAME[SEP.BF16X2_CASE]
    got = SEP.device_outputs(case, gpu, ("bf16x2", "fp32"), profile=False)
    sd = SEP.weights(case)
    x, lens = SEP.inputs(case)
    plans = {"fp32": SEP.plan(case, "fp32", _cus(gpu))[case.under:]}
    ref, _, _ = SEP.chain(got["bf16x2"]["lead"].double(), SEP.lens_chain(lens, case.blocks[:case.under]), sd,
                          case.blocks[case.under:], case.under, plans)
    y = got["bf16x2"]["y"].double()
    err = max(float((y[b] - ref[b]).abs().max()) / max(1.0, float(ref[b].abs().max())) for b in range(case.B))
    _record("sep_block_bf16x2", case=case.name, err=err)
    assert err <= 2e-3, err


def _child(tmp_path, tag, env, names):
    """The named cases in f16x2 and bf16x3 on the devtools build with `env`, in ONE child process -> its arrays."""
    from viet_asr_amd import _lib
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    path = str(tmp_path / f"{tag}.npz")
    out = subprocess.run([sys.executable, os.path.join(HERE, "sep_child.py"), path] + list(names),
                         env={**os.environ, "VASR_LIB_PATH": dev, **env}, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "SEP_CHILD_OK" in out.stdout, (env, out.stdout[-2000:], out.stderr[-2000:])
    return dict(np.load(path))


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


FUSED_CASES = ["c256_b48", "c256_b48_res", "c256_t300_b16_res"]


def test_fused_tile_widths_give_the_same_bits_per_block(gpu, tmp_path):
    """64- and 128-frame tiles of the fused kernel forced (VASR_FUSED_MIN_TILES=1, VASR_FUSED_TILE, devtools build, one child
    process each): the same bits, equal to the product's own choice where that is a fused form, and inside the bound."""
    cus = _cus(gpu)
    outs = {t: _child(tmp_path, f"fused{t}", {"VASR_FUSED_MIN_TILES": "1", "VASR_FUSED_TILE": t}, FUSED_CASES)
            for t in ("64", "128")}
    for n in FUSED_CASES:
        case = SEP.BY_NAME[n]
        # every sub-layer of the block is fused, but one that writes the encoder output (no trailing block)
        fused = case.blocks[case.under]["repeat"] - (1 if case.under + 1 == len(case.blocks) else 0)
        for t in ("64", "128"):
            assert int(outs[t][f"{n}/f16x2/counts"][0]) == fused, (n, t)
        assert _same_bits(outs["64"][f"{n}/f16x2"], outs["128"][f"{n}/f16x2"]), n
        got = SEP.device_outputs(case, gpu, ("f16x2",))
        r = SEP.check_case(case, got, cus, ("f16x2",))
        assert not r["failures"], r["failures"]
        if any(f.startswith("fused") for f in r["forms"]["f16x2"]):
            assert _same_bits(got["f16x2"]["y"].numpy(), outs["64"][f"{n}/f16x2"]), n
        _record("sep_block_bits", case=n, what="fused 64 == 128", same=True)


def test_forced_split_tiles_and_the_chunked_kernel_give_the_products_bits(gpu, tmp_path):
    """VASR_PW3_TILE=1..5 and VASR_PW_LAT=0 (devtools build, one child process per setting) on the small-batch cases: the
    bits of the product's choice, in f16x2 and bf16x3 -- the reduction order depends neither on the tile nor on the
    latency kernel.  The product's outputs are judged against float64 by the parametrised test above."""
    base = {}
    for n in SEP.FORCED:
        got = SEP.device_outputs(SEP.BY_NAME[n], gpu, ("f16x2", "bf16x3"), profile=False)
        for a, g in got.items():
            base[f"{n}/{a}"] = g["y"].numpy()
    settings = [{"VASR_PW3_TILE": str(t)} for t in sorted(SEP.SPLIT_TILES)] + [{"VASR_PW_LAT": "0"}]
    for env in settings:
        tag = "_".join(f"{k}{v}" for k, v in env.items())
        forced = _child(tmp_path, tag, env, SEP.FORCED)
        for key, y in base.items():
            same = _same_bits(forced[key], y)
            _record("sep_block_bits", case=key, what=tag, same=same)
            assert same, (env, key)
