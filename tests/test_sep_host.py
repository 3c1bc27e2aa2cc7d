"""CPU checks of tests/sep_reference.py, the float64 chain, error bound and kernel-choice restatement tests/test_gpu_sep.py
judges the separable block by: the chain against the oracle's float64 graph, the bound against honest float32 arithmetic
(not tighter than that) and against six defects (far tighter than those), the case table against the list of forms it
claims to reach, and the restated choice against the library's own host arithmetic."""
import numpy as np
import pytest
import torch

import sep_reference as SEP

CUS = 256          # the table's claims are stated for an MI355X's 256 compute units (the GPU test takes the device's count)
SMALL = [c for c in SEP.CASES if c.B <= 24]


def _lead(case, x, lens):
    """Stand-in for the device's own leading-block output: the float32 evaluation of the leading blocks."""
    sd = SEP.weights(case)
    if not case.under:
        return sd, torch.from_numpy(x), lens
    v, lo = SEP.f32_chain(torch.from_numpy(x), lens, sd, case.blocks[:case.under], 0, under=-1)
    return sd, v, lo


def _reference(case):
    x, lens = SEP.inputs(case)
    sd, lead, lens_u = _lead(case, x, lens)
    plans = {a: SEP.plan(case, a, CUS)[case.under:] for a in SEP.ARITHS}
    ref, bounds, lo = SEP.chain(lead.double(), lens_u, sd, case.blocks[case.under:], case.under, plans)
    return sd, lead, lens_u, lens, ref, bounds, lo


@pytest.mark.parametrize("case", SMALL, ids=repr)
def test_chain_equals_the_oracles_float64_graph(case):
    """The restatement that carries the magnitudes computes the oracle's function (BN written as an affine: a few float64
    roundings apart), lengths included; the inputs hold what they promise."""
    from oracle import quartznet_oracle as O
    x, lens = SEP.inputs(case)
    assert x.shape == (case.B, case.feat_in, case.T) and int(lens.max()) == case.T and int(lens.min()) == 1
    short = int(np.argmin(lens))
    assert float(np.abs(x[short, :, lens[short]:]).max()) > 0                 # what lies past a length is not zero
    sd = SEP.weights(case)
    plans = {"fp32": SEP.plan(case, "fp32", CUS)}
    ref, bounds, lo = SEP.chain(torch.from_numpy(x).double(), lens, sd, case.blocks, 0, plans)
    want, wlen = O.encoder_forward(x, torch.from_numpy(lens), sd, case.blocks, dtype=torch.float64)
    assert ref.shape == want.shape
    assert np.array_equal(wlen.numpy().astype(np.float32), lo.astype(np.float32))
    assert float(((ref - want).abs() / bounds["fp32"]).max()) < 1e-6
    assert (bounds["fp32"] >= SEP.TINY).all() and torch.isfinite(bounds["fp32"]).all()


STRUCTURAL = ("mask_late", "res_lens", "dw_pad", "k_chunk", "shift_before_res")


def _applies(mutant, case):
    """res_lens: the length vectors of a block's input and output are equal in every layout the product runs (a residual
    across a strided block is refused), so the wrong vector is the encoder's input lengths, and the defect exists only
    behind the stride-2 prologue."""
    cfg = case.blocks[case.under]
    if mutant == "res_lens":
        return cfg["residual"] and any(b["stride"][0] > 1 for b in case.blocks[:case.under])
    if mutant in ("k_chunk", "shift_before_res"):
        return cfg["residual"]
    if mutant in ("mask_late", "dw_pad"):
        return cfg["separable"]
    return True


@pytest.mark.parametrize("case", SEP.CASES, ids=repr)
def test_float32_stays_inside_the_bound_and_defects_leave_it(case):
    """The bound is not vacuous: a plain sequential float32 evaluation of the judged chain stays inside the fp32 bound,
    every element (the split arithmetics' bounds are no tighter than the fp32 one).  And it is tight enough for what it is
    for: every structural defect that can occur in the case's block leaves the bound of EVERY arithmetic, on every case up to
    B = 64 -- each family of the table (256-, 512-, 768-filter blocks, the width-changing and the unfoldable residual, the
    prologue, the final shape, T = 300) and the fused kernel's bound among them; the larger batches of a family differ in the
    tile alone, which this host evaluation does not have."""
    sd, lead, lens_u, lens, ref, bounds, lo = _reference(case)
    y, yl = SEP.f32_chain(lead, lens_u, sd, case.blocks[case.under:], case.under)
    assert np.array_equal(yl, lo)
    worst, msg = SEP.judge(y, ref, bounds["fp32"])
    assert msg is None, msg
    assert worst > 1e-4                                                    # ... and float32 really differs from float64 here
    for a in ("f16x2", "bf16x3"):
        assert (bounds[a] >= bounds["fp32"]).all(), a
    if case.B > 64:
        return
    missed = []
    for mutant in STRUCTURAL:
        if not _applies(mutant, case):
            continue
        y, _ = SEP.f32_chain(lead, lens_u, sd, case.blocks[case.under:], case.under, under=0, mutant=mutant, first_lens=lens)
        ratios = {a: SEP.judge(y, ref, bounds[a])[0] for a in SEP.ARITHS}
        print(case, mutant, " ".join(f"{a} {r:.3g}" for a, r in ratios.items()))
        missed += [(mutant, a, r) for a, r in ratios.items() if not r > 1.0]
    assert not missed, missed


def test_every_structural_defect_is_tried_on_every_family():
    tried = {m: [c.name for c in SEP.CASES if c.B <= 64 and _applies(m, c)] for m in STRUCTURAL}
    assert tried["res_lens"] == ["pro_b16_then_res"]
    for m in ("mask_late", "dw_pad"):
        for family in ("c256_b", "c512_b", "c512w_", "r512_b", "c768_", "pro_", "c256_t300", "c512_t300", "r512_t300"):
            assert any(n.startswith(family) for n in tried[m]), (m, family)
    for m in ("k_chunk", "shift_before_res"):
        for family in ("c256_b", "c512_b", "c512w_", "r512_b", "c768_", "c256_t300", "c512_t300", "r512_t300"):
            assert any(n.startswith(family) for n in tried[m]), (m, family)
    fused = {f for c in SEP.CASES if c.B <= 64 for f in SEP.form_names(SEP.plan(c, "f16x2", CUS)[c.under])}
    assert {"fused64", "fused64+res"} <= fused


def test_an_11_bit_weight_is_rejected():
    """The low fp16 weight plane dropped (every 1x1 weight of the block rounded to 11 bits) leaves the bound of every
    arithmetic on at least one case.  Not on all: the defect is a random relative 2^-12 a weight, ~ 2^-12 sqrt(C) of the
    typical magnitude in the sum, and the bound is the worst case C u A of the block's layers propagated through the
    later ones; from K = 512 on the bit equalities of test_gpu_sep.py are what would see it."""
    hit = {a: [] for a in SEP.ARITHS}
    for case in SEP.CASES:
        if case.B > 16 or case.T > 201:
            continue
        sd, lead, lens_u, lens, ref, bounds, lo = _reference(case)
        y, _ = SEP.f32_chain(lead, lens_u, sd, case.blocks[case.under:], case.under, under=0, mutant="w_11bit")
        for a in SEP.ARITHS:
            r = SEP.judge(y, ref, bounds[a])[0]
            print(case, "w_11bit", a, f"{r:.3g}")
            if r > 1.0:
                hit[a].append(case.name)
    assert all(hit.values()), hit


def test_the_table_meets_every_form():
    """Computed by the restated choice at 256 compute units: all five split tiles and the latency kernel, both fused widths
    with and without the folded residual, DUAL and RES at every tile the product can pick them at, the masked form on the
    port, Toeplitz / packed-FMA / generic depthwise -- each in a block under test."""
    seen = {a: set() for a in SEP.ARITHS}
    for c in SEP.CASES:
        for a in SEP.ARITHS:
            seen[a].update(SEP.form_names(SEP.plan(c, a, CUS)[c.under]))
    f16 = seen["f16x2"]
    assert {"fused64", "fused64+res", "fused128", "fused128+res", "dw:toeplitz", "dw:fma", "dw:generic"} <= f16
    tiles = ["512x128", "256x128", "128x64", "256x64", "lat"]
    for t in tiles:
        assert f"{t}:plain:f16x2" in f16, t
        assert f"{t}:DUAL:f16x2" in f16 or f"{t}:DUAL:f16x2:port" in f16, t
        assert f"{t}:RES:f16x2:port" in f16, t
    assert "64x32:DUAL:f16x2" in f16 or "64x32:DUAL:f16x2:port" in f16          # K = 512 + 256: no latency form
    assert {"lat:masked:f16x2:port", "512x128:masked:f16x2:port"} <= f16
    assert any(n.endswith(":masked:bf16x3") for n in f16)                     # a residual GEMM whose source has no maxima
    for a in ("bf16x3", "fp32"):
        assert {"dw:fma", "dw:generic"} <= seen[a] and not any(n.startswith(("fused", "dw:toeplitz", "lat")) for n in seen[a])
    for t in ["512x128", "256x128", "128x64", "256x64", "64x32"]:
        got = seen["bf16x3"]
        assert f"{t}:plain:bf16x3" in got, t
        assert f"{t}:DUAL:bf16x3" in got or f"{t}:DUAL:bf16x3:port" in got, t
        assert f"{t}:RES:bf16x3:port" in got, t
    # both folded forms at each tile a 512-filter block can take: K = 512 + 512 and the width-changing K = 512 + 256
    dual = {a: set() for a in SEP.ARITHS}
    for c in SEP.CASES:
        for a in ("f16x2", "bf16x3"):
            dual[a].update((l["tile"], l["K"]) for l in SEP.plan(c, a, CUS)[c.under]
                           if l["kind"] == "gemm" and l["epi"] == "DUAL" and l["M"] == 512)
    assert dual["f16x2"] >= {(t, k) for t in (1, 2, 3, 5) for k in (768, 1024)} | {(4, 768), ("lat", 1024)}, dual["f16x2"]
    assert dual["bf16x3"] >= {(t, k) for t in (1, 2, 3, 4, 5) for k in (768, 1024)}, dual["bf16x3"]
    # a first and a later sub-layer are both seen: every separable block under test repeats
    assert all(c.blocks[c.under]["repeat"] >= 2 for c in SEP.CASES if c.blocks[c.under]["separable"] and c.under)
    # the batch ranges of the 256-channel block at T = 100, as the product's arithmetic gives them at 256 units
    form = lambda B: SEP.form_names(SEP.plan(SEP._c256("x", B, 33, False), "f16x2", CUS)[1])
    assert form(47)[:2] == ["dw:toeplitz", "lat:plain:f16x2"] and form(48)[0] == "fused64" and form(128)[0] == "fused64"
    assert form(129)[:2] == ["dw:toeplitz", "128x64:plain:f16x2"] and form(191)[1] == "128x64:plain:f16x2"
    assert form(192)[1] == "256x64:plain:f16x2" and form(204)[1] == "256x64:plain:f16x2" and form(205)[0] == "fused128"
    tile = lambda B: SEP.split_tile(512, 128, B, CUS)
    assert [tile(B) for B in (23, 24, 95, 96, 191, 192, 217, 218, 256)] == [4, 3, 3, 2, 2, 5, 5, 1, 1]
    assert SEP.split_tile(768, 128, 64, CUS) == 2 and SEP.split_tile(768, 128, 63, CUS) == 3


def test_restated_choice_equals_the_librarys():
    """fused_tile_choice against vasr_fused_tile_choice (devtools library, pure host arithmetic) over (tiles, units); the
    Toeplitz shapes against vasr_depthwise_mfma_table_size; the pitch against vasr_padded_frames."""
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    for cus in (1, 7, 64, 104, 192, 208, 228, 255, 256, 304):
        for tiles in list(range(0, 700)) + [1023, 1024, 1025, 6144, 100000]:
            assert SEP.fused_tile_choice(tiles, cus) == L.vasr_fused_tile_choice(tiles, cus), (tiles, cus)
    for k in range(1, 100, 2):
        for dil in (1, 2, 3):
            assert ((k, dil) in SEP.TOEPLITZ) == (L.vasr_depthwise_mfma_table_size(k, dil) > 0), (k, dil)
    for T in (1, 100, 128, 129, 300, 1030):
        assert SEP.padded(T) == int(L.vasr_padded_frames(T))
