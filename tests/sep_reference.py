"""What the separable-block tests share (tests/test_gpu_sep.py, tests/test_gpu_act_f64.py, tests/test_sep_host.py): a float64 restatement of a short chain
of JasperBlocks with an ELEMENTWISE error bound per arithmetic, the restatement of the product's kernel choice (which form
every sub-layer takes), the case table and its inputs, a device-like float32 evaluation with switchable defects, and the
runner that puts one case through asr.JasperEncoder (vasr_encoder_f32) and lists what it finds wrong.

A case is an encoder of one to three blocks: an optional cheap LEADING block (a 1x1 conv 64 -> C; a sub-layer whose input
carries no published maxima can take neither the Toeplitz nor the fused form, so the block under test must not come first), the
block UNDER TEST, and an optional TRAILING block that passes every channel through: a 1x1 conv C -> C whose weight is the
identity matrix and whose BatchNorm is the identity (gamma 1, beta 0, mean 0, var chosen so that the float32 alpha is exactly
1; weights() overwrites synth's draw).  The trailing block is there because the last sub-layer of an encoder's LAST block
writes the port tensor and is never fused (encoder_run.cpp run_encoder: !enc_out): the fused kernel with its folded residual, and
the dual-source GEMM on a padded interior buffer, are only reached by a block that is not the last one.

THE REFERENCE is the float64 graph of oracle.quartznet_oracle (jasper_block_forward; chain() below restates it so that the
magnitudes can be carried along, and test_sep_host.py holds the two equal) evaluated on the DEVICE'S OWN output of the leading
block: that block is run once more as the last block of a one-block encoder with the same weights (same kernel, same tile:
its GEMM tiles the same padded pitch) and its float32 output, converted exactly, is the input of the reference.  The leading
block's error is therefore not part of the bound.  A trailing block IS part of the judged chain, at little cost to
what the bound says about the block under test: |W_trail| |alpha| = I hands every element's bound on unmixed, and the trailing
block's own terms are relative to |y| itself (one non-zero product a row: A_acc = |y|), which the block's own A dominates.
(Behind a dense trailing conv the bound of an output is the sum of all C channels' bounds and exceeds the output itself.)

THE BOUND.  chain() carries the values v and, per arithmetic, an elementwise error bound E through the graph: E_out =
|op|(E_in) + the layer's own terms (first order; ReLU and the masks are 1-Lipschitz, |op| = the same operation with |w_dw|,
|W_pw| |alpha|).  A layer's own terms are relative to the magnitude A of what that layer sums, computed in float64 from the
absolute values of ITS operands: A_dw = |w_dw| * |x masked|, A_acc = |W| |d|, A_y = |alpha| A_acc + |b| + |mean alpha|, the
residual branch likewise.  (The magnitudes restart from |v| at every layer: carried through the whole block instead they
would grow by each layer's cancellation, ~ sqrt(K C) a sub-layer, and the bound with them -- the float32 evaluation of
test_sep_host.py would then sit at 5e-5 of it.)  With u = 2^-24 (EPS), per layer:

  depthwise, packed / generic FMA kernels and the fused kernel's producers (float32 FMAs):      K u A_dw
  depthwise, Toeplitz form on the matrix pipe (f16x2 mode; encoder_dw_mfma.hip):    K u A_dw + the f16x2 terms below
  1x1 GEMM, every arithmetic: n = C (C + C_res over both K ranges of a folded residual) accumulations into float32: n u A_acc
    -- the split arithmetics form three (f16x2) or six (bf16x3) products per K index, but on the matrix pipe: every kernel
    here issues 16- or 32-deep MFMAs (32x32x16; the Toeplitz form 16x16x32), so an accumulator is rounded 3 C / 16 resp.
    6 C / 16 <= C times, not once per product.  The premise, which the test thereby holds the kernels to: the products
    inside one instruction are summed with no more error than one float32 rounding per K index.
  BatchNorm affine y = alpha acc + beta, alpha = g / sqrt(var + 1e-3), beta = b - mean alpha in float32 (model_build.cpp
    bn_affine): alpha carries 4 roundings (var + eps, sqrt, 1 / x, the product), beta 2 more on |b| + |mean alpha|, the
    epilogue's multiply and add one each; a folded residual rounds alpha W once more instead of multiplying in the epilogue:
                                                                                                    7 u A_y
  residual add (RES epilogue) and the sum of two folded shifts:                                     1 u (A_y + A_res)

  f16x2 (pack_pointwise_weights_f16x2, split2h, f16_scale): an operand v is multiplied by a power of two s that puts the
    tensor's maximum M into [2^14, 2^15), then hi = rne16(s v), lo = rne16(s v - hi).  fp16 has 11 significant bits and a
    subnormal spacing of 2^-24: |s v - hi| <= 2^-11 |s v| and |(s v - hi) - lo| <= max(2^-22 |s v|, 2^-25).  Unscaled, with
    1 / s <= 2^-14 M:  |v - v^| <= 2^-22 |v| + 2^-39 M.  The kernels add hi hi + hi lo + lo hi and drop lo lo <= 2^-22 |w||x|
    (to first order), so per product  |w x - kept| <= 3 * 2^-22 |w||x| + 2^-39 (M_x |w| + M_w |x|):
        relative 3 * 2^-22 (1 + 2^-10) A_acc,   floor 2^-39 (1 + 2^-10) (M_x sum_k |W_mk| + M_w sum_k A_k)
    -- (1 + 2^-10) covers every product of two of these terms (each at most 2^-11 of a first-order one).  M_w = the largest
    |w| of the pack (per layer; per channel for the Toeplitz taps), M_x = the utterance's maximum the producer published,
    i.e. max over valid frames of the device's tensor <= max(|v| + E); in the fused kernel M_x = max |x| * dw_l1
    (encoder_fused.hip: a bound taken before the depthwise output exists), and a dual source takes the larger of both maxima.
  bf16x3 (pack_pointwise_weights_bf16x3, split3): three bf16 planes of 8 significant bits hold a float32 exactly
    (|mid| <= 2^-8 |v|, |lo| <= 2^-16 |v|); six of the nine products are kept, mid lo + lo mid + lo lo are dropped:
        relative (2^-23 + 2^-32) A_acc.

The bound is the sum over the chain, + 2^-126 so that exact zeros compare.  Every element of the stored tensor is judged, the
columns past a row's length too: the reference computes them from the masked inputs (relu(shift (+ residual))).

HARDTANH, SELU AND MAX RESIDUALS (vasr_set_activation; Case.activation / Case.residual_mode, the encoder's: every block of a case
runs them; ACT_CASES, PROBES, tests/test_gpu_act_f64.py).  With activation "relu" and residual_mode "add" everything above is
computed exactly as before, same bits.  Otherwise, behind a layer's pre-activation y with bound E_in:
  hardtanh = min(max(y, -1), 1): 1-Lipschitz, and min and max round nothing:                        E_out = E_in
  SELU = lambda y (y > 0), lambda alpha expm1(y) (y <= 0), torch's constants:       E_out = L E_in + S u |selu(y)|
    L = the supremum of |selu'| over [y - E_in, y + E_in]: selu' is lambda on x > 0 and lambda alpha e^x on x <= 0, so L = lambda
    where y - E_in > 0 and lambda alpha exp(min(y + E_in, 0)) elsewhere -- at most lambda alpha = 1.7581, and small for deeply
    negative y (this L is a true Lipschitz constant over the interval, not a first-order one).  S = 4 (SELU_OWN): expm1f within
    1 ulp (ROCm's published device-math accuracy), the float32 rounding of the constant lambda alpha, one multiply, one spare.
    S is a constant of the bound, not a knob: an element that exceeds it on the identity probes is a finding.
  max residual, y = max(a, r) before the activation (RES epilogue with res_max; never folded, so no DUAL and no fused kernel
    with a folded residual; the residual GEMM itself is Epilogue<0> with the relu flag clear, as under add: no clamp):
    |max(a, r) - max(a', r')| <= max(E_a, E_r), and the "1 u (A_y + A_res)" term of the add disappears with the add (max rounds
    nothing); A = max(A_y, A_res).
The columns past a row's length then hold selu(shift (+ residual shift)) resp. act(max(shift, residual shift)), and are judged.
An ACT_CASE's block under test has the gamma and beta of its BNs scaled per channel by 2^-14 ... 2^6 (spread_scales; under max
beta of the two max arguments one unit lower), so that its pre-activations lie on both sides of, at and far beyond every point
where an activation changes behaviour -- test_sep_host.py asserts the shares --, and its trailing block is not the identity but
alpha = 1/2, beta = 1/4 (weights() says why).  An identity PROBE (_probe) is a first block whose conv and BN are the identity:
its pre-activation is the input itself, a sweep (probe_values), and with `sparse` its GEMMs' accumulation terms count the one
non-zero weight of a row, so that the probe's bound is ~ 12 u |act(x)|: the affine's 7, SELU's 4, one product.
"""
import numpy as np
import torch

EPS = 2.0 ** -24
TINY = 2.0 ** -126
R16 = 3 * 2.0 ** -22 * (1 + 2.0 ** -10)       # f16x2, relative
F16 = 2.0 ** -39 * (1 + 2.0 ** -10)           # f16x2, floor per unit of (M_x |w| + M_w |x|)
R3 = 2.0 ** -23 + 2.0 ** -32                  # bf16x3, the three dropped cross products
AFFINE = 7
ARITHS = ("f16x2", "bf16x3", "fp32")
SPLIT_TILES = {1: (512, 128), 2: (256, 128), 3: (128, 64), 4: (64, 32), 5: (256, 64)}
TOEPLITZ = {(33, 1), (39, 1), (51, 1), (63, 1), (75, 1), (87, 2)}    # depthwise_mfma_table_size(K, dilation) > 0


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def same_padding(K, stride, dil):
    if stride > 1 and dil > 1:
        raise ValueError("Only stride OR dilation may be greater than 1")
    return (dil * K) // 2 - 1 if dil > 1 else K // 2


def out_frames(T, K, stride, dil):
    return (T + 2 * same_padding(K, stride, dil) - dil * (K - 1) - 1) // stride + 1


def lens_out(lens, K, stride, dil):
    """MaskedConv1d.get_seq_len followed by the next mask's .to(long)."""
    lf = (np.asarray(lens, dtype=np.int64) + 2 * same_padding(K, stride, dil) - dil * (K - 1) - 1).astype(np.float32)
    return np.trunc(lf / np.float32(stride) + np.float32(1)).astype(np.int64)


def padded(T):
    return (T + 127) // 128 * 128


def blk(filters, kernel, repeat=1, residual=False, separable=True, stride=1, dilation=1):
    return dict(filters=filters, repeat=repeat, kernel=[kernel], stride=[stride], dilation=[dilation], dropout=0.0,
                residual=residual, separable=separable)


def _geo(cfg):
    return cfg["kernel"][0], cfg["stride"][0], cfg["dilation"][0]


# ---- the product's kernel choice, restated -----------------------------------------------------------------------------------
def fused_tile_choice(tiles128, cus):
    """vasr_internal.h fused_tile_choice."""
    if tiles128 <= 0 or cus <= 0:
        return 0
    rounds = -(-tiles128 // cus)
    if tiles128 >= 3 * cus // 4 and tiles128 >= 0.8 * (rounds * cus):
        return 128
    if 2 * tiles128 >= 3 * cus // 8 and 2 * tiles128 <= cus:
        return 64
    return 0


def split_tile(M, cols, batch, cus, groups=1):
    """encoder_pw_split.hip launch_pointwise_split: the VASR_PW3_TILE number of the tile an M-row GEMM over `cols` columns
    (the padded pitch of its input) of `batch` utterances takes."""
    blocks = lambda bm, bn: (M // bm) * (-(-cols // bn)) * batch
    mg = M // groups if groups > 1 else M
    tile = 4
    if mg % 512 == 0 and blocks(512, 128) >= 192:
        tile = 1
    elif mg % 256 == 0 and blocks(256, 128) >= 192:
        tile = 2
    elif mg % 128 == 0 and blocks(128, 64) >= 192:
        tile = 3
    if tile == 2 and mg == 256 and blocks(256, 64) >= 384:
        tile = 5
    if tile == 1:
        n1 = blocks(512, 128)
        if n1 < 0.85 * (-(-n1 // cus) * cus):
            tile = 5
    return tile


def latency_supported(M, K, K1):
    """encoder_pw_lat.hip pointwise_latency_supported."""
    return M % 128 == 0 and K in (256, 512, 1024) and (K1 == 0 or K1 % 256 == 0)


def residual_folds(cfg, cin, residual_mode="add"):
    """model_build.cpp build_encoder: the residual 1x1 conv becomes a second K range of the block's last GEMM (the fold sums:
    add mode only)."""
    k, stride, _ = _geo(cfg)
    if not cfg["residual"] or stride != 1 or not (cfg["separable"] or k == 1) or residual_mode == "max":
        return False
    f = cfg["filters"]
    k1 = f if cfg["repeat"] > 1 else cin
    chunk = 128 if f % 512 == 0 else (64 if f % 256 == 0 else 32)
    return k1 % chunk == 0 and cin % chunk == 0


def plan(case, arith, cus, fused=True):
    """-> list (one entry per block) of lists of launches, in run_encoder's order.  A launch is a dict: kind = "fused" (cols 64
    / 128, dual), "dw" (form toeplitz / fma / generic) or "gemm" (tile = 1 .. 5 or "lat" or "fp32", arith = the arithmetic that
    runs -- a GEMM whose source has no published maxima keeps 3 x bf16 in f16x2 mode --, epi = plain / masked / RES / DUAL,
    port = it writes the unpadded encoder output, mx = whose maximum scales the activations: "in", "dw", "l1").
    Under residual_mode "max" (build_encoder / run_encoder) the residual is never folded: no DUAL GEMM, no fused kernel with a
    folded residual, the last sub-layer of a residual block is not fused and ends in the RES epilogue (with res_max).  The
    activation changes no choice: under hardtanh or SELU in add mode the residual folds as under ReLU.  fused=False: the
    two-kernel form of every sub-layer (VASR_FUSED=0 on the devtools build)."""
    B, T = case.B, case.T
    mode = getattr(case, "residual_mode", "add")
    split = arith != "fp32"
    f16 = arith == "f16x2"
    cin = case.feat_in
    first = case.blocks[0]
    in_place = first["separable"] and not first["residual"]
    ld = T if in_place else padded(T)
    has_amax = False
    out = []
    for i, cfg in enumerate(case.blocks):
        last_block = i + 1 == len(case.blocks)
        k, stride, dil = _geo(cfg)
        f, rep, sep, res = cfg["filters"], cfg["repeat"], cfg["separable"], cfg["residual"]
        fold = residual_folds(cfg, cin, mode)
        blk_amax, blk_ld, blk_cin = has_amax, ld, cin
        L = []

        def gemm(M, K, K1, cols, src_amax, epi, port, mx):
            a = ("f16x2" if f16 and src_amax and (not K1 or blk_amax) else "bf16x3") if split else "fp32"
            tile = split_tile(M, cols, B, cus) if split else "fp32"
            if a == "f16x2" and tile == 4 and latency_supported(M, K, K1):
                tile = "lat"
            return dict(kind="gemm", M=M, K=K, tile=tile, arith=a, epi=epi, port=port, mx=mx)

        if res and not fold:
            L.append(gemm(f, cin, 0, ld, blk_amax, "masked", False, "in"))
        c = cin
        for r in range(rep):
            last_sub = r + 1 == rep
            enc_out = last_block and last_sub
            fuse_res = last_sub and fold
            if (fused and f16 and sep and c == 256 and f == 256 and stride == 1 and dil == 1 and k in (33, 39) and has_amax
                    and not (last_sub and res and not fold) and (not fuse_res or (blk_amax and blk_ld == ld and blk_cin == 256))
                    and ld % 128 == 0 and not enc_out):
                cols = fused_tile_choice(B * (ld // 128), cus)
                if cols:
                    L.append(dict(kind="fused", cols=cols, dual=fuse_res, arith="f16x2"))
                    c = f
                    continue
            g_ld, src_amax, mx = ld, has_amax, "in"
            if sep:
                tiled = stride == 1 and (k, dil) in TOEPLITZ
                form = "toeplitz" if f16 and has_amax and tiled and ld % 4 == 0 else ("fma" if tiled and ld % 4 == 0 else "generic")
                L.append(dict(kind="dw", form=form, K=k))
                T = out_frames(T, k, stride, dil)
                g_ld, src_amax, mx = padded(T), f16, "dw"
            epi = "DUAL" if fuse_res else ("RES" if last_sub and res else ("plain" if sep else "masked"))
            L.append(gemm(f, (c + cin) if fuse_res else c, c if fuse_res else 0, g_ld, src_amax, epi, enc_out, mx))
            ld = g_ld
            has_amax = f16 and not enc_out
            c = f
        cin = f
        out.append(L)
    return out


def launch_counts(p):
    """The profile classes of a plan: (fused, depthwise, pointwise) launches."""
    flat = [l for L in p for l in L]
    return tuple(sum(l["kind"] == k for l in flat) for k in ("fused", "dw", "gemm"))


def form_names(p_block):
    """Short names of a block's launches, for the coverage check and the records."""
    names = []
    for l in p_block:
        if l["kind"] == "fused":
            names.append(f"fused{l['cols']}" + ("+res" if l["dual"] else ""))
        elif l["kind"] == "dw":
            names.append("dw:" + l["form"])
        else:
            t = l["tile"] if isinstance(l["tile"], str) else "%dx%d" % SPLIT_TILES[l["tile"]]
            names.append(f"{t}:{l['epi']}:{l['arith']}" + (":port" if l["port"] else ""))
    return names


def epilogue_kind(relu, activation, res_max):
    """vasr_internal.h epilogue_kind: the EPI template argument of a GEMM or fused launch."""
    if relu and activation == "selu":
        return 2
    return 1 if (relu and activation != "relu") or res_max else 0


def act_forms(case, arith, cus):
    """The launches of the block under test as (kernel, form, EPI, max, arithmetic, port): kernel = a tile "512x128" ..., "lat",
    "fp32", "fused64" / "fused128"; form = plain / masked / RES / DUAL, a fused kernel's "plain" or "+res"; max = the launch
    combines a residual by max (a RES epilogue in max mode).  The launchers hand epilogue_kind the launch's OWN max, not the
    encoder's mode: RES && a.res_max (encoder_pw_split.hip, encoder_pw_lat.hip), a.res && a.res_max (encoder_pw.hip), false
    (encoder_fused.hip) -- test_sep_host.py reads those call sites.  So under max only the RES launch takes EPI 1 on account of
    the max; a ReLU / max block's plain first sub-layer runs Epilogue<0>, and so does the block's own residual GEMM under every
    activation: run_encoder builds it from pw_args' defaults (relu flag clear, no residual tensor, res_max 0).  The flag-clear
    Epilogue<1> (bounds -inf, +inf) needs a launch that takes a max with the flag clear: the last sub-layer before an SE, or
    the in-place gemm_max chain of a dense max residual.  Neither can be built from the blocks of this table (both have
    float64 suites of their own to extend)."""
    cfg = case.blocks[case.under]
    res_max = case.residual_mode == "max"
    p = plan(case, arith, cus)[case.under]
    cin = case.blocks[case.under - 1]["filters"] if case.under else case.feat_in
    own_res = cfg["residual"] and not residual_folds(cfg, cin, case.residual_mode)
    out = []
    for n, l in enumerate(p):
        relu = not (own_res and n == 0)
        if l["kind"] == "fused":
            epi = epilogue_kind(relu, case.activation, False)
            out.append((f"fused{l['cols']}", "+res" if l["dual"] else "plain", epi, False, "f16x2", False))
        elif l["kind"] == "gemm":
            mx = res_max and l["epi"] == "RES"
            t = l["tile"] if isinstance(l["tile"], str) else "%dx%d" % SPLIT_TILES[l["tile"]]
            out.append((t, l["epi"], epilogue_kind(relu, case.activation, mx), mx, l["arith"], l["port"]))
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """blocks[under] is the block under test; blocks before it are run alone on the device first (their output is the
    reference's input), blocks after it belong to the judged chain."""

    def __init__(self, name, feat_in, blocks, under, B, T=100, kind="gauss", activation="relu", residual_mode="add"):
        self.name, self.feat_in, self.blocks, self.under, self.B, self.T, self.kind = name, feat_in, blocks, under, B, T, kind
        self.activation, self.residual_mode = activation, residual_mode       # the encoder's: every block of the case
        self.spread = False       # ACT_CASES: the BNs of the block under test scaled per channel (weights())
        self.probe = False        # PROBES: the block under test is the identity, the input a sweep (weights(), inputs())
        self.seed = 100 + sum(map(ord, name)) % 97

    def small(self, B):
        """The same case at another batch, for plan() (the rows themselves are taken from this case's inputs)."""
        c = Case(self.name, self.feat_in, self.blocks, self.under, B, self.T, self.kind, self.activation, self.residual_mode)
        c.spread, c.probe = self.spread, self.probe
        return c

    def __repr__(self):
        return self.name


LEAD = lambda c: blk(c, 1, separable=False)
TRAIL = lambda c: blk(c, 1, separable=False)       # weights() makes it the identity


def _c256(name, B, k, res, T=100, kind="gauss"):
    """64 -> 256 lead, the 256-channel block (repeat 2), and with a residual the trailing block (so that the last
    sub-layer, the one with the folded residual, is an interior one)."""
    return Case(name, 64, [LEAD(256), blk(256, k, 2, res)] + ([TRAIL(256)] if res else []), 1, B, T, kind)


def _c512(name, B, k, dil=1, cin=512, trail=False, T=100, kind="gauss"):
    return Case(name, 64, [LEAD(cin), blk(512, k, 2, True, dilation=dil)] + ([TRAIL(512)] if trail else []), 1, B, T, kind)


def _res512(name, B, k, dil=1, T=100, kind="gauss"):
    """320 -> 512: k2 = 320 is no multiple of the 128-row chunk, so the residual is its own GEMM and the last sub-layer
    takes the RES epilogue.  (Every block's filters are a multiple of 128, so 320 channels can only be the encoder input.)"""
    return Case(name, 320, [blk(512, k, 2, True, dilation=dil)], 0, B, T, kind)


CASES = [
    # 256 -> 256, T = 100 (one 128-column tile per utterance): the batch picks the form
    _c256("c256_b16", 16, 33, False), _c256("c256_b16_res", 16, 39, True, kind="relu"),
    _c256("c256_b48", 48, 39, False, kind="wide"), _c256("c256_b48_res", 48, 33, True),
    _c256("c256_b130", 130, 33, False, kind="relu"), _c256("c256_b130_res", 130, 39, True, kind="wide"),
    _c256("c256_b192", 192, 39, False), _c256("c256_b192_res", 192, 33, True, kind="relu"),
    _c256("c256_b205", 205, 33, False, kind="wide"), _c256("c256_b205_res", 205, 39, True),
    # 512 -> 512 with the folded residual (DUAL, K = 512 + 512), last sub-layer on the port or (trail) on a padded buffer
    _c512("c512_b16", 16, 87, dil=2, kind="wide"), _c512("c512_b24", 24, 63, trail=True), _c512("c512_b96", 96, 75, kind="relu"),
    _c512("c512_b192", 192, 51, trail=True), _c512("c512_b218", 218, 51),
    # a width-changing block: K = 512 + 256, at every tile again
    _c512("c512w_b8", 8, 63, cin=256), _c512("c512w_b24", 24, 75, cin=256, kind="relu"),
    _c512("c512w_b96", 96, 51, cin=256, trail=True), _c512("c512w_b192", 192, 75, cin=256, kind="wide"),
    _c512("c512w_b218", 218, 63, cin=256, trail=True, kind="wide"),
    # 320 -> 512: the separate residual GEMM and the RES epilogue
    _res512("r512_b16", 16, 87, dil=2), _res512("r512_b24", 24, 51, kind="relu"), _res512("r512_b96", 96, 63, kind="wide"),
    _res512("r512_b192", 192, 75), _res512("r512_b218", 218, 63, kind="relu"),
    # 768 filters: 256 x 128 tiles with M = 768, residual folded on 64-row chunks (K = 768 + 256)
    Case("c768_b64", 64, [LEAD(256), blk(768, 33, 2, True), TRAIL(768)], 1, 64, kind="wide"),
    # the stride-2 prologue: generic depthwise kernel on the unpadded port pitch, halved frames
    Case("pro_b16", 64, [blk(256, 33, 1, False, stride=2)], 0, 16, 101, "gauss"),
    Case("pro_b16_then_res", 64, [blk(256, 33, 1, False, stride=2), blk(256, 33, 2, True)], 1, 16, 201, "relu"),
    # the final shape: 512 -> 1024, K = 1, not separable, last block: masked plain form, store_cols = frames
    Case("fin_b8", 64, [LEAD(512), blk(1024, 1, separable=False)], 1, 8, kind="wide"),
    Case("fin_b110", 64, [LEAD(512), blk(1024, 1, separable=False)], 1, 110, kind="relu"),
    # T = 300 (pitch 384): a row spans three tiles, the last one partial
    _c256("c256_t300_b16_res", 16, 33, True, T=300, kind="wide"), _c256("c256_t300_b70", 70, 39, False, T=300),
    _c512("c512_t300_b8", 8, 51, trail=True, T=300, kind="relu"), _res512("r512_t300_b3", 3, 75, T=300, kind="wide"),
]
BY_NAME = {c.name: c for c in CASES}
BF16X2_CASE = "c512_b24"       # the opt-in reduced arithmetic: one case, held to test_gpu_jasper.py's bf16-level bound
FORCED = ["c256_b16_res", "c512_b16", "r512_b16", "fin_b8"]       # small batches: every forced tile applies


# ---- hardtanh, SELU and max residuals (vasr_set_activation): tests/test_gpu_act_f64.py -------------------------------------------
def _act(case, activation, residual_mode):
    """The case as `<name>_<activation>_<mode>` with the encoder's options set and the spread BNs of weights()."""
    c = Case(f"{case.name}_{activation}_{residual_mode}", case.feat_in, case.blocks, case.under, case.B, case.T, case.kind,
             activation, residual_mode)
    c.spread = True
    return c


ACT_CASES = [
    # max: the residual is its own GEMM (masked, relu flag clear: Epilogue<0>, see act_forms), the block's first sub-layer
    # plain and its last one RES with res_max, all three on the tile the batch picks; r512: on the port (scalar apply), the
    # others on a padded interior buffer (apply4).  Per tile one case with EPI 1 and one with EPI 2 (SELU); the EPI 1 cases
    # are hardtanh ones but at 128 x 64, where the ReLU / max case reaches EPI 1 in its RES launch alone and the plain
    # hardtanh form comes from c512_b24_hardtanh_add.
    _act(_res512("r512_b16", 16, 87, dil=2), "selu", "max"), _act(_c256("c256_b16_res", 16, 39, True, kind="relu"), "hardtanh", "max"),
    _act(_res512("r512_b24", 24, 51, kind="relu"), "selu", "max"), _act(_c256("c256_b130_res", 130, 39, True, kind="wide"), "relu", "max"),
    _act(Case("c768_b64", 64, [LEAD(256), blk(768, 33, 2, True), TRAIL(768)], 1, 64, kind="wide"), "selu", "max"),
    _act(_res512("r512_b96", 96, 63, kind="wide"), "hardtanh", "max"),
    _act(_c256("c256_b192_res", 192, 33, True, kind="relu"), "selu", "max"), _act(_res512("r512_b192", 192, 75), "hardtanh", "max"),
    _act(Case("r512t_b218", 320, [blk(512, 51, 2, True), TRAIL(512)], 0, 218), "selu", "max"), _act(_res512("r512_b218", 218, 63, kind="relu"), "hardtanh", "max"),
    # K = 768 has no latency form: the 64 x 32 tile in the fp16 split, plain (second of three sub-layers) and RES
    _act(Case("c768_b8", 64, [LEAD(256), blk(768, 33, 3, True), TRAIL(768)], 1, 8), "hardtanh", "max"),
    _act(Case("c768_b8", 64, [LEAD(256), blk(768, 33, 3, True), TRAIL(768)], 1, 8, kind="relu"), "selu", "max"),
    # add: the residual folds as under ReLU -- the fused kernel in both widths without (first sub-layer) and with it, DUAL
    _act(_c256("c256_b48_res", 48, 33, True), "hardtanh", "add"), _act(_c256("c256_b48_res", 48, 33, True), "selu", "add"),
    _act(_c256("c256_b205_res", 205, 39, True), "hardtanh", "add"), _act(_c256("c256_b205_res", 205, 39, True), "selu", "add"),
    _act(_c512("c512_b16", 16, 87, dil=2, kind="wide"), "selu", "add"), _act(_c512("c512_b24", 24, 63, trail=True), "hardtanh", "add"),
    # the final shape on the port, the block behind the stride-2 prologue, three tiles a row
    _act(Case("fin_b8", 64, [LEAD(512), blk(1024, 1, separable=False)], 1, 8, kind="wide"), "selu", "add"),
    _act(Case("pro_b16_then_res", 64, [blk(256, 33, 1, False, stride=2), blk(256, 33, 2, True)], 1, 16, 201, "relu"), "relu", "max"),
    _act(_c256("c256_t300_b16_res", 16, 33, True, T=300, kind="wide"), "hardtanh", "add"),
]
ACT_FORCED = ["c512_b16_selu_add", "c256_b16_res_hardtanh_max", "r512_b16_selu_max", "pro_b16_then_res_relu_max"]
ACT_FUSED = ["c256_b48_res_hardtanh_add", "c256_b48_res_selu_add"]


def _probe(C, B, T, activation, residual_mode, last):
    """An identity probe: the block under test is the encoder's FIRST block, a 1x1 conv C -> C with the identity weight and the
    identity BN (a max probe: with a residual whose conv is -I, i.e. max(x, -x)), so its pre-activation is the input itself:
    exactly in fp32 and in 3 x bf16 (which the first block's GEMM runs in f16x2 mode too: its source has no published maxima).
    last: the probe writes the port (scalar apply); else a TRAILING identity block follows (the probe stores through apply4,
    and in f16x2 mode the trailing GEMM runs the fp16 split on the maxima the probe published and applies the activation once
    more, in ITS instantiation, to act(x), on the port).  last = 2 trailing blocks ("in2"): the first of them is an interior
    fp16-split GEMM, the float4 path of that arithmetic on the probe's values."""
    res = residual_mode == "max"
    trail = 2 if last == 2 else (0 if last else 1)
    c = Case(f"probe_c{C}_b{B}_t{T}_{activation}_{residual_mode}_{('last', 'in', 'in2')[trail]}", C,
             [blk(C, 1, 1, res, separable=False)] + [TRAIL(C)] * trail, 0, B, T, "probe", activation, residual_mode)
    c.probe = True
    return c


PROBES = [
    _probe(256, 8, 100, "selu", "add", False), _probe(256, 8, 100, "selu", "add", True),
    _probe(512, 130, 100, "selu", "add", True), _probe(512, 8, 300, "selu", "add", False),
    _probe(256, 130, 300, "selu", "add", False),
    _probe(256, 8, 100, "hardtanh", "add", False), _probe(512, 8, 300, "hardtanh", "add", True),
    _probe(512, 130, 100, "hardtanh", "add", False),
    _probe(256, 8, 100, "relu", "max", False), _probe(512, 130, 100, "relu", "max", True),
    _probe(512, 8, 300, "hardtanh", "max", False), _probe(256, 130, 300, "hardtanh", "max", True),
    _probe(256, 8, 100, "selu", "max", True), _probe(512, 130, 100, "selu", "max", False),
    _probe(256, 130, 300, "selu", "max", True),
    _probe(256, 130, 100, "selu", "add", 2), _probe(512, 8, 100, "hardtanh", "add", 2),
]
BY_NAME.update({c.name: c for c in ACT_CASES + PROBES})


def probe_values():
    """What an identity probe's input holds: both signs of 8 magnitudes an octave from 2^-24 to 2^6, exact +-1, +-0 and
    +-(1 +- 2^-23), and values below -88 (there expm1f is -1 exactly), with +88.5 beside them."""
    mags = np.exp2(np.linspace(-24, 6, 241)).astype(np.float32)
    one = np.float32(1)
    edge = [one, -one, np.float32(0), -np.float32(0), one + np.float32(2.0 ** -23), one - np.float32(2.0 ** -23),
            -(one + np.float32(2.0 ** -23)), -(one - np.float32(2.0 ** -23))]
    return np.concatenate([mags, -mags, np.asarray(edge, dtype=np.float32),
                           np.asarray([-87.5, -88.5, -89, -100, -1000, 88.5], dtype=np.float32)])


def spread_scales(C):
    """Per-channel factors on gamma and beta of the BNs of an ACT_CASE's block under test: powers 2^-14 ... 2^6, log-spaced
    and permuted over the channels, so that one tensor's pre-activations lie deep inside, around and far outside every range
    an activation treats differently (hardtanh's [-1, 1]; SELU's (-2^-10, 0) and below -10) and both arguments of a max, scaled
    alike, win."""
    return np.exp2(np.linspace(-14, 6, C))[(np.arange(C) * 37) % C].astype(np.float32)


def weights(case):
    """synth's weights for the chain (BN statistics with scale != 1 and shift != 0), channel 3's taps of the block under test
    a thousand times smaller, a trailing block the identity: weight I, BN with alpha = 1 and beta = 0 exactly in float32.
    A probe's block under test is the identity too (its residual conv -I); an ACT_CASE has the BNs of its block under test
    spread over the channels and a trailing block that halves and lifts (below)."""
    from viet_asr_amd import synth
    sd = synth.encoder_state_dict(case.blocks, case.feat_in, case.seed)
    if case.blocks[case.under]["separable"]:
        sd[f"encoder.{case.under}.mconv.0.conv.weight"][3] *= np.float32(1e-3)
    var = np.float32(1) - np.float32(1e-3)
    assert np.float32(var + np.float32(1e-3)) == np.float32(1)

    def identity(conv, bn, c, sign=1):
        assert sd[conv + ".conv.weight"].shape == (c, c, 1)
        sd[conv + ".conv.weight"][...] = np.float32(sign) * np.eye(c, dtype=np.float32)[:, :, None]
        for key, val in (("weight", 1), ("bias", 0), ("running_mean", 0), ("running_var", var)):
            sd[bn + "." + key][...] = np.float32(val)

    for i in range(case.under + (0 if case.probe else 1), len(case.blocks)):
        identity(f"encoder.{i}.mconv.0", f"encoder.{i}.mconv.1", case.blocks[i]["filters"])
    if case.probe and case.blocks[case.under]["residual"]:       # max(x, -x)
        identity(f"encoder.{case.under}.res.0.0", f"encoder.{case.under}.res.0.1", case.blocks[case.under]["filters"], -1)
    if case.spread:
        # Behind ReLU or hardtanh an identity block would apply the same idempotent clamp again and hide what the block under
        # test clamped wrongly (max taken after the activation: clamp(max(clamp(y), r)) = clamp(max(y, r))).  An ACT_CASE's
        # trailing block therefore halves and lifts, alpha = 1/2 and beta = 1/4 exactly: still one product a row.
        for i in range(case.under + 1, len(case.blocks)):
            sd[f"encoder.{i}.mconv.1.weight"][...] = np.float32(0.5)
            sd[f"encoder.{i}.mconv.1.bias"][...] = np.float32(0.25)
        s = spread_scales(case.blocks[case.under]["filters"])
        bns = [key[:-len(".running_var")] for key in sd if key.startswith(f"encoder.{case.under}.") and key.endswith(".running_var")]
        last = max((b for b in bns if ".mconv." in b), key=lambda b: int(b.rsplit(".", 1)[1]))
        for bn in bns:
            sd[bn + ".weight"] = sd[bn + ".weight"] * s
            # (the larger of two symmetric arguments is negative a quarter of the time: both one unit down under max)
            down = case.residual_mode == "max" and (bn == last or ".res." in bn)
            sd[bn + ".bias"] = (sd[bn + ".bias"] - np.float32(1 if down else 0)) * s
    return sd


def edge_lengths(T):
    """Rows of 1-3 frames, lengths at and one past multiples of 32 / 64 / 128 (rows that leave whole time tiles empty: the
    zero_from skip), and the full width."""
    out = [1, 2, 3]
    for bn in (32, 64, 128, 256):
        out += [bn, bn + 1]
    return [n for n in out if n < T] + [T]


def inputs(case):
    """-> (x [B, feat_in, T] float32, lens [B] int64), as test_gpu_jasper._conv_input: rows at the edge lengths, the others at
    random lengths in [T/2, T], one of them full; Gaussian / ReLU'd / "wide" (2^-24 ... 2^6 inside one utterance); utterance 1
    at 37.5 x; what lies past a row's length is NOT zero."""
    rng = np.random.default_rng(case.seed)
    B, T = case.B, case.T
    edges = edge_lengths(T)
    lens = np.concatenate([edges, rng.integers(T // 2, T + 1, max(0, B - len(edges)))])[:B].astype(np.int64)
    lens[rng.integers(len(edges), B) if B > len(edges) else -1] = T
    rng.shuffle(lens)
    if case.probe:       # every value of probe_values() in every row of 495 elements or more, in all channels and columns
        vals = probe_values()
        b, c, t = np.ogrid[:B, :case.feat_in, :T]
        return vals[(b * 131 + c * T + t) % len(vals)], lens
    x = rng.standard_normal((B, case.feat_in, T)).astype(np.float32)
    if case.kind == "relu":
        x = np.maximum(x, 0)
    if case.kind == "wide":
        x = x * np.exp2(rng.integers(-24, 7, x.shape)).astype(np.float32)
    x[1] *= np.float32(37.5)
    return x, lens


def sub_state_dict(sd, n_blocks):
    """The weights of the first n_blocks blocks alone."""
    keep = tuple(f"encoder.{i}." for i in range(n_blocks))
    return {k: v for k, v in sd.items() if k.startswith(keep)}


# ---- the float64 chain with magnitudes and bounds ------------------------------------------------------------------------------
def bn_affine(sd, prefix):
    """model_build.cpp bn_affine in float32 -> (alpha, beta) as the device holds them, and |b| + |mean alpha| (float64)."""
    g, b, m, v = (np.asarray(sd[prefix + s], dtype=np.float32) for s in (".weight", ".bias", ".running_mean", ".running_var"))
    invstd = np.float32(1.0) / np.sqrt(v + np.float32(1e-3))
    alpha = g * invstd
    beta = b - m * alpha
    return alpha, beta, np.abs(b).astype(np.float64) + np.abs(m.astype(np.float64) * alpha.astype(np.float64))


def _bn64(sd, prefix):
    g, b, m, v = (torch.as_tensor(np.asarray(sd[prefix + s])).double()
                  for s in (".weight", ".bias", ".running_mean", ".running_var"))
    alpha = g / torch.sqrt(v + 1e-3)
    return alpha, b - m * alpha


def _mask(t, lens):
    keep = (torch.arange(t.shape[-1])[None, :] < torch.as_tensor(lens)[:, None])[:, None, :]
    return torch.where(keep, t, torch.zeros((), dtype=t.dtype))


def _rowmax(t, lens):
    """max over channels and valid frames per utterance."""
    return _mask(t, lens).amax((1, 2))


def _mm(W, xs):
    """W [O, K] applied to each [B, K, T] of xs, in one product."""
    n = [x.shape[0] for x in xs]
    y = torch.einsum("ok,bkt->bot", W, torch.cat(xs, 0))
    return list(torch.split(y, n, 0))


def _gemm_own(arith, n, Aacc, Wabs, Asrc, Mx, Mw):
    """The own error of an n-term GEMM in `arith` before the affine: accumulation + operand representation."""
    if arith == "fp32":
        return n * EPS * Aacc
    if arith == "bf16x3":
        return (n * EPS + R3) * Aacc
    floor = Mx[:, None, None] * Wabs.sum(1)[None, :, None] + Mw * Asrc.sum(1, keepdim=True)
    return (n * EPS + R16) * Aacc + F16 * floor


SELU_LAMBDA = 1.0507009873554804934193349852946       # torch's constants (nn.SELU)
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_OWN = 4                                          # S: expm1f <= 1 ulp, the rounded constant, one multiply, one spare


def act64(activation, y):
    """The activation in y's dtype, as oracle.quartznet_oracle.activation_fn."""
    if activation == "relu":
        return torch.relu(y)
    if activation == "hardtanh":
        return torch.clamp(y, -1.0, 1.0)
    if activation == "selu":
        return torch.nn.functional.selu(y)
    raise KeyError(activation)


def _act_bound(activation, y, E):
    """-> (act(y), the bound behind the activation) for one arithmetic's bound E on y (float64)."""
    v = act64(activation, y)
    if activation != "selu":
        return v, E                                   # ReLU, hardtanh: 1-Lipschitz, min and max are exact
    L = torch.where(y - E > 0, torch.full_like(y, SELU_LAMBDA),
                    SELU_LAMBDA * SELU_ALPHA * torch.exp(torch.clamp(y + E, max=0.0)))
    return v, L * E + SELU_OWN * EPS * v.abs()


def chain(x, lens, sd, blocks, i0, plans, activation="relu", residual_mode="add", sparse=False, pre=None):
    """The blocks `blocks` (encoder indices i0 ...) on x [B, C, T] float64 (taken as exact), lens [B] int64.  plans:
    {arith: plan(...)[i0:]} for the arithmetics wanted.  -> (ref [B, C', T'] float64, {arith: bound}, lens').
    activation, residual_mode: the encoder's.  sparse: a GEMM's accumulation term counts the non-zero weights of its fullest
    row, not K (the identity probes: adding an exact zero rounds nothing).  pre: a list that receives, per sub-layer,
    dict(block, sub, y = the pre-activation, args = the two arguments of a max residual or None, lens)."""
    ariths = list(plans)
    lens = np.asarray(lens, dtype=np.int64)
    terms = (lambda W: int((W != 0).sum(1).max())) if sparse else (lambda W: W.shape[1])
    v = x
    E = {a: torch.zeros_like(x) for a in ariths}
    with torch.no_grad():
        for bi, cfg in enumerate(blocks):
            i = i0 + bi
            k, stride, dil = _geo(cfg)
            pad = same_padding(k, stride, dil)
            rep, sep, res = cfg["repeat"], cfg["separable"], cfg["residual"]
            it = {a: iter(plans[a][bi]) for a in ariths}
            blk_in = (_mask(v, lens), _mask(v, lens).abs(), {a: _mask(E[a], lens) for a in ariths})
            blk_mx = {a: _rowmax(v.abs() + E[a], lens) for a in ariths}
            fold = residual_folds(cfg, v.shape[1], residual_mode)
            R = None
            if res and not fold:
                W = torch.as_tensor(sd[f"encoder.{i}.res.0.0.conv.weight"][:, :, 0]).double()
                al, be, ash = bn_affine(sd, f"encoder.{i}.res.0.1")
                al, be, ash = (torch.as_tensor(t).double()[None, :, None] for t in (al, be, ash))
                al64, be64 = _bn64(sd, f"encoder.{i}.res.0.1")
                rv, = _mm(W, [blk_in[0]])
                rv = al64[None, :, None] * rv + be64[None, :, None]
                got = _mm(W.abs(), [blk_in[1]] + [blk_in[2][a] for a in ariths])
                Aacc = got[0]
                RA = al.abs() * Aacc + ash
                RE = {}
                for a, Ein in zip(ariths, got[1:]):
                    l = next(it[a])
                    assert l["kind"] == "gemm" and l["epi"] == "masked"
                    own = _gemm_own(l["arith"], terms(W), Aacc, W.abs(), blk_in[1], blk_mx[a], float(W.abs().max()))
                    RE[a] = al.abs() * (Ein + own) + AFFINE * EPS * RA
                R = (rv, RA, RE)
            j = 0
            for r in range(rep):
                last_sub = r + 1 == rep
                launches = {a: next(it[a]) for a in ariths}
                in_mx = {a: _rowmax(v.abs() + E[a], lens) for a in ariths}
                vm = _mask(v, lens)
                Am = vm.abs()
                Em = {a: _mask(E[a], lens) for a in ariths}
                mx = dict(in_mx)
                if sep:
                    w = torch.as_tensor(sd[f"encoder.{i}.mconv.{j}.conv.weight"]).double()        # [C, 1, K]
                    C = w.shape[0]
                    conv = lambda t, ww: torch.nn.functional.conv1d(t, ww, None, stride, pad, dil, C)
                    dv, dA = conv(vm, w), conv(Am, w.abs())
                    l1 = w.abs().sum((1, 2))
                    lens = lens_out(lens, k, stride, dil)
                    for a in ariths:
                        l = launches[a]
                        dE = conv(Em[a], w.abs())
                        if l["kind"] == "fused":
                            dE = dE + k * EPS * dA
                            # pack_fused_taps: max_c sum_k |w|, rounded to float32 and one ulp up
                            top = float(np.nextafter(np.float32(float(l1.max())), np.float32(3e38)))
                            mx[a] = in_mx[a] * top * (1 + EPS)
                        else:
                            assert l["kind"] == "dw", (l, a)
                            if l["form"] == "toeplitz":
                                floor = in_mx[a][:, None, None] * l1[None, :, None] + w.abs().amax((1, 2))[None, :, None] * \
                                    conv(Am, torch.ones_like(w))
                                dE = dE + (k * EPS + R16) * dA + F16 * floor
                            else:
                                dE = dE + k * EPS * dA
                            launches[a] = next(it[a])
                            mx[a] = _rowmax(dv.abs() + dE, lens)
                        Em[a] = _mask(dE, lens)
                    vm = _mask(dv, lens)
                    Am = vm.abs()
                    j += 1
                # the 1x1 conv, its BN, the residual
                W = torch.as_tensor(sd[f"encoder.{i}.mconv.{j}.conv.weight"][:, :, 0]).double()
                bn = f"encoder.{i}.mconv.{j + 1}"
                j += 2 + (2 if not last_sub else 0)
                al, be, ash = bn_affine(sd, bn)
                al64, be64 = _bn64(sd, bn)
                Wd = al.astype(np.float64)[:, None] * W.numpy()                       # what the folded pack holds, before rounding
                al, ash = (torch.as_tensor(t).double()[None, :, None] for t in (al, ash))
                yv = al64[None, :, None] * _mm(W, [vm])[0] + be64[None, :, None]
                got = _mm(W.abs(), [Am] + [Em[a] for a in ariths])
                Aacc = got[0]
                yA = al.abs() * Aacc + ash
                dual = last_sub and res and fold
                if dual:
                    W2 = torch.as_tensor(sd[f"encoder.{i}.res.0.0.conv.weight"][:, :, 0]).double()
                    al2, be2, ash2 = bn_affine(sd, f"encoder.{i}.res.0.1")
                    al264, be264 = _bn64(sd, f"encoder.{i}.res.0.1")
                    Wd2 = al2.astype(np.float64)[:, None] * W2.numpy()
                    al2, ash2 = (torch.as_tensor(t).double()[None, :, None] for t in (al2, ash2))
                    yv = yv + al264[None, :, None] * _mm(W2, [blk_in[0]])[0] + be264[None, :, None]
                    got2 = _mm(W2.abs(), [blk_in[1]] + [blk_in[2][a] for a in ariths])
                    A2 = got2[0]
                    yA2 = al2.abs() * A2 + ash2
                yE = {}
                for idx, a in enumerate(ariths):
                    l = launches[a]
                    if dual:
                        assert (l["kind"] == "fused" and l["dual"]) or l["epi"] == "DUAL", (l, a)
                        Mx = torch.maximum(mx[a], blk_mx[a])
                        Mw = max(float(np.abs(Wd).max()), float(np.abs(Wd2).max())) * (1 + EPS)
                        n = W.shape[1] + W2.shape[1]
                        # one GEMM over both K ranges: the scaled weights' magnitudes, both sources' activations
                        Acc = al.abs() * Aacc + al2.abs() * A2
                        src = torch.cat([Am, blk_in[1]], 1)
                        Wabs = torch.cat([al[0].abs() * W.abs(), al2[0].abs() * W2.abs()], 1)
                        own = _gemm_own(l["arith"], n, Acc, Wabs, src, Mx, Mw)
                        yE[a] = al.abs() * got[1 + idx] + al2.abs() * got2[1 + idx] + own + AFFINE * EPS * (yA + yA2) + \
                            EPS * (yA + yA2)
                    else:
                        assert l["kind"] == "fused" or l["epi"] in ("plain", "masked", "RES"), (l, a)
                        own = _gemm_own(l["arith"], terms(W), Aacc, W.abs(), Am, mx[a], float(W.abs().max()))
                        yE[a] = al.abs() * (got[1 + idx] + own) + AFFINE * EPS * yA
                        if last_sub and res:
                            assert l["epi"] == "RES", (l, a)
                            if residual_mode == "max":
                                yE[a] = torch.maximum(yE[a], R[2][a])
                            else:
                                yE[a] = yE[a] + R[2][a] + EPS * (yA + R[1])
                args = None
                if dual:
                    yA = yA + yA2
                elif last_sub and res and residual_mode == "max":
                    args = (yv, R[0])
                    yv, yA = torch.maximum(yv, R[0]), torch.maximum(yA, R[1])
                elif last_sub and res:
                    yv, yA = yv + R[0], yA + R[1]
                if pre is not None:
                    pre.append(dict(block=i, sub=r, y=yv, args=args, lens=lens))
                if activation == "relu":
                    v, E = torch.relu(yv), yE
                else:
                    E = {a: _act_bound(activation, yv, yE[a])[1] for a in ariths}
                    v = act64(activation, yv)
    return v, {a: E[a] + TINY for a in ariths}, lens


# ---- a device-like float32 evaluation, with defects ---------------------------------------------------------------------------
MUTANTS = ("mask_late", "res_lens", "dw_pad", "k_chunk", "w_11bit", "shift_before_res")
ACT_MUTANTS = ("selu_exp_minus_1", "hardtanh_as_relu", "max_as_add", "max_after_act", "clamp_without_relu_flag")


def act32(activation, y, mut=None):
    """The activation in float32 as vasr_device.h writes it (SELU: lambda v, (lambda alpha) expm1f(v) with the product of the
    two float32 constants), or one of its defects."""
    if activation == "relu":
        return torch.relu(y)
    if activation == "hardtanh":
        return torch.clamp(y, 0.0 if mut == "hardtanh_as_relu" else -1.0, 1.0)
    lam, la = np.float32(SELU_LAMBDA), np.float32(SELU_LAMBDA) * np.float32(SELU_ALPHA)
    neg = torch.exp(y) - 1 if mut == "selu_exp_minus_1" else torch.expm1(y)
    return torch.where(y > 0, float(lam) * y, float(la) * neg)


def f32_chain(x, lens, sd, blocks, i0, under=0, mutant=None, first_lens=None, activation="relu", residual_mode="add"):
    """The same blocks in plain float32 on the CPU (sequential torch), arranged as the device arranges them: BN as the
    float32 affine of bn_affine in the GEMM's epilogue, a folded residual as ONE product over both K ranges with the scaled
    weights and the sum of both shifts.  mutant (applied to block `under` of the list only):
      mask_late         the depthwise input mask one column late
      res_lens          the residual source masked with another length vector (first_lens: the encoder's input lengths)
      dw_pad            the depthwise padding off by one
      k_chunk           one 64-wide K chunk of the second source (the residual) dropped
      w_11bit           the 1x1 weights rounded to 11 bits: the low fp16 plane dropped
      shift_before_res  a folded residual's shift left out (only the main branch's shift is applied)
    and, with an activation or residual mode of vasr_set_activation (ACT_MUTANTS):
      selu_exp_minus_1         SELU's negative side as float32 exp(x) - 1
      hardtanh_as_relu         hardtanh's lower bound 0 instead of -1
      max_as_add               the max residual added
      max_after_act            the activation applied to the branch output alone, then max with the raw residual (under
                               ReLU the same function, max(0, y, r); under hardtanh different where r > 1)
      clamp_without_relu_flag  the residual GEMM of a max block (Epilogue<0> with the relu flag clear: act_forms) clamping
                               at ReLU's floor 0 anyway.  (The flag-clear Epilogue<1> itself, bounds -inf and +inf, is not
                               reachable by this chain: it needs an SE block or a dense max residual, act_forms says why.)
                               Only SELU + max can show it: ReLU's and hardtanh's clamps are
                               monotone and idempotent, clamp(max(y, clamp(r))) = clamp(max(y, r)), so under those two the
                               defect changes no output and is none."""
    lens = np.asarray(lens, dtype=np.int64)
    v = x.float()
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    with torch.no_grad():
        for bi, cfg in enumerate(blocks):
            i = i0 + bi
            mut = mutant if bi == under else None
            k, stride, dil = _geo(cfg)
            pad = same_padding(k, stride, dil)
            rep, sep, res = cfg["repeat"], cfg["separable"], cfg["residual"]
            rl = lens
            if mut == "res_lens":
                rl = np.asarray(first_lens, dtype=np.int64)
            blk_in = _mask(v, rl)
            fold = residual_folds(cfg, v.shape[1], residual_mode)
            j = 0
            for r in range(rep):
                last_sub = r + 1 == rep
                vm = _mask(v, lens + 1 if mut == "mask_late" and sep else lens)
                if sep:
                    w = f32(sd[f"encoder.{i}.mconv.{j}.conv.weight"])
                    if mut == "dw_pad":
                        vm = torch.roll(vm, 1, 2)
                        vm[:, :, 0] = 0
                    vm = torch.nn.functional.conv1d(vm, w, None, stride, pad, dil, w.shape[0])
                    lens = lens_out(lens, k, stride, dil)
                    vm = _mask(vm, lens)
                    j += 1
                W = f32(sd[f"encoder.{i}.mconv.{j}.conv.weight"][:, :, 0])
                if mut == "w_11bit":
                    W = W.half().float()
                al, be, _ = bn_affine(sd, f"encoder.{i}.mconv.{j + 1}")
                al, be = f32(al), f32(be)
                j += 2 + (2 if not last_sub else 0)
                if last_sub and res:
                    W2 = f32(sd[f"encoder.{i}.res.0.0.conv.weight"][:, :, 0])
                    al2, be2, _ = bn_affine(sd, f"encoder.{i}.res.0.1")
                    al2, be2 = f32(al2), f32(be2)
                    src2 = blk_in
                    if mut == "k_chunk":
                        src2 = src2.clone()
                        src2[:, 64:128] = 0
                    if fold:
                        Wf = torch.cat([al[:, None] * W, al2[:, None] * W2], 1)
                        sh = be if mut == "shift_before_res" else be + be2
                        y = torch.einsum("ok,bkt->bot", Wf, torch.cat([vm, src2], 1)) + sh[None, :, None]
                    else:
                        R = al2[None, :, None] * torch.einsum("ok,bkt->bot", W2, src2)
                        if mut != "shift_before_res":
                            R = R + be2[None, :, None]
                        if mut == "clamp_without_relu_flag":
                            R = torch.relu(R)
                        y = al[None, :, None] * torch.einsum("ok,bkt->bot", W, vm) + be[None, :, None]
                        if mut == "max_after_act":
                            v = torch.maximum(act32(activation, y), R)
                            continue
                        y = y + R if residual_mode == "add" or mut == "max_as_add" else torch.maximum(y, R)
                else:
                    y = al[None, :, None] * torch.einsum("ok,bkt->bot", W, vm) + be[None, :, None]
                v = act32(activation, y, mut)
    return v, lens


def judge(y, ref, bound):
    """-> (worst |y - ref| / bound, message or None).  Every element is judged."""
    if tuple(y.shape) != tuple(ref.shape):
        return float("inf"), f"shape {tuple(y.shape)} != {tuple(ref.shape)}"
    ratio = torch.nan_to_num((y.double() - ref).abs() / bound, nan=float("inf"), posinf=float("inf"))
    worst = float(ratio.max())
    if worst <= 1.0:
        return worst, None
    b, c, t = np.unravel_index(int(ratio.argmax()), ratio.shape)
    return worst, (f"|y - ref| = {abs(float(y[b, c, t]) - float(ref[b, c, t])):.3e} > bound {float(bound[b, c, t]):.3e} at b={b} "
                   f"c={c} t={t} (ref {float(ref[b, c, t]):.4e}; {int((ratio > 1).sum())} elements outside)")


# ---- the runner ------------------------------------------------------------------------------------------------------------------
def lens_chain(lens, blocks):
    lens = np.asarray(lens, dtype=np.int64)
    for cfg in blocks:
        k, stride, dil = _geo(cfg)
        for _ in range(cfg["repeat"]):
            lens = lens_out(lens, k, stride, dil)
    return lens


def encoder(blocks, feat_in, sd, activation="relu", residual_mode="add"):
    from viet_asr_amd import asr
    enc = asr.JasperEncoder(jasper=blocks, activation=activation, feat_in=feat_in, residual_mode=residual_mode)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return enc


def device_outputs(case, device, ariths=ARITHS, profile=True):
    """The case on the device -> {arith: dict(y = encoder output (host), lens, lead = the leading blocks' output run alone
    (host; the input itself without leading blocks), counts = (fused, depthwise, pointwise) launches of the whole encoder)}."""
    sd = weights(case)
    x, lens = inputs(case)
    xd, ld = torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device)
    full = encoder(case.blocks, case.feat_in, sd, case.activation, case.residual_mode)
    head = encoder(case.blocks[:case.under], case.feat_in, sub_state_dict(sd, case.under), case.activation,
                   case.residual_mode) if case.under else None
    out = {}
    for a in ariths:
        h = full._get_handle()
        h.set_gemm_mode(a)
        counts = None
        if profile:
            h.profile_begin()
        y, yl = full.forward(xd, ld)
        torch.cuda.synchronize()
        if profile:
            p = h.profile_end()
            counts = tuple(int(p[k]["launches"]) for k in ("fused", "depthwise", "pointwise"))
        lead = torch.from_numpy(x)
        if head is not None:
            head._get_handle().set_gemm_mode(a)
            lead = head.forward(xd, ld)[0].cpu()
        out[a] = dict(y=y.cpu(), lens=yl.cpu(), lead=lead, counts=counts)
    return out


def sampled_rows(case):
    """Up to six rows of a case's batch: a shortest and a full-length one, utterance 1 (37.5 x) and rows spread over the rest."""
    _, lens = inputs(case)
    rows = {int(np.argmin(lens)), int(np.argmax(lens)), 1 % case.B}
    rows.update(int(r) for r in np.linspace(0, case.B - 1, 4))
    return sorted(rows)[:6]


def device_rows(case, device, rows, ariths):
    """The sampled rows of the case as a batch of their own (every GEMM then takes the 64 x 32 tile or the latency kernel, no
    sub-layer is fused) -> {arith: encoder output (host)}."""
    sd = weights(case)
    x, lens = inputs(case)
    xd, ld = torch.from_numpy(x[rows]).to(device), torch.from_numpy(lens[rows]).to(device)
    enc = encoder(case.blocks, case.feat_in, sd, case.activation, case.residual_mode)
    out = {}
    for a in ariths:
        enc._get_handle().set_gemm_mode(a)
        out[a] = enc.forward(xd, ld)[0].cpu()
    return out


def check_case(case, got, cus, ariths=ARITHS, fused=True):
    """got: device_outputs(case).  -> dict(failures = [...], ratios = {arith: worst |y - ref| / bound}, valid = the same
    over the frames below each row's length only, forms = {arith: names of the launches of the block under test}).
    fused: as plan()'s."""
    sd = weights(case)
    x, lens = inputs(case)
    lens_u = lens_chain(lens, case.blocks[:case.under])
    plans = {a: plan(case, a, cus, fused) for a in ariths}
    bad, ratios, forms, valid = [], {}, {}, {}
    groups = {}
    for a in ariths:       # arithmetics that produced the same leading output share one reference
        groups.setdefault(got[a]["lead"].numpy().tobytes(), []).append(a)
    for members in groups.values():
        lead = got[members[0]]["lead"].double()
        ref, bounds, lo = chain(lead, lens_u, sd, case.blocks[case.under:], case.under, {a: plans[a][case.under:] for a in members},
                                case.activation, case.residual_mode, case.probe)
        for a in members:
            forms[a] = form_names(plans[a][case.under])
            want = launch_counts(plans[a])
            if got[a]["counts"] is not None and got[a]["counts"] != want:
                bad.append(f"{case} {a}: launches (fused, depthwise, pointwise) {got[a]['counts']} != predicted {want}")
            if not np.array_equal(got[a]["lens"].numpy().astype(np.float32), lo.astype(np.float32)):
                bad.append(f"{case} {a}: encoded lengths differ")
            ratios[a], msg = judge(got[a]["y"], ref, bounds[a])
            if tuple(got[a]["y"].shape) == tuple(ref.shape):       # (the frames below each row's length alone, for the record)
                valid[a] = float(_mask((got[a]["y"].double() - ref).abs() / bounds[a], lo).max())
            if msg:
                bad.append(f"{case} {a} {forms[a]}: {msg}")
    return dict(failures=bad, ratios=ratios, forms=forms, valid=valid)
