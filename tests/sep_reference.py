"""What the separable-block tests share (tests/test_gpu_sep.py, tests/test_sep_host.py): a float64 restatement of a short chain
of JasperBlocks with an ELEMENTWISE error bound per arithmetic, the restatement of the product's kernel choice (which form
every sub-layer takes), the case table and its inputs, a device-like float32 evaluation with switchable defects, and the
runner that puts one case through asr.JasperEncoder (vasr_encoder_f32) and lists what it finds wrong.

A case is an encoder of one to three blocks: an optional cheap LEADING block (a 1x1 conv 64 -> C; a sub-layer whose input
carries no published maxima can take neither the Toeplitz nor the fused form, so the block under test must not come first), the
block UNDER TEST, and an optional TRAILING block that passes every channel through: a 1x1 conv C -> C whose weight is the
identity matrix and whose BatchNorm is the identity (gamma 1, beta 0, mean 0, var chosen so that the float32 alpha is exactly
1; weights() overwrites synth's draw).  The trailing block is there because the last sub-layer of an encoder's LAST block
writes the port tensor and is never fused (vasr_api.cpp run_encoder: !enc_out): the fused kernel with its folded residual, and
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
  BatchNorm affine y = alpha acc + beta, alpha = g / sqrt(var + 1e-3), beta = b - mean alpha in float32 (vasr_api.cpp
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


def residual_folds(cfg, cin):
    """vasr_api.cpp build_encoder: the residual 1x1 conv becomes a second K range of the block's last GEMM."""
    k, stride, _ = _geo(cfg)
    if not cfg["residual"] or stride != 1 or not (cfg["separable"] or k == 1):
        return False
    f = cfg["filters"]
    k1 = f if cfg["repeat"] > 1 else cin
    chunk = 128 if f % 512 == 0 else (64 if f % 256 == 0 else 32)
    return k1 % chunk == 0 and cin % chunk == 0


def plan(case, arith, cus):
    """-> list (one entry per block) of lists of launches, in run_encoder's order.  A launch is a dict: kind = "fused" (cols 64
    / 128, dual), "dw" (form toeplitz / fma / generic) or "gemm" (tile = 1 .. 5 or "lat" or "fp32", arith = the arithmetic that
    runs -- a GEMM whose source has no published maxima keeps 3 x bf16 in f16x2 mode --, epi = plain / masked / RES / DUAL,
    port = it writes the unpadded encoder output, mx = whose maximum scales the activations: "in", "dw", "l1")."""
    B, T = case.B, case.T
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
        fold = residual_folds(cfg, cin)
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
            if (f16 and sep and c == 256 and f == 256 and stride == 1 and dil == 1 and k in (33, 39) and has_amax
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


# ---- cases -------------------------------------------------------------------------------------------------------------------
class Case:
    """blocks[under] is the block under test; blocks before it are run alone on the device first (their output is the
    reference's input), blocks after it belong to the judged chain."""

    def __init__(self, name, feat_in, blocks, under, B, T=100, kind="gauss"):
        self.name, self.feat_in, self.blocks, self.under, self.B, self.T, self.kind = name, feat_in, blocks, under, B, T, kind
        self.seed = 100 + sum(map(ord, name)) % 97

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


def weights(case):
    """synth's weights for the chain (BN statistics with scale != 1 and shift != 0), channel 3's taps of the block under test
    a thousand times smaller, a trailing block the identity: weight I, BN with alpha = 1 and beta = 0 exactly in float32."""
    from viet_asr_amd import synth
    sd = synth.encoder_state_dict(case.blocks, case.feat_in, case.seed)
    if case.blocks[case.under]["separable"]:
        sd[f"encoder.{case.under}.mconv.0.conv.weight"][3] *= np.float32(1e-3)
    var = np.float32(1) - np.float32(1e-3)
    assert np.float32(var + np.float32(1e-3)) == np.float32(1)
    for i in range(case.under + 1, len(case.blocks)):
        c = case.blocks[i]["filters"]
        pre = f"encoder.{i}.mconv."
        assert sd[pre + "0.conv.weight"].shape == (c, c, 1)
        sd[pre + "0.conv.weight"][...] = np.eye(c, dtype=np.float32)[:, :, None]
        for key, val in (("weight", 1), ("bias", 0), ("running_mean", 0), ("running_var", var)):
            sd[pre + "1." + key][...] = np.float32(val)
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
    """vasr_api.cpp bn_affine in float32 -> (alpha, beta) as the device holds them, and |b| + |mean alpha| (float64)."""
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


def chain(x, lens, sd, blocks, i0, plans):
    """The blocks `blocks` (encoder indices i0 ...) on x [B, C, T] float64 (taken as exact), lens [B] int64.  plans:
    {arith: plan(...)[i0:]} for the arithmetics wanted.  -> (ref [B, C', T'] float64, {arith: bound}, lens')."""
    ariths = list(plans)
    lens = np.asarray(lens, dtype=np.int64)
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
            fold = residual_folds(cfg, v.shape[1])
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
                    own = _gemm_own(l["arith"], W.shape[1], Aacc, W.abs(), blk_in[1], blk_mx[a], float(W.abs().max()))
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
                        own = _gemm_own(l["arith"], W.shape[1], Aacc, W.abs(), Am, mx[a], float(W.abs().max()))
                        yE[a] = al.abs() * (got[1 + idx] + own) + AFFINE * EPS * yA
                        if last_sub and res:
                            assert l["epi"] == "RES", (l, a)
                            yE[a] = yE[a] + R[2][a] + EPS * (yA + R[1])
                if dual:
                    yA = yA + yA2
                elif last_sub and res:
                    yv, yA = yv + R[0], yA + R[1]
                v, E = torch.relu(yv), yE
    return v, {a: E[a] + TINY for a in ariths}, lens


# ---- a device-like float32 evaluation, with defects ---------------------------------------------------------------------------
MUTANTS = ("mask_late", "res_lens", "dw_pad", "k_chunk", "w_11bit", "shift_before_res")


def f32_chain(x, lens, sd, blocks, i0, under=0, mutant=None, first_lens=None):
    """The same blocks in plain float32 on the CPU (sequential torch), arranged as the device arranges them: BN as the
    float32 affine of bn_affine in the GEMM's epilogue, a folded residual as ONE product over both K ranges with the scaled
    weights and the sum of both shifts.  mutant (applied to block `under` of the list only):
      mask_late         the depthwise input mask one column late
      res_lens          the residual source masked with another length vector (first_lens: the encoder's input lengths)
      dw_pad            the depthwise padding off by one
      k_chunk           one 64-wide K chunk of the second source (the residual) dropped
      w_11bit           the 1x1 weights rounded to 11 bits: the low fp16 plane dropped
      shift_before_res  a folded residual's shift left out (only the main branch's shift is applied)."""
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
            fold = residual_folds(cfg, v.shape[1])
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
                        y = al[None, :, None] * torch.einsum("ok,bkt->bot", W, vm) + be[None, :, None] + R
                else:
                    y = al[None, :, None] * torch.einsum("ok,bkt->bot", W, vm) + be[None, :, None]
                v = torch.relu(y)
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


def encoder(blocks, feat_in, sd):
    from viet_asr_amd import asr
    enc = asr.JasperEncoder(jasper=blocks, activation="relu", feat_in=feat_in)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    return enc


def device_outputs(case, device, ariths=ARITHS, profile=True):
    """The case on the device -> {arith: dict(y = encoder output (host), lens, lead = the leading blocks' output run alone
    (host; the input itself without leading blocks), counts = (fused, depthwise, pointwise) launches of the whole encoder)}."""
    sd = weights(case)
    x, lens = inputs(case)
    xd, ld = torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device)
    full = encoder(case.blocks, case.feat_in, sd)
    head = encoder(case.blocks[:case.under], case.feat_in, sub_state_dict(sd, case.under)) if case.under else None
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
    enc = encoder(case.blocks, case.feat_in, sd)
    out = {}
    for a in ariths:
        enc._get_handle().set_gemm_mode(a)
        out[a] = enc.forward(xd, ld)[0].cpu()
    return out


def check_case(case, got, cus, ariths=ARITHS):
    """got: device_outputs(case).  -> dict(failures = [...], ratios = {arith: worst |y - ref| / bound}, valid = the same
    over the frames below each row's length only, forms = {arith: names of the launches of the block under test})."""
    sd = weights(case)
    x, lens = inputs(case)
    lens_u = lens_chain(lens, case.blocks[:case.under])
    plans = {a: plan(case, a, cus) for a in ariths}
    bad, ratios, forms, valid = [], {}, {}, {}
    groups = {}
    for a in ariths:       # arithmetics that produced the same leading output share one reference
        groups.setdefault(got[a]["lead"].numpy().tobytes(), []).append(a)
    for members in groups.values():
        lead = got[members[0]]["lead"].double()
        ref, bounds, lo = chain(lead, lens_u, sd, case.blocks[case.under:], case.under, {a: plans[a][case.under:] for a in members})
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
