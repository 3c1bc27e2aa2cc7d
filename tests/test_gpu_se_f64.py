"""-m gpu: squeeze-and-excitation blocks (csrc/encoder_se.hip and the plan around each SE in encoder_run.cpp run_encoder) against
the float64 oracle (oracle.quartznet_oracle, se_mean="rows": each row's own frames, the device's documented time mean).

Block level: one to three blocks through asr.JasperEncoder (vasr_encoder_f32) in f16x2, bf16x3 and fp32 on ragged batches --
rows of 1, 2, 3, 63-65, 127-129 frames and the full width, non-zero garbage past every row's length, one row scaled by 37.5 --
at batch sizes that make the layers around the SE take the latency GEMM and each split tile (asserted with
test_gpu_jasper.split_tile), in three excitation regimes: the synthetic weights (s close to 1), mixed signs (s across
(0, 1)), and "deep": one SE crafted so that every channel's pre-sigmoid value of some rows lies in [-25, -15] (s ~ 2^-36 ...
2^-21) while the other rows get ReLU-clamped hidden units (s = 0.5), with every BN shift zero so that the layers behind it
are measured against their own magnitude.  That regime is where the maxima table se_scale_kernel republishes matters: with
the GEMM's pre-SE maxima the next fp16-split operand would go subnormal.

Model level: an SE QuartzNet 15x5 and an SE Jasper-dense model at 64 ragged rows x ~10 s in default mode (fused kernel and
large tiles) in each arithmetic: sampled rows against the oracle, every row against its own batch-1 row-independent call.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_gpu_jasper import SPLIT_TILES, split_tile
from test_gpu_parity import _record

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ARITHMETICS = ("f16x2", "bf16x3", "fp32")
LOGP_REL = 2e-5
LOGP_ABS = 5e-4

# fp32 round-off bound of a row: FP32_REL * sqrt(reach / 1024) * max(1, |row|), reach = the reduction lengths of the chain
# (K * C_in per non-separable conv, K + C_in per separable sub-layer, C_in per residual pane); the deep regime's rows are held
# to their own magnitude (no floor of 1), plus the SE's own sensitivity there (SE_DEEP_REL * max|z| * cond: s = sigmoid(z) at
# z ~ -20 moves by |dz| relative, and z = W2 relu(W1 m) inherits the conditioning cond = sum|d_c m_c| / |d . m| of the
# crafted first layer).  Split arithmetics: worst error at most 1.5 x the fp32 chain's + 1e-7 of the largest output.
FP32_REL = 2e-6
SE_DEEP_REL = 1.2e-7
CPU32_FACTOR = 2.0      # ... and at least twice the float32 oracle's own error on the row (see bound() below)


def _blk(C, ratio, repeat=1, k=11, residual=False, separable=True, se=True, stride=1, dense=False):
    d = dict(filters=C, repeat=repeat, kernel=[k], stride=[stride], dilation=[1], dropout=0.0, residual=residual,
             separable=separable)
    if dense:
        d["residual_dense"] = True
    if se:
        d.update(se=True, se_reduction_ratio=ratio)
    return d


def _layout(kind, C, ratio):
    """-> (jasper list, (block, sub-layer or None for the residual pane 0) of the SE the deep regime crafts)."""
    if kind == "sep_res":           # separable residual block, repeat 3: SE on the residual pane, separate-residual GEMM
        return [_blk(C, ratio, repeat=3, residual=True)], (0, None)
    if kind == "nores":             # non-residual, repeat 3: SE after every sub-layer (the last one's before the output ReLU);
        # the only block, wider than its input: its sub-layer outputs live in the mid-pipeline buffers
        return [_blk(C, ratio, repeat=3, k=13)], (0, 0)
    if kind == "dense":             # a dense run of three SE blocks: every pane's SE scaled onto R
        return [_blk(C, ratio, repeat=2, k=5, residual=True, separable=False, dense=True) for _ in range(3)], (0, None)
    if kind == "k_s2":              # K-tap stride-2 non-separable SE block, pooled at the strided lengths, then a plain block
        return [_blk(C, ratio, k=11, separable=False, stride=2), _blk(C, ratio, k=9, residual=True, se=False)], (0, 0)
    if kind == "last":              # a plain block, then SE as the last block (its SE output is the encoder output)
        return [_blk(C, ratio, k=7, residual=True, se=False), _blk(C, ratio, repeat=2, k=9)], (1, 0)
    if kind == "then_plain":        # SE block, then a plain separable residual block: the republished maxima feed its
        return [_blk(C, ratio, k=11), _blk(C, ratio, k=15, residual=True, se=False)], (0, 0)   # Toeplitz dw + residual GEMM
    raise ValueError(kind)


# (id, layout, C_in, C, ratio, batch, T (input frames), input kind, regime, split tile of the SE block's GEMMs, "lat" for the
# batch <= 5 latency GEMM)
CASES = [
    ("sepres_c128_h1", "sep_res", 64, 128, 128, 12, 300, "gauss", "synth", 4),
    ("sepres_c128_hC_t3", "sep_res", 128, 128, 1, 40, 300, "relu", "mixed", 3),
    ("nores_c384_r5_t3", "nores", 64, 384, 5, 16, 260, "wide", "synth", 3),
    ("nores_c128_deep", "nores", 64, 128, 16, 10, 200, "gauss", "deep", 4),
    ("dense3_c128", "dense", 64, 128, 8, 9, 200, "gauss", "synth", 4),
    ("dense3_c384_mixed", "dense", 128, 384, 5, 6, 200, "relu", "mixed", 4),
    ("k11s2_c384_mixed", "k_s2", 64, 384, 5, 14, 400, "gauss", "mixed", 4),
    ("last_c128_wide", "last", 64, 128, 4, 5, 300, "wide", "synth", 4),
    ("then_plain_c128_deep", "then_plain", 64, 128, 8, 8, 300, "gauss", "deep", 4),
    ("then_plain_c1024_r8_deep_lat", "then_plain", 256, 1024, 8, 4, 256, "gauss", "deep", "lat"),
    ("then_plain_c1024_r1_deep_t3", "then_plain", 256, 1024, 1, 12, 256, "relu", "deep", 3),
    ("sepres_c1024_r1_t1", "sep_res", 256, 1024, 1, 64, 256, "relu", "synth", 1),
    ("nores_c1024_r8_t5", "nores", 256, 1024, 8, 48, 256, "gauss", "mixed", 5),
    ("then_plain_c1024_r8_t2", "then_plain", 256, 1024, 8, 32, 256, "wide", "deep", 2),
]
EDGE_LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129)
MAX_ORACLE_ROWS = 12            # the float64 oracle runs on at most this many rows of a case (the edge rows first)


def _input(cid, cin, B, T, kind):
    """Rows at the edge lengths (those shorter than T), one at T, the others uniform in [T/2, T]; row 1 scaled by 37.5;
    Gaussian / ReLU'd Gaussian / "wide" (2^-24 ... 2^6 inside one row); non-zero garbage past every row's length."""
    rng = np.random.default_rng(sum(map(ord, cid)))
    edges = [n for n in EDGE_LENGTHS if n < T]
    lens = np.concatenate([[T], edges, rng.integers(T // 2, T + 1, max(0, B - len(edges) - 1))])[:B].astype(np.int64)
    lens[0] = T
    rng.shuffle(lens)
    x = rng.standard_normal((B, cin, T)).astype(np.float32)
    if kind == "relu":
        x = np.maximum(x, 0)
    if kind == "wide":
        x = x * np.exp2(rng.integers(-24, 7, x.shape)).astype(np.float32)
    x[1] *= 37.5
    for b, n in enumerate(lens):
        x[b, :, n:] = rng.uniform(-50, 50, (cin, T - n)).astype(np.float32)
    return x, lens


def _sample_rows(lens, B):
    """Every row when the batch is small, else the edge-length rows, row 1 (x 37.5), the full-width rows and a few others."""
    if B <= MAX_ORACLE_ROWS:
        return list(range(B))
    pick = [b for b in range(B) if int(lens[b]) in EDGE_LENGTHS] + [1, int(np.argmax(lens)), B - 1]
    return sorted(dict.fromkeys(pick))[:MAX_ORACLE_ROWS]


def _se_prefix(jas, blk, sub):
    """State-dict prefix of block blk's SE after sub-layer `sub` (None: residual pane 0's SE)."""
    if sub is None:
        return f"encoder.{blk}.res.0.2"
    b = jas[blk]
    per = 3 if b.get("separable", False) else 2
    j = 0
    for r in range(sub + 1):
        j += per
        if r != b["repeat"] - 1:
            j += 2
        if r == sub:
            return f"encoder.{blk}.mconv.{j}"
        j += 1


def _se_input(x, lens, sd, jas, prefix):
    """The float64 tensor and lengths the oracle's SE `prefix` sees (the oracle up to that block, the SE call captured)."""
    from oracle import quartznet_oracle as O
    blk = int(prefix.split(".")[1])
    seen = {}
    orig = O.squeeze_excite

    def spy(t, l, sd_, p, se_mean="rows"):
        if p == prefix and p not in seen:
            seen[p] = (t.clone(), l.clone())
        return orig(t, l, sd_, p, se_mean)
    O.squeeze_excite = spy
    try:
        O.encoder_forward(x, torch.from_numpy(lens), sd, jas[:blk + 1], dtype=torch.float64)
    finally:
        O.squeeze_excite = orig
    return seen[prefix]


def _craft_deep(sd, jas, x, lens, prefix, rng):
    """W1 = w d^T, W2[c] = z_c w / |w|^2 with d the minimum-norm solution of m_b . d = +1 on the even rows ("deep") and -1 on
    the odd ones, m_b the float64 row mean at the SE's input: the deep rows get pre-sigmoid z_c in [-25, -15] on every channel,
    the others hidden units clamped to 0 (s = 0.5).  Every BN shift of the model is zeroed.  -> per row, max|z| * cond."""
    for k in list(sd):
        if k.endswith(".running_mean") or (k.endswith(".bias") and not k.startswith("decoder")):
            sd[k] = np.zeros_like(sd[k])
    t, l = _se_input(x, lens, sd, jas, prefix)
    n = l.to(torch.long).clamp(min=1)
    keep = (torch.arange(t.shape[2])[None, :] < n[:, None]).double()
    m = ((t * keep[:, None, :]).sum(2) / n[:, None].double()).numpy()
    B, C = m.shape
    target = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    d = np.linalg.lstsq(m, target, rcond=None)[0]
    H = sd[prefix + ".fc.0.weight"].shape[0]
    w = rng.uniform(0.5, 1.5, H)
    z = rng.uniform(-25.0, -15.0, C)
    sd[prefix + ".fc.0.weight"] = np.outer(w, d).astype(np.float32)
    sd[prefix + ".fc.2.weight"] = (z[:, None] * w[None, :] / float(w @ w)).astype(np.float32)
    d32 = sd[prefix + ".fc.0.weight"].astype(np.float64)[0] / w[0]
    q = m @ d32
    assert np.all(np.sign(q) == target), q          # the crafted split holds with the stored float32 weights
    cond = np.abs(m * d32[None, :]).sum(1) / np.abs(q)
    return np.where(target > 0, np.abs(z).max() * cond, 0.0)


def _mixed(sd, rng):
    """Every SE's weights redrawn with mixed signs: W1 ~ N(0, 1/C), W2 ~ N(0, 9/h) -- s spread over (0.02, 0.98)."""
    for k in list(sd):
        if k.endswith(".fc.0.weight"):
            h, c = sd[k].shape
            sd[k] = rng.normal(0, 1 / np.sqrt(c), (h, c)).astype(np.float32)
        elif k.endswith(".fc.2.weight"):
            c, h = sd[k].shape
            sd[k] = rng.normal(0, 3 / np.sqrt(h), (c, h)).astype(np.float32)


def _reach(jas, cin):
    r, c = 0, cin
    for b in jas:
        k = b["kernel"][0]
        for _ in range(b["repeat"]):
            r += (k + c) if b.get("separable", False) else k * c
            c = b["filters"]
        if b["residual"]:
            r += cin
    return r


_CACHE = {}


def _case(cid):
    if cid not in _CACHE:
        from viet_asr_amd import synth
        from oracle import quartznet_oracle as O
        case = next(c for c in CASES if c[0] == cid)
        _, kind, cin, C, ratio, B, T, inp, regime, _tile = case
        jas, (blk, sub) = _layout(kind, C, ratio)
        sd = synth.encoder_state_dict(jas, cin, 300 + C + ratio)
        x, lens = _input(cid, cin, B, T, inp)
        rows = _sample_rows(lens, B)
        rng = np.random.default_rng(sum(map(ord, cid)) + 1)
        deep = np.zeros(B)
        if regime == "mixed":
            _mixed(sd, rng)
        if regime == "deep":
            sub_x, sub_l = x[rows], lens[rows]
            cond = _craft_deep(sd, jas, sub_x, sub_l, _se_prefix(jas, blk, sub), rng)
            deep[rows] = cond          # (the deep / clamped split is over the oracle's rows: even / odd among them)
        want, wlen = O.encoder_forward(x[rows], torch.from_numpy(lens[rows]), sd, jas, dtype=torch.float64)
        w32, _ = O.encoder_forward(x[rows], torch.from_numpy(lens[rows]), sd, jas, dtype=torch.float32)
        cpu32 = [float((w32[k, :, :int(wlen[k])].double() - want[k, :, :int(wlen[k])]).abs().max()) for k in range(len(rows))]
        _CACHE[cid] = (case, jas, sd, x, lens, rows, want, wlen, deep, cpu32)
    return _CACHE[cid]


def _run(gpu, jas, sd, cin, x, lens):
    from viet_asr_amd import asr
    enc = asr.JasperEncoder(jasper=jas, activation="relu", feat_in=cin)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    xd, ld = torch.from_numpy(x).to(gpu), torch.from_numpy(lens).to(gpu)
    out = {}
    for gemm in ARITHMETICS:
        enc._get_handle().set_gemm_mode(gemm)
        y, yl = enc.forward(xd, ld)
        out[gemm] = (y.cpu(), yl.cpu())
    return out


def _gemm_cols(jas, T):
    """Padded column count of the SE block's pointwise / CONV GEMMs (every block of a layout but a strided one keeps T)."""
    from test_gpu_jasper import _conv_out
    b = jas[0]
    t = _conv_out(T, b["kernel"][0], b["stride"][0], 1)
    return -(-t // 128) * 128


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_se_blocks_against_float64(gpu, case):
    cid, kind, cin, C, ratio, B, T, inp, regime, tile = case
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    got_tile = split_tile(-(-C // 128) * 128, _gemm_cols(_layout(kind, C, ratio)[0], T), B, cus)
    if tile == "lat":
        # launch_pointwise_split hands an f16x2 GEMM on the 64 x 32 tile to the latency kernel when
        # pointwise_latency_supported(M, K) holds (encoder_pw_lat.hip: M % 128 == 0, K in {256, 512, 1024}); the two kernels
        # give the same bits, so the selection rule is what is checked here
        assert got_tile == 4 and C % 128 == 0 and C in (256, 512, 1024) and cin in (256, 512, 1024), cid
    else:
        assert got_tile == tile, (cid, got_tile)
    _, jas, sd, x, lens, rows, want, wlen, deep, cpu32 = _case(cid)
    got = _run(gpu, jas, sd, cin, x, lens)
    reach = _reach(jas, cin)
    errs, pad_errs, tops = {}, {}, []
    for k, b in enumerate(rows):
        f = int(wlen[k])
        tops.append(float(want[k, :, :f].abs().max()))
    for gemm in ARITHMETICS:
        y, yl = got[gemm]
        assert tuple(y.shape) == (B,) + tuple(want.shape[1:]), (cid, gemm)
        assert np.array_equal(yl.numpy()[rows].astype(np.float32), wlen.numpy().astype(np.float32)), (cid, gemm)
        assert bool(torch.isfinite(y).all()), (cid, gemm)
        errs[gemm], pad_errs[gemm] = [], []
        for k, b in enumerate(rows):
            f = int(wlen[k])
            d = (y[b].double() - want[k]).abs()
            errs[gemm].append(float(d[:, :f].max()))
            pad_errs[gemm].append(float(d[:, f:].max()) if f < d.shape[1] else 0.0)

    def bound(k):
        # never below twice what the oracle's own float32 run of the graph misses by: through three 1024-channel SE
        # sub-layers with mixed-sign excitation the row of 37.5 x gauss input (nores_c1024_r8_t5) ends at 1.2e-3 against
        # 6.0e-4 from the reach rule, and the float32 restatement at 4.3e-3 -- the reach rule, scaled by the output's
        # magnitude, does not see the larger pre-SE magnitudes the round-off came from
        b = rows[k]
        base = FP32_REL * (reach / 1024) ** 0.5
        if deep[b] > 0:
            return max((base + SE_DEEP_REL * deep[b]) * tops[k], CPU32_FACTOR * cpu32[k])
        return max(base * max(1.0, tops[k]), CPU32_FACTOR * cpu32[k])
    ratios = {g: max(e / bound(k) for k, e in enumerate(errs[g])) for g in ARITHMETICS}
    is_deep = [deep[b] > 0 for b in rows]
    _record("se_f64", case=cid, tile="lat" if tile == "lat" else "%dx%d" % SPLIT_TILES[tile], batch=B, regime=regime,
            rows=len(rows), **{g: ratios[g] for g in ARITHMETICS},
            **{"pad_" + g: max(e / bound(k) for k, e in enumerate(pad_errs[g])) for g in ARITHMETICS},
            deep_rel={g: max([e / tops[k] for k, e in enumerate(errs[g]) if is_deep[k]], default=0.0) for g in ARITHMETICS},
            worst_f32=max(errs["fp32"]), worst_cpu32=max(cpu32), scale=max(tops))
    # the split arithmetics against the fp32 chain, over the rows at ordinary magnitude, then over the deep rows, each
    # relative to its own magnitude
    plain = [k for k in range(len(rows)) if not is_deep[k]]
    deeps = [k for k in range(len(rows)) if is_deep[k]]
    for gemm in ("f16x2", "bf16x3"):
        if plain:
            w32 = max(errs["fp32"][k] for k in plain)
            assert max(errs[gemm][k] for k in plain) <= 1.5 * w32 + 1e-7 * max(tops[k] for k in plain), (cid, gemm)
        if deeps:
            w32 = max(errs["fp32"][k] / tops[k] for k in deeps)
            assert max(errs[gemm][k] / tops[k] for k in deeps) <= 1.5 * w32 + 1e-7, (cid, gemm, "deep")
    for k, b in enumerate(rows):
        for gemm in ARITHMETICS:
            assert errs[gemm][k] <= bound(k), (cid, gemm, b, int(lens[b]), errs[gemm][k], bound(k))
            # padded frames of the encoder output: no SE zeroes them there (zero_lens is null at the output), so they hold
            # what the reference computes from the masked inputs, as without SE
            assert pad_errs[gemm][k] <= bound(k), (cid, gemm, b, "padded frames", pad_errs[gemm][k], bound(k))


def test_multi_sublayer_last_block_wider_than_its_input(gpu):
    """Without SE: a non-residual separable block of three sub-layers, 64 -> 128 channels, as the only block.  Its first two
    sub-layer outputs (and their depthwise outputs) live in the mid-pipeline buffers, which were sized by the block input's 64
    channels when the block is the last one: each 128-channel write ran into the next buffer, and in fp32 a row of 127 frames
    (of 10) came out up to 5.2 off.  Every row of every arithmetic against float64."""
    from oracle import quartznet_oracle as O
    from viet_asr_amd import synth
    jas = [_blk(128, 8, repeat=3, k=13, se=False)]
    sd = synth.encoder_state_dict(jas, 64, 7)
    x, lens = _input("mid_buffers", 64, 10, 200, "gauss")
    want, wlen = O.encoder_forward(x, torch.from_numpy(lens), sd, jas, dtype=torch.float64)
    got = _run(gpu, jas, sd, 64, x, lens)
    base = FP32_REL * (_reach(jas, 64) / 1024) ** 0.5
    for gemm, (y, yl) in got.items():
        for b in range(len(lens)):
            f = int(wlen[b])
            err = float((y[b, :, :f].double() - want[b, :, :f]).abs().max())
            assert err <= base * max(1.0, float(want[b, :, :f].abs().max())), (gemm, b, int(lens[b]), err)


# ---------------------------------------------------------------------------------------------------------------------------
# Default-mode batches: 64 ragged rows x ~10 s through QuartzNetCTC.forward (fused kernel, large tiles), every arithmetic.

B64_SAMPLES = 160000
B64_MODELS = ("se_15x5_rows3", "se_dense_rows3")
# sampled rows' frames whose float64 margin lies inside the tolerance (measured: one frame of the 15x5 rows, every arithmetic)
EXPECTED_B64_NEAR_TIES = {"se_15x5_rows3": 1, "se_dense_rows3": 0}


def _tol(logp):
    return max(LOGP_ABS, LOGP_REL * float(np.abs(np.asarray(logp)).max()))


_B64 = {}


def _b64(gpu, name):
    if name not in _B64:
        from viet_asr_amd import configs, synth
        from viet_asr_amd.engine import QuartzNetCTC
        from oracle import quartznet_oracle as O
        g = np.load(os.path.join(HERE, "golden", name + ".npz"))
        jas = json.loads(str(g["definition"]))
        cfg = configs.jasper_definition(jas)
        seed = int(g["seed"]) + 64
        enc_sd = synth.encoder_state_dict(jas, 64, seed)
        dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, seed)
        samples = B64_SAMPLES if name == "se_15x5_rows3" else B64_SAMPLES // 4
        sig, lens = synth.audio_batch(64, samples, seed, ragged=True)
        lens[9] = 4000
        lens[33] = 480                                           # four mel frames
        for b in range(64):
            sig[b, lens[b]:] = 0
        rows = sorted({int(np.argmin(lens)), int(np.argmax(lens)), 9, 40, 57})
        refs = {}
        for b in rows:
            # the row as the batch holds it, zero-padded to the batch width: in default mode a row's STFT frames near its end
            # see the padding's zeros (the reference's collate + torch.stft(center=True)), where an unpadded call of the row
            # sees the reflection of its own samples -- so default mode is compared with the reference's BATCHED semantics
            ref = O.forward_all(sig[b:b + 1], lens[b:b + 1], enc_sd, dec_sd, jas)
            e64, _ = O.encoder_forward(ref["mel"], ref["seq"], enc_sd, jas, dtype=torch.float64)
            top2 = torch.topk(O.decoder_forward(e64, dec_sd), 2, dim=-1).values
            refs[b] = (ref, (top2[..., 0] - top2[..., 1]).numpy())
        _B64[name] = (QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu), sig, lens, refs)
    return _B64[name]


@pytest.mark.parametrize("gemm", ARITHMETICS)
@pytest.mark.parametrize("name", B64_MODELS)
def test_default_mode_b64_against_the_oracle_and_batch1_calls(gpu, name, gemm):
    """64 ragged rows in default mode: sampled rows (the shortest, the longest, a 25-frame and a 4-frame row among them),
    zero-padded to the batch width as the batch holds them, against the float64-checked oracle -- log-probs of every frame
    within max(5e-4, 2e-5 |lp|), equal encoded lengths, flips only at float64 near-ties (counted exactly) --, and EVERY row
    within the same tolerance of its own batch-1 default-mode call on that same padded row (64x32 tiles, no fused kernel:
    the plan a batch of one takes), with equal predictions except where that call's own top-2 margin lies inside the
    tolerance.  (A row-independent call on the unpadded row is the other semantics: it differs from the padded row by up to
    8 in log-prob near the row's end, with or without SE, because its STFT reflects the row's own samples there.)"""
    eng, sig, lens, refs = _b64(gpu, name)
    eng.handle.set_gemm_mode(gemm)
    eng.handle.profile_begin()
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
    torch.cuda.synchronize()
    fused = int(eng.handle.profile_end()["fused"]["launches"])
    near_total, worst = 0, 0.0
    for b, (ref, margin64) in refs.items():
        want = ref["logp"][0].numpy()
        f = want.shape[0]
        got = r["logp"][b, :f].cpu().numpy()
        tol = _tol(want)
        err = float(np.abs(got - want).max())
        worst = max(worst, err / tol)
        assert err <= tol, (name, gemm, b, err, tol)
        assert float(r["enc_len"][b]) == float(ref["enc_len"][0]), (name, gemm, b)
        near = margin64[0] < tol
        flips = r["pred"][b, :f].cpu().numpy() != ref["pred"][0].numpy()
        assert not (flips & ~near).any(), (name, gemm, b, np.argwhere(flips & ~near)[:5])
        near_total += int(near.sum())
    worst1, flips1 = 0.0, 0
    for b in range(64):
        n = int(lens[b])
        one = eng.forward(torch.from_numpy(np.ascontiguousarray(sig[b:b + 1])).to(gpu), torch.tensor([n], device=gpu),
                          want_logp=True)
        lp1 = one["logp"][0].cpu().numpy()
        f = lp1.shape[0]
        tol = _tol(lp1)
        err = float(np.abs(r["logp"][b, :f].cpu().numpy() - lp1).max())
        worst1 = max(worst1, err / tol)
        assert err <= tol, (name, gemm, b, "batch-1", err, tol)
        top2 = np.sort(lp1, axis=-1)[:, -2:]
        flips = r["pred"][b, :f].cpu().numpy() != one["pred"][0].cpu().numpy()
        assert not (flips & ~(top2[:, 1] - top2[:, 0] < 2 * tol)).any(), (name, gemm, b, "batch-1 flips")
        flips1 += int(flips.sum())
    eng.handle.set_gemm_mode("f16x2")
    _record("se_b64", model=name, gemm=gemm, rows=sorted(refs), worst_err_over_tol=worst, near_ties=near_total,
            worst_vs_batch1=worst1, flips_vs_batch1=flips1, fused_launches=fused)
    assert near_total == EXPECTED_B64_NEAR_TIES[name]


def test_random_se_architectures_in_batches_of_every_size_class(gpu):
    """Twenty SE cases of the fuzzers (tests/devtools/fuzz_encoder.py and fuzz_jasper.py with se=True: SE drawn per block,
    ratio and excitation regime -- synthetic, mixed signs, strong -- drawn too) in ragged batches of 1-5 / 6-20 / 21-72 rows
    against the oracle (row means)."""
    sys.path.insert(0, os.path.join(HERE, "devtools"))
    import fuzz_encoder
    import fuzz_jasper
    for mod in (fuzz_encoder, fuzz_jasper):      # the non-SE slices of this process have added to the module counters
        for k, v in mod.STATS.items():
            mod.STATS[k] = [0] * len(v) if isinstance(v, list) else type(v)(0)
    bad = [m for m in (fuzz_encoder.encoder_case(c, se=True) for c in range(10)) if m]
    bad += [m for m in (fuzz_jasper.jasper_case(c, se=True) for c in range(10)) if m]
    _record("se_fuzz", encoder=str(fuzz_encoder.STATS), jasper=str(fuzz_jasper.STATS))
    assert not bad, bad
    classes = [a + b for a, b in zip(fuzz_encoder.STATS["by_batch_class"], fuzz_jasper.STATS["by_batch_class"])]
    assert min(classes) > 0, classes
    assert fuzz_encoder.STATS["se_blocks"] > 0 and fuzz_jasper.STATS["se_blocks"] > 0
