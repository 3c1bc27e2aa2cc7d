"""What the CTC head's tests share (tests/test_gpu_head.py, tests/test_head_host.py): the float64 reference of the head (1x1
conv with bias -> log-softmax over the classes -> arg-max, frame-major), an ELEMENTWISE error bound, the restatement of the
product's kernel choice for the head's GEMM and epilogue, the case tables and their inputs, a float32 evaluation in the
kernel's order with switchable defects, and the runners that put one case on the device.

THE REFERENCE.  GEMM + epilogue: oracle.quartznet_oracle.decoder_forward on the float32 input converted exactly to float64.
The epilogue alone (decode.hip logsoftmax_argmax_kernel through vasr_bench_ctc_head): torch.log_softmax of the float32
logits converted exactly to float64.

THE BOUND, elementwise, with u = 2^-24 (sep_reference.EPS), first order.

  Logits z = W x + b, per arithmetic.  The GEMM terms are sep_reference._gemm_own (its docstring derives them: K float32
  accumulations, the f16x2 relative term R16 and floor F16 with M_x = the utterance's maximum over its valid frames -- every
  frame of the port tensor: vasr_decoder_logsoftmax_f32 takes it with launch_amax over all frames -- and M_w = the largest
  |w|; the bf16x3 dropped products R3).  The head's BN scale is 1 and its shift the bias: fmaf(acc, 1, b) is ONE rounding
  of a value of magnitude <= A_acc + |b| (A_acc = |W| |x|), and the f16x2 output scale is a power of two (exact):
      E_z = _gemm_own(arith, K, A_acc, |W|, |x|, M_x, M_w) + u (A_acc + |b|)
  Through the log-softmax lp_v = z_v - log sum_w exp z_w, whose derivative is delta_vw - p_w:
      E_z[v] + sum_w p_w E_z[w]
  The epilogue's own float32 terms, in the order the kernel computes (mx = max_w z_w is exact; d_w = |z_w - mx|;
  s = sum_w exp(z_w - mx) in [1, V]; lp = (z - mx) - log s):
      u d_v                                  the subtraction z_v - mx
      sum_w p_w (u d_w + C_E u)              the exponentials (relative error C_E u each) of the rounded arguments (an absolute
                                             u d_w in the argument is a relative u d_w in the exponential); an error of
                                             relative size r_w in term w of s moves log s by p_w r_w
      (V - 1) u                              the ascending one-accumulator sum of V positive terms: relative (V - 1) u in s
      C_L u |log s|                          logf
      u |lp_v|                               the final subtraction
      2^-126                                 so that exact values compare
  C_E and C_L are the accuracy of the device library's expf and logf in units of u.  THEY ARE AN ASSUMPTION, NOT A DERIVATION:
  the library's documented ulp figures were not at hand, so both start from 2 ulps (one ulp is at most 2 u relative: C = 4).
  Calibration on the CPU: the float32 restatement below (numpy's expf / logf) reaches 0.62 of the cruder bound
  u (d_v + V + 2 + 2 |lp_v|) at worst over V in {2, 29, 33, 64, 91, 128}, Gaussian logits at gains 1, 8 and 60 (|lp| up to
  480), 4000 frames each.  What the device reaches is recorded per case by tests/test_gpu_head.py and stated in its docstring:
  0.84 of this bound (0.58 of the cruder one) at worst on an MI355X, so both constants ENDED WHERE THEY STARTED, at 4.  They
  are to be raised only if the epilogue-alone ratio exceeds 1 AND the excess is traced to expf / logf.

  A frame whose logits are not all finite has no bound: the kernel must give what torch.log_softmax gives, which is a whole
  row of NaN as soon as one logit is NaN or +inf or all are -inf (prediction 0: NaN counts as a maximum and the first one is at
  index 0), and -inf exactly where a single logit is -inf.

THE KERNEL CHOICE, restated (head_plan): the head's GEMM has M = 128 packed rows of which V are stored (PwArgs.m_store), so only
the 128 x 64 and 64 x 32 split tiles divide it: 128 x 64 from B * ceil(ld / 64) >= 192 workgroups on (sep_reference.split_tile),
else 64 x 32 on two row blocks -- or, in f16x2 at K in {256, 512, 1024}, the latency kernel (128 rows per workgroup;
sep_reference.latency_supported).  The fp32 mode (encoder_pw.hip launch_pointwise): M % 256 != 0 and K % 64 == 0 give the
128 x 128 tile on four row wavefronts.  A row block m0 .. m0 + BM is "full" (vector stores, m0 + BM <= V), "partial" (scalar
stores of the rows < V) or "empty" (m0 >= V); every column tile is whole (the logits' pitch is padded).  The epilogue
instantiation is VMAX = V rounded up to 32; a thread's quarter holds VMAX / 4 classes.
"""
import ctypes as C

import numpy as np
import torch

import sep_reference as SEP
from sep_reference import EPS, F16, R16, R3, TINY, _gemm_own  # noqa: F401  (R16, F16, R3: re-exported for the docstring's names)

C_E = 4.0          # expf: 2 ulps, in units of u (assumed)
C_L = 4.0          # logf: 2 ulps, in units of u (assumed)
ARITHS = SEP.ARITHS
CLASS_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 98, 127, 128)
EPI_FRAMES = (1, 63, 64, 65, 130)
GEMM_FRAMES = (1, 33, 64, 100, 300)
GEMM_K = (64, 192, 256, 512, 1024)
NEAR_TIE_CAP = 0.03
LOGP_SENTINEL = np.float32(-12345.678)
PRED_SENTINEL = -7777
GUARD = 256


def vmax_of(V):
    """decode.hip launch_logsoftmax_argmax: the instantiation a class count selects."""
    return 32 if V <= 32 else 64 if V <= 64 else 96 if V <= 96 else 128


# ---- the product's kernel choice for the head, restated ----------------------------------------------------------------------
def _block_state(m0, bm, V):
    return "full" if m0 + bm <= V else ("empty" if m0 >= V else "partial")


def head_plan(V, K, B, T, arith, cus, force_tile=0, lat=True):
    """-> dict(kernel = "lat" | "128x64" | "64x32" | "fp32", blocks = the state of each row block, vmax).  force_tile /
    lat: the devtools switches VASR_PW3_TILE and VASR_PW_LAT."""
    ld = SEP.padded(T)
    if arith == "fp32":
        kernel, bm = "fp32", 128          # launch_pointwise: M = 128 is no multiple of 256, K % 64 == 0 -> launch_t<4, 1>
    else:
        tile = force_tile or SEP.split_tile(128, ld, B, cus)
        assert tile in (3, 4), tile
        kernel, bm = ("128x64", 128) if tile == 3 else ("64x32", 64)
        if arith == "f16x2" and not force_tile and lat and tile == 4 and SEP.latency_supported(128, K, 0):
            kernel, bm = "lat", 128
    return dict(kernel=kernel, blocks=tuple(_block_state(m0, bm, V) for m0 in range(0, 128, bm)), vmax=vmax_of(V))


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class EpiCase:
    """Logits for the epilogue alone.  kind: "gauss" (Gaussian at `gain`, frame 0 of every utterance steered so that the LAST
    class wins) or a planted kind, see logits()."""

    def __init__(self, V, frames, B, kind="gauss", gain=1.0):
        self.V, self.frames, self.B, self.kind, self.gain = V, frames, B, kind, gain
        self.name = f"v{V}_t{frames}_b{B}_{kind}" + (f"{gain:g}" if kind == "gauss" else "")
        self.seed = 300 + sum(map(ord, self.name)) % 211
        self.planted = kind != "gauss"

    def __repr__(self):
        return self.name


def _epi_table():
    # class count -> frame counts: every VMAX meets 1, 64 and 65 (test_head_host.py asserts it), B alternates 1 and 3
    frames = {1: (1, 130), 2: (64,), 31: (65,), 32: (63, 64), 33: (1, 65), 63: (64, 130), 64: (65, 63), 65: (1, 64),
              95: (65, 63), 96: (64, 130), 97: (1, 63), 98: (64, 65), 127: (65, 130), 128: (1, 64, 130)}
    out, i = [], 0
    for V in CLASS_COUNTS:
        for t in frames[V]:
            out.append(EpiCase(V, t, (1, 3)[i % 2], "gauss", (1.0, 8.0, 60.0)[i % 3]))
            i += 1
    # a tie between the last class of one quarter and the first of the next, in each instantiation (V < VMAX in two of them)
    out += [EpiCase(V, 65, 1, "tie_quarters") for V in (31, 64, 95, 128)]
    out += [EpiCase(33, 64, 3, "tie_ends"), EpiCase(98, 65, 1, "tie_ends")]
    out += [EpiCase(65, 63, 1, "all_equal"), EpiCase(128, 65, 3, "all_equal")]
    out += [EpiCase(32, 65, 1, "nonfinite"), EpiCase(98, 130, 3, "nonfinite")]
    out += [EpiCase(31, 64, 1, "span170"), EpiCase(98, 65, 3, "span170")]
    return out


EPI_CASES = _epi_table()


def logits(case):
    """-> (z [B][V][ld] float32 with NaN in the padding columns frames .. ld - 1, expect {(b, t): class} = the prediction a
    planted frame must get)."""
    rng = np.random.default_rng(case.seed)
    B, V, T = case.B, case.V, case.frames
    ld = SEP.padded(T)
    z = np.full((B, V, ld), np.nan, dtype=np.float32)
    expect = {}
    g = rng.standard_normal((B, V, T)).astype(np.float32)
    if case.kind == "gauss":
        g *= np.float32(case.gain)
        g[:, V - 1, 0] = g[:, :, 0].max(1) + np.float32(case.gain)       # the last class wins frame 0
    elif case.kind == "span170":
        g = rng.uniform(-170, 170, (B, V, T)).astype(np.float32)
        g[:, V - 1, 0] = np.float32(171)
    elif case.kind == "tie_quarters":
        vq = vmax_of(V) // 4
        top = np.float32(7.25)
        for t in range(T):
            e = (1 + t % 3) * vq                                          # first class of quarter 1, 2, 3
            g[:, e - 1, t] = g[:, e, t] = top
            for b in range(B):
                expect[(b, t)] = e - 1
    elif case.kind == "tie_ends":
        g[:, 0, :] = g[:, V - 1, :] = np.float32(6.5)
        expect = {(b, t): 0 for b in range(B) for t in range(T)}
    elif case.kind == "all_equal":
        g[...] = rng.standard_normal((B, 1, T)).astype(np.float32) * np.float32(20)
        expect = {(b, t): 0 for b in range(B) for t in range(T)}
    elif case.kind == "nonfinite":
        g *= np.float32(4)
        for b in range(B):
            g[b, (5 + b) % V, 3] = np.nan                                 # one NaN
            g[b, (9 + b) % V, 10] = np.inf                                # one +inf
            g[b, :, 20] = -np.inf                                         # all -inf
            g[b, V - 1 - b, 40] = -np.inf                                 # a single -inf (the last class in utterance 0)
            g[b, 0, T - 1] = np.nan                                       # the NaN in the first class of the last frame
            for t in (3, 10, 20, T - 1):
                expect[(b, t)] = 0
    else:
        raise ValueError(case.kind)
    z[:, :, :T] = g
    return z, expect


class GemmCase:
    """The head on a [B][K][T] port tensor.  wgain multiplies synth's decoder weights (gain 2)."""

    def __init__(self, V, K, B, T, wgain=1.0):
        self.V, self.K, self.B, self.T, self.wgain = V, K, B, T, wgain
        self.name = f"v{V}_k{K}_b{B}_t{T}" + (f"_g{wgain:g}" if wgain != 1.0 else "")
        self.seed = 500 + sum(map(ord, self.name)) % 193
        self.planted = False

    def __repr__(self):
        return self.name


BIG = (96, 100)          # B, T': 96 * ceil(128 / 64) = 192 workgroups, the smallest batch at T' = 100 that takes the 128 x 64 tile


def _gemm_table():
    out = []
    for i, V in enumerate(CLASS_COUNTS):
        # a latency shape (f16x2: latency kernel, bf16x3: 64 x 32 chunked), a depth the latency kernel refuses, the large batch
        out.append(GemmCase(V, (256, 512, 1024)[i % 3], 1 + (i + i // 3) % 3, GEMM_FRAMES[i % 5]))
        out.append(GemmCase(V, (64, 192)[i % 2], 1 + (i + 1) % 3, GEMM_FRAMES[(i + 2) % 5]))
        out.append(GemmCase(V, 64, *BIG))
    out.append(GemmCase(98, 1024, 2, 100, wgain=30.0))                    # |lp| in the hundreds: the relative terms
    return out


GEMM_CASES = _gemm_table()
BITS_CASES = [GemmCase(V, K, 2, 100) for K in (256, 1024) for V in (29, 64, 65, 128)]      # head_child.py: forced tiles
BITS_SETTINGS = ({"VASR_PW3_TILE": "3"}, {"VASR_PW3_TILE": "4"}, {"VASR_PW_LAT": "0"})
BY_NAME = {c.name: c for c in GEMM_CASES + BITS_CASES}


def head_weights(case):
    from viet_asr_amd import synth
    sd = synth.decoder_state_dict(case.K, case.V, case.seed)
    sd["decoder_layers.0.weight"] = (sd["decoder_layers.0.weight"] * np.float32(case.wgain)).astype(np.float32)
    return sd


def head_input(case):
    """x [B][K][T] float32: rectified Gaussians, utterance 1 (utterance 0 of a single one: its second half of the frames) at 300
    times the level of the rest -- the f16x2 scale is per utterance --, and frame 0 of every utterance steered along the last
    class's weights so that THAT class wins there (the defects that lose the last row or the last term are then seen at any T)."""
    rng = np.random.default_rng(case.seed)
    B, K, T, V = case.B, case.K, case.T, case.V
    x = np.maximum(rng.standard_normal((B, K, T)), 0).astype(np.float32)
    sd = head_weights(case)
    W = sd["decoder_layers.0.weight"][:, :, 0].astype(np.float64)
    b = sd["decoder_layers.0.bias"].astype(np.float64)
    if B > 1:
        x[1] *= np.float32(300)
    else:
        x[0, :, T // 2 + 1:] *= np.float32(300)
    if V > 1:
        # x0 + s relu(W[V - 1]) moves logit w by s c_w: the smallest s >= 0 that puts the last class 2 wgain above every other
        z0 = W @ x[:, :, 0].astype(np.float64).T + b[:, None]             # [V, B]
        dirn = np.maximum(W[V - 1], 0)
        c = W @ dirn
        assert (c[V - 1] > 1.25 * c[:V - 1]).all()
        step = ((z0[:V - 1] - z0[V - 1] + 2.0 * case.wgain) / (c[V - 1] - c[:V - 1])[:, None]).max(0).clip(0)
        x[:, :, 0] += (dirn[None, :] * step[:, None]).astype(np.float32)
    return x


# ---- reference and bound -------------------------------------------------------------------------------------------------------
def epilogue_bound(z):
    """z [B, V, T] float64 logits (taken as exact) -> (lp [B, T, V] = log_softmax, the epilogue's own bound [B, T, V]).  Frames
    with a non-finite logit carry NaN in the bound (judge() compares them for equality instead)."""
    V = z.shape[1]
    zt = z.transpose(1, 2)
    lp = torch.log_softmax(zt, -1)
    p = lp.exp()
    d = (zt - zt.amax(-1, keepdim=True)).abs()
    pd = torch.where(p > 0, p * d, torch.zeros_like(p))                   # (a single -inf: p = 0, d = inf)
    log_s = -lp.amax(-1, keepdim=True)
    own = EPS * d + (EPS * pd + C_E * EPS * p).sum(-1, keepdim=True) + (V - 1) * EPS + C_L * EPS * log_s.abs() + EPS * lp.abs()
    return lp, own + TINY


def crude_epilogue_bound(z):
    """u (d_v + V + 2 + 2 |lp_v|): the calibration figure of the docstring is stated against this."""
    zt = z.transpose(1, 2)
    lp = torch.log_softmax(zt, -1)
    return EPS * ((zt - zt.amax(-1, keepdim=True)).abs() + z.shape[1] + 2 + 2 * lp.abs())


def head_reference(case, x=None, ariths=ARITHS):
    """-> (ref logp [B, T, V] float64 = the oracle's decoder_forward, {arith: bound [B, T, V]})."""
    from oracle import quartznet_oracle as O
    sd = head_weights(case)
    x = torch.from_numpy(head_input(case) if x is None else x).double()
    ref = O.decoder_forward(x, sd)
    W = torch.from_numpy(sd["decoder_layers.0.weight"][:, :, 0]).double()
    b = torch.from_numpy(sd["decoder_layers.0.bias"]).double()
    z = torch.einsum("vk,bkt->bvt", W, x) + b[None, :, None]
    Ax = x.abs()
    Aacc = torch.einsum("vk,bkt->bvt", W.abs(), Ax)
    Mx, Mw = Ax.amax((1, 2)), float(W.abs().max())
    lp, own = epilogue_bound(z)
    assert float((lp - ref).abs().max()) < 1e-9 * max(1.0, float(ref.abs().max()))
    p = lp.exp()
    bounds = {}
    for a in ariths:
        Ez = (_gemm_own(a, case.K, Aacc, W.abs(), Ax, Mx, Mw) + EPS * (Aacc + b.abs()[None, :, None])).transpose(1, 2)
        bounds[a] = Ez + (p * Ez).sum(-1, keepdim=True) + own
    return ref, bounds


def top2_gap(ref):
    """The float64 top-2 gap of every frame and the classes that hold it -> (gap [B, T], first [B, T], second [B, T])."""
    if ref.shape[-1] == 1:
        z = torch.zeros(ref.shape[:-1], dtype=torch.int64)
        return torch.full(ref.shape[:-1], float("inf"), dtype=ref.dtype), z, z
    v, i = torch.topk(ref, 2, dim=-1)
    return v[..., 0] - v[..., 1], i[..., 0], i[..., 1]


def decided(ref, bound):
    """Frames whose float64 top-2 gap exceeds twice the bound (of the two classes that hold it): there an arg-max of values
    inside the bound cannot differ from the reference's.  -> bool [B, T]."""
    gap, i1, i2 = top2_gap(ref)
    b = torch.maximum(bound.gather(-1, i1[..., None]), bound.gather(-1, i2[..., None]))[..., 0]
    return gap > 2 * b


def first_argmax(lp):
    """numpy's arg-max: the FIRST index of the maximum, NaN counting as a maximum (as torch.argmax)."""
    return np.argmax(np.asarray(lp), axis=-1).astype(np.int64)


def judge(y, ref, bound):
    """-> (worst |y - ref| / bound over the finite reference values, message or None).  Where the reference is not finite the
    value must be the same non-finite one."""
    y = torch.as_tensor(np.asarray(y)).double()
    if tuple(y.shape) != tuple(ref.shape):
        return float("inf"), f"shape {tuple(y.shape)} != {tuple(ref.shape)}"
    fin = torch.isfinite(ref)
    odd = ~fin & ~((torch.isnan(ref) & torch.isnan(y)) | (ref == y))
    if bool(odd.any()):
        i = tuple(int(v) for v in odd.nonzero()[0])
        return float("inf"), f"reference {float(ref[i])} but got {float(y[i])} at {i} ({int(odd.sum())} such)"
    ratio = torch.where(fin, torch.nan_to_num((y - ref).abs() / bound, nan=float("inf"), posinf=float("inf")), torch.zeros_like(ref))
    worst = float(ratio.max())
    if worst <= 1.0:
        return worst, None
    i = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
    return worst, (f"|y - ref| = {abs(float(y[i]) - float(ref[i])):.3e} > bound {float(bound[i]):.3e} at (b, t, v) = {i} "
                   f"(ref {float(ref[i]):.6e}; {int((ratio > 1).sum())} elements outside)")


# ---- the float32 restatement, with defects -------------------------------------------------------------------------------------
MUTANTS = ("last_row", "batch_stride", "no_bias", "sum_short", "edge_clamp", "tie_later", "k_tail", "w_hi", "pitch")
GEMM_MUTANTS = ("last_row", "batch_stride", "no_bias", "k_tail", "w_hi")


def applies(mutant, case):
    """Whether the defect changes anything the tests look at on this case (a case of either table)."""
    V, B = case.V, case.B
    T = case.frames if isinstance(case, EpiCase) else case.T
    if mutant in GEMM_MUTANTS and isinstance(case, EpiCase):
        return False
    if mutant == "batch_stride":
        return B >= 2 and 2 <= V < 128
    if mutant == "pitch":
        return T >= 2                         # one row per 64-frame block has no pitch
    if mutant == "edge_clamp":
        # a quarter's first class below the last class (and the two not equal by construction)
        return vmax_of(V) // 4 <= V - 2 and getattr(case, "kind", "") != "all_equal"
    if mutant == "tie_later":                 # seen in the prediction alone, where a tie spans two quarters
        return getattr(case, "kind", "") in ("tie_quarters", "tie_ends", "all_equal")
    if mutant == "w_hi":
        return V >= 2 and case.K <= W_HI_MAX_K
    return V >= 2                             # one class: the log-prob is 0 whatever the logit


# The low fp16 weight plane dropped is a random relative 2^-12 a weight: ~ 2^-12 A_acc / sqrt(K) in a logit, against a bound
# whose accumulation term is the worst case K u A_acc.  The two cross near K = 2^8; above it the defect is what the bit
# equalities of test_gpu_head.py are for (as tests/sep_reference.py says of its 11-bit weights).
W_HI_MAX_K = 192


def f32_epilogue(z, mutant=None):
    """z [B, V, T] float32 -> (logp [B, T, V] float32, pred [B, T] int64) in the kernel's order: the maximum (fmaxf: NaN is
    skipped), expf of the differences, their ascending sum in one accumulator, logf, (z - mx) - ls; the arg-max first within a
    quarter of VMAX / 4 classes (strict >, from best = -inf, arg = 0), then the quarters in order (strict >).  Defects:
      sum_short   the sum of exponentials stops at V - 1
      edge_clamp  the first class of the last quarter edge below V - 1 is read as class V - 1
      tie_later   a tie between quarters goes to the later quarter
      pitch       the transposed 64-frame tile is written at pitch V + 1 instead of V (the buffer beyond holds NaN)"""
    z = np.array(z, dtype=np.float32)
    B, V, T = z.shape
    vq = vmax_of(V) // 4
    if mutant == "edge_clamp":
        e = max(q * vq for q in (1, 2, 3) if q * vq <= V - 2)
        z[:, e] = z[:, V - 1]
    with np.errstate(all="ignore"):
        mx = np.fmax.reduce(z, axis=1, initial=-np.inf)
        zm = (z - mx[:, None, :]).astype(np.float32)
        e = np.exp(zm).astype(np.float32)
        s = np.zeros((B, T), dtype=np.float32)
        for v in range(V - 1 if mutant == "sum_short" else V):
            s = (s + e[:, v]).astype(np.float32)
        ls = np.log(s).astype(np.float32)
        lp = (zm - ls[:, None, :]).astype(np.float32)
        best = np.full((B, T), -np.inf, dtype=np.float32)
        arg = np.zeros((B, T), dtype=np.int64)
        for q in range(4):
            bq = np.full((B, T), -np.inf, dtype=np.float32)
            aq = np.zeros((B, T), dtype=np.int64)
            for v in range(q * vq, min((q + 1) * vq, V)):
                hit = lp[:, v] > bq
                bq, aq = np.where(hit, lp[:, v], bq), np.where(hit, v, aq)
            if q == 0:
                best, arg = bq, aq
            else:
                hit = (bq >= best) if mutant == "tie_later" else (bq > best)
                best, arg = np.where(hit, bq, best), np.where(hit, aq, arg)
    out = np.ascontiguousarray(lp.transpose(0, 2, 1))
    if mutant == "pitch":
        flat = np.full(B * T * V + 64 * (V + 1), np.nan, dtype=np.float32)
        for b in range(B):
            for t0 in range(0, T, 64):
                base = (b * T + t0) * V
                for r in range(min(64, T - t0)):
                    flat[base + r * (V + 1): base + r * (V + 1) + V] = out[b, t0 + r]
        out = flat[:B * T * V].reshape(B, T, V).copy()
    return out, arg


def f32_head(x, sd, mutant=None):
    """The head in plain float32 (sequential torch GEMM, one rounding for the bias), then f32_epilogue.  Defects:
      last_row      the last class's row of logits is not stored (the workspace there holds 0)
      batch_stride  the epilogue steps 128 rows from utterance to utterance instead of V (past the buffer: 0)
      no_bias       the bias is dropped
      k_tail        the last 64 of K are dropped
      w_hi          the weights keep their fp16 high plane only (scaled as pack_pointwise_weights_f16x2 scales them)"""
    W = np.array(sd["decoder_layers.0.weight"][:, :, 0], dtype=np.float32)
    b = np.array(sd["decoder_layers.0.bias"], dtype=np.float32)
    V, K = W.shape
    if mutant == "w_hi":
        s = np.float32(2.0) ** (14 - np.floor(np.log2(np.abs(W).max())))
        W = ((W * s).astype(np.float16).astype(np.float32) / s).astype(np.float32)
    if mutant == "k_tail":
        W[:, K - 64:] = 0
    if mutant == "no_bias":
        b = np.zeros_like(b)
    with torch.no_grad():
        z = (torch.einsum("vk,bkt->bvt", torch.from_numpy(W), torch.from_numpy(np.asarray(x, dtype=np.float32))) +
             torch.from_numpy(b)[None, :, None]).numpy()
    B, _, T = z.shape
    if mutant == "last_row":
        z[:, V - 1] = 0
    if mutant == "batch_stride":
        rows = np.concatenate([z.reshape(B * V, T), np.zeros((B * 128, T), dtype=np.float32)])
        z = np.stack([rows[b * 128: b * 128 + V] for b in range(B)])
    return f32_epilogue(z, mutant if mutant not in GEMM_MUTANTS else None)


# ---- the runners ---------------------------------------------------------------------------------------------------------------
def device_epilogue(case, device, want_logp=True, want_pred=True):
    """The case's logits through vasr_bench_ctc_head -> dict(logp [B, T, V] float32 | None, pred [B, T] int64 | None, bad = what
    the guard bands and the sentinel found wrong).  Each output sits between two guard bands and is filled with a sentinel
    before the call: every element inside must be written, nothing outside."""
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    z, _ = logits(case)
    B, V, T = case.B, case.V, case.frames
    zd = torch.from_numpy(z).to(device)
    n = B * T * V
    lbuf = torch.full((GUARD + n + GUARD,), float(LOGP_SENTINEL), dtype=torch.float32, device=device)
    pbuf = torch.full((GUARD + B * T + GUARD,), PRED_SENTINEL, dtype=torch.int64, device=device)
    lptr = lbuf.data_ptr() + 4 * GUARD if want_logp else None
    pptr = pbuf.data_ptr() + 8 * GUARD if want_pred else None
    _lib.check(L.vasr_bench_ctc_head(zd.data_ptr(), B, T, V, lptr, pptr, torch.cuda.current_stream().cuda_stream), L)
    torch.cuda.synchronize()
    lh, ph = lbuf.cpu().numpy(), pbuf.cpu().numpy()
    bad = []
    for name, h, inner, sent, want in (("logp", lh, n, LOGP_SENTINEL, want_logp), ("pred", ph, B * T, PRED_SENTINEL, want_pred)):
        if not (h[:GUARD] == sent).all() or not (h[GUARD + inner:] == sent).all():
            bad.append(f"{case}: {name}: a guard band was written")
        body = h[GUARD: GUARD + inner]
        if want and (body == sent).any():
            bad.append(f"{case}: {name}: {int((body == sent).sum())} elements were not written")
        if not want and not (body == sent).all():
            bad.append(f"{case}: {name}: written although NULL was passed")
    return dict(logp=lh[GUARD: GUARD + n].reshape(B, T, V).copy() if want_logp else None,
                pred=ph[GUARD: GUARD + B * T].reshape(B, T).copy() if want_pred else None, bad=bad)


def check_epilogue(case, got):
    """got: device_epilogue(case) with both outputs -> dict(failures, ratio = worst |logp - ref| / bound, crude = the same against
    crude_epilogue_bound, excluded = the share of frames the gap rule leaves out)."""
    z, expect = logits(case)
    z64 = torch.from_numpy(z[:, :, :case.frames]).double()
    ref, bound = epilogue_bound(z64)
    bad = list(got["bad"])
    ratio, msg = judge(got["logp"], ref, bound)
    if msg:
        bad.append(f"{case}: {msg}")
    fin = torch.isfinite(ref).all(-1)
    crude = float(torch.where(torch.isfinite(ref), (torch.from_numpy(got["logp"]).double() - ref).abs() / crude_epilogue_bound(z64),
                              torch.zeros_like(ref)).nan_to_num(nan=float("inf")).max())
    own = first_argmax(got["logp"])
    if not np.array_equal(got["pred"], own):
        bad.append(f"{case}: pred differs from the first maximum of the device's own logp in {int((got['pred'] != own).sum())} frames")
    sure = (decided(torch.nan_to_num(ref, nan=0.0, neginf=-1e300), torch.nan_to_num(bound, nan=0.0, posinf=0.0)) & fin).numpy()
    want = first_argmax(ref.numpy())
    if not np.array_equal(got["pred"][sure], want[sure]):
        bad.append(f"{case}: pred differs from the float64 arg-max in {int((got['pred'][sure] != want[sure]).sum())} decided frames")
    for (b, t), c in expect.items():
        if int(got["pred"][b, t]) != c:
            bad.append(f"{case}: planted frame (b, t) = ({b}, {t}): pred {int(got['pred'][b, t])}, expected {c}")
    excluded = float(1 - sure[fin.numpy()].mean()) if bool(fin.any()) else 0.0
    if not case.planted and excluded > NEAR_TIE_CAP:
        bad.append(f"{case}: {excluded:.1%} of the frames are near-ties (cap {NEAR_TIE_CAP:.0%})")
    return dict(failures=bad, ratio=ratio, crude=crude, excluded=excluded)


def device_head(case, device, ariths=ARITHS, rows=None):
    """The case (rows: those utterances as a batch of their own) through _lib.Handle(dec_feat_in, num_classes) + stages.decoder
    (vasr_decoder_logsoftmax_f32) -> {arith: logp [B, T, V] float32 on the host}."""
    from viet_asr_amd import _lib, stages
    h = _lib.Handle(dec_feat_in=case.K, num_classes=case.V)
    h.load_state_dict(head_weights(case))
    h.finalize()
    x = head_input(case)
    xd = torch.from_numpy(x if rows is None else x[rows]).to(device)
    out = {}
    for a in ariths:
        h.set_gemm_mode(a)
        out[a] = stages.decoder(h, xd).cpu().numpy()
    torch.cuda.synchronize()
    h.close()
    return out


def check_head(case, got, cus):
    """got: device_head(case) -> dict(failures, ratios = {arith: worst |logp - ref| / bound}, lse = {arith: worst |logsumexp| /
    the row's largest bound}, excluded = {arith: share of near-tie frames}, forms = {arith: kernel and row-block states})."""
    ref, bounds = head_reference(case, ariths=tuple(got))
    bad, ratios, lse, excluded, forms = [], {}, {}, {}, {}
    want = first_argmax(ref.numpy())
    for a, y in got.items():
        p = head_plan(case.V, case.K, case.B, case.T, a, cus)
        forms[a] = f"{p['kernel']}:{'+'.join(p['blocks'])}:vmax{p['vmax']}"
        ratios[a], msg = judge(y, ref, bounds[a])
        if msg:
            bad.append(f"{case} {a} {forms[a]}: {msg}")
            continue
        # a row of log-probs whose errors are e_v has logsumexp = sum_v p_v e_v to first order: at most the row's largest bound
        l = torch.logsumexp(torch.from_numpy(y).double(), -1).abs() / bounds[a].amax(-1)
        lse[a] = float(l.max())
        if not lse[a] <= 1.0:
            bad.append(f"{case} {a}: a row is no log-distribution: |logsumexp| = {lse[a]:.3g} of the row's bound")
        sure = decided(ref, bounds[a]).numpy()
        got_arg = first_argmax(y)
        if not np.array_equal(got_arg[sure], want[sure]):
            bad.append(f"{case} {a}: arg-max differs from float64's in {int((got_arg[sure] != want[sure]).sum())} decided frames")
        excluded[a] = float(1 - sure.mean())
        if excluded[a] > NEAR_TIE_CAP:
            bad.append(f"{case} {a}: {excluded[a]:.1%} of the frames are near-ties (cap {NEAR_TIE_CAP:.0%})")
    return dict(failures=bad, ratios=ratios, lse=lse, excluded=excluded, forms=forms)


def null_pointer_call(L, batch, frames, num_classes, logp=True, pred=True):
    """vasr_bench_ctc_head with pointers that are never dereferenced: for the refusals that come before any launch."""
    fake = C.c_void_p(4096)
    return int(L.vasr_bench_ctc_head(fake, batch, frames, num_classes, fake if logp else None, fake if pred else None, None))
