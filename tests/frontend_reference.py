"""Float64 restatement of the mel front end (csrc/frontend.hip: stft_logmel_kernel, seq_len_kernel, the normalisation
kernels), the elementwise error bounds its device tests judge by, the restated choice between the kernel's two forms, and
the case table.  numpy only for the chain and the bounds; the case's library description (window values, Slaney bank) comes
from viet_asr_amd.frontend_tables like the product's.

1. The chain (FilterbankFeatures.forward, parts/features.py:245-301, in the project's conventions)
    seq     = ceil(float32(len) / float32(hop))                       the float32 quirk of seq_len_kernel
    y[n]    = x[n] - float32(p) * x[n-1],  y[0] = x[0]                 off when preemph is None
    padding = reflection by 256 at the padded batch width L; in row-independent mode at the row's own length
              (n < 0 -> -n;  n >= ns -> 2 (ns - 1) - n;  what is still outside reads as 0, as the kernel's guard does)
    frame t = samples t hop - 256 .. t hop + 255 of the padded row, times the float32 window placed at (512 - win) // 2
    X       = rfft (float64),  P = |X|^2,  acc = fb P  (float32 filterbank values as float64)
    raw     = log(acc + g)  or  log(max(acc, g));  frames >= seq are exactly 0
    per_feature / all_features: (raw - mean) / (std + float32(1e-5)), unbiased std, over the frames below seq
    (features.py:17-39); frames >= seq stay 0.

2. The bound on the raw log-mel, from the kernel's arithmetic (u = 2^-24, the unit roundoff of float32)
    dX   = u (c sqrt(E_t) + sqrt(E_p))
    dP_k = 2 |X_k| dX + dX^2 + a u P_k
    dacc = |fb| dP + b u |fb| P
    r    = dacc / (acc + g)            [clamp: dacc / max(acc, g), and 0 where acc + dacc < g]
    bound = max(r, min(-log(1 - r), log(den / g))) + d u max(|ref|, 1)
 E_t is the energy of the windowed pre-emphasised frame, sum (w y)^2; by Parseval it is the mean square of a spectrum bin,
 so an error of relative size e in the 2-norm of the transform is e sqrt(E_t) per bin when it is spread over the bins as
 rounding errors are.  (Concentrated in ONE bin it could be sqrt(512) times that: a bound for that case would be vacuous.)
 The count, each operation at its worst-case constant in units of u:
    c = 12   1    the subtraction of the pre-emphasis (relative to y)
             1    the window product
             4 x 2 x 1     four radix-4 stages of the 256-point complex FFT, two levels of additions each, every
                           addition relative to its own result
             3 x sqrt(5)   a complex product with a float32 twiddle in three of the stages (Brent, Percival, Zimmermann
                           2007), and 3 x 1 for the rounded twiddles themselves
             the real split: e and o one addition each (|e|^2 + |o|^2 sum to |Z|^2: one 1 between them), the twiddle
                           product sqrt(5) and the rounded twiddle 1 on o, the final addition 1
         Added linearly (every rounding in the same direction in every stage) these are 25; the bound is then 2e-3 on
         white noise in the 128-row cases of the table, i.e. it would let a wrong digit through where it should not.  They
         are roundings of distinct operations, independent of each other, so they are added in quadrature:
         sqrt(2 + 8 + 3 (5 + 1) + (1 + 5 + 1 + 1)) = sqrt(36) = 6 is the scale of one bin's error, and c is TWICE that: an
         element is judged against two such scales.  That factor is not taken from the kernel: torch's float32 STFT, the
         reference's own arithmetic, reaches 0.41 of the resulting bound at its worst element of the table, an honest
         float32 restatement with numpy's FFT 0.26 (test_frontend_host.py prints both per case), and with c = 6 a float32
         transform that is one half less accurate than those two would already be refused.
    E_p      the FIRST rounding of the pre-emphasis, fl(p x[n-1]), is relative to p x[n-1] and not to y: it has its own
             energy sum (w p x[n-1])^2 with the constant 1 (0.49 E_t on white noise; what dominates on a DC offset).
    a = 2    two squares and their sum, (1 + u)^2 (an fma only removes one).
    b = 33   32 fmaf of the tap loop (the usual n u of a recursive sum; all products are non-negative), + 1 for acc + g.
    d = 4    logf is documented at 1 ulp = 2 u of |ref|; twice that.  max(|ref|, 1) keeps the term from vanishing at log 1.
 The first term is the exact effect of dacc on the logarithm: up by at most r, down by -log(1 - r), and never below
 log(g), since no product of the tap sum is negative (every bank here is non-negative) -- for small r it is the r of the
 form above.  Under clamp the reference sits at log(g) where acc < g, and so does the device unless acc + dacc >= g.

3. The bound on the normalisation alone, with the device's own float32 raw log-mel x as the input of both sides.  The kernels
 keep their sums in double (error ~ n 2^-53, covered by the factor below) and then round: mean to float32 (u |mu|), the root
 to float32 and the sum with 1e-5f (2 u of D = std + 1e-5), one subtraction (u |x - mu|), one division (u |ref|):
    bound = 1.001 (u (|mu| + |x - mu|) / D + 3 u |ref|)
 The dominant term is u |mu| / D: a row of log-mels near -16 with a small deviation loses its digits in the float32 mean, on
 the device as in the reference's float32.  torch sums its statistics in float32 on the CPU: the oracle is
 judged with ceil(log2 n) u more on the mean and on the deviation (normalize(float32_sums=True)), the device never is.

4. The form: launch_stft_logmel takes 8 frames per workgroup when ceil(T / 32) * B < 128, else 32.  LDS of a form:
 4 ((fpb - 1) hop + 512 rounded up to 4) + 16384 + 8 * 292 * 4 + 64 (fpb + 1) 4 -- above 64 KB from hop 237 in the 32-frame form.
"""
import math
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
NFFT, NBINS, NMELS, MEL_TAPS = 512, 257, 64, 32
C_X, A_P, B_ACC, D_LOG = 12.0, 2.0, 33.0, 4.0
EPS32 = float(np.float32(1e-5))
TINY32 = float(np.finfo(np.float32).tiny)


def form(B, T):
    """Frames per workgroup launch_stft_logmel picks (frontend.hip)."""
    return 8 if -(-T // 32) * B < 128 else 32


def lds_bytes(fpb, hop):
    seg = (fpb - 1) * hop + NFFT
    return ((seg + 3) & ~3) * 4 + 8 * 256 * 8 + 8 * (260 + MEL_TAPS) * 4 + 64 * (fpb + 1) * 4


def seq_len(lens, hop):
    return np.ceil(np.asarray(lens).astype(np.float32) / np.float32(hop)).astype(np.int64)


# --------------------------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    name: str
    win: int
    hop: int
    B: int
    L: int
    signal: str = "white"        # "white": every row white noise at 0.1;  "mix": the signal list below;  "norm": section 3's rows
    window: str = "hann"
    bank: str = "slaney"
    preemph: object = 0.97
    guard: float = 2.0 ** -24
    guard_type: str = "add"
    own: bool = False            # row-independent mode
    norm: bool = False           # also judged through per_feature and all_features

    def __repr__(self):
        return self.name

    @property
    def T(self):
        return 1 + self.L // self.hop

    @property
    def form(self):
        return form(self.B, self.T)


KINDS = ("white", "quant", "faint", "gap", "zero", "tone", "lowpass", "dc", "imp0", "implen", "impL", "alt")
# (kind, length option) of the first rows of a "mix" batch: every kind once with a length that lets its feature be judged,
# then the lengths 1 and 0 on noise.  Later rows cycle kinds (period 12) against length options (period 7).
MIX_ROWS = (("white", 0), ("quant", 3), ("faint", 0), ("gap", 0), ("zero", 2), ("tone", 1), ("lowpass", 0), ("dc", 4),
            ("imp0", 5), ("implen", 3), ("impL", 0), ("alt", 2), ("white", 6), ("white", 5))
NORM_SEQ = (2, 255, 256, 257, None, 1, 0, None)      # valid frames of the "norm" rows (None: all T); the last row is all zero


def _len_options(L, hop):
    k = max(2, min((L - 1) // hop, -(-400 // hop)))
    return [L, k * hop - 1, k * hop, k * hop + 1, 257, 1, 0]


def _row(kind, L, n, hop, seed):
    """One float32 row of L samples whose stated length is n; what lies past n is not zero unless the kind says so."""
    rng = np.random.default_rng([L, seed, KINDS.index(kind)])
    t = np.arange(L)
    if kind == "white":
        x = 0.1 * rng.standard_normal(L)
    elif kind == "quant":                                   # 16-bit PCM at almost full scale
        x = np.round(rng.uniform(-0.9, 0.9, L) * 32768.0) / 32768.0
    elif kind == "faint":                                   # the mel sums sit beside the guard
        x = 1e-4 * rng.standard_normal(L)
    elif kind == "gap":                                     # exact zeros longer than 512 + hop: acc == 0 inside noise
        x = 0.1 * rng.standard_normal(L)
        x[300:300 + NFFT + hop + 200] = 0.0
    elif kind == "zero":
        x = np.zeros(L)
    elif kind == "tone":                                    # 1 kHz over noise 60 dB down
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t / 16000.0) + 0.0005 * rng.standard_normal(L)
    elif kind == "lowpass":                                 # nothing above 2 kHz but the float32 rounding of the samples
        s = np.fft.rfft(0.1 * rng.standard_normal(L))
        s[int(L * 2000 / 16000):] = 0
        x = np.fft.irfft(s, L)
    elif kind == "dc":
        x = 0.5 + 0.1 * rng.standard_normal(L)
    elif kind in ("imp0", "implen", "impL"):
        x = np.zeros(L)
        at = {"imp0": 0, "implen": max(n - 1, 0), "impL": L - 1}[kind]
        x[at] = 1.0
    elif kind == "alt":
        x = 0.5 * (1 - 2 * (t & 1))
    return x.astype(np.float32)


def inputs(case):
    """-> (x [B, L] float32, lens [B] int64).  Row i of two cases of equal L, hop and signal is the same row."""
    opts = _len_options(case.L, case.hop)
    rows, lens = [], []
    for i in range(case.B):
        if case.signal == "white":
            kind, n = "white", opts[i % 7]
        elif case.signal == "mix":
            kind, o = MIX_ROWS[i] if i < len(MIX_ROWS) else (KINDS[i % 12], i % 7)
            n = opts[o]
        else:
            s = NORM_SEQ[i % len(NORM_SEQ)]
            kind = "zero" if i % len(NORM_SEQ) == len(NORM_SEQ) - 1 else "white"
            n = case.L if s is None else (s * case.hop if s != 1 else case.hop - 60)
        rows.append(_row(kind, case.L, n, case.hop, i))
        lens.append(n)
    return np.stack(rows), np.asarray(lens, dtype=np.int64)


def one_hot_bank(j):
    """Bank j of five: filter m is bin 64 j + m alone (j < 4), or bin 256 - m (j = 4): between them every bin 0..256."""
    fb = np.zeros((NMELS, NBINS), np.float32)
    for m in range(NMELS):
        fb[m, 64 * j + m if j < 4 else 256 - m] = 1.0
    return fb


def boxcar_bank(span=MEL_TAPS):
    """64 filters of `span` consecutive equal weights from bin 4 m, cut off at bin 256."""
    fb = np.zeros((NMELS, NBINS), np.float32)
    for m in range(NMELS):
        fb[m, 4 * m:min(4 * m + span, NBINS)] = 1.0 / span
    return fb


def description(case, normalize="none", bank=None):
    """The library's front-end dict for a case (frontend_tables.frontend_description with the case's bank put in)."""
    from viet_asr_amd.frontend_tables import frontend_description
    bank = bank or case.bank
    lo, hi = (300, 3400) if bank == "slaney300" else (0, 8000)
    d = frontend_description(dict(sample_rate=16000, window_size=None, window_stride=None, n_window_size=case.win,
                                  n_window_stride=case.hop, n_fft=NFFT, window=case.window, features=NMELS, lowfreq=lo,
                                  highfreq=hi, preemph=case.preemph, log_zero_guard_type=case.guard_type,
                                  log_zero_guard_value=case.guard, normalize=None if normalize == "none" else normalize))
    if bank.startswith("onehot"):
        d["filterbank"] = one_hot_bank(int(bank[-1]))
    elif bank == "boxcar":
        d["filterbank"] = boxcar_bank()
    elif bank == "boxcar33":
        d["filterbank"] = boxcar_bank(MEL_TAPS + 1)
    elif bank == "zerorows":
        d["filterbank"] = d["filterbank"].copy()
        d["filterbank"][[5, 63]] = 0.0
    return d


def _cases():
    out = []
    # forms, on the shipped 320 / 160 front end
    out += [Case("form_a", 320, 160, 1, 2137), Case("form_b", 320, 160, 3, 2137), Case("form_c", 320, 160, 127, 700),
            Case("form_d", 320, 160, 128, 700), Case("form_e", 320, 160, 26, 160 * 133 + 57, norm=True),
            Case("form_e1", 320, 160, 1, 160 * 133 + 57)]
    # window and hop, each in both forms (the 32-frame form from the fewest short rows that reach the threshold)
    for win, hop in ((320, 160), (400, 160), (401, 160), (200, 80), (16, 3), (320, 320), (512, 512), (511, 237)):
        L8 = 301 if hop == 3 else hop * 13 + 57
        L32 = 301 if hop == 3 else hop * 4 + 57
        out.append(Case(f"wh_{win}_{hop}_f8", win, hop, 3, L8))
        out.append(Case(f"wh_{win}_{hop}_f32", win, hop, -(-128 // -(-(1 + L32 // hop) // 32)), L32))
    out.append(Case("wh_400_160_hamming_f8", 400, 160, 3, 2137, window="hamming"))
    out.append(Case("wh_400_160_hamming_f32", 400, 160, 128, 697, window="hamming"))
    # whole 32-frame workgroups above 64 KB of LDS: all 32 frame offsets of the staged segment
    out.append(Case("wh_511_237_full", 511, 237, 26, 237 * 133 + 57))
    out.append(Case("wh_512_512_full", 512, 512, 64, 512 * 33 + 57))
    # signals, lengths and mask
    out += [Case("mix_f8", 320, 160, 14, 2137, "mix", norm=True), Case("mix_f32", 320, 160, 128, 2137, "mix", norm=True),
            Case("mix_own_f8", 320, 160, 14, 2137, "mix", own=True), Case("mix_own_f32", 320, 160, 128, 2137, "mix", own=True),
            Case("mix_401_own_f8", 401, 160, 14, 2137, "mix", own=True)]
    # filterbanks
    out.append(Case("bank_slaney300", 320, 160, 3, 2137, bank="slaney300"))
    out += [Case(f"bank_onehot{j}", 320, 160, 3, 2137, bank=f"onehot{j}") for j in range(5)]
    out += [Case("bank_onehot0_f32", 320, 160, 128, 700, bank="onehot0"), Case("bank_onehot4_f32", 320, 160, 128, 700, bank="onehot4"),
            Case("bank_boxcar", 320, 160, 3, 2137, bank="boxcar"), Case("bank_boxcar_f32", 320, 160, 128, 700, bank="boxcar"),
            Case("bank_zerorows", 320, 160, 3, 2137, bank="zerorows")]
    # options
    out += [Case("opt_preemph0", 320, 160, 14, 2137, "mix", preemph=0.0), Case("opt_preemph_none", 320, 160, 14, 2137, "mix", preemph=None),
            Case("opt_clamp_1e5", 320, 160, 14, 2137, "mix", guard=1e-5, guard_type="clamp", norm=True),
            Case("opt_clamp_tiny", 320, 160, 14, 2137, "mix", guard=TINY32, guard_type="clamp")]
    # normalisation: 2, 255, 256, 257, T, 1 and 0 valid frames, and a constant row
    out.append(Case("norm_counts", 320, 160, 8, 160 * 260 + 57, "norm", norm=True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# pairs whose common rows (the first min(B) of each) must be bit-equal: the same rows in the other form, or in another batch
PAIRS = (("form_a", "form_b"), ("form_c", "form_d"), ("form_e1", "form_e"), ("mix_f8", "mix_f32"), ("mix_own_f8", "mix_own_f32"),
         ("opt_preemph0", "opt_preemph_none"))       # x - 0 x[n-1] is x: the coefficient 0 and no pre-emphasis, the same bits


# --------------------------------------------------------------------------------------------------------------- chain
def _pad_index(ns, L, left="reflect", right="reflect"):
    """Source sample of each position -256 .. L + 255 of a row that ends at ns, and whether there is one."""
    n = np.arange(-NFFT // 2, L + NFFT // 2)
    n = np.where(n < 0, -n - (left == "symmetric"), n)
    n = np.where(n >= ns, 2 * ns - 1 - n - (right == "reflect"), n)
    ok = (n >= 0) & (n < ns)
    return np.where(ok, n, 0), ok


def _drop_tap(fb, last):
    fb = fb.copy()
    for f in range(fb.shape[0]):
        nz = np.flatnonzero(fb[f])
        if nz.size:
            fb[f, nz[-1] if last else nz[0]] = 0.0
    return fb


def chain(x, lens, *, window, hop, fb, preemph, guard, clamp, own=False, dtype=np.float64, defect=None):
    """The raw log-mel of section 1 and what the bound of section 2 needs.  dtype float32: the same steps rounded to
    float32 after each (an honest float32 front end; numpy's FFT in place of the kernel's).  defect: one of DEFECTS.
    -> dict(raw [B, 64, T], seq [B], judged [B, T] bool, bound [B, 64, T])."""
    f = dtype
    x = np.asarray(x, np.float32)
    B, L = x.shape
    T = 1 + L // hop
    seq = seq_len(lens, hop)
    fb = np.asarray(fb, np.float32)
    win = np.asarray(window, np.float32)
    if defect == "tap_last" or defect == "tap_first":
        fb = _drop_tap(fb, defect == "tap_last")
    if defect == "guard_2e-23":
        guard = 2 * guard
    if defect == "clamp_for_add":
        clamp = not clamp
    if defect == "reflect_swapped":
        own = not own
    if defect == "win_periodic":
        win = periodic_window(win.size, "hamming" if win[0] > 0.01 else "hann")
    off = (NFFT - win.size) // 2 + (defect == "win_off")
    w512 = np.zeros(NFFT, f)
    w512[off:off + win.size] = win

    xs = x.astype(f)
    prev = np.concatenate([np.zeros((B, 1), f), xs[:, :-1]], axis=1)
    # y[0] against a literal zero is x[0], the right value; what a kernel without the n > 0 test reads is the sample in
    # front of the row in memory: the last one of the row before
    if defect == "y0_prev_row":
        prev[1:, 0] = xs[:-1, -1]
    p = f(np.float32(preemph)) if preemph is not None else f(0)
    pprev = (p * prev).astype(f)
    y = (xs - pprev).astype(f) if preemph is not None else xs
    left = "symmetric" if defect == "pad_sym_left" else "reflect"
    right = "symmetric" if defect == "pad_sym_right" else "reflect"
    yp, pp = np.zeros((B, L + NFFT), f), np.zeros((B, L + NFFT), f)
    for b in range(B):
        ns = min(int(lens[b]), L) if own else L
        idx, ok = _pad_index(ns, L, left, right)
        if defect == "preemph_after_pad" and preemph is not None:
            xp = np.where(ok, xs[b, idx], 0).astype(f)
            q = (p * np.concatenate([[0], xp[:-1]])).astype(f)
            yp[b], pp[b] = (xp - q).astype(f), q
        else:
            yp[b], pp[b] = np.where(ok, y[b, idx], 0), np.where(ok, pprev[b, idx], 0)
    at = (np.arange(T) * hop)[:, None] + np.arange(NFFT)[None, :]
    fr = (yp[:, at] * w512).astype(f)                               # [B, T, 512]
    X = np.fft.rfft(fr, axis=-1)
    if defect == "nyquist_zero":
        X[..., 256] = 0
    if defect == "dc_double":
        X[..., 0] *= 2
    P = (X.real.astype(f) ** 2 + X.imag.astype(f) ** 2).astype(f)
    fbf = fb.astype(f)
    acc = (P @ fbf.T).astype(f)                                     # [B, T, 64]
    g = f(guard)
    raw = np.log(np.maximum(acc, g)) if clamp else np.log((acc + g).astype(f))
    raw = np.transpose(raw.astype(f), (0, 2, 1)).astype(np.float64)
    t = np.arange(T)[None, :]
    judged = t < seq[:, None]
    keep = t < (seq[:, None] - 1) if defect == "mask_gt" else judged
    raw = np.where(keep[:, None, :], raw, 0.0)
    out = dict(raw=raw, seq=seq, judged=judged)
    if own:
        out["judged"] = judged & (np.asarray(lens)[:, None] > NFFT // 2)
    if dtype is np.float64 and defect is None:
        fr64, P64, acc64 = fr, P, acc
        E_t = (fr64 ** 2).sum(-1)
        E_p = ((pp[:, at] * w512) ** 2).sum(-1) if preemph is not None else 0.0
        dX = (U * (C_X * np.sqrt(E_t) + np.sqrt(E_p)))[..., None]
        dP = 2 * np.abs(X) * dX + dX ** 2 + A_P * U * P64
        fa = np.abs(fb).astype(np.float64)
        dacc = dP @ fa.T + B_ACC * U * (P64 @ fa.T)
        den = np.maximum(acc64, guard) if clamp else acc64 + guard
        r = dacc / den
        if clamp:
            r = np.where(acc64 + dacc < guard, 0.0, r)
        down = np.minimum(np.where(r < 1, -np.log1p(-np.minimum(r, 1 - 1e-16)), np.inf), np.log(den / guard))
        first = np.maximum(r, down)
        bound = np.transpose(first, (0, 2, 1)) + D_LOG * U * np.maximum(np.abs(raw), 1.0)
        out["bound"] = np.where(judged[:, None, :], bound, 0.0)
    return out


def periodic_window(n, name):
    """torch.hann_window / hamming_window(n, periodic=True): the window of n + 1 points without its last."""
    a = 0.5 if name == "hann" else 0.54
    return (a - (1 - a) * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def case_chain(case, x=None, lens=None, **kw):
    if x is None:
        x, lens = inputs(case)
    d = description(case)
    return chain(x, lens, window=d["window"], hop=case.hop, fb=d["filterbank"], preemph=case.preemph, guard=case.guard,
                 clamp=case.guard_type == "clamp", own=case.own, **kw)


# DEFECTS: name -> the cases it can occur in (test_frontend_host.py asserts that it leaves the bound on each of them)
def _mix(c):
    return c.signal == "mix"


def _ragged_reach(c):
    """Some judged frame reaches past its row's length where the window still has weight: the length k hop + 1 puts the
    centre of frame k on the row's last sample, and the length 257 (or 1) ends inside a frame of every window here.  Those
    are the fourth and later rows of a batch."""
    return c.B >= 5


DEFECTS = {
    "tap_last": lambda c: True,
    "tap_first": lambda c: True,
    "win_off": lambda c: c.win % 2 == 1,
    "win_periodic": lambda c: True,
    "pad_sym_right": lambda c: True,
    "pad_sym_left": lambda c: True,
    "reflect_swapped": _ragged_reach,
    "preemph_after_pad": lambda c: bool(c.preemph),
    "y0_prev_row": lambda c: bool(c.preemph) and c.B > 1,
    "guard_2e-23": lambda c: c.guard_type == "add" and (_mix(c) or c.bank == "zerorows"),
    "clamp_for_add": lambda c: c.guard_type == "add" and (_mix(c) or c.bank == "zerorows"),
    "nyquist_zero": lambda c: c.bank in ("onehot4", "boxcar"),
    "dc_double": lambda c: c.bank in ("onehot0", "boxcar"),
    "mask_gt": lambda c: True,
}
NORM_DEFECTS = ("std_biased", "eps_under_root", "all_padded")


# --------------------------------------------------------------------------------------------------------------- normalisation
def normalize(raw, seq, mode, defect=None, float32_sums=False):
    """Section 1's normalisation of a float32 raw log-mel [B, 64, T] in float64 -> (ref, bound); NaN where the reference's
    statistics are (one valid frame under per_feature), 0 at frames >= seq and in rows without a valid frame.
    float32_sums: the bound for statistics summed in float32, as torch's are on the CPU (the kernels sum in double): a
    pairwise sum of n values of one sign is off by up to ceil(log2 n) u of itself, in the mean and in the variance."""
    x = np.asarray(raw, np.float64)
    B, F, T = x.shape
    ref, bound = np.zeros_like(x), np.zeros_like(x)
    for b in range(B):
        n = int(min(max(seq[b], 0), T))
        if n == 0:
            continue
        v = x[b, :, :n]
        if mode == "per_feature":
            axis, cnt = 1, n
        else:
            axis, cnt = None, n * F
            if defect == "all_padded":
                axis, cnt, v = None, T * F, x[b]
        mu = v.mean(axis=axis, keepdims=True)
        dof = cnt if defect == "std_biased" else cnt - 1
        with np.errstate(invalid="ignore", divide="ignore"):
            var = ((v - mu) ** 2).sum(axis=axis, keepdims=True) / dof if dof > 0 else np.full_like(mu, np.nan)
            D = np.sqrt(var + EPS32) if defect == "eps_under_root" else np.sqrt(var) + EPS32
            r = (x[b, :, :n] - mu) / D
            ref[b, :, :n] = r
            k = math.ceil(math.log2(cnt)) if float32_sums else 0
            bound[b, :, :n] = 1.001 * (U * ((1 + k) * np.abs(mu) + np.abs(x[b, :, :n] - mu)) / D + (3 + k) * U * np.abs(r))
    return ref, bound


# --------------------------------------------------------------------------------------------------------------- judging
def judge(got, ref, bound, judged=None):
    """Every stored element (judged given: of the judged frames): |got - ref| <= bound where the reference is finite, NaN
    exactly where it is NaN.  -> (worst |got - ref| / bound, largest bound, list of failures)."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    fails = []
    nan_ref = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan_ref):
        fails.append(f"NaN pattern differs at {int((np.isnan(got) != nan_ref).sum())} elements")
    ok = ~nan_ref & ~np.isnan(got)
    if judged is not None:
        ok = ok & np.broadcast_to(judged[:, None, :], got.shape)
    err = np.where(ok, np.abs(got - ref), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err > 0, err / bound, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    if not worst <= 1.0:
        i = np.unravel_index(np.argmax(ratio), got.shape)
        fails.append(f"{int((ratio > 1).sum())} elements outside the bound; worst at {tuple(int(v) for v in i)}: got {got[i]!r} "
                     f"ref {ref[i]!r} bound {bound[i]:.3e}")
    return worst, (float(np.where(ok, bound, 0.0).max()) if ratio.size else 0.0), fails


def worst_element(got, ref, bound, judged):
    """(row, mel bin, frame) of the judged element with the largest |got - ref| / bound."""
    ok = np.broadcast_to(judged[:, None, :], np.shape(got)) & ~np.isnan(ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ok & (np.asarray(got, np.float64) != ref), np.abs(np.asarray(got, np.float64) - ref) / bound, 0.0)
    return tuple(int(v) for v in np.unravel_index(np.argmax(ratio), ratio.shape))
