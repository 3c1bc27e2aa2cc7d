"""What the CTC-loss tests and tests/golden/make_golden_ctc.py share: a float64 restatement of vasr_ctc_loss_f32
(include/vasr.h) -- the recursion and the library's conventions --, a float32 restatement in the kernel's order, and the
per-row bound on |loss32 - loss64|.

The entry point, per row, over T = clamp(frames, 0, Tmax) frames and L = clamp(tgt_len, 0, W) ids: the extended sequence e
has S = 2 L + 1 states (blank, y1, blank, ..., yL, blank);

    alpha(0, 0) = logp[0][blank], alpha(0, 1) = logp[0][y1], alpha(0, s) = -inf for s >= 2
    x0 = alpha(t-1, s), x1 = alpha(t-1, s-1), x2 = alpha(t-1, s-2) only where e_s != blank and e_s != e_(s-2)
    lse = m + log((exp(x0 - m) + exp(x1 - m)) + exp(x2 - m)),  m = max(x0, x1, x2);  -inf where m = -inf
    alpha(t, s) = lse + logp[t][e_s]
    loss = -lse(alpha(T-1, S-1), alpha(T-1, S-2))

a term that does not exist counts as -inf (it adds an exact zero).  Conventions: a negative length on either side -> NaN; an
id inside the row's length that is < 0, >= C or == blank -> NaN; T == 0 -> 0 for L == 0 and +inf otherwise; T < L -> +inf.
Nothing behind the lengths is read.

The bound.  log-sum-exp is a convex combination: d lse / d x_i = exp(x_i - lse) >= 0 and these sum to 1, so errors delta in
the three inputs move lse by at most max |delta| -- a frame's error ADDS to the previous frame's, it is never multiplied.
With u = 2^-24 (float32's unit roundoff; 1 ulp is at most 2 u relative) one frame adds, per state:

  * the subtractions x_i - m round to u |x_i - m|, a relative error of exp(x_i - m) of the same size; |d| exp(d) <= 1 / e
    and the sum is >= 1 (the largest term is exp(0) = 1 exactly), so the two smaller terms move the logarithm by < 0.74 u;
  * expf, budgeted at 2 ulps: a relative error of the sum of at most 4 u, an absolute error of its logarithm;
  * the two additions of the sum: 2 u, relative, again absolute in the logarithm;
  * logf, budgeted at 2 ulps of a result in [0, log 3]: 4 u (ulp(log 3) = 2^-23);
  * m + log(.) and (.) + logp[t][e_s]: u at their magnitudes, each at most A_t, the largest finite |lse| or |alpha(t, s)| of
    the frame over all states.

Frame 0 copies and rounds nothing; the final lse is one more step without the emission.  Hence, per row,

    |loss32 - loss64| <= u * sum over the frames t = 1 .. T-1 and the final step of (C0 + K * A_t),   C0 = 11, K = 2.

A_t is taken over ALL finite states of the frame, not only those on paths into the final states: larger, never smaller.  It
comes from the float64 run; the float32 run's own magnitudes differ from it in second order (bound * u).  Values that are
-inf by structure or because a log-prob is -inf are -inf in both runs and carry no error.  Derived from the order of the
code, not from its output.

``broken`` runs the float64 restatement with one rule broken (tests/test_ctc_host.py: the bound is not vacuous):
"skip_equal" allows alpha(s-2) across equal labels, "skip_blank" allows it out of a blank into a blank, "final_one" takes
the last state alone, "extra_frames" walks one frame past the row's length."""
import numpy as np

U = 2.0 ** -24
C0, K = 11.0, 2.0
BROKEN = ("skip_equal", "skip_blank", "final_one", "extra_frames")


def _lse3(x0, x1, x2, dtype):
    """the kernel's order, elementwise in ``dtype``: m by comparisons, then m + log((e0 + e1) + e2); -inf where m is -inf"""
    x0, x1, x2 = (np.asarray(x, dtype=dtype) for x in (x0, x1, x2))
    m = x0.copy()
    m = np.where(x1 > m, x1, m)
    m = np.where(x2 > m, x2, m)
    dead = np.isneginf(m)
    ms = np.where(dead, dtype(0), m).astype(dtype)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        s = (np.exp((x0 - ms).astype(dtype)) + np.exp((x1 - ms).astype(dtype))).astype(dtype)
        s = (s + np.exp((x2 - ms).astype(dtype))).astype(dtype)
        out = (ms + np.log(s).astype(dtype)).astype(dtype)
    return np.where(dead, dtype(-np.inf), out).astype(dtype)


def _row(logp, frames, tgt, tgt_len, blank, dtype, broken=None):
    """-> (loss, sum over the steps of (C0 + K * A_t)) of one row; logp [Tmax][C], tgt [W]"""
    logp = np.asarray(logp)
    tgt = np.asarray(tgt).astype(np.int64)
    Tmax, C = logp.shape
    frames, tgt_len = int(frames), int(tgt_len)
    if frames < 0 or tgt_len < 0:
        return dtype(np.nan), 0.0
    T, L = min(frames, Tmax), min(tgt_len, tgt.shape[0])
    if broken == "extra_frames":
        T = min(T + 1, Tmax)
    y = tgt[:L]
    if ((y < 0) | (y >= C) | (y == blank)).any():
        return dtype(np.nan), 0.0
    if T == 0:
        return dtype(0.0 if L == 0 else np.inf), 0.0
    if T < L:
        return dtype(np.inf), 0.0
    S = 2 * L + 1
    e = np.full(S, blank, dtype=np.int64)
    e[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (e[2:] != blank) & (e[2:] != e[:-2])
    if broken == "skip_equal":
        skip[2:] = e[2:] != blank
    elif broken == "skip_blank":
        skip[2:] |= e[2:] == blank
    x = logp[:T].astype(dtype)
    ninf = dtype(-np.inf)
    alpha = np.full(S, ninf, dtype=dtype)
    alpha[0] = x[0, blank]
    if S > 1:
        alpha[1] = x[0, e[1]]
    steps = 0.0

    def magnitude(*vs):
        a = 0.0
        for v in vs:
            v = np.asarray(v, dtype=np.float64)
            v = v[np.isfinite(v)]
            if v.size:
                a = max(a, float(np.abs(v).max()))
        return a

    for t in range(1, T):
        x1 = np.concatenate([[ninf], alpha[:-1]]).astype(dtype)
        x2 = np.where(skip, np.concatenate([[ninf, ninf], alpha[:-2]])[:S], ninf).astype(dtype)
        lse = _lse3(alpha, x1, x2, dtype)
        with np.errstate(invalid="ignore"):
            alpha = (lse + x[t, e]).astype(dtype)
        steps += C0 + K * magnitude(lse, alpha)
    last = alpha[S - 1]
    prev = alpha[S - 2] if (S > 1 and broken != "final_one") else ninf
    fin = _lse3(np.array([last]), np.array([prev]), np.array([ninf]), dtype)[0]
    steps += C0 + K * magnitude(fin)
    return dtype(-fin), steps


def loss64(logp, frames, tgt, tgt_len, blank, broken=None):
    """The float64 restatement of one row (``broken``: module docstring)."""
    return float(_row(logp, frames, tgt, tgt_len, blank, np.float64, broken)[0])


def loss32(logp, frames, tgt, tgt_len, blank):
    """The float32 restatement of one row, in the kernel's order (numpy's exp / log in place of expf / logf)."""
    return np.float32(_row(logp, frames, tgt, tgt_len, blank, np.float32)[0])


def loss_bound(logp, frames, tgt, tgt_len, blank):
    """The bound on |loss32 - loss64| of one row with a finite loss (module docstring); 0 for a row whose value is exact by
    definition (NaN, +inf, T == 0)."""
    return U * _row(logp, frames, tgt, tgt_len, blank, np.float64)[1]


def batch(logp, frames, tgt, tgt_len, blank):
    """logp [B][Tmax][C], frames [B], tgt [B][W], tgt_len [B] -> (loss64 [B], bound [B])"""
    out = [_row(logp[b], frames[b], tgt[b], tgt_len[b], blank, np.float64) for b in range(len(frames))]
    return np.array([float(o[0]) for o in out], dtype=np.float64), np.array([U * o[1] for o in out], dtype=np.float64)


def close(got, want64, bound):
    """got within bound of want64, with +inf and NaN matched exactly"""
    got, want64 = float(got), float(want64)
    if np.isnan(want64):
        return bool(np.isnan(got))
    if np.isinf(want64):
        return got == want64
    return bool(np.isfinite(got)) and abs(got - want64) <= bound


def min_frames(tgt, tgt_len):
    """L + the number of adjacent equal label pairs: the fewest frames with a path"""
    y = np.asarray(tgt)[: int(tgt_len)]
    return int(len(y) + (y[1:] == y[:-1]).sum())


def mean_bound(bounds, mean64):
    """Bound on |mean32 - mean64| of a float32 mean of float32 values within ``bounds`` of their float64 values: the mean of
    the bounds plus the roundings of the sum and the division (n + 1 at most, whatever the order of the sum) at the
    magnitude of the mean (all values are >= 0 up to their bounds, so no partial sum exceeds the total)."""
    n = len(bounds)
    return float(np.mean(bounds)) + U * (n + 1) * abs(float(mean64))
