"""What the forced-alignment tests share: a float64 restatement of vasr_ctc_align_f32 (include/vasr.h) -- the recursion, the
tie-break and the library's conventions --, a float32 restatement in the kernel's order, a validator of paths and spans, the
float64 score of a given path, brute-force enumeration for tiny rows, and the bound on |score32 - score64|.

The entry point, per row, over T = clamp(frames, 0, Tmax) frames and L = clamp(tgt_len, 0, W) ids: the extended sequence e
has S = 2 L + 1 states (blank, y1, blank, ..., yL, blank);

    delta(0, 0) = logp[0][blank], delta(0, 1) = logp[0][y1], delta(0, s) = -inf for s >= 2
    x0 = delta(t-1, s), x1 = delta(t-1, s-1), x2 = delta(t-1, s-2) only where e_s != blank and e_s != e_(s-2)
    best = x0, bp = 0;  if x1 > best: best = x1, bp = 1;  if x2 > best: best = x2, bp = 2
    delta(t, s) = best + logp[t][e_s]
    final state S-1 unless delta(T-1, S-2) > delta(T-1, S-1); score = that delta; the path follows bp back to frame 0

Conventions: a negative length on either side -> NaN score; an id inside the row's length that is < 0, >= C or == blank ->
NaN; T == 0 -> 0 for L == 0 and -inf otherwise; a score of -inf -> no path.  Token j holds the frames [start, end) whose
state is 2 j + 1; token_logp is the sum of logp[t][y_j] over them, ascending, starting from the first term.  Unfilled entries
(j >= L, t >= T, rows without a path or with a NaN score) are -1 and 0.0.  Nothing behind the lengths is read.

The float32 restatement.  The recursion has only comparisons and additions of float32 values, each rounded to nearest even:
numpy's float32 `+` and `>` are those IEEE operations, and so are the device's v_add_f32 and v_cmp_gt_f32 on normal numbers
(the generators of the tests keep subnormals out).  There is no multiply that could be fused and no library function.  The
same recursion in the same order therefore gives the same BITS: score, back-pointers, path, spans, token sums.

The bound on |score32 - score64|.  Write d(t) = max over s of |delta32(t, s) - delta64(t, s)| over the states that are finite
(a state is -inf in both runs or in neither: -inf comes from structure or from a -inf log-prob, never from rounding).
Frame 0 copies log-probs: d(0) = 0.  max is 1-Lipschitz in the sup norm: |max(a) - max(b)| <= max |a_i - b_i|, whichever
candidates win in the two runs, so `best` differs by at most d(t-1).  The one addition of frame t rounds once: the float32
result is (best + p)(1 + r), |r| <= u = 2^-24, an absolute error of at most u |delta(t, s)| <= u A_t, where A_t is the
largest finite |delta(t, .)|.  (The float64 run rounds at 2^-53: nothing next to u.)  Hence d(t) <= d(t-1) + u A_t and

    |score32 - score64| <= d(T-1) <= u * sum over t = 1 .. T-1 of A_t.

The choice between the two final states is a max too and adds nothing.  A_t is taken from the float64 run over ALL finite
states of the frame; the float32 run's own magnitudes differ from it in second order (bound * u).  Derived from the order of
the code, not from its output.  The two runs may pick DIFFERENT paths where two candidates lie within the bound of each
other; each path's own float64 score is then within 2 * bound of the float64 optimum (path_score64).

``broken`` runs a restatement with one rule broken (tests/test_ctc_align_host.py: the checks are not vacuous): "skip_equal"
allows delta(s-2) across equal labels, "skip_blank" allows it out of a blank into a blank, "final_one" takes the last state
alone, "tie_reversed" lets a later candidate win a tie."""
import itertools

import numpy as np

U = 2.0 ** -24
BROKEN = ("skip_equal", "skip_blank", "final_one", "tie_reversed")


def _clamped(logp, frames, tgt, tgt_len):
    return min(int(frames), logp.shape[0]), min(int(tgt_len), tgt.shape[0])


def _unfilled(score, Tmax, W, dtype):
    return dict(score=dtype(score), path=np.full(Tmax, -1, np.int32), start=np.full(W, -1, np.int32),
                end=np.full(W, -1, np.int32), token_logp=np.zeros(W, dtype), magnitudes=0.0)


def spans_of(path, L, W):
    """(start [W], end [W]) of the token states along a path of states; -1 for a token the path never visits"""
    start, end = np.full(W, -1, np.int32), np.full(W, -1, np.int32)
    for t, s in enumerate(path):
        if s & 1:
            j = int(s) >> 1
            if start[j] < 0:
                start[j] = t
            end[j] = t + 1
    assert (start[L:] == -1).all()
    return start, end


def _row(logp, frames, tgt, tgt_len, blank, dtype, broken=None):
    logp = np.asarray(logp)
    tgt = np.asarray(tgt).astype(np.int64)
    Tmax, C = logp.shape
    W = tgt.shape[0]
    if int(frames) < 0 or int(tgt_len) < 0:
        return _unfilled(np.nan, Tmax, W, dtype)
    T, L = _clamped(logp, frames, tgt, tgt_len)
    y = tgt[:L]
    if ((y < 0) | (y >= C) | (y == blank)).any():
        return _unfilled(np.nan, Tmax, W, dtype)
    if T == 0:
        return _unfilled(0.0 if L == 0 else -np.inf, Tmax, W, dtype)
    S = 2 * L + 1
    e = np.full(S, blank, dtype=np.int64)
    e[1::2] = y
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (e[2:] != blank) & (e[2:] != e[:-2])
    if broken == "skip_equal":
        skip[2:] = e[2:] != blank
    elif broken == "skip_blank":
        skip[2:] |= e[2:] == blank
    wins = (lambda a, b: a >= b) if broken == "tie_reversed" else (lambda a, b: a > b)
    x = logp[:T].astype(dtype)
    ninf = dtype(-np.inf)
    delta = np.full(S, ninf, dtype=dtype)
    delta[0] = x[0, blank]
    if S > 1:
        delta[1] = x[0, e[1]]
    bps = np.zeros((T, S), dtype=np.uint8)
    mags = 0.0
    for t in range(1, T):
        x1 = np.concatenate([[ninf], delta[:-1]]).astype(dtype)
        x2 = np.where(skip, np.concatenate([[ninf, ninf], delta[:-2]])[:S], ninf).astype(dtype)
        best, bp = delta.copy(), np.zeros(S, dtype=np.uint8)
        m = wins(x1, best)
        best, bp = np.where(m, x1, best), np.where(m, 1, bp)
        m = wins(x2, best)
        best, bp = np.where(m, x2, best), np.where(m, 2, bp)
        delta = (best.astype(dtype) + x[t, e]).astype(dtype)
        bps[t] = bp
        fin = np.abs(delta[np.isfinite(delta)].astype(np.float64))
        mags += float(fin.max()) if fin.size else 0.0
    s = S - 1
    if S > 1 and broken != "final_one" and wins(delta[S - 2], delta[S - 1]):
        s = S - 2
    score = delta[s]
    if np.isneginf(score):
        return _unfilled(-np.inf, Tmax, W, dtype)
    path = np.full(Tmax, -1, np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s -= int(bps[t, s])
    start, end = spans_of(path[:T], L, W)
    tok = np.zeros(W, dtype)
    for j in range(L):
        if start[j] >= 0:
            acc = x[start[j], y[j]]
            for t in range(start[j] + 1, end[j]):
                acc = dtype(acc + x[t, y[j]])
            tok[j] = acc
    return dict(score=dtype(score), path=path, start=start, end=end, token_logp=tok, magnitudes=mags)


def align64(logp, frames, tgt, tgt_len, blank, broken=None):
    """The float64 restatement of one row -> dict(score, path [Tmax], start [W], end [W], token_logp [W], magnitudes)."""
    return _row(logp, frames, tgt, tgt_len, blank, np.float64, broken)


def align32(logp, frames, tgt, tgt_len, blank, broken=None):
    """The float32 restatement of one row, in the kernel's order: what the device has to return bit for bit."""
    return _row(logp, frames, tgt, tgt_len, blank, np.float32, broken)


def bound(row64):
    """The bound on |score32 - score64| of a row from its float64 run (module docstring); 0 for a row whose value is exact by
    definition (NaN, -inf, T == 0)."""
    return U * row64["magnitudes"]


def close(got, want64, bnd):
    """got within bnd of want64, with -inf and NaN matched exactly"""
    got, want64 = float(got), float(want64)
    if np.isnan(want64):
        return bool(np.isnan(got))
    if np.isinf(want64):
        return got == want64
    return bool(np.isfinite(got)) and abs(got - want64) <= bnd


def validate(path, start, end, frames, tgt, tgt_len, Tmax=None):
    """Raises AssertionError unless path [>= T] is a valid CTC path of tgt[:L] over T frames -- it starts in state 0 or 1, ends
    in S-1 or S-2, steps by 0 or 1, or by 2 only into a token state whose label differs from the token before it -- and
    start / end are the spans of its token states, every token with end > start, unfilled (-1) behind L and behind T."""
    path, tgt = np.asarray(path), np.asarray(tgt)
    T, L = min(int(frames), len(path) if Tmax is None else Tmax), min(int(tgt_len), tgt.shape[0])
    S = 2 * L + 1
    p = path[:T]
    assert T >= 1 and (path[T:] == -1).all(), "entries behind the row's frames must be -1"
    assert p[0] in (0, 1) and p[0] < S, f"starts in state {p[0]}"
    assert p[-1] in (S - 1, S - 2) and p[-1] >= 0, f"ends in state {p[-1]} of {S}"
    step = np.diff(p)
    assert ((step >= 0) & (step <= 2)).all(), "steps by other than 0, 1, 2"
    for t in np.nonzero(step == 2)[0]:
        s = int(p[t + 1])
        assert s & 1, f"frame {t + 1}: a skip into the blank state {s}"
        assert tgt[s >> 1] != tgt[(s >> 1) - 1], f"frame {t + 1}: a skip between equal labels into state {s}"
    want_start, want_end = spans_of(p, L, tgt.shape[0])
    assert (np.asarray(start) == want_start).all() and (np.asarray(end) == want_end).all(), "spans differ from the path's"
    assert (want_end[:L] > want_start[:L]).all() and (want_start[:L] >= 0).all(), "a token without a frame"
    assert (want_start[1:L] >= want_end[: L - 1]).all() if L > 1 else True, "tokens out of order"


def path_score64(logp, path, frames, tgt, blank):
    """The float64 sum, frame by frame, of the log-probs along a path of states."""
    logp, tgt = np.asarray(logp), np.asarray(tgt)
    T = min(int(frames), logp.shape[0])
    total = 0.0
    for t in range(T):
        s = int(path[t])
        x = float(logp[t, tgt[s >> 1] if s & 1 else blank])
        total = total + x if t else x
    return total


def brute_force(logp, T, y, blank):
    """Every valid path of the ids y over the first T frames, enumerated -> (best score, the best path under the recursion's
    tie-break) or (-inf, None).  The scores are summed frame by frame in float64, as the recursion sums them.  The tie-break:
    the final state is the larger one unless the smaller is strictly better, and every back-pointer prefers the larger
    predecessor -- the best path that is LARGEST when read from the last frame backwards.  (Meant for log-probs whose sums
    are exact, such as small multiples of 1/8: a tie is then a tie in every order of summation.)"""
    logp = np.asarray(logp, dtype=np.float64)
    L = len(y)
    S = 2 * L + 1
    e = [blank if s % 2 == 0 else int(y[s >> 1]) for s in range(S)]
    best, best_path = -np.inf, None

    def paths(prefix):
        if len(prefix) == T:
            if prefix[-1] >= S - 2:
                yield tuple(prefix)
            return
        a = prefix[-1]
        for b in range(a, min(a + 2, S - 1) + 1):
            if b - a == 2 and (b % 2 == 0 or e[b] == e[a]):
                continue
            yield from paths(prefix + [b])

    for path in itertools.chain.from_iterable(paths([s0]) for s0 in range(min(2, S))):
        total = logp[0, e[path[0]]]
        for t in range(1, T):
            total = total + logp[t, e[path[t]]]
        if np.isneginf(total):
            continue
        if total > best or (total == best and path[::-1] > best_path[::-1]):
            best, best_path = total, path
    return float(best), (None if best_path is None else np.array(best_path, dtype=np.int32))


def min_frames(tgt, tgt_len):
    """L + the number of adjacent equal label pairs: the fewest frames with a path"""
    y = np.asarray(tgt)[: int(tgt_len)]
    return int(len(y) + (y[1:] == y[:-1]).sum())
