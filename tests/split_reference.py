"""What the split-at-silences tests share: the float64 restatement of vasr_split_silence_f32 / _pcm16 (include/vasr.h), a
second, literal transcription of ``librosa.effects.split``'s published form, the decidability conditions and the case table.

The restatement, per row x of n samples (frame_length, hop_length, top_db as for the trim, m = min_silence_frames >= 1,
M = max_segment_frames, 0 = no limit or >= 2), written independently of the kernel's order:

    A. flags   non-silent frames from ``trim_reference.frame_energies`` in the log form librosa writes:
               10 log10(max(amin, mse)) - 10 log10(max(amin, max mse)) > -top_db; n == 0: no frame, no segment
    B. runs    maximal stretches that start and end on a non-silent frame and hold no m or more consecutive silent frames
    C. cuts    a run [s, e) with e - s > M is cut at the frame of the smallest float64 frame sum among s + ceil(M / 2) .. s + M,
               the lowest index among equals; [s, c) is a segment, the rule goes on with [c, e)
    D. bounds  frames [f0, f1) -> samples [min(n, f0 hop), min(n, f1 hop))

With (m, M) = (1, 0) this is ``librosa.effects.split(y, top_db, ref=np.max, frame_length, hop_length)`` of librosa < 0.10
(third-party arithmetic restated from its published form, parity unpinned: librosa is not available to the tests).

Decidability.  Flags: the trim's band (``trim_reference.band``).  Cuts: a float64 sum of at most 2 048 float32 squares, in any
order, is accurate to 2^-42 relative, so a cut is DECIDABLE when the window's smallest frame sum is below the second smallest by
more than 2^-40 relative -- or when the row's sums are exact in any order (``sums_exact``: int16 rows, all-zero rows, rows of
+-2^-20), where equal sums are equal bits and the lowest index wins on every side.  tests/test_split_host.py asserts both for
every case, both dtypes and every (m, M) below; no case is left out.

A note on the below-amin rows: a row whose loudest frame is below amin has every frame non-silent, but its cuts still follow
the frame SUMS (rule C), which differ from frame to frame for a noise row.  Every cut is a tie, and falls at s + ceil(M / 2),
where the sums are equal: the all-zero rows and the ``below_amin_flat`` family (+-2^-20: every frame sum is frame_length * 2^-40
exactly, mse 9.1e-13 < amin).
"""
import functools

import numpy as np

import trim_reference as T

AMIN = T.AMIN
FORMS = T.FORMS
PAIRS = ((1, 0), (8, 0), (1, 40), (8, 40), (3, 7), (1, 2))       # (min_silence_frames, max_segment_frames)
DTYPES = T.DTYPES
CUT_MARGIN = 2.0 ** -40


# ---- the restatement --------------------------------------------------------------------------------------------------
def frame_flags(x, top_db=60.0, frame_length=2048, hop_length=512):
    """-> (non-silent [F] bool, frame sums [F] float64); empty for n == 0"""
    mse = T.frame_energies(x, frame_length, hop_length)
    if mse.size == 0:
        return np.zeros(0, bool), np.zeros(0, np.float64)
    db = 10.0 * np.log10(np.maximum(AMIN, mse)) - 10.0 * np.log10(max(AMIN, mse.max()))
    y = np.pad(T.as_float64(x), frame_length // 2, mode="reflect")
    frames = np.lib.stride_tricks.sliding_window_view(y, frame_length)[::hop_length][: mse.size]
    return db > -top_db, np.sum(frames ** 2, axis=1)


def bridged_runs(flags, m):
    """[(s, e)] in frames: rule B in plain Python"""
    runs, start, last = [], None, None
    for f, on in enumerate(flags):
        if not on:
            continue
        if start is None:
            start = f
        elif f - last - 1 >= m:                         # m or more silent frames since the last non-silent one
            runs.append((start, last + 1))
            start = f
        last = f
    if start is not None:
        runs.append((start, last + 1))
    return runs


def cut_run(s, e, sums, M):
    """rule C on one run -> ([(s, e)] pieces, [(window sums, chosen offset)] one per cut)"""
    pieces, windows = [], []
    while M > 0 and e - s > M:
        lo = s + (M + 1) // 2
        w = sums[lo : s + M + 1]
        c = lo + int(np.argmin(w))                      # np.argmin: the first of equal minima
        windows.append((w, c - lo))
        pieces.append((s, c))
        s = c
    pieces.append((s, e))
    return pieces, windows


def split_frames(x, top_db, frame_length, hop_length, m, M):
    """-> (segments [(f0, f1)] in frames, runs, windows of every cut, flags)"""
    flags, sums = frame_flags(x, top_db, frame_length, hop_length)
    runs = bridged_runs(flags, m)
    segs, windows = [], []
    for s, e in runs:
        p, w = cut_run(s, e, sums, M)
        segs += p
        windows += w
    return segs, runs, windows, flags


def split(x, top_db=60.0, frame_length=2048, hop_length=512, m=1, M=0):
    """-> [(start, end)] in samples: the restatement of vasr_split_silence_*"""
    n = int(np.asarray(x).shape[0])
    segs = split_frames(x, top_db, frame_length, hop_length, m, M)[0]
    return [(min(n, f0 * hop_length), min(n, f1 * hop_length)) for f0, f1 in segs]


def librosa_split(x, top_db=60.0, frame_length=2048, hop_length=512):
    """``librosa.effects.split`` as published (librosa < 0.10), line by line: np.diff of the flags, the two outer edges,
    frames_to_samples, np.minimum, reshape.  n == 0 (librosa raises there): no interval."""
    non_silent = frame_flags(x, top_db, frame_length, hop_length)[0]
    if non_silent.size == 0:
        return []
    edges = np.flatnonzero(np.diff(non_silent.astype(int)))
    edges = [edges + 1]
    if non_silent[0]:
        edges.insert(0, [0])
    if non_silent[-1]:
        edges.append([len(non_silent)])
    edges = np.concatenate(edges).astype(np.int64) * hop_length          # frames_to_samples, n_fft=None
    edges = np.minimum(edges, np.asarray(x).shape[-1])
    return [(int(a), int(b)) for a, b in edges.reshape((-1, 2))]


def sums_exact(x, max_sum):
    """True where every frame sum of the row (the largest is max_sum) is exact in float64 in ANY order: the squares are whole
    multiples of one power of two q -- the lowest set bit among them -- and max_sum stays below 2^53 q, so that every partial
    sum of non-negative terms is a whole multiple of q that float64 holds exactly."""
    sq = T.as_float64(x) ** 2
    sq = sq[sq > 0]
    if sq.size == 0:
        return True
    mant, exp = np.frexp(sq)                            # sq = mant * 2^exp, mant in [0.5, 1): 53 bits
    bits = (mant * 2.0 ** 53).astype(np.int64)
    low = np.log2((bits & -bits).astype(np.float64)).astype(np.int64) + exp.astype(np.int64) - 53
    return bool(max_sum < 2.0 ** (53 + int(low.min())))


def cut_margin(window):
    """relative distance of the smallest sum of a cut window from the second smallest (0 for a tie)"""
    w = np.sort(window)
    return float((w[1] - w[0]) / w[1]) if w[1] > 0 else 0.0


# ---- the case table -----------------------------------------------------------------------------------------------------
SILENCE, SPEECH, DIP = T.SILENCE, T.SPEECH, 0.01      # the dip is 20 dB below speech: quieter, still non-silent at 60 dB


def _noise(n, amp, seed):
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


def make_signal(family, n, frame_length, hop, seed):
    R = frame_length // hop
    if family in T.NOISE_FAMILIES or family in ("click_first", "click_last"):
        return T.make_signal(family, n, hop, seed)
    amp = np.full(n, SILENCE, np.float64)
    if family == "pauses":
        # bursts of 2 hops separated by pauses of (R - 1 + g) hops, g = 1 .. 10 and again: the frames that lie wholly inside
        # a pause are silent, g or g - 1 of them, so the gaps straddle every m - 1, m, m + 1 of the pairs
        at, g = 3 * hop, 0
        while at + 2 * hop <= n:
            amp[at : at + 2 * hop] = SPEECH
            at += 2 * hop + (R - 1 + 1 + g % 10) * hop
            g += 1
    elif family == "many":
        # a burst of half a hop every R + 2 hops: more than 256 runs in a row of 300 periods
        for at in range(hop, n - hop, (R + 2) * hop):
            amp[at : at + hop // 2] = SPEECH
    elif family == "dips":
        amp[:] = SPEECH
        for at in range(11 * hop, n, 23 * hop):         # three quieter frames every 23: the cuts land there
            amp[at : at + 3 * hop] = DIP
    elif family == "last_burst":                        # n a multiple of hop, speech in the last half hop only
        amp[n - hop // 2 :] = SPEECH
    elif family == "below_amin_flat":
        sign = np.random.default_rng(seed).integers(0, 2, n) * 2 - 1
        return (sign * 2.0 ** -20).astype(np.float32)
    else:
        raise KeyError(family)
    return (np.random.default_rng(seed).standard_normal(n) * amp).astype(np.float32)


LENGTHS = {(2048, 512): (1, 511, 512, 513, 2049, 18000), (64, 16): (0, 1, 15, 16, 17, 65, 1000),
           (256, 256): (0, 1, 255, 256, 257, 2560, 5000)}
BIG = {(2048, 512): 600 * 512, (64, 16): 1500 * 16, (256, 256): 900 * 256}     # rows of more than 256 frames


def _table():
    """[(name, family, n, frame_length, hop_length, top_db, seed)]"""
    rows = []
    for (fl, hop) in FORMS:
        R = fl // hop
        for fam in T.NOISE_FAMILIES:
            for n in LENGTHS[(fl, hop)]:
                rows.append((fam, n, fl, hop, 60.0))
        rows.append(("pauses", 160 * hop, fl, hop, 60.0))
        rows.append(("pauses", 160 * hop + hop // 2 + 1, fl, hop, 60.0))
        rows.append(("dips", 120 * hop + 7, fl, hop, 60.0))
        rows.append(("dips", BIG[(fl, hop)], fl, hop, 60.0))             # > 256 frames; > 256 segments under M = 2
        if (fl, hop) != (2048, 512):
            rows.append(("many", 300 * (R + 2) * hop, fl, hop, 60.0))    # > 256 runs as they are
        for fam in ("zeros", "below_amin_flat", "below_amin"):
            rows.append((fam, 100 * hop + 5, fl, hop, 60.0))             # longer than M = 40 frames
        for fam in ("click_last", "last_burst", "click_first"):
            rows.append((fam, 32 * hop, fl, hop, 60.0))
        for n in (hop - 1, hop, hop + 1):
            rows.append(("no_silence", n, fl, hop, 60.0))
        rows.append(("pauses", 160 * hop, fl, hop, 20.0))
    seen, out = set(), []
    for i, (fam, n, fl, hop, top_db) in enumerate(rows):
        name = f"{fam}-n{n}-f{fl}h{hop}-db{top_db:g}"
        if name not in seen:
            seen.add(name)
            out.append((name, fam, n, fl, hop, top_db, 2000 + i))
    return out


TABLE = _table()
LONG = 100000                                           # rows beyond this many samples are launched apart


@functools.lru_cache(maxsize=None)
def case(index, dtype):
    """-> dict(name, x, n, frame_length, hop_length, top_db) of table row `index` as float32 or int16; computed once, shared,
    read-only"""
    name, fam, n, fl, hop, top_db, seed = TABLE[index]
    x = make_signal(fam, n, fl, hop, seed)
    if dtype == "int16":
        x = T.to_int16(x)
    x.setflags(write=False)
    return dict(name=name, family=fam, x=x, n=n, frame_length=fl, hop_length=hop, top_db=top_db)


@functools.lru_cache(maxsize=None)
def expected(index, dtype, m, M):
    """-> the restatement's [(start, end)] of a case under (m, M); computed once, shared"""
    c = case(index, dtype)
    return tuple(split(c["x"], c["top_db"], c["frame_length"], c["hop_length"], m, M))


def groups():
    """The table's rows grouped by what one launch shares: {(frame_length, hop_length, top_db, long): [index]}; the long rows
    apart (with two short neighbours) so that no batch is padded to their width."""
    out = {}
    for i, (_, _, n, fl, hop, top_db, _) in enumerate(TABLE):
        out.setdefault((fl, hop, top_db, n > LONG), []).append(i)
    for key in [k for k in out if k[3]]:
        fl, hop, top_db, _ = key
        out[key] += out[(fl, hop, top_db, False)][:2]
    return out
