"""What the silence-trim tests share: the float64 restatement of vasr_trim_silence_f32 / _pcm16 (include/vasr.h), the
decidability band and the case table.

The restatement is librosa < 0.10's ``librosa.effects.trim(y, top_db, ref=np.max, frame_length, hop_length)`` -- the call of
``AudioSegment(trim=True)`` (parts/segment.py:19-32) -- written from its published form (third-party arithmetic, parity
unpinned: librosa is not available to the tests).  For a row x of n samples:

    y      = np.pad(x, frame_length // 2, mode="reflect")            (n == 0: no frame energy at all, start = end = 0)
    F      = 1 + n // hop_length frames, frame f = y[f hop : f hop + frame_length], mse[f] = mean(frame ** 2)
    ref    = max mse, amin = 1e-10
    frame f is non-silent iff 10 log10(max(amin, mse[f])) - 10 log10(max(amin, ref)) > -top_db
    start  = first * hop, end = min(n, (last + 1) * hop) over the non-silent frames; 0, 0 when there is none

int16 rows are scaled by 2^-15 first (AudioSegment._convert_samples_to_float32).

The decidability band.  The device may decide in the product form max(amin, mse) > max(amin, ref) * 10^(-top_db / 10), and
may sum in float32 in any order.  A sum of frame_length non-negative float32 terms in any order has a relative error of at most
frame_length * 2^-24 (first order); the comparison involves two such sums (the frame's and the loudest frame's), the squares,
the division by frame_length and the product with the factor each round once more: (2 * frame_length + 16) * 2^-24 covers
them.  A frame is DECIDABLE when its ratio max(amin, mse) / (max(amin, ref) * 10^(-top_db / 10)) is farther from 1 than that:
then every such evaluation, and the log form, give the answer of the float64 restatement.  The figure is derived from the
number formats, not measured.  tests/test_trim_host.py asserts that every frame of every case of the table is decidable.
"""
import functools

import numpy as np

AMIN = 1e-10
FORMS = ((2048, 512), (64, 16), (256, 256))      # (frame_length, hop_length): librosa's, a small one, one frame = one hop


def mirror_index(i, n):
    """numpy's `reflect` as a formula: periodic mirroring with period 2 (n - 1), the edge sample not repeated; n >= 1."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    m = np.mod(i, period)
    return np.where(m < n, m, period - m)


def as_float64(x):
    """A row as the energies see it: int16 scaled by 2^-15 (exact), float32 as it is."""
    x = np.asarray(x)
    return x.astype(np.float64) * 2.0 ** -15 if x.dtype == np.int16 else x.astype(np.float64)


def frame_energies(x, frame_length=2048, hop_length=512):
    """mse [F] in float64 of a row (float32 or int16); F = 1 + n // hop; empty for n == 0."""
    x = as_float64(x)
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, np.float64)
    y = np.pad(x, frame_length // 2, mode="reflect")
    F = 1 + n // hop_length
    frames = np.lib.stride_tricks.sliding_window_view(y, frame_length)[::hop_length][:F]
    assert frames.shape[0] == F
    return np.mean(frames ** 2, axis=1)


def threshold_ratios(mse, top_db):
    """max(amin, mse) / (max(amin, ref) * 10^(-top_db / 10)) per frame: > 1 is non-silent in the product form."""
    ref = mse.max()
    return np.maximum(AMIN, mse) / (max(AMIN, ref) * 10.0 ** (-top_db / 10.0))


def band(frame_length):
    return (2 * frame_length + 16) * 2.0 ** -24


def trim_bounds(x, top_db=60.0, frame_length=2048, hop_length=512):
    """-> (start, end) of the float64 restatement (the log form, as librosa writes it)."""
    n = int(np.asarray(x).shape[0])
    mse = frame_energies(x, frame_length, hop_length)
    if mse.size == 0:
        return 0, 0
    db = 10.0 * np.log10(np.maximum(AMIN, mse)) - 10.0 * np.log10(max(AMIN, mse.max()))
    nz = np.flatnonzero(db > -top_db)
    if nz.size == 0:
        return 0, 0
    return int(nz[0]) * hop_length, min(n, (int(nz[-1]) + 1) * hop_length)


def trim(x, top_db=60.0, frame_length=2048, hop_length=512):
    """-> (x[start:end], start): what the host would hand the front end."""
    s, e = trim_bounds(x, top_db, frame_length, hop_length)
    return np.asarray(x)[s:e], s


# ---- the case table -------------------------------------------------------------------------------------------------
SILENCE, SPEECH = 1e-5, 0.1


def _levels(n, edges, amps, seed):
    """seeded Gaussian noise of n samples with piecewise-constant amplitude: amps[k] on [edges[k], edges[k + 1])"""
    g = np.random.default_rng(seed).standard_normal(n)
    a = np.zeros(n, np.float64)
    for k, amp in enumerate(amps):
        a[edges[k]:edges[k + 1]] = amp
    return (g * a).astype(np.float32)


def _click(n, at):
    x = np.zeros(n, np.float32)
    x[at] = 0.9
    return x


def make_signal(family, n, hop, seed):
    """float32 row of a family; the segment edges are fractions of n, for `hop_aligned` multiples of hop"""
    if family == "sil_speech_sil":
        return _levels(n, [0, (3 * n) // 10, (7 * n) // 10, n], [SILENCE, SPEECH, SILENCE], seed)
    if family == "no_silence":
        return _levels(n, [0, n], [SPEECH], seed)
    if family == "zeros":
        return np.zeros(n, np.float32)
    if family == "below_amin":
        return _levels(n, [0, n], [1e-6], seed)
    if family == "below_amin_steps":
        return _levels(n, [0, n // 3, (2 * n) // 3, n], [1e-7, 3e-6, 1e-7], seed)
    if family == "inner_gap":
        return _levels(n, [0, n // 4, n // 2, (3 * n) // 4, n], [SPEECH, SILENCE, SPEECH, SILENCE], seed)
    if family == "hop_aligned":
        f = n // hop
        return _levels(n, [0, (f // 3) * hop, ((2 * f) // 3) * hop, n], [SILENCE, SPEECH, SILENCE], seed)
    if family == "click_first":
        return _click(n, 0)
    if family == "click_last":
        return _click(n, n - 1)
    raise KeyError(family)


def to_int16(x):
    return np.clip(np.round(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


NOISE_FAMILIES = ("sil_speech_sil", "no_silence", "zeros", "below_amin", "below_amin_steps", "inner_gap", "hop_aligned")
SMALL_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 1000)
LARGE_LENGTHS = (1, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 18000)
LONG_ROW = 600000                                      # more than 1024 frames at hop 512


def _table():
    """[(name, family, n, frame_length, hop_length, top_db, seed)]"""
    rows = []
    for (fl, hop), lengths in (((2048, 512), LARGE_LENGTHS), ((64, 16), SMALL_LENGTHS)):
        for fam in NOISE_FAMILIES:
            for n in lengths:
                rows.append((fam, n, fl, hop, 60.0))
        for fam in ("click_first", "click_last"):
            rows.append((fam, 8192, fl, hop, 60.0))
        rows.append(("sil_speech_sil", LONG_ROW, fl, hop, 60.0))
        rows.append(("sil_speech_sil", lengths[-1], fl, hop, 20.0))
        rows.append(("sil_speech_sil", lengths[-1], fl, hop, -1.0))
    for fam, n in (("sil_speech_sil", 5000), ("inner_gap", 255), ("hop_aligned", 2560), ("click_last", 8192)):
        rows.append((fam, n, 256, 256, 60.0))
    return [(f"{fam}-n{n}-f{fl}h{hop}-db{top_db:g}", fam, n, fl, hop, top_db, 1000 + i)
            for i, (fam, n, fl, hop, top_db) in enumerate(rows)]


TABLE = _table()
DTYPES = ("float32", "int16")


@functools.lru_cache(maxsize=None)
def case(index, dtype):
    """-> dict(x, n, frame_length, hop_length, top_db, mse, start, end) of table row `index` as float32 or int16; computed
    once, shared, read-only."""
    name, fam, n, fl, hop, top_db, seed = TABLE[index]
    x = make_signal(fam, n, hop, seed)
    if dtype == "int16":
        x = to_int16(x)
    x.setflags(write=False)
    mse = frame_energies(x, fl, hop)
    start, end = trim_bounds(x, top_db, fl, hop)
    return dict(name=name, x=x, n=n, frame_length=fl, hop_length=hop, top_db=top_db, mse=mse, start=start, end=end)


def groups():
    """The table's rows grouped by what one launch shares: {(frame_length, hop_length, top_db): [index]}, the long row apart
    (with two short neighbours) so that no batch is padded to its width."""
    out = {}
    for i, (_, _, n, fl, hop, top_db, _) in enumerate(TABLE):
        out.setdefault((fl, hop, top_db, n == LONG_ROW), []).append(i)
    for key in [k for k in out if k[3]]:
        fl, hop, top_db, _ = key
        out[key] += out[(fl, hop, top_db, False)][:2]
    return out
