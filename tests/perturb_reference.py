"""Float64 restatements of the audio perturbations (include/vasr.h: vasr_mean_square_f32, vasr_noise_plan_f64, vasr_mix_f32,
vasr_convolve_f32; viet-asr_amd/perturb.py), the case tables and the bounds of tests/test_perturb_host.py and
tests/test_gpu_perturb.py.  numpy only.

The formulas are those of nemo/collections/asr/parts/perturb.py and segment.py, written out:
  gain     y = x * 10^(gain_db / 20)
  shift    s = int(shift_ms * sr // 1000); y[t] = x[t + s] where 0 <= t + s < n, else 0; ignored when |shift_ms| / 1000 > n / sr
  noise    gain_db = min(rms_db(x) - rms_db(v) - snr_db, max_gain_db), rms_db = 10 log10(mean(x^2));
           start = int(round(uniform(0, N / sr - n / sr) * sr)); y = x + v[start : start + n] * 10^(gain_db / 20)
  impulse  y = fftconvolve(x, h, "full")

Bounds.
  mean square: a float32 square is exact in float64 and any order of adding n non-negative terms in float64 is within
    (n - 1) 2^-53 of their sum (first order); the division by n is one more rounding: n 2^-53 sum(x^2) / n on the mean.
  plan: the scale is a float64 expression of a handful of operations rounded to float32 once: 2 ulp of float32 leaves room for
    the device's pow (a few float64 ulps, which move the float32 rounding only at a tie).
  mix: the kernel computes fl(fma(c, v, fl(g x))) in float32, u = 2^-24: fl(g x) = g x (1 + d1), the fma rounds once more:
    result = (c v + g x (1 + d1)) (1 + d2), |error| <= u |g x| + u (|c v| + |g x|) + O(u^2) <= 2 u (|g x| + |c v|) (1 + u).
    MIX_BOUND_ULPS = 4 is twice that.
  convolution: an FFT's error is normwise, |error| <= c 2^-24 |h|_2 |x|_2 per row.  C_REF is the largest such c that
    scipy.signal.fftconvolve on float32 inputs -- the reference's own call -- shows against np.convolve in float64 over
    CONV_CASES with the inputs of conv_inputs(); measure_c_ref() is the script that measured it (python tests/perturb_reference.py
    prints it).  The device gets 4 C_REF: its partition sums and its fixed transform length of 2048 differ from scipy's
    single transform of the next fast length.
"""
import numpy as np

# the kernel's constants (perturb.hip / vasr_internal.h), restated
CONV_N = 2048           # transform length
CONV_TAPS = 1024        # taps per partition, Lp
CONV_OUT = 1024         # outputs per workgroup, L
CONV_MAX_TAPS = 32768
MS_CHUNK = 4096         # samples per partial sum of the mean square

MIX_BOUND_ULPS = 4.0
SCALE_ULPS = 2

# measured by measure_c_ref() with scipy 1.15.3 (pocketfft in float32): the largest ratio was 1.189, at n = 2, m = 2 -- the
# short cases lead, where |h|_2 |x|_2 is a handful of products and a single float32 rounding is a large share of it; the
# constant is that figure rounded up to two digits.  The device's own worst ratio over the same table, measured on one MI355X
# in all three layouts: 1.489 (0.621 on the mixed batch of tests/test_gpu_perturb.py), against the 4.8 it is held to.
C_REF = 1.2
C_DEVICE = 4.0 * C_REF

_L, _LP = CONV_OUT, CONV_TAPS
CONV_N_CASES = (0, 1, 2, _L - 1, _L, _L + 1, 2 * _L + 3)
CONV_M_CASES = (1, 2, _LP - 1, _LP, _LP + 1, 2 * _LP + 1)
CONV_CASES = [(n, m) for n in CONV_N_CASES for m in CONV_M_CASES] + [(2, CONV_MAX_TAPS)]
MS_N_CASES = (0, 1, MS_CHUNK - 1, MS_CHUNK, MS_CHUNK + 1, 3 * MS_CHUNK + 5)

# (name, ld_in(n_max), ld_out(ld_in, extra)): `same` packs the rows, `wider_out` leaves room behind the output, `odd_ld` breaks
# every 16-byte alignment after the first row
LAYOUTS = {
    "same": (lambda n: n, lambda ld, extra: ld + extra),
    "wider_out": (lambda n: n, lambda ld, extra: ld + extra + 37),
    "odd_ld": (lambda n: n + (2 if n % 2 else 3), lambda ld, extra: ld + extra + (0 if (ld + extra) % 2 else 1)),
}


def layout(name, n_max, extra=0):
    """-> (ld_in, ld_out) for rows of at most n_max samples whose outputs grow by `extra`; both at least 1."""
    f_in, f_out = LAYOUTS[name]
    ld_in = max(int(f_in(n_max)), 1)
    return ld_in, max(int(f_out(ld_in, extra)), 1)


def mean_square(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum(x * x) / x.size) if x.size else 0.0


def mean_square_bound(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.sum(x * x)) * 2.0 ** -53          # n 2^-53 sum / n


def noise_scale(ms_x, ms_v, snr_db, max_gain_db):
    cap = min(10.0 ** (max_gain_db / 20.0), float(np.finfo(np.float32).max))
    if ms_x == 0.0:
        return 0.0
    if ms_v == 0.0:
        return cap
    return min(np.sqrt(ms_x / ms_v) * 10.0 ** (-snr_db / 20.0), cap)


def noise_start(n, N, u, sample_rate):
    """Python doubles, as the reference: start_time = 0.0 + (N / sr - n / sr) * random(); int(round(start_time * sr))."""
    if N <= n:
        return 0
    sr = float(sample_rate)
    start_time = 0.0 + (N / sr - n / sr) * u
    return min(max(int(round(start_time * sr)), 0), N - n)


def shift_samples(shift_ms, sample_rate, n):
    """ShiftPerturbation's sample count, 0 where the reference ignores the shift."""
    if abs(shift_ms) / 1000 > n / float(sample_rate):
        return 0
    return int(shift_ms * sample_rate // 1000)


def mix(x, gain=1.0, shift=0, v=None, scale=0.0, start=0):
    """-> (y float64 [n], bound [n]): y[t] = gain x[t + shift] + scale v[(start + t) mod N]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    if abs(shift) > n:
        shift = 0
    t = np.arange(n)
    src = t + shift
    ok = (src >= 0) & (src < n)
    gx = np.zeros(n)
    gx[ok] = float(gain) * x[src[ok]]
    cv = np.zeros(n)
    if v is not None and scale != 0.0 and len(v) > 0:
        v = np.asarray(v, dtype=np.float64)
        cv = float(scale) * v[(int(start) + t) % v.size]
    return gx + cv, MIX_BOUND_ULPS * 2.0 ** -24 * (np.abs(gx) + np.abs(cv))


def convolve(x, h):
    x, h = np.asarray(x, dtype=np.float64), np.asarray(h, dtype=np.float64)
    return np.convolve(x, h) if x.size else np.zeros(0)


def conv_ratio(y, x, h):
    """max |y - convolve(x, h)| in units of 2^-24 |h|_2 |x|_2."""
    want = convolve(x, h)
    if want.size == 0:
        return 0.0
    scale = 2.0 ** -24 * np.linalg.norm(np.asarray(h, np.float64)) * np.linalg.norm(np.asarray(x, np.float64))
    return float(np.abs(np.asarray(y, np.float64) - want).max() / scale)


def conv_inputs(n, m, seed=0):
    """Unit-scale random x [n] and h [m] float32: a misplaced sample is an O(1) error."""
    rng = np.random.RandomState(1000003 * seed + 7919 * n + m)
    return rng.standard_normal(n).astype(np.float32), rng.standard_normal(m).astype(np.float32)


def measure_c_ref():
    """The largest conv_ratio of scipy.signal.fftconvolve on float32 inputs over CONV_CASES; None without scipy."""
    try:
        from scipy import signal
    except ImportError:
        return None
    worst = (0.0, None)
    for n, m in CONV_CASES:
        if n == 0:
            continue
        x, h = conv_inputs(n, m)
        worst = max(worst, (conv_ratio(signal.fftconvolve(x, h, "full"), x, h), (n, m)))
    return worst


# ---- the draw order of AudioAugmentor.perturb, per utterance (perturb.py:137-141 and each perturb()) ----
def draw_row(pipeline, aug_rng, n, sample_rate):
    """pipeline: [(prob, kind, cfg, rng)] with kind in gain / shift / noise / impulse / white_noise and cfg a dict holding the
    constructor's values (noise: + "lengths", impulse: + "count", the manifests' sizes).  Consumes aug_rng (random.Random) and
    each entry's rng exactly as the reference does for ONE utterance of n samples; -> list of (kind, params) for the entries
    that fired.  The noise start is reported as its u; the length n changes behind an impulse (the caller tracks it)."""
    out = []
    for prob, kind, cfg, rng in pipeline:
        if not aug_rng.random() < prob:
            continue
        if kind == "gain":
            out.append((kind, dict(gain_db=rng.uniform(cfg["min_gain_dbfs"], cfg["max_gain_dbfs"]))))
        elif kind == "shift":
            out.append((kind, dict(shift_ms=rng.uniform(cfg["min_shift_ms"], cfg["max_shift_ms"]))))
        elif kind == "noise":
            snr = rng.uniform(cfg["min_snr_db"], cfg["max_snr_db"])
            row = rng.sample(range(len(cfg["lengths"])), 1)[0]
            out.append((kind, dict(snr_db=snr, row=row, u=rng.random())))
        elif kind == "impulse":
            out.append((kind, dict(row=rng.sample(range(cfg["count"]), 1)[0])))
        elif kind == "white_noise":
            out.append((kind, dict(level_db=int(rng.randint(cfg["min_level"], cfg["max_level"], dtype="int32")))))
        else:
            raise ValueError(kind)
    return out


class Recorder:
    """Wraps a generator (random.Random or numpy RandomState): every value handed out is logged as [tag, method, value] -- how
    tests/golden/make_golden_perturb.py records the reference's draws and tests/test_perturb_host.py this project's."""

    def __init__(self, rng, tag, log):
        self._rng, self._tag, self._log = rng, tag, log

    def _note(self, name, v):
        self._log.append([self._tag, name, v])
        return v

    def random(self):
        return self._note("random", self._rng.random())

    def uniform(self, a, b):
        return self._note("uniform", self._rng.uniform(a, b))

    def sample(self, population, k):
        got = self._rng.sample(population, k)
        self._note("sample", [population.index(g) for g in got])
        return got

    def randint(self, lo, hi, dtype="int32"):
        return self._note("randint", int(self._rng.randint(lo, hi, dtype=dtype)))

    def randn(self, n):
        self._note("randn", int(n))
        return self._rng.randn(n)


if __name__ == "__main__":
    print("c_ref (scipy.signal.fftconvolve, float32 inputs, against np.convolve in float64):", measure_c_ref())
