"""GPU checks of the audio perturbations (csrc/perturb.hip through the C ABI, then viet-asr_amd/perturb.py and the engines)
against the float64 restatements of tests/perturb_reference.py.  Every output buffer starts as NaN (every element must be
written) and every input holds NaN behind its rows' lengths (none of it may be read as data)."""
import json
import random

import numpy as np
import pytest
import torch

import perturb_reference as R

pytestmark = pytest.mark.gpu

LAYOUTS = tuple(R.LAYOUTS)
NAN = float("nan")


def _stream(gpu):
    return torch.cuda.current_stream(gpu).cuda_stream


def _collate(rows, ld, fill=NAN):
    batch = np.full((len(rows), ld), fill, dtype=np.float32)
    for b, x in enumerate(rows):
        batch[b, : len(x)] = x
    return batch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def _i64(gpu, v):
    return torch.tensor([int(i) for i in v], dtype=torch.int64, device=gpu)


def _mean_square(gpu, rows, ld_in):
    from viet_asr_amd import _lib
    L = _lib.lib()
    x = torch.from_numpy(_collate(rows, ld_in)).to(gpu)
    ln = _i64(gpu, [len(r) for r in rows])
    ms = torch.full((len(rows),), NAN, dtype=torch.float64, device=gpu)
    need = int(L.vasr_mean_square_workspace_bytes(len(rows), ld_in))
    assert need > 0
    ws = torch.full((need,), 255, dtype=torch.uint8, device=gpu)
    _lib.check(L.vasr_mean_square_f32(x.data_ptr(), ld_in, ln.data_ptr(), len(rows), ms.data_ptr(), ws.data_ptr(), need, _stream(gpu)))
    return ms.cpu().numpy()


def _ms_rows():
    rng = np.random.RandomState(5)
    return [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32) for n in R.MS_N_CASES]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mean_square_against_float64(gpu, layout):
    rows = _ms_rows()
    ld_in, _ = R.layout(layout, max(len(r) for r in rows))
    got = _mean_square(gpu, rows, ld_in)
    for b, x in enumerate(rows):
        want, bound = R.mean_square(x), R.mean_square_bound(x)
        assert abs(got[b] - want) <= bound, (len(x), got[b], want)
    assert got[0] == 0.0                                   # n == 0


def test_mean_square_bits_do_not_depend_on_the_batch(gpu):
    rows = _ms_rows()
    batch = _mean_square(gpu, rows, R.layout("odd_ld", max(len(r) for r in rows))[0])
    for b, x in enumerate(rows):
        alone = _mean_square(gpu, [x], max(len(x), 1))
        assert _bits(alone)[0] == _bits(batch)[b], len(x)


def _plan(gpu, n, ms_x, row, snr, u, noise_len, ms_v, max_gain_db, sr):
    from viet_asr_amd import _lib
    B = len(n)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=gpu)
    args = [_i64(gpu, n), f64(ms_x), torch.tensor(row, dtype=torch.int32, device=gpu), f64(snr), f64(u)]
    nl, mv = _i64(gpu, noise_len), f64(ms_v)
    scale = torch.full((B,), NAN, dtype=torch.float32, device=gpu)
    start = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    _lib.check(_lib.lib().vasr_noise_plan_f64(*[a.data_ptr() for a in args], B, nl.data_ptr(), mv.data_ptr(), len(noise_len),
                                              float(max_gain_db), int(sr), scale.data_ptr(), start.data_ptr(), _stream(gpu)))
    return scale.cpu().numpy(), start.cpu().numpy()


def test_noise_plan(gpu):
    sr, n = 16000, 4001
    noise_len = [n - 1, n, n + 1, 3 * n, 16000 + n]
    ms_v = [0.25, 1e-3, 0.0, 3.7e-5, 0.5]
    us = [0.0, 0.5, 1.0 - 2.0 ** -53, 0.3000000000000001]
    rows, cases = [], []
    for r in range(len(noise_len)):
        for u in us:
            for ms_x, snr, cap in ((0.01, 20.0, 300.0), (0.0, 10.0, 300.0), (2.5e-4, -5.5, 300.0), (0.3, 40.0, -30.0)):
                cases.append((n, ms_x, r, snr, u, cap))
    cases.append((n, 0.01, -1, 20.0, 0.5, 300.0))           # no noise row
    for cap in sorted({c[5] for c in cases}):
        grp = [c for c in cases if c[5] == cap]
        scale, start = _plan(gpu, [c[0] for c in grp], [c[1] for c in grp], [c[2] for c in grp], [c[3] for c in grp],
                             [c[4] for c in grp], noise_len, ms_v, cap, sr)
        for b, (nn, ms_x, r, snr, u, _) in enumerate(grp):
            if r < 0:
                assert scale[b] == 0.0 and start[b] == 0
                continue
            want = np.float32(R.noise_scale(ms_x, ms_v[r], snr, cap))
            ulp = np.spacing(np.abs(want)) if want != 0 else 0.0
            assert abs(float(scale[b]) - float(want)) <= R.SCALE_ULPS * float(ulp), (grp[b], scale[b], want)
            assert int(start[b]) == R.noise_start(nn, noise_len[r], u, sr), (grp[b], start[b])
    # half-way ties, exact in binary: sr = 8192, n / sr = 0.25, N / sr = 1.25, u = (k + 0.5) / sr -> rint(k + 0.5), half to even
    ks = [2, 3, 4096, 8191]
    scale, start = _plan(gpu, [2048] * 4, [0.01] * 4, [0] * 4, [20.0] * 4, [(k + 0.5) / 8192 for k in ks], [2048 + 8192], [0.5],
                         300.0, 8192)
    assert start.tolist() == [2, 4, 4096, 8192] == [R.noise_start(2048, 2048 + 8192, (k + 0.5) / 8192, 8192) for k in ks]


def _mix(gpu, rows, ld_in, ld_out, gain=None, shift=None, add=None, add_len=None, add_row=None, scale=None, start=None):
    from viet_asr_amd import _lib
    B = len(rows)
    x = torch.from_numpy(_collate(rows, ld_in)).to(gpu)
    ln = _i64(gpu, [len(r) for r in rows])
    out = torch.full((B, ld_out), NAN, dtype=torch.float32, device=gpu)
    keep = [None if gain is None else torch.tensor(gain, dtype=torch.float32, device=gpu),
            None if shift is None else _i64(gpu, shift),
            None if add is None else torch.from_numpy(add).to(gpu),
            None if add_len is None else _i64(gpu, add_len),
            None if add_row is None else torch.tensor(add_row, dtype=torch.int32, device=gpu),
            None if scale is None else torch.tensor(scale, dtype=torch.float32, device=gpu),
            None if start is None else _i64(gpu, start)]
    p = [None if t is None else t.data_ptr() for t in keep]
    ld_add, add_rows = (add.shape[1], add.shape[0]) if add is not None else (0, 0)
    _lib.check(_lib.lib().vasr_mix_f32(x.data_ptr(), ld_in, ln.data_ptr(), B, p[0], p[1], p[2], ld_add, add_rows, p[3], p[4], p[5],
                                       p[6], out.data_ptr(), ld_out, _stream(gpu)))
    return out.cpu().numpy()


def _check_mix(out, rows, ld_out, gain=None, shift=None, noise=None, add_row=None, scale=None, start=None):
    for b, x in enumerate(rows):
        n = len(x)
        g = np.float32(1.0 if gain is None else gain[b])
        s = 0 if shift is None else shift[b]
        v = None if noise is None or add_row[b] < 0 else noise[add_row[b]]
        want, bound = R.mix(x, g, s, v, np.float32(0.0 if scale is None else scale[b]), 0 if start is None else start[b])
        err = np.abs(out[b, :n].astype(np.float64) - want)
        assert (err <= bound).all(), (b, n, s, float(err.max()))
        assert _bits(out[b, n:ld_out]).any() == False, (b, "zeros behind the length")       # noqa: E712  (+0.0, not NaN)


MIX_N = 5003          # more than one 4096-element tile, no multiple of 4


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mix_gain_shift_noise(gpu, layout):
    rng = np.random.RandomState(11)
    n = MIX_N
    shifts = [0, 1, -1, n - 1, -(n - 1), n, -n, n + 1, -(n + 1), 37, -4]
    rows = [rng.standard_normal(n).astype(np.float32) for _ in shifts] + [rng.standard_normal(k).astype(np.float32) for k in (0, 1, 3)]
    shifts += [0, 1, -2]
    B = len(rows)
    ld_in, ld_out = R.layout(layout, n)
    gains = (10.0 ** (rng.uniform(-10, 10, B) / 20.0)).astype(np.float32)
    # noises shorter than, as long as and longer than the rows: the short ones wrap
    noise = [rng.standard_normal(k).astype(np.float32) for k in (1, 7, n - 1, n, n + 1, 3 * n)]
    ld_add = 3 * n + (3 if layout == "odd_ld" else 0)
    bank = _collate(noise, ld_add)
    add_row = [b % len(noise) for b in range(B)]
    add_row[4] = -1
    scale = (10.0 ** rng.uniform(-2, 0, B)).astype(np.float32)
    start = [int(rng.randint(0, len(noise[r]))) if r >= 0 else 0 for r in add_row]
    start[5] = 2 * n                                        # row 5 reads noise 5 (3 n samples) from its last third on
    nl = [len(v) for v in noise]
    _check_mix(_mix(gpu, rows, ld_in, ld_out, gain=gains), rows, ld_out, gain=gains)
    _check_mix(_mix(gpu, rows, ld_in, ld_out, shift=shifts), rows, ld_out, shift=shifts)
    got = _mix(gpu, rows, ld_in, ld_out, add=bank, add_len=nl, add_row=add_row, scale=scale, start=start)
    _check_mix(got, rows, ld_out, noise=noise, add_row=add_row, scale=scale, start=start)
    got = _mix(gpu, rows, ld_in, ld_out, gain=gains, shift=shifts, add=bank, add_len=nl, add_row=add_row, scale=scale, start=start)
    _check_mix(got, rows, ld_out, gain=gains, shift=shifts, noise=noise, add_row=add_row, scale=scale, start=start)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mix_identity_is_a_bit_copy_and_a_zero_scale_reads_no_addend(gpu, layout):
    rng = np.random.RandomState(12)
    rows = [rng.standard_normal(k).astype(np.float32) for k in (MIX_N, 4096, 1, 0, 77)]
    rows[0][:4] = [-0.0, 1e-42, np.float32(np.inf), -1e38]  # a signed zero, a denormal, an infinity
    ld_in, ld_out = R.layout(layout, MIX_N)
    B = len(rows)
    want = _collate(rows, ld_out, fill=0.0)
    assert np.array_equal(_bits(_mix(gpu, rows, ld_in, ld_out)), _bits(want))
    ones, zeros = [1.0] * B, [0] * B
    poison = np.full((2, 64), NAN, dtype=np.float32)
    got = _mix(gpu, rows, ld_in, ld_out, gain=ones, shift=zeros, add=poison, add_len=[64, 64], add_row=[b % 2 for b in range(B)],
               scale=[0.0] * B, start=zeros)
    assert np.array_equal(_bits(got), _bits(want))


def _bank(gpu, irs, ld_ir):
    from viet_asr_amd import _lib
    L = _lib.lib()
    h = torch.from_numpy(_collate(irs, ld_ir)).to(gpu)
    hl = _i64(gpu, [len(v) for v in irs])
    need = int(L.vasr_convolve_spectra_bytes(len(irs), ld_ir))
    assert need == (len(irs) * ((-(-ld_ir // R.CONV_TAPS) + 1) // 2) * R.CONV_N + R.CONV_N // 2) * 8
    sp = torch.full((need // 4,), NAN, dtype=torch.float32, device=gpu)
    _lib.check(L.vasr_convolve_prepare_f32(h.data_ptr(), ld_ir, hl.data_ptr(), len(irs), sp.data_ptr(), need, _stream(gpu)))
    return dict(h=h, len=hl, spectra=sp, R=len(irs), ld=ld_ir)


def _convolve(gpu, rows, ld_in, bank, ir_row, ld_out):
    from viet_asr_amd import _lib
    B = len(rows)
    x = torch.from_numpy(_collate(rows, ld_in)).to(gpu)
    ln = _i64(gpu, [len(r) for r in rows])
    rr = torch.tensor(ir_row, dtype=torch.int32, device=gpu)
    out = torch.full((B, ld_out), NAN, dtype=torch.float32, device=gpu)
    len_out = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    _lib.check(_lib.lib().vasr_convolve_f32(x.data_ptr(), ld_in, ln.data_ptr(), B, rr.data_ptr(), bank["len"].data_ptr(),
                                            bank["spectra"].data_ptr(), bank["R"], bank["ld"], out.data_ptr(), ld_out,
                                            len_out.data_ptr(), _stream(gpu)))
    return out.cpu().numpy(), len_out.cpu().numpy()


def _check_conv(out, len_out, rows, irs, ir_row, ld_out, worst):
    for b, x in enumerate(rows):
        n, r = len(x), ir_row[b]
        if r < 0:
            assert int(len_out[b]) == n and np.array_equal(_bits(out[b, :n]), _bits(x)), (b, "copied bit for bit")
            m = 1
        else:
            m = len(irs[r])
            assert int(len_out[b]) == (n + m - 1 if n else 0), (b, n, m, len_out[b])
            if n:
                ratio = R.conv_ratio(out[b, : n + m - 1], x, irs[r])
                worst[0] = max(worst[0], ratio)
                assert ratio <= R.C_DEVICE, (n, m, ratio)
        lo = int(len_out[b])
        assert not _bits(out[b, lo:ld_out]).any(), (b, "zeros behind the length")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_convolve_the_case_table(gpu, layout):
    worst = [0.0]
    irs = [R.conv_inputs(0, m)[1] for m in R.CONV_M_CASES]
    ld_ir, _ = R.layout(layout, max(R.CONV_M_CASES))
    bank = _bank(gpu, irs, ld_ir)
    rows, ir_row = [], []
    for n in R.CONV_N_CASES:
        for r, m in enumerate(R.CONV_M_CASES):
            rows.append(R.conv_inputs(n, m)[0])
            ir_row.append(r)
    ld_in, ld_out = R.layout(layout, max(R.CONV_N_CASES), ld_ir - 1)
    out, len_out = _convolve(gpu, rows, ld_in, bank, ir_row, ld_out)
    _check_conv(out, len_out, rows, irs, ir_row, ld_out, worst)
    # the longest response the call takes, against two samples
    x, h = R.conv_inputs(2, R.CONV_MAX_TAPS)
    big = _bank(gpu, [h], R.CONV_MAX_TAPS)
    ld_in, ld_out = R.layout(layout, 2, R.CONV_MAX_TAPS - 1)
    out, len_out = _convolve(gpu, [x], ld_in, big, [0], ld_out)
    _check_conv(out, len_out, [x], [h], [0], ld_out, worst)
    print(f"convolve, layout {layout}: worst ratio {worst[0]:.3f} of 2^-24 |h| |x| (bound {R.C_DEVICE})")


def test_convolve_mixed_batch_deltas_and_row_independence(gpu):
    worst = [0.0]
    Lp, L = R.CONV_TAPS, R.CONV_OUT
    m = 2 * Lp + 1
    irs = []
    for k in (0, 1, Lp - 1, Lp, m - 1):                     # h = delta_k: the output is x delayed by k, exactly
        h = np.zeros(m, dtype=np.float32)
        h[k] = 1.0
        irs.append(h)
    irs += [R.conv_inputs(0, mm)[1] for mm in (3, Lp + 1, m)]
    bank = _bank(gpu, irs, m + 2)
    lens = [2 * L + 3, L + 1, 5, 2 * L + 3, L, 2 * L + 3, 0, 777, L - 1, 2 * L + 3, 1]
    ir_row = [0, 1, 2, 3, 4, 5, 6, -1, 7, 7, -1]
    rows = [R.conv_inputs(n, 17 + b)[0] for b, n in enumerate(lens)]
    ld_in = max(lens) + 1
    ld_out = ld_in + m + 2 - 1
    out, len_out = _convolve(gpu, rows, ld_in, bank, ir_row, ld_out)
    _check_conv(out, len_out, rows, irs, ir_row, ld_out, worst)
    for b, k in enumerate((0, 1, Lp - 1, Lp, m - 1)):
        n = lens[b]
        delayed = np.zeros(n + m - 1, dtype=np.float64)
        delayed[k : k + n] = rows[b]
        scale = 2.0 ** -24 * np.linalg.norm(rows[b].astype(np.float64))
        assert np.abs(out[b, : n + m - 1] - delayed).max() <= R.C_DEVICE * scale, (k, "a delayed copy")
    # a row alone, at its own pitch, gives the bits it gave in the batch
    for b in (0, 3, 8, 9, 7):
        alone, alone_len = _convolve(gpu, [rows[b]], max(lens[b], 1), bank, [ir_row[b]], max(lens[b], 1) + m + 2 - 1)
        lo = int(len_out[b])
        assert int(alone_len[0]) == lo and np.array_equal(_bits(alone[0, :lo]), _bits(out[b, :lo])), b
    print(f"convolve, mixed batch: worst ratio {worst[0]:.3f}")


# ---- end to end: perturb.AudioAugmentor, the engine and VietASR ------------------------------------------------------------
SR = 16000


def _banks(seed):
    rng = np.random.RandomState(seed)
    noises = [((rng.standard_normal(n) * 0.05).astype(np.float32), SR) for n in (2000, 9000, 30011)]
    irs = [((rng.standard_normal(m) * np.exp(-np.arange(m) / (m / 6.0))).astype(np.float32), SR) for m in (1, 300, 2500)]
    return noises, irs


def _augmentor(seed, prob, noises, irs, order=("gain", "shift", "noise", "impulse")):
    from viet_asr_amd import perturb as P
    make = {
        "gain": lambda r: P.GainPerturbation(min_gain_dbfs=-10, max_gain_dbfs=10, rng=r),
        "shift": lambda r: P.ShiftPerturbation(min_shift_ms=-40.0, max_shift_ms=40.0, rng=r),
        "noise": lambda r: P.NoisePerturbation(min_snr_db=0, max_snr_db=30, rng=r, signals=noises),
        "impulse": lambda r: P.ImpulsePerturbation(rng=r, signals=irs),
    }
    ptbs = [(prob, make[k](random.Random(seed + 1 + i))) for i, k in enumerate(order)]
    return P.AudioAugmentor(perturbations=ptbs, rng=random.Random(seed))


def _dev_batch(rows, gpu, fill=NAN):
    lens = [len(r) for r in rows]
    return torch.from_numpy(_collate(rows, max(lens), fill)).to(gpu), torch.tensor(lens, dtype=torch.int64, device=gpu)


@pytest.mark.parametrize("order", [("gain", "shift", "noise", "impulse"), ("impulse", "noise", "shift", "gain")])
def test_perturb_batch_is_the_composition_of_the_restatements(gpu, order):
    noises, irs = _banks(3)
    rng = np.random.RandomState(4)
    rows = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in (4000, 5003, 1200, 4096, 333, 4500, 2048, 4999)]
    x, ln = _dev_batch(rows, gpu)
    got, got_len = _augmentor(21, 0.6, noises, irs, order).perturb_batch(x, ln, SR, lengths_host=[len(r) for r in rows])
    torch.cuda.synchronize()
    got, got_len = got.cpu().numpy(), got_len.cpu().numpy()
    plan = _augmentor(21, 0.6, noises, irs, order).draw_batch([len(r) for r in rows], SR)     # the same seeds: the same draws
    fired = set()
    u = 2.0 ** -24
    for b, row in enumerate(rows):
        y, bound = row.astype(np.float64), np.zeros(len(row))
        for k, kind in enumerate(order):
            d = plan[k][b]
            if d is None:
                continue
            fired.add(kind)
            if kind == "gain":
                g = float(np.float32(10.0 ** (d["gain_db"] / 20.0)))
                y, e = R.mix(y, gain=g)
                bound = abs(g) * bound + e
            elif kind == "shift":
                assert d["shift"] == R.shift_samples(d["shift_ms"], SR, y.size)
                y, _ = R.mix(y, shift=d["shift"])
                bound = R.mix(bound, shift=d["shift"])[0]       # a copy: the bound moves with the samples
            elif kind == "noise":
                v = noises[d["row"]][0]
                c = float(np.float32(R.noise_scale(R.mean_square(y), R.mean_square(v), d["snr_db"], 300.0)))
                st = R.noise_start(y.size, v.size, d["u"], SR)
                y2, e = R.mix(y, v=v, scale=c, start=st)
                # the device's scale comes from the device's row: SCALE_ULPS of float32, and the row's own relative error
                rel = (R.SCALE_ULPS + 1) * 2 * u + np.linalg.norm(bound) / max(np.linalg.norm(y), 1e-30)
                bound = bound + e + rel * np.abs(y2 - y)
                y = y2
            elif kind == "impulse":
                h = irs[d["row"]][0]
                e = R.C_DEVICE * u * np.linalg.norm(h.astype(np.float64)) * np.linalg.norm(y)
                bound = R.convolve(bound, np.abs(h)) + e
                y = R.convolve(y, h)
        assert int(got_len[b]) == y.size, (b, got_len[b], y.size)
        err = np.abs(got[b, : y.size] - y)
        assert (err <= bound + 1e-30).all(), (b, float(err.max()), float(bound.max()))
        assert not _bits(got[b, y.size:]).any(), (b, "zeros behind the length")
    assert fired == set(order)


def _tiny_asr(tmp_path):
    from conftest import load_golden
    from viet_asr_amd.infer import VietASR
    _, cfg, _, _, enc_sd, dec_sd = load_golden("vi12x1_b1_tiny")
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in enc_sd.items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in dec_sd.items()}, dec_p)
    return VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy"), cfg


def test_engines_take_an_augmentor(gpu, tmp_path):
    from viet_asr_amd import audio, perturb as P
    asr, cfg = _tiny_asr(tmp_path)
    rng = np.random.RandomState(8)
    rows = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in (9000, 12001, 7000, 10500, 8000)]
    texts = ["ab", "", "xin chao", "a b c", "mot hai"]
    lines = []
    for i, (x, t) in enumerate(zip(rows, texts)):
        path = str(tmp_path / f"a{i}.wav")
        audio.write_wav(path, x, SR)
        lines.append(dict(audio_filepath=path, duration=len(x) / SR, text=t))
    man = str(tmp_path / "manifest.json")
    with open(man, "w") as f:
        f.write("\n".join(json.dumps(e) for e in lines) + "\n")
    noises, irs = _banks(5)
    never = _augmentor(31, 0.0, noises, irs)
    plain = asr.evaluate_manifest(man, batch_size=3)
    assert asr.evaluate_manifest(man, batch_size=3, augmentor=never) == plain          # transcripts and counts, bit for bit
    assert asr.evaluate_manifest(man, batch_size=3, augmentor=never, eval_loss=True) == asr.evaluate_manifest(man, batch_size=3, eval_loss=True)
    assert asr.transcribe_batch(rows, row_independent=True, augmentor=never) == asr.transcribe_batch(rows, row_independent=True)
    # gain 0 dB and the response delta_0: the same signal up to the transform's rounding
    delta = [(np.ones(1, dtype=np.float32), SR)]
    same = P.AudioAugmentor([(1.0, P.GainPerturbation(min_gain_dbfs=0, max_gain_dbfs=0, rng=random.Random(1))),
                             (1.0, P.ImpulsePerturbation(rng=random.Random(2), signals=delta))], rng=random.Random(3))
    eng = asr._fused_engine()
    x, ln = _dev_batch(rows, gpu, fill=0.0)
    a = eng.forward(x, ln, want_logp=True, row_independent=True, augmentor=same, _lengths_host=[len(r) for r in rows])
    b = eng.forward(x, ln, want_logp=True, row_independent=True)
    torch.cuda.synchronize()
    assert a["length"].cpu().tolist() == [len(r) for r in rows]
    al, bl = a["logp"].cpu().numpy(), b["logp"].cpu().numpy()
    worst = 0.0
    for r in range(len(rows)):
        t1 = eng.frames(len(rows[r]))[1]
        worst = max(worst, float(np.abs(al[r, :t1] - bl[r, :t1]).max()))
    tol = 5e-4 + 2e-5 * float(np.abs(bl).max())                # the parity tests' log-prob tolerance
    print(f"gain 0 dB + delta_0: log-prob max-abs difference {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    # a real perturbation goes through every call and changes the result; align and score accept it
    loud = _augmentor(41, 1.0, noises, irs)
    hyps, res = asr.evaluate_manifest(man, batch_size=3, augmentor=loud)
    assert len(hyps) == len(rows) and res["ref_words"] == plain[1]["ref_words"]
    assert len(asr.score(rows, [t or "a" for t in texts], augmentor=_augmentor(41, 1.0, noises, irs))) == len(rows)
    spans = asr.align(rows, augmentor=_augmentor(41, 1.0, noises, irs))
    assert len(spans) == len(rows) and all("chars" in s for s in spans)
    with pytest.raises(TypeError):
        eng.forward(x, ln, augmentors=never)


def test_white_noise_samples_come_from_the_device(gpu):
    from viet_asr_amd import perturb as P
    aug = P.AudioAugmentor([(1.0, P.WhiteNoisePerturbation(min_level=-40, max_level=-39, rng=np.random.RandomState(1)))],
                           rng=random.Random(0))
    rows = [np.zeros(n, dtype=np.float32) for n in (20000, 5003)]
    x, ln = _dev_batch(rows, gpu)
    y, ln2 = aug.perturb_batch(x, ln, SR, lengths_host=[len(r) for r in rows])
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert ln2.cpu().tolist() == [20000, 5003] and y.shape == (2, 20000)
    for b, n in enumerate((20000, 5003)):
        # randint(-40, -39) is -40 dB: 0.01 times unit normal samples; the sample deviation of n draws is within 5 / sqrt(2 n)
        assert abs(y[b, :n].astype(np.float64).std() / 0.01 - 1.0) <= 5.0 / np.sqrt(2 * n), b
        assert not _bits(y[b, n:]).any()
