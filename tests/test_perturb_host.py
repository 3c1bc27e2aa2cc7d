"""CPU checks of the audio perturbations: the float64 restatements of tests/perturb_reference.py against what the REAL reference
produced (tests/golden/perturb_draws.json, written by tests/golden/make_golden_perturb.py), the order in which
viet-asr_amd/perturb.py consumes its generators, the reference's config keys, and the refusals of the C ABI (no device is
touched by any of them)."""
import json
import os
import random
import re

import numpy as np
import pytest

import perturb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "perturb_draws.json")) as f:
        return json.load(f)


def _arrays(golden, names):
    return [np.asarray(golden["files"][k], dtype=np.float32) for k in names]


def _replay(golden, case):
    """The case's output from the recorded draws through the float64 restatements -> (y, tolerance)."""
    sr = golden["sample_rate"]
    x = np.asarray(golden["signals"][case["signal"]], dtype=np.float64)
    noises, irs = _arrays(golden, golden["noise_files"]), _arrays(golden, golden["impulse_files"])
    draws = list(case["draws"])
    for k, (kind, prob, cfg) in enumerate(case["pipeline"]):
        tag, name, u = draws.pop(0)
        assert (tag, name) == (-1, "random")
        if not u < prob:
            continue
        if kind == "gain":
            x = R.mix(x, gain=10.0 ** (draws.pop(0)[2] / 20.0))[0]
        elif kind == "shift":
            x = R.mix(x, shift=R.shift_samples(draws.pop(0)[2], sr, x.size))[0]
        elif kind == "noise":
            snr, row, start_time = draws.pop(0)[2], draws.pop(0)[2][0], draws.pop(0)[2]
            v = noises[row]
            scale = R.noise_scale(R.mean_square(x), R.mean_square(v), snr, cfg["max_gain_db"])
            x = R.mix(x, v=v, scale=scale, start=int(round(start_time * sr)))[0]
        elif kind == "impulse":
            x = R.convolve(x, irs[draws.pop(0)[2][0]])
    assert not draws
    return x


def test_restatements_reproduce_the_reference(golden):
    assert len(golden["cases"]) >= 12
    kinds = set()
    for case in golden["cases"]:
        want = np.asarray(case["output"], dtype=np.float64)
        got = _replay(golden, case)
        assert got.shape == want.shape, case["pipeline"]
        # the reference works in float32 (its rms_db too): a few float32 roundings of the largest sample
        assert np.abs(got - want).max() <= 2e-5 * max(np.abs(want).max(), 1e-30), case["pipeline"]
        kinds |= {k for k, _, _ in case["pipeline"]}
    assert kinds == {"gain", "shift", "noise", "impulse"}


def _pipeline(golden, case, log):
    from viet_asr_amd import perturb as P
    sr = golden["sample_rate"]
    noise = [(x, sr) for x in _arrays(golden, golden["noise_files"])]
    irs = [(x, sr) for x in _arrays(golden, golden["impulse_files"])]
    ptbs = []
    for k, (kind, prob, cfg) in enumerate(case["pipeline"]):
        rng = R.Recorder(random.Random(case["seeds"][k + 1]), k, log)
        extra = {"noise": dict(signals=noise), "impulse": dict(signals=irs)}.get(kind, {})
        ptbs.append((prob, P.perturbation_types[kind](rng=rng, **cfg, **extra)))
    return P.AudioAugmentor(perturbations=ptbs, rng=R.Recorder(random.Random(case["seeds"][0]), -1, log))


def test_the_generators_are_consumed_as_the_reference_consumes_them(golden):
    sr = golden["sample_rate"]
    noise_len = [len(golden["files"][k]) for k in golden["noise_files"]]
    for case in golden["cases"]:
        log = []
        aug = _pipeline(golden, case, log)
        n = len(golden["signals"][case["signal"]])
        plan = aug.draw_batch([n], sr)
        assert len(log) == len(case["draws"]), case["pipeline"]
        for mine, ref in zip(log, case["draws"]):
            if (mine[1], ref[1]) == ("random", "uniform"):       # the noise start: uniform(0.0, d) is 0.0 + d * random()
                assert mine[0] == ref[0]
                continue
            assert mine == ref, (case["pipeline"], mine, ref)
        # ... and the start that the one random() gives is the reference's
        length = n
        for k, (kind, _, _) in enumerate(case["pipeline"]):
            d = plan[k][0]
            if d is None:
                continue
            if kind == "noise":
                start_time = [e[2] for e in case["draws"] if e[0] == k and e[1] == "uniform"][1]
                N = noise_len[d["row"]]
                assert start_time == 0.0 + (N / float(sr) - length / float(sr)) * d["u"]
                assert R.noise_start(length, N, d["u"], sr) == min(int(round(start_time * sr)), N - length)
            if kind == "impulse":
                length += len(golden["files"][golden["impulse_files"][d["row"]]]) - 1
            if kind == "shift":
                assert d["shift"] == R.shift_samples(d["shift_ms"], sr, length)
        # the restated draw order of the reference file consumes fresh generators the same way
        pipe = []
        for k, (kind, prob, cfg) in enumerate(case["pipeline"]):
            cfg = dict(cfg, lengths=noise_len, count=len(golden["impulse_files"]))
            pipe.append((prob, kind, cfg, random.Random(case["seeds"][k + 1])))
        fired = R.draw_row(pipe, random.Random(case["seeds"][0]), n, sr)
        assert [k for k, _ in fired] == [case["pipeline"][k][0] for k in range(len(plan)) if plan[k][0] is not None]


def test_white_noise_level_is_drawn_as_the_reference_draws_it(golden):
    from viet_asr_amd import perturb as P
    w = golden["white_noise"]
    p = P.WhiteNoisePerturbation(min_level=w["min_level"], max_level=w["max_level"], rng=np.random.RandomState(w["seed"]))
    ref = [e for e in w["draws"] if e[1] == "randint"]
    # the reference's randn between two levels advances the generator: only the first level is comparable without it
    assert p.draw(8, golden["sample_rate"])["level_db"] == ref[0][2]


def test_noise_start_equals_the_references_also_at_a_tie(golden):
    sr = golden["sample_rate"]
    ties = 0
    for s in golden["starts"]:
        assert R.noise_start(s["n"], s["N"], s["u"], sr) == min(s["start"], s["N"] - s["n"]), s
        ties += (s["u"] * sr) % 1 == 0.5
    assert ties >= 2


def test_from_config_takes_the_references_keys(golden):
    from viet_asr_amd import perturb as P
    assert sorted(P.perturbation_types) == golden["perturbation_types"]
    sr = golden["sample_rate"]
    irs = [(x, sr) for x in _arrays(golden, golden["impulse_files"])]
    aug = P.AudioAugmentor.from_config([
        {"aug_type": "gain", "prob": 0.5, "cfg": {"min_gain_dbfs": -3, "max_gain_dbfs": 3}},
        {"aug_type": "shift", "prob": 0.25, "cfg": {"min_shift_ms": -2.0, "max_shift_ms": 2.0}},
        {"aug_type": "white_noise", "prob": 1.0, "cfg": {"min_level": -80, "max_level": -50}},
        {"aug_type": "impulse", "prob": 1.0, "cfg": {"signals": irs}},
        {"aug_type": "unknown", "prob": 1.0, "cfg": {}},
    ])
    assert [type(p).__name__ for _, p in aug._pipeline] == ["GainPerturbation", "ShiftPerturbation", "WhiteNoisePerturbation",
                                                            "ImpulsePerturbation"]
    assert aug.max_augmentation_length(1000, sr) == 1000 + max(len(x) for x, _ in irs) - 1
    with pytest.raises(NotImplementedError):
        P.AudioAugmentor.from_config([{"aug_type": "speed", "prob": 1.0, "cfg": {}}])
    with pytest.raises(NotImplementedError):
        P.SpeedPerturbation()


def test_scipy_stays_within_c_ref():
    worst = R.measure_c_ref()
    if worst is None:
        pytest.skip("scipy is not installed")
    print("scipy.signal.fftconvolve: worst ratio", worst)
    assert worst[0] <= R.C_REF


def test_kernel_constants_are_the_restated_ones():
    src = open(os.path.join(ROOT, "viet-asr_amd", "csrc", "vasr_internal.h")).read()
    for name, want in (("kMsChunk", R.MS_CHUNK), ("kConvN", R.CONV_N), ("kConvTaps", R.CONV_TAPS), ("kConvOut", R.CONV_OUT),
                       ("kConvMaxTaps", R.CONV_MAX_TAPS)):
        assert int(re.search(r"constexpr \w+ %s = (\d+);" % name, src).group(1)) == want, name
    assert R.CONV_OUT + R.CONV_TAPS - 1 <= R.CONV_N


INVALID, UNSUPPORTED = -1, -5


def test_c_abi_refusals_and_sizes():
    from viet_asr_amd import _lib
    L = _lib.lib()
    p = 4096                                                 # a stand-in for a device pointer: every refusal comes first
    err = lambda: L.vasr_last_error().decode()
    # sizes
    assert L.vasr_mean_square_workspace_bytes(3, 10000) == 3 * 3 * 8 + 256
    assert L.vasr_mean_square_workspace_bytes(1, 0) == 256 and L.vasr_mean_square_workspace_bytes(0, 10) == 0
    assert L.vasr_mean_square_workspace_bytes(1, -1) == 0
    pair, head = R.CONV_N * 8, R.CONV_N // 2 * 8            # a pair of partitions; the twiddle table in front
    assert L.vasr_convolve_spectra_bytes(1, 1) == head + pair and L.vasr_convolve_spectra_bytes(2, 2 * R.CONV_TAPS) == head + 2 * pair
    assert L.vasr_convolve_spectra_bytes(3, 2 * R.CONV_TAPS + 1) == head + 3 * 2 * pair
    assert L.vasr_convolve_spectra_bytes(1, R.CONV_MAX_TAPS) == head + 16 * pair
    assert L.vasr_convolve_spectra_bytes(1, R.CONV_MAX_TAPS + 1) == 0 and L.vasr_convolve_spectra_bytes(0, 8) == 0
    # mean square
    assert L.vasr_mean_square_f32(None, 8, p, 1, p, p, 512, None) == INVALID
    assert L.vasr_mean_square_f32(p, 8, p, 1, p, None, 512, None) == INVALID
    assert L.vasr_mean_square_f32(p, -1, p, 1, p, p, 512, None) == INVALID
    assert L.vasr_mean_square_f32(p, 8, p, 0, p, p, 512, None) == INVALID
    assert L.vasr_mean_square_f32(p, 8, p, 1, p, p, 263, None) == INVALID and "264" in err()
    # plan
    assert L.vasr_noise_plan_f64(p, p, p, p, None, 1, p, p, 1, 300.0, 16000, p, p, None) == INVALID
    assert L.vasr_noise_plan_f64(p, p, p, p, p, 1, p, p, 0, 300.0, 16000, p, p, None) == INVALID
    assert L.vasr_noise_plan_f64(p, p, p, p, p, 1, p, p, 1, 300.0, 0, p, p, None) == INVALID
    assert L.vasr_noise_plan_f64(p, p, p, p, p, 1, p, p, 1, float("nan"), 16000, p, p, None) == INVALID
    # mix
    q = p + 4096
    assert L.vasr_mix_f32(None, 8, p, 1, None, None, None, 0, 0, None, None, None, None, q, 8, None) == INVALID
    assert L.vasr_mix_f32(p, 8, p, 1, None, None, None, 0, 0, None, None, None, None, p, 8, None) == INVALID      # aliased
    assert L.vasr_mix_f32(p, 8, p, 1, None, None, None, 0, 0, None, None, None, None, q, 7, None) == INVALID      # ld_out < ld_in
    assert L.vasr_mix_f32(p, 8, p, 1, None, None, p, 8, 1, p, p, None, None, q, 8, None) == INVALID               # no scale
    assert L.vasr_mix_f32(p, 8, p, 1, None, None, p, 8, 0, p, p, p, None, q, 8, None) == INVALID                  # add_rows
    # convolution
    ok = dict(d_in=p, ld_in=8, d_len=p, batch=1, d_ir_row=p, d_ir_len=p, d_spectra=p, R=1, ld_ir=4, d_out=q, ld_out=11, d_len_out=p)

    def conv(**kw):
        a = dict(ok, **kw)
        return L.vasr_convolve_f32(a["d_in"], a["ld_in"], a["d_len"], a["batch"], a["d_ir_row"], a["d_ir_len"], a["d_spectra"],
                                   a["R"], a["ld_ir"], a["d_out"], a["ld_out"], a["d_len_out"], None)
    for name in ("d_in", "d_len", "d_ir_row", "d_ir_len", "d_spectra", "d_out", "d_len_out"):
        assert conv(**{name: None}) == INVALID, name
    assert conv(d_out=p) == INVALID and conv(batch=0) == INVALID and conv(R=0) == INVALID and conv(ld_ir=0) == INVALID
    assert conv(ld_out=10) == INVALID and "11" in err()      # ld_out >= ld_in + ld_ir - 1
    assert conv(d_spectra=p + 4) == INVALID
    big = R.CONV_MAX_TAPS + 1
    assert conv(ld_ir=big, ld_out=8 + big - 1) == UNSUPPORTED and str(R.CONV_MAX_TAPS) in err()
    assert conv(ld_ir=big, ld_out=8 + big - 1, d_len=None) == INVALID       # an argument error wins over the limit
    assert conv(ld_ir=big, ld_out=8) == INVALID
    assert conv(ld_ir=R.CONV_MAX_TAPS, ld_out=8 + R.CONV_MAX_TAPS - 2) == INVALID
    assert L.vasr_convolve_prepare_f32(None, 4, p, 1, p, head + pair, None) == INVALID
    assert L.vasr_convolve_prepare_f32(p, 4, p, 1, p, head + pair - 1, None) == INVALID and str(head + pair) in err()
    assert L.vasr_convolve_prepare_f32(p, big, p, 1, p, 1 << 30, None) == UNSUPPORTED
    assert L.vasr_convolve_prepare_f32(p, big, None, 1, p, 1 << 30, None) == INVALID
    assert L.vasr_convolve_prepare_f32(p, 4, p, 70000, p, 1 << 40, None) == UNSUPPORTED


def test_data_layers_point_at_the_engine_argument(tmp_path):
    from viet_asr_amd.data_layer import AudioToSpeechLabelDataLayer
    man = tmp_path / "m.json"
    man.write_text("")
    with pytest.raises(NotImplementedError, match="augmentor="):
        AudioToSpeechLabelDataLayer(str(man), ["a"], 2, augmentor=object())
