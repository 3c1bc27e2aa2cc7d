#!/usr/bin/env python3
"""Generate tests/golden/perturb_draws.json by running the REAL reference perturbations (nemo/collections/asr/parts/perturb.py)
on the CPU -- dev container only.

    python tests/golden/make_golden_perturb.py     # needs the reference checkout, numpy and scipy

The reference module is loaded from its file.  What it imports and this image lacks is stubbed: ``librosa`` and ``soundfile`` as
empty modules, ``nemo.logging`` as a no-op, ``collections.ASRAudioText`` as a list of records; ``AudioSegment.from_file`` is
patched to return segments built from arrays, ``np.sctypes`` is restored where numpy 2 dropped it.  Stored, data only:
  inputs   small seeded signals, noise recordings and impulse responses (float32 as nine-digit decimals), the sample rate;
  cases    per case the pipeline (kind, prob, constructor arguments, seeds), the signal it ran on, the reference's output, and
           the SEQUENCE of values every generator handed out while the reference ran (recorded by wrapping the generators'
           methods) -- the draw order tests/test_perturb_host.py replays;
  starts   NoisePerturbation's start samples for chosen (n, N, u), half-way ties included, through the reference's
           ``subsegment`` arithmetic.
"""
import importlib.util
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from perturb_reference import Recorder  # noqa: E402
REF = "/root/reference"
SR = 8192                 # a power of two: n / sr and k + 0.5 are exact, so half-way ties can be built


def reference_modules():
    if not hasattr(np, "sctypes"):
        np.sctypes = {"int": [np.int8, np.int16, np.int32, np.int64], "float": [np.float16, np.float32, np.float64]}
    for name in ("librosa", "soundfile"):
        sys.modules.setdefault(name, types.ModuleType(name))
    parts = os.path.join(REF, "nemo", "collections", "asr", "parts")
    nemo = types.ModuleType("nemo")
    nemo.logging = types.SimpleNamespace(debug=lambda *a, **k: None, warning=lambda *a, **k: None)
    pkgs = {"nemo": nemo}
    for name in ("nemo.collections", "nemo.collections.asr", "nemo.collections.asr.parts"):
        pkgs[name] = types.ModuleType(name)
    coll = types.ModuleType("nemo.collections.asr.parts.collections")
    coll.ASRAudioText = lambda manifest_path, parser=None: types.SimpleNamespace(
        data=[{"audio_filepath": p} for p in manifest_path.split(",")])
    pars = types.ModuleType("nemo.collections.asr.parts.parsers")
    pars.make_parser = lambda labels: None
    pkgs["nemo.collections.asr.parts.collections"], pkgs["nemo.collections.asr.parts.parsers"] = coll, pars
    sys.modules.update(pkgs)
    pkgs["nemo.collections.asr.parts"].collections, pkgs["nemo.collections.asr.parts"].parsers = coll, pars

    def load(name):
        spec = importlib.util.spec_from_file_location("nemo.collections.asr.parts." + name, os.path.join(parts, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        return mod
    segment = load("segment")
    return load("perturb"), segment


def f32_list(x):
    """float32 values as the shortest decimals that read back to the same float32 (nine significant digits)"""
    return [float("%.9g" % v) for v in np.asarray(x, dtype=np.float32)]


def main():
    P, S = reference_modules()
    gen = np.random.RandomState(20240607)
    signals = {f"x{n}": (gen.standard_normal(n) * 0.1).astype(np.float32) for n in (1, 40, 64)}
    files = {f"noise{n}": (gen.standard_normal(n) * 0.02).astype(np.float32) for n in (65, 90, 130)}
    files.update({f"ir{m}": (gen.standard_normal(m) * np.exp(-np.arange(m) / 8.0)).astype(np.float32) for m in (1, 5, 16)})
    S.AudioSegment.from_file = classmethod(lambda cls, filename, target_sr=None, **kw: cls(files[filename].copy(), SR))
    noise_manifest = ",".join(k for k in files if k.startswith("noise"))
    ir_manifest = ",".join(k for k in files if k.startswith("ir"))

    specs = {
        "gain": lambda r: P.GainPerturbation(min_gain_dbfs=-12, max_gain_dbfs=7, rng=r),
        "shift": lambda r: P.ShiftPerturbation(min_shift_ms=-9.0, max_shift_ms=9.0, rng=r),
        "noise": lambda r: P.NoisePerturbation(manifest_path=noise_manifest, min_snr_db=5, max_snr_db=25, max_gain_db=300.0, rng=r),
        "impulse": lambda r: P.ImpulsePerturbation(manifest_path=ir_manifest, rng=r),
    }
    cfgs = {
        "gain": dict(min_gain_dbfs=-12, max_gain_dbfs=7),
        "shift": dict(min_shift_ms=-9.0, max_shift_ms=9.0),
        "noise": dict(min_snr_db=5, max_snr_db=25, max_gain_db=300.0),
        "impulse": dict(),
    }
    pipelines = [
        [("gain", 1.0)], [("shift", 1.0)], [("noise", 1.0)], [("impulse", 1.0)],
        [("gain", 0.5), ("shift", 0.5), ("noise", 0.5), ("impulse", 0.5)],
        [("impulse", 0.7), ("noise", 0.7), ("shift", 0.7), ("gain", 0.7)],
    ]
    cases = []
    for pi, pipe in enumerate(pipelines):
        for si, name in enumerate(("x40", "x64", "x1")):
            if name == "x1" and any(k == "noise" for k, _ in pipe):
                continue                      # one sample rounds to an empty noise slice in the reference: numpy broadcasts it
            log = []
            seeds = [1000 * pi + 10 * si + k for k in range(len(pipe) + 1)]
            ptbs = [(prob, specs[kind](Recorder(random.Random(seeds[k + 1]), k, log))) for k, (kind, prob) in enumerate(pipe)]
            aug = P.AudioAugmentor(perturbations=ptbs, rng=Recorder(random.Random(seeds[0]), -1, log))
            seg = S.AudioSegment(signals[name].copy(), SR)
            try:
                aug.perturb(seg)
            except ValueError:
                continue                      # the noise slice came out one sample off: the reference cannot add it
            cases.append(dict(pipeline=[[k, p, cfgs[k]] for k, p in pipe], seeds=seeds, signal=name,
                              output=f32_list(seg._samples),
                              output_dtype=str(seg._samples.dtype), draws=log))
    # the noise start alone, through the reference's subsegment(): start_sample = int(round(start_time * sr))
    starts = []
    for n, N, u in ((2048, 2048 + SR, 2.5 / SR), (2048, 2048 + SR, 3.5 / SR), (2048, 2048 + SR, 4096.5 / SR), (40, 65, 0.0),
                    (40, 65, 0.5), (40, 65, 1.0 - 2.0 ** -53), (64, 65, 0.75), (100, 2000, 0.123456789)):
        noise = S.AudioSegment(np.zeros(N, dtype=np.float32), SR)
        start_time = 0.0 + (noise.duration - n / float(SR)) * u          # random.uniform(0.0, d) with random() == u
        starts.append(dict(n=n, N=N, u=u, start=int(round(start_time * SR))))
    white = Recorder(np.random.RandomState(5), 0, [])
    levels = [P.WhiteNoisePerturbation(min_level=-90, max_level=-46, rng=white).perturb(
        S.AudioSegment(np.zeros(8, dtype=np.float32), SR)) for _ in range(4)]
    del levels
    out = dict(sample_rate=SR, signals={k: f32_list(x) for k, x in signals.items()},
               files={k: f32_list(x) for k, x in files.items()}, noise_files=noise_manifest.split(","),
               impulse_files=ir_manifest.split(","), cases=cases, starts=starts,
               white_noise=dict(seed=5, min_level=-90, max_level=-46, draws=white._log),
               perturbation_types=sorted(P.perturbation_types))
    path = os.path.join(HERE, "perturb_draws.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
