#!/usr/bin/env python3
"""Generate tests/golden/specaug_cases.{npz,json} by running the REAL reference SpecAugment / SpecCutout
(nemo/collections/asr/parts/spectr_augment.py) on the CPU -- dev container only.

    python tests/golden/make_golden_specaug.py     # needs the reference checkout, numpy and torch

The reference module needs only ``random`` and ``torch`` and is loaded from its file.  ``SpectrogramAugmentation``
(audio_preprocessing.py:578-608) composes the two classes in a dozen lines that depend on NeMo's module base; that composition
is restated here around the real classes: the cutout exists only if rect_masks > 0, the augment only if freq_masks + time_masks
> 0, both get the ONE generator, the cutout runs first.  Every case of tests/specaug_reference.CASES runs with
``random.Random(seed)`` on a tensor of ones.  Stored, data only:
  specaug_cases.json   per case its name, kind, constructor arguments, seed, shape, and the SEQUENCE of values the generator
                       handed out while the reference ran (perturb_reference.Recorder): the draw order
                       tests/test_specaug_host.py replays;
  specaug_cases.npz    per case name the resulting mask (output == 0), ``np.packbits`` of its B * D * T bits.
"""
import importlib.util
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from perturb_reference import Recorder  # noqa: E402
from specaug_reference import CASES  # noqa: E402
REF = "/root/reference"


def reference_module():
    path = os.path.join(REF, "nemo", "collections", "asr", "parts", "spectr_augment.py")
    spec = importlib.util.spec_from_file_location("reference_spectr_augment", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def spectrogram_augmentation(SA, rng, freq_masks=0, time_masks=0, freq_width=10, time_width=10, rect_masks=0, rect_time=5,
                             rect_freq=20):
    """audio_preprocessing.py:578-608 around the real classes"""
    cutout = SA.SpecCutout(rect_masks=rect_masks, rect_time=rect_time, rect_freq=rect_freq, rng=rng) if rect_masks > 0 \
        else (lambda x: x)
    augment = SA.SpecAugment(freq_masks=freq_masks, time_masks=time_masks, freq_width=freq_width, time_width=time_width,
                             rng=rng) if freq_masks + time_masks > 0 else (lambda x: x)
    return lambda x: augment(cutout(x))


def main():
    SA = reference_module()
    meta, masks = [], {}
    for c in CASES:
        log = []
        rng = Recorder(random.Random(c["seed"]), 0, log)
        if c["kind"] == "augment":
            run = SA.SpecAugment(rng=rng, **c["args"])
        elif c["kind"] == "cutout":
            run = SA.SpecCutout(rng=rng, **c["args"])
        else:
            run = spectrogram_augmentation(SA, rng, **c["args"])
        x = torch.ones(c["shape"], dtype=torch.float32)
        y = run(x)
        assert bool((x == 1).all()), "the reference modified its input"
        mask = (y == 0).numpy()
        share = mask.reshape(mask.shape[0], -1).mean(axis=1)
        print(f"{c['name']}: {len(log)} draws, masked share per row {np.round(share, 3).tolist()}")
        masks[c["name"]] = np.packbits(mask.reshape(-1))
        meta.append(dict(name=c["name"], kind=c["kind"], args=c["args"], seed=c["seed"], shape=list(c["shape"]), draws=log))
    np.savez_compressed(os.path.join(HERE, "specaug_cases.npz"), **masks)
    with open(os.path.join(HERE, "specaug_cases.json"), "w") as f:
        json.dump(dict(cases=meta), f)
    for name in ("specaug_cases.npz", "specaug_cases.json"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
