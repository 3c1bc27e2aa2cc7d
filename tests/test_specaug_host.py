"""CPU checks of SpecAugment / SpecCutout / SpectrogramAugmentation / MultiplyBatch: the host half of the feature masks.  The
draws are held to the REAL reference's (tests/golden/specaug_cases.*, recorded by tests/golden/make_golden_specaug.py): every
golden case must consume exactly the recorded values and rasterise to the stored mask bit for bit.  Then the constructors and
ports, the C ABI's refusals (all before a device is touched) and the exported symbols."""
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

import specaug_reference as R
from perturb_reference import Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -5


def _module(asr, case, rng):
    cls = {"augment": asr.SpecAugment, "cutout": asr.SpecCutout, "both": asr.SpectrogramAugmentation}[case["kind"]]
    return cls(rng=rng, **case["args"])


def _draw(mod, B, D, T):
    """(rects, row_begin) of one forward on [B, D, T], for the two plain classes through their per-row draws"""
    if hasattr(mod, "draw"):
        return mod.draw(B, D, T)
    return R.csr([mod.draw_row(D, T) for _ in range(B)])


@pytest.mark.parametrize("case,mask", R.load_cases(), ids=[c["name"] for c in R.CASES])
def test_draws_and_masks_equal_the_references(case, mask):
    from viet_asr_amd import asr
    log = []
    mod = _module(asr, case, Recorder(random.Random(case["seed"]), 0, log))
    B, D, T = case["shape"]
    rects, row_begin = _draw(mod, B, D, T)
    assert log == case["draws"]                           # the same values in the same order, none more, none fewer
    rects = np.asarray(rects).reshape(-1, 4)
    if len(rects):                                        # what is uploaded is resolved: inside the tensor, half-open
        assert rects.min() >= 0 and (rects[:, 1] <= D).all() and (rects[:, 3] <= T).all()
    got = R.rasterise(rects, row_begin, B, D, T)
    assert got.shape == mask.shape and (got == mask).all()
    assert 0 < mask.sum()                                 # the fixture is not vacuous


def test_golden_cases_are_the_tables_cases():
    got = [(c["name"], c["kind"], c["args"], c["seed"], tuple(c["shape"])) for c, _ in R.load_cases()]
    assert got == [(c["name"], c["kind"], c["args"], c["seed"], tuple(c["shape"])) for c in R.CASES]
    negative = [c for c, _ in R.load_cases() if any(d[2] < 0 for d in c["draws"])]
    assert len(negative) >= 3                             # tensors narrower than a width: negative ranges are in the fixture


def test_row_independent_draws_are_batch_1_draws():
    from viet_asr_amd import asr
    args = dict(freq_masks=1, time_masks=2, rect_masks=3, rect_time=120, rect_freq=50)
    frames = [37, 12, 300]
    rects, begin = asr.SpectrogramAugmentation(rng=random.Random(5), **args).draw(3, 64, 300, row_frames=frames)
    single = asr.SpectrogramAugmentation(rng=random.Random(5), **args)
    for b, t in enumerate(frames):
        r1, b1 = single.draw(1, 64, t)
        assert (rects[begin[b]:begin[b + 1]] == r1).all() and b1.tolist() == [0, len(r1)]
    with pytest.raises(ValueError):
        single.draw(3, 64, 300, row_frames=[1, 2])


def test_constructors_ports_and_exports_are_the_references():
    from viet_asr_amd import asr

    def defaults(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]
    assert defaults(asr.SpecAugment.__init__) == [("freq_masks", 0), ("time_masks", 0), ("freq_width", 10), ("time_width", 10),
                                                  ("rng", None)]
    assert defaults(asr.SpecCutout.__init__) == [("rect_masks", 0), ("rect_time", 5), ("rect_freq", 20), ("rng", None)]
    assert defaults(asr.SpectrogramAugmentation.__init__) == [
        ("freq_masks", 0), ("time_masks", 0), ("freq_width", 10), ("time_width", 10), ("rect_masks", 0), ("rect_time", 5),
        ("rect_freq", 20), ("rng", None)]
    assert defaults(asr.MultiplyBatch.__init__) == [("mult_batch", 1)]
    assert {"SpecAugment", "SpecCutout", "SpectrogramAugmentation", "MultiplyBatch"} <= set(asr.__all__)
    m = asr.SpectrogramAugmentation(rect_masks=5, rect_time=120, rect_freq=50)
    assert list(m.input_ports) == ["input_spec"] and list(m.output_ports) == ["augmented_spec"]
    assert m.input_ports["input_spec"].axes is not None and m.spec_cutout.rect_time == 120
    marker = object()
    assert m.spec_augment(marker) is marker               # a part that does not exist is the identity, as in the reference
    mb = asr.MultiplyBatch(mult_batch=3)
    assert list(mb.input_ports) == ["in_x", "in_x_len", "in_y", "in_y_len"]
    assert list(mb.output_ports) == ["out_x", "out_x_len", "out_y", "out_y_len"]
    # neither part exists without masks: nothing is drawn
    rects, begin = asr.SpectrogramAugmentation(rng=random.Random(1)).draw(2, 64, 10)
    assert rects.shape == (0, 4) and rects.dtype == np.int32 and begin.tolist() == [0, 0, 0] and begin.dtype == np.int32


def test_rng_none_gives_two_independent_generators():
    from viet_asr_amd import asr
    m = asr.SpectrogramAugmentation(freq_masks=1, rect_masks=1)
    assert isinstance(m.spec_cutout._rng, random.Random) and isinstance(m.spec_augment._rng, random.Random)
    assert m.spec_cutout._rng is not m.spec_augment._rng
    shared = random.Random(3)
    m = asr.SpectrogramAugmentation(freq_masks=1, rect_masks=1, rng=shared)
    assert m.spec_cutout._rng is shared and m.spec_augment._rng is shared


def test_multiply_batch_repeats_on_cpu_tensors():
    from viet_asr_amd import asr
    x, xl = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4), torch.tensor([4, 2])
    y, yl = torch.arange(2 * 5).reshape(2, 5), torch.tensor([5, 1])
    ox, oxl, oy, oyl = asr.MultiplyBatch(mult_batch=3).forward(x, xl, y, yl)
    assert ox.shape == (6, 3, 4) and torch.equal(ox, x.repeat(3, 1, 1)) and torch.equal(oxl, xl.repeat(3))
    assert torch.equal(oy, y.repeat(3, 1)) and torch.equal(oyl, yl.repeat(3))


def test_forward_has_no_cpu_fallback():
    from viet_asr_amd import _lib, asr
    x = torch.ones(1, 8, 8)
    for mod in (asr.SpectrogramAugmentation(rect_masks=1), asr.SpecAugment(freq_masks=1), asr.SpecCutout(rect_masks=1)):
        with pytest.raises(_lib.VasrError):
            mod.forward(x)
    assert bool((x == 1).all())


def test_configs_carry_the_shipped_section():
    from viet_asr_amd import configs
    for name in ("quartznet15x5", "quartznet12x1", "quartznet12x1_vi"):
        want = {"rect_masks": 5, "rect_time": 120, "rect_freq": 50}
        assert configs.spectrogram_augmentation(name) == want and configs.builtin(name)["SpectrogramAugmentation"] == want
    assert configs.spectrogram_augmentation("jasper10x5dr") is None
    with pytest.raises(ValueError):
        configs.spectrogram_augmentation("no_such_model")


def test_kernel_constants_are_the_named_ones():
    src = open(os.path.join(ROOT, "viet-asr_amd", "csrc", "vasr_internal.h")).read()
    for name, want in (("kSpecTile", R.TIME_TILE), ("kSpecRows", R.ROW_TILE), ("kSpecChunk", R.RECT_CHUNK)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) == want, name
    widths = {s[2] for s in R.KERNEL_SHAPES}
    assert {R.TIME_TILE - 1, R.TIME_TILE, R.TIME_TILE + 1, R.VEC - 1, R.VEC, R.VEC + 1} <= widths


def test_c_abi_refusals_come_before_a_device_is_touched():
    from viet_asr_amd import _lib
    L = _lib.lib()
    p, q, r = 1 << 20, 1 << 21, 1 << 22                     # stand-ins for device pointers: every refusal comes first
    err = lambda: L.vasr_last_error().decode()
    ok = dict(d_in=p, ld_in=16, d_out=q, ld_out=16, batch=2, feat=4, frames=10, d_rects=r, d_row_begin=r + 4096)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vasr_spec_mask_f32(a["d_in"], a["ld_in"], a["d_out"], a["ld_out"], a["batch"], a["feat"], a["frames"],
                                    a["d_rects"], a["d_row_begin"], None)
    for name in ("d_in", "d_out", "d_rects", "d_row_begin"):
        assert call(**{name: None}) == INVALID and "NULL" in err(), name
    for name in ("batch", "feat", "frames"):
        assert call(**{name: 0}) == INVALID and call(**{name: -1}) == INVALID, name
    assert call(ld_in=9) == INVALID and call(ld_out=9) == INVALID and "ld >= frames" in err()
    assert call(d_in=p + 2) == INVALID and call(d_out=q + 1) == INVALID
    # overlapping without being equal: another pitch at the same pointer, a shifted pointer, the end of one in the other
    size = 4 * ((2 * 4 - 1) * 16 + 10)                      # bytes the tensor spans
    assert call(d_out=p, ld_out=20) == INVALID and "overlap" in err()
    assert call(d_out=p + 4) == INVALID and call(d_out=p + size - 4) == INVALID and call(d_in=q + size - 4) == INVALID
    assert call(frames=2 ** 31 - 1024, ld_in=2 ** 31, ld_out=2 ** 31, d_out=1 << 50) == UNSUPPORTED and "workgroups" in err()
    assert call(frames=2 ** 31 - 1024, ld_in=2 ** 31, ld_out=2 ** 31, d_out=1 << 50, d_rects=None) == INVALID
    assert call(batch=2 ** 20, feat=2 ** 20, d_out=1 << 62) == UNSUPPORTED          # 2^37 workgroups
    # the setter: a handle, and the two pointers together or not at all
    assert L.vasr_set_feature_masks(None, r, r) == INVALID
    h = _lib.Handle(dec_feat_in=1024, num_classes=29)
    try:
        assert L.vasr_set_feature_masks(h.h, r, None) == INVALID and L.vasr_set_feature_masks(h.h, None, r) == INVALID
        assert "together" in err()
        assert L.vasr_set_feature_masks(h.h, r, r + 64) == 0 and L.vasr_set_feature_masks(h.h, None, None) == 0
        h.set_feature_masks(r, r + 64)
        h.set_feature_masks()
        with pytest.raises(ValueError):
            h.set_feature_masks(r, None)
    finally:
        h.close()


def test_symbols_header_and_signatures_agree():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    assert re.search(r"#define VASR_ABI_VERSION 8\b", header) and _lib.lib().vasr_abi_version() == 8
    for name in ("vasr_spec_mask_f32", "vasr_set_feature_masks"):
        decl = re.search(r"VASR_API int %s\(([^;]*)\);" % name, header)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        getattr(_lib.lib(), name)
        getattr(_lib.dev_lib(), name)


def test_engine_and_infer_take_the_argument():
    from viet_asr_amd import engine, infer
    for f in (engine.QuartzNetCTC.forward, engine.QuartzNetCTC.transcribe, engine.QuartzNetCTC.transcribe_beam,
              engine.QuartzNetCTC.launch, engine._Slot.launch, infer.VietASR.transcribe_batch, infer.VietASR.transcribe_manifest,
              infer.VietASR.evaluate_manifest, infer.VietASR.score, infer.VietASR.align):
        assert inspect.signature(f).parameters["spec_augment"].default is None, f.__qualname__
    assert "read-back" in " ".join(engine.QuartzNetCTC.forward.__doc__.split())
    assert hasattr(infer.VietASR, "spectrogram_augmentation")
