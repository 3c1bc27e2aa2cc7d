"""CPU checks of the silence trim: the float64 restatement (tests/trim_reference.py) against closed forms and hand-computed
tiny rows, the mirror against the period formula, the decidability of every frame of every table case, the amin consequence,
the exported symbols / signatures / header declarations with the ABI still 8, every refusal of vasr_trim_silence_* before a
device is touched, the workspace size, audio.trim_silence's refusal of host tensors, the "config" switch and the offset
arithmetic of ``VietASR.align``."""
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import trim_reference as R
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -5


def test_click_cases_in_closed_form():
    """A single 0.9 sample among 8191 zeros: the frames that hold it are non-silent (0.81 / frame_length against amin at
    -60 dB of it: a ratio of 1e6 * 1e-10 * frame_length / 0.81 < 1), the others sit at the amin floor."""
    first, last = np.zeros(8192, np.float32), np.zeros(8192, np.float32)
    first[0], last[-1] = 0.9, 0.9
    # (2048, 512): sample 0 is padded sample 1024, inside frames 0, 1, 2; sample 8191 is 9215, inside frames 14 .. 17, of which
    # 1 + 8192 // 512 = 17 exist (14, 15, 16)
    assert R.trim_bounds(first) == (0, 1536) and R.trim_bounds(last) == (7168, 8192)
    # (64, 16): sample 0 is padded sample 32 (frames 0, 1, 2), sample 8191 is 8223 (frames 510 .. 513 of 0 .. 512)
    assert R.trim_bounds(first, 60.0, 64, 16) == (0, 48) and R.trim_bounds(last, 60.0, 64, 16) == (8160, 8192)
    # (256, 256): one frame per hop, shifted by half a frame: the last sample lies in frame 32 alone, which starts at n
    assert R.trim_bounds(last, 60.0, 256, 256) == (8192, 8192) and R.trim_bounds(first, 60.0, 256, 256) == (0, 256)
    for dtype in R.DTYPES:
        for name, want in (("click_first-n8192-f2048h512-db60", (0, 1536)), ("click_last-n8192-f2048h512-db60", (7168, 8192))):
            c = R.case([t[0] for t in R.TABLE].index(name), dtype)
            assert (c["start"], c["end"]) == want


def test_hand_computed_tiny_rows():
    # n = 1: every padded sample is that sample; 1 frame; kept whole
    assert np.array_equal(R.frame_energies(np.array([0.5], np.float32), 4, 2), [0.25])
    assert R.trim_bounds(np.array([0.5], np.float32), 60.0, 4, 2) == (0, 1)
    # n = 3, frame 4, hop 2: y = [3, 2 | 1, 2, 3 | 2, 1]; frames y[0:4], y[2:6]
    x = np.array([1.0, 2.0, 3.0], np.float32)
    assert np.array_equal(R.frame_energies(x, 4, 2), [(9 + 4 + 1 + 4) / 4, (1 + 4 + 9 + 4) / 4])
    assert R.trim_bounds(x, 60.0, 4, 2) == (0, 3)
    # n = 6, frame 2, hop 2: y = [b | a, b, c, d, e, f | e]; frames (b, a), (b, c), (d, e), (f, e): 1 + 6 // 2 = 4
    x = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0], np.float32)
    assert np.array_equal(R.frame_energies(x, 2, 2), [0.0, 0.0, 0.5, 0.0])
    assert R.trim_bounds(x, 60.0, 2, 2) == (4, 6)                 # frame 2 alone: start 2 * 2, end min(6, 3 * 2)
    x = np.array([0.0, 1.0, 0.0, 0.0, 0.0, 0.0009], np.float32)  # frames (1, 0), (1, 0), (0, 0), (0.0009, 0): the last at -60.9 dB
    assert R.trim_bounds(x, 60.0, 2, 2) == (0, 4) and R.trim_bounds(x, 62.0, 2, 2) == (0, 6)
    # int16 is scaled by 2^-15: y = [0 | 0.5, 0 | 0.5], frames (0, 0.5), (0.5, 0), (0, 0.5)
    assert np.array_equal(R.frame_energies(np.array([16384, 0], np.int16), 2, 1), [0.125, 0.125, 0.125])
    # n == 0, and no frame passing (top_db < 0)
    assert R.trim_bounds(np.zeros(0, np.float32)) == (0, 0) and R.trim_bounds(np.ones(100, np.float32), -1.0, 64, 16) == (0, 0)
    # an inner gap is kept
    x = np.concatenate([np.zeros(64), np.ones(64), np.zeros(640), np.ones(64), np.zeros(64)]).astype(np.float32)
    s, e = R.trim_bounds(x, 60.0, 16, 16)
    # frame f covers samples [16 f - 8, 16 f + 8): the first with a one is frame 4 (56 .. 71), the last frame 52 (824 .. 839)
    assert (s, e) == (4 * 16, 53 * 16)


def test_mirror_is_numpy_reflect():
    for n in (1, 2, 3, 5, 16, 17):
        x = np.arange(n, dtype=np.float64) + 1
        for pad in (0, 1, n - 1, n, 2 * n + 1, 7 * n + 3, 1024):
            want = np.pad(x, pad, mode="reflect")
            got = x[R.mirror_index(np.arange(-pad, n + pad), n)]
            assert np.array_equal(got, want), (n, pad)


def test_every_frame_of_every_case_is_decidable():
    """The condition on the GPU tests: in float32 or float64, in any summation order, in the log or the product form, every frame
    of the table falls on the same side of the threshold."""
    names = [t[0] for t in R.TABLE]
    assert len(set(names)) == len(names)
    for fam in R.NOISE_FAMILIES:
        for n in R.SMALL_LENGTHS:
            assert f"{fam}-n{n}-f64h16-db60" in names
        for n in R.LARGE_LENGTHS:
            assert f"{fam}-n{n}-f2048h512-db60" in names
    assert sum(t[2] == R.LONG_ROW for t in R.TABLE) == 2 and 1 + R.LONG_ROW // 512 > 1024
    assert {t[5] for t in R.TABLE} == {60.0, 20.0, -1.0} and {(t[3], t[4]) for t in R.TABLE} == set(R.FORMS)
    assert sorted(i for g in R.groups().values() for i in set(g)) != [] and set().union(*R.groups().values()) == set(range(len(names)))
    closest, frames = np.inf, 0
    for i, dtype in itertools.product(range(len(R.TABLE)), R.DTYPES):
        c = R.case(i, dtype)
        if c["n"] == 0:
            assert (c["start"], c["end"]) == (0, 0)
            continue
        ratio = R.threshold_ratios(c["mse"], c["top_db"])
        dist = np.abs(ratio - 1.0).min()
        assert dist > R.band(c["frame_length"]), (c["name"], dtype, dist)
        closest, frames = min(closest, dist), frames + ratio.size
        # the product form decides as the log form does
        nz = np.flatnonzero(ratio > 1.0)
        prod = (0, 0) if nz.size == 0 else (int(nz[0]) * c["hop_length"], min(c["n"], (int(nz[-1]) + 1) * c["hop_length"]))
        assert prod == (c["start"], c["end"]), c["name"]
        if c["top_db"] < 0:
            assert prod == (0, 0)
    print(f"{frames} frames, closest ratio to the threshold: |r - 1| = {closest:.3g}; band {R.band(2048):.3g}")
    assert R.band(2048) == (2 * 2048 + 16) * 2.0 ** -24


def test_the_amin_consequence_and_the_kept_loudest_frame():
    names = [t[0] for t in R.TABLE]
    for dtype in R.DTYPES:
        for fam in ("zeros", "below_amin", "below_amin_steps"):
            for (fl, hop), lengths in (((2048, 512), R.LARGE_LENGTHS), ((64, 16), R.SMALL_LENGTHS)):
                for n in lengths:
                    c = R.case(names.index(f"{fam}-n{n}-f{fl}h{hop}-db60"), dtype)
                    assert c["mse"].size == 0 or c["mse"].max() < R.AMIN
                    assert (c["start"], c["end"]) == (0, n)              # the loudest frame is below amin: not trimmed at all
        # frame_length >= 2 hop, top_db = 60: at least min(n, hop) samples are kept
        for i, t in enumerate(R.TABLE):
            c = R.case(i, dtype)
            if t[5] == 60.0 and t[3] >= 2 * t[4]:
                assert c["end"] - c["start"] >= min(c["n"], c["hop_length"]), c["name"]
    gap = R.case(names.index("inner_gap-n18000-f2048h512-db60"), "float32")
    assert gap["start"] == 0 and 9000 + 4500 <= gap["end"] < 18000      # the gap inside is kept, the tail is cut


NAMES = ("vasr_trim_silence_f32", "vasr_trim_silence_pcm16", "vasr_trim_silence_workspace_bytes")


def test_new_symbols_are_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    for n in NAMES:
        assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert len(_lib.SIGNATURES[NAMES[0]][1]) == len(_lib.SIGNATURES[NAMES[1]][1]) == 14 and len(_lib.SIGNATURES[NAMES[2]][1]) == 4
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    for n in NAMES[:2]:
        decl = header[header.index(f" {n}("):]
        assert decl[: decl.index(";")].count(",") == 13
    assert "parity unpinned" in header[header.index("Leading / trailing silence trim"): header.index(f" {NAMES[0]}(")]
    makefile = open(os.path.join(ROOT, "viet-asr_amd", "csrc", "Makefile")).read()
    assert " trim.hip" in makefile


@pytest.mark.parametrize("entry", NAMES[:2])
@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which, entry):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f, size = getattr(L, entry), L.vasr_trim_silence_workspace_bytes
    p, q = 4096, 8192
    ok = dict(x=p, ld=1000, ln=p, b=2, db=60.0, fl=2048, hop=512, out=q, ldo=1000, lno=p, st=p, ws=p, wsb=None)

    def call(**kw):
        a = dict(ok, **kw)
        wsb = a["wsb"] if a["wsb"] is not None else max(size(a["b"], max(a["ld"], 0), a["fl"], a["hop"]), 1)
        return f(a["x"], a["ld"], a["ln"], a["b"], a["db"], a["fl"], a["hop"], a["out"], a["ldo"], a["lno"], a["st"], a["ws"],
                 wsb, None)

    for name in ("x", "ln", "out", "lno", "ws"):
        assert call(**{name: None}) == INVALID, name
    assert call(out=p) == INVALID                                                  # d_out must not alias d_in
    assert call(b=0) == INVALID and call(b=-3) == INVALID
    assert call(ld=-1) == INVALID and call(ldo=-1, ld=0) == INVALID and call(ldo=999) == INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert call(db=bad) == INVALID
    need = size(2, 1000, 2048, 512)
    assert need > 0 and call(wsb=need - 1) == INVALID and call(wsb=0) == INVALID
    assert str(need).encode() in L.vasr_last_error()
    for fl, hop in ((2048, 0), (2048, -512), (2048, 500), (0, 512), (-2048, 512), (8704, 512), (16384, 16384), (512, 1024)):
        assert call(fl=fl, hop=hop) == UNSUPPORTED, (fl, hop)
        assert b"8192" in L.vasr_last_error()
        assert call(fl=fl, hop=hop, b=0) == INVALID and call(fl=fl, hop=hop, ws=None) == INVALID    # an argument error wins
    with pytest.raises(NotImplementedError):
        _lib.check(call(fl=2048, hop=500), L)
    with pytest.raises(ValueError):
        _lib.check(call(b=0), L)


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_workspace_bytes_is_monotone(which):
    from viet_asr_amd import _lib
    size = getattr(_lib, which)().vasr_trim_silence_workspace_bytes
    assert size(0, 10, 64, 16) == size(-1, 10, 64, 16) == size(2, -1, 64, 16) == 0
    assert size(2, 10, 64, 0) == size(2, 10, 60, 16) == size(2, 10, 8704, 512) == size(2, 10, 16, 64) == 0
    batches, lds = (1, 2, 7, 512), (0, 1, 15, 16, 17, 160000, 480000)
    shapes = ((1, 1), (16, 16), (64, 16), (256, 256), (2048, 512), (8192, 512), (8192, 1))      # (frame_length, hop_length)
    for b, ld, (fl, hop) in itertools.product(batches, lds, shapes):
        n = size(b, ld, fl, hop)
        chunks = ld // hop + fl // hop                      # one float64 per hop of the padded row, one int64 per row
        assert b * chunks * 8 + b * 8 <= n <= b * chunks * 8 + b * 8 + 512, (b, ld, fl, hop, n)
    for (b0, ld0), (b1, ld1) in itertools.product(itertools.product(batches, lds), repeat=2):
        if b0 <= b1 and ld0 <= ld1:
            for fl, hop in shapes:
                assert size(b0, ld0, fl, hop) <= size(b1, ld1, fl, hop)
    for b, ld in itertools.product(batches, lds):
        assert size(b, ld, 1024, 512) <= size(b, ld, 2048, 512) <= size(b, ld, 8192, 512)      # growing with frame_length
        assert size(b, ld, 2048, 2048) <= size(b, ld, 2048, 512) <= size(b, ld, 2048, 16)      # and as hop_length shrinks
    assert size(2 ** 31 - 1, 2 ** 62, 8192, 1) == 2 ** 64 - 1                     # what does not fit fits no workspace


def test_audio_trim_silence_refuses_host_tensors():
    from viet_asr_amd import _lib, audio
    with pytest.raises(_lib.VasrError):
        audio.trim_silence(torch.zeros(2, 100), torch.tensor([100, 50]))
    with pytest.raises(_lib.VasrError):
        audio.trim_silence(torch.zeros(2, 100, dtype=torch.int16), torch.tensor([100, 50]))
    assert list(inspect.signature(audio.trim_silence).parameters)[:5] == ["signal", "length", "top_db", "frame_length", "hop_length"]
    d = {k: v.default for k, v in inspect.signature(audio.trim_silence).parameters.items()}
    assert (d["top_db"], d["frame_length"], d["hop_length"]) == (60.0, 2048, 512)


def test_config_switch_and_keywords():
    from viet_asr_amd import configs, engine, infer
    assert infer.resolve_trim_silence("config", configs.builtin("quartznet15x5")) is True
    for name in ("quartznet12x1", "quartznet12x1_vi", "jasper10x5dr"):
        assert infer.resolve_trim_silence("config", configs.builtin(name)) is False
    assert infer.resolve_trim_silence("config", {"labels": []}) is False
    assert infer.resolve_trim_silence("config", {"AudioToTextDataLayer": {"trim_silence": True, "eval": {"shuffle": False}}}) is True
    cfg = configs.builtin("quartznet12x1_vi")
    assert infer.resolve_trim_silence(True, cfg) is True and infer.resolve_trim_silence(False, configs.builtin("quartznet15x5")) is False
    for bad in ("yes", "Config", 2, None):
        with pytest.raises(ValueError):
            infer.resolve_trim_silence(bad, cfg)
    # the keyword exists everywhere the batch path is entered, and defaults to off
    for owner, names in ((engine.QuartzNetCTC, ("forward", "transcribe", "transcribe_beam", "launch")),
                         (engine.QuartzNetClassifier, ("forward", "classify", "classify_topk", "evaluate_manifest")),
                         (infer.VietASR, ("transcribe_batch", "transcribe_manifest", "evaluate_manifest", "score", "align"))):
        for n in names:
            assert inspect.signature(getattr(owner, n)).parameters["trim_silence"].default is False, (owner, n)


def test_offset_arithmetic_of_align():
    from viet_asr_amd.infer import alignment_entries
    chars, start, end, logp = list("ab c"), [0, 3, 5, 9], [2, 5, 7, 12], [-0.5, -0.25, -1.0, -2.0]
    sec, rate, trim_start = 0.02, 16000.0, 7168
    off = trim_start / rate
    plain = alignment_entries(chars, start, end, logp, sec)
    assert plain == alignment_entries(chars, start, end, logp, sec, 0.0)
    moved_c, moved_w = alignment_entries(chars, start, end, logp, sec, off)
    assert off == 0.448
    for a, b in zip(moved_c + moved_w, plain[0] + plain[1]):
        assert a["start"] == b["start"] + off and a["end"] == b["end"] + off and a["logp"] == b["logp"]
        assert a.get("char") == b.get("char") and a.get("word") == b.get("word")
    assert [w["word"] for w in moved_w] == ["ab", "c"] and moved_w[0]["start"] == off and moved_w[1]["end"] == 12 * sec + off
