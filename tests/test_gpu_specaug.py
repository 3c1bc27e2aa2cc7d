"""GPU checks of the feature masks (SpecAugment / SpecCutout): vasr_spec_mask_f32 in both forms against the numpy rasteriser,
bit for bit, on inputs full of NaN / inf / -0.0 and outputs in NaN guard bands; the modules against the reference's stored
masks; the fused path with masks set against the CPU oracle run on its own features with the same mask applied."""
import json
import random

import numpy as np
import pytest
import torch

import specaug_reference as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc00000          # torch.full(..., nan)
LOGP_TOL, LOGP_REL = 5e-4, 2e-5    # tests/test_gpu_parity.py: the fused path's parity tolerance (logp_tol)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _nan(shape, gpu):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=gpu)


def _tables(B, D, T):
    """the hand-made tables, and the golden cases' own rectangles where the shape is a golden shape"""
    from viet_asr_amd import asr
    tabs = dict(R.rect_tables(B, D, T))
    for c in R.CASES:
        if tuple(c["shape"]) == (B, D, T):
            cls = {"augment": asr.SpecAugment, "cutout": asr.SpecCutout, "both": asr.SpectrogramAugmentation}[c["kind"]]
            mod = cls(rng=random.Random(c["seed"]), **c["args"])
            tabs["golden_" + c["name"]] = mod.draw(B, D, T) if hasattr(mod, "draw") else R.csr([mod.draw_row(D, T) for _ in range(B)])
    return tabs


def _run_both_forms(gpu, B, D, T, ld, rects, row_begin, seed, what):
    """One table through both forms -> asserts.  The input sits in a [B + 2, D, ld] buffer (one guard batch row on each side,
    columns T .. ld behind every row), the out-of-place output in a NaN buffer 4 columns wider."""
    from viet_asr_amd import stages
    want_mask = R.rasterise(rects, row_begin, B, D, T)
    src_bits = R.special_bits((B + 2) * D * ld, seed).reshape(B + 2, D, ld)
    want = src_bits[1:B + 1, :, :T].copy()
    want[want_mask] = 0
    dr, db = stages.upload_masks(rects, row_begin, gpu)
    # out of place
    src = torch.from_numpy(src_bits).to(gpu).view(torch.float32)
    ld_out = ld + 4
    out = _nan((B + 2, D, ld_out), gpu)
    got = stages.spec_mask(src[1:B + 1, :, :T], dr, db, out=out[1:B + 1, :, :T])
    assert got.data_ptr() == out[1:B + 1].data_ptr()
    o = _bits(out)
    assert (o[1:B + 1, :, :T] == want).all(), (what, "out of place")
    assert (o[0] == NAN_BITS).all() and (o[B + 1] == NAN_BITS).all() and (o[:, :, T:] == NAN_BITS).all(), (what, "guard")
    assert (_bits(src) == src_bits).all(), (what, "the input changed")
    # a new contiguous tensor when no `out` is given
    fresh = stages.spec_mask(src[1:B + 1, :, :T], dr, db)
    assert fresh.is_contiguous() and (_bits(fresh) == want).all(), (what, "fresh output")
    # in place: everything outside the rectangles, guard rows and pitch columns included, keeps its bits
    x = src.clone()
    same = stages.spec_mask(x[1:B + 1, :, :T], dr, db, out=x[1:B + 1, :, :T])
    assert same.data_ptr() == x[1:B + 1].data_ptr()
    want_all = src_bits.copy()
    want_all[1:B + 1, :, :T] = want
    assert (_bits(x) == want_all).all(), (what, "in place")


@pytest.mark.parametrize("shape", R.KERNEL_SHAPES, ids=["x".join(map(str, s)) for s in R.KERNEL_SHAPES])
def test_kernel_both_forms_equal_the_rasteriser_bit_for_bit(gpu, shape):
    B, D, T, ld = shape
    for k, (name, (rects, row_begin)) in enumerate(sorted(_tables(B, D, T).items())):
        _run_both_forms(gpu, B, D, T, ld, rects, row_begin, 7 * k + B + D + T, (shape, name))


def test_golden_rectangles_on_their_own_shapes(gpu):
    """(the golden shapes that are not kernel shapes: 2x64x7, 1x5x130, 3x64x300, 4x80x257)"""
    seen = set()
    for c in R.CASES:
        B, D, T = c["shape"]
        if (B, D, T) in seen or any(s[:3] == (B, D, T) for s in R.KERNEL_SHAPES):
            continue
        seen.add((B, D, T))
        for name, (rects, row_begin) in _tables(B, D, T).items():
            if name.startswith("golden_"):
                _run_both_forms(gpu, B, D, T, T, rects, row_begin, T, (c["shape"], name))


def test_rectangles_are_clipped_inside_a_nan_guard_band(gpu):
    """Device rectangles up to 8 cells outside the tensor on every side, applied to a tensor embedded 8 cells deep in NaN: 8
    feature rows in front of the first batch row and behind the last, 8 columns on either side of every row (the pitch).  A
    store outside the tensor lands in the band or in the neighbouring batch row, where the rasteriser expects other bits."""
    from viet_asr_amd import stages
    B, D, T, G = 3, 11, 21, 8
    ld = T + 2 * G
    per_row = [(-8, 3, -8, 3), (D - 2, D + 8, T - 3, T + 8), (-8, D + 8, 5, 6), (2, 3, -8, T + 8), (5, 2, 3, 9), (4, 6, 9, 3),
               (D, D + 8, 0, T), (0, D, T, T + 8), (-8, 0, 0, T), (0, D, -8, 0)]
    tables = {"every row": R.csr([per_row] * B),
              # equal and decreasing row_begin pairs are empty lists; a negative begin too
              "empty pairs": (R.csr([per_row])[0], np.array([0, len(per_row), len(per_row), 3], dtype=np.int32)),
              # (row 0: begin -2, empty; row 1: 0 .. 0, empty; row 2: the first four rectangles, which reach inside)
              "negative begin": (R.csr([per_row])[0], np.array([-2, 0, 0, 4], dtype=np.int32))}
    for name, (rects, row_begin) in tables.items():
        mask = R.rasterise(rects, row_begin, B, D, T)
        assert mask.any() and not mask.all()
        inner_bits = R.special_bits(B * D * T, 5).reshape(B, D, T)
        want = inner_bits.copy()
        want[mask] = 0
        for form in ("in place", "out of place"):
            band = _nan((G + B * D + G, ld), gpu)
            x = band[G:G + B * D].view(B, D, ld)[:, :, G:G + T]
            src = torch.from_numpy(inner_bits).to(gpu).view(torch.float32)
            if form == "in place":
                x.copy_(src)
                stages.spec_mask(x, rects, row_begin, out=x)
            else:
                stages.spec_mask(src, rects, row_begin, out=x)
            got = _bits(band)
            inner = got[G:G + B * D].reshape(B, D, ld)[:, :, G:G + T]
            assert (inner == want).all(), (name, form)
            outside = np.ones(got.shape, dtype=bool)
            outside[G:G + B * D].reshape(B, D, ld)[:, :, G:G + T] = False
            assert (got[outside] == NAN_BITS).all(), (name, form, "the guard band was written")


@pytest.mark.parametrize("case,mask", R.load_cases(), ids=[c["name"] for c in R.CASES])
def test_modules_forward_equals_the_references_masks(gpu, case, mask):
    from viet_asr_amd import asr
    cls = {"augment": asr.SpecAugment, "cutout": asr.SpecCutout, "both": asr.SpectrogramAugmentation}[case["kind"]]
    mod = cls(rng=random.Random(case["seed"]), **case["args"])
    B, D, T = case["shape"]
    bits = R.special_bits(B * D * T, case["seed"]).reshape(B, D, T)
    x = torch.from_numpy(bits).to(gpu).view(torch.float32)
    y = mod.forward(x)
    want = bits.copy()
    want[mask] = 0
    assert y.shape == x.shape and y.data_ptr() != x.data_ptr() and y.is_contiguous()
    assert (_bits(y) == want).all()
    assert (_bits(x) == bits).all()                       # the input tensor is not modified
    for bad in (x.double(), x[:, :, ::2], x[0]):
        with pytest.raises(ValueError):
            mod.forward(bad)


def test_multiply_batch_equals_repeat(gpu):
    from viet_asr_amd import asr
    x = torch.randn(2, 5, 7, device=gpu)
    xl = torch.tensor([7, 4], device=gpu)
    y = torch.randint(0, 9, (2, 6), device=gpu)
    yl = torch.tensor([6, 2], device=gpu)
    ox, oxl, oy, oyl = asr.MultiplyBatch(mult_batch=3).forward(x, xl, y, yl)
    assert torch.equal(ox, x.repeat(3, 1, 1)) and torch.equal(oxl, xl.repeat(3))
    assert torch.equal(oy, y.repeat(3, 1)) and torch.equal(oyl, yl.repeat(3))
    assert ox.device == x.device and ox.shape == (6, 5, 7)


# ---- the fused path ----

SHIPPED = dict(rect_masks=5, rect_time=120, rect_freq=50)
MIXED = dict(freq_masks=2, time_masks=2, freq_width=12, time_width=9, **SHIPPED)


@pytest.fixture(scope="module")
def tiny():
    """the smallest shipped model (QuartzNet 12x1, Vietnamese labels) with synthetic weights, a ragged batch of 4 x about 1 s"""
    from conftest import load_golden, oracle_pre_kwargs
    from viet_asr_amd import synth
    from viet_asr_amd.engine import QuartzNetCTC
    _, cfg, _, _, enc_sd, dec_sd = load_golden("vi12x1_b1_tiny")
    sig, lens = synth.audio_batch(4, 16000, 23, ragged=True)
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd)
    return dict(cfg=cfg, enc_sd=enc_sd, dec_sd=dec_sd, sig=sig, lens=lens, eng=eng, pre=oracle_pre_kwargs(cfg))


def _oracle_masked(tiny, B, seed, args, batch=None):
    """the CPU oracle on its own features with the module's mask applied in numpy -> (sig, lens, logp, pred, mask); batch: (sig,
    lens) in place of the fixture's first B rows"""
    from oracle import quartznet_oracle as O
    from viet_asr_amd import asr
    sig, lens = (tiny["sig"][:B], tiny["lens"][:B]) if batch is None else batch
    L = int(lens.max())
    sig = np.ascontiguousarray(sig[:, :L])
    mel, seq = O.melspec_forward(sig, lens, **tiny["pre"])
    mel = np.array(mel, dtype=np.float32)
    rects, row_begin = asr.SpectrogramAugmentation(rng=random.Random(seed), **args).draw(*mel.shape)
    mask = R.rasterise(rects, row_begin, *mel.shape)
    assert 0.02 < mask.mean() < 0.98
    mel[mask] = 0.0
    enc, _ = O.encoder_forward(mel, seq, tiny["enc_sd"], tiny["cfg"]["JasperEncoder"]["jasper"])
    logp = O.decoder_forward(enc, tiny["dec_sd"])
    return sig, lens, logp.numpy(), O.greedy_argmax(logp).numpy(), mask


def _compare_with_oracle(gpu, tiny, B, seed, args, what, batch=None):
    from viet_asr_amd import asr
    sig, lens, ref_logp, ref_pred, _ = _oracle_masked(tiny, B, seed, args, batch)
    aug = asr.SpectrogramAugmentation(rng=random.Random(seed), **args)
    r = tiny["eng"].forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True, spec_augment=aug)
    torch.cuda.synchronize()
    logp = r["logp"].cpu().numpy()
    err, tol = float(np.abs(logp - ref_logp).max()), max(LOGP_TOL, LOGP_REL * float(np.abs(ref_logp).max()))
    print(f"{what}: log-prob max-abs-err {err:.3e} (tolerance {tol:.3e}, scale {float(np.abs(ref_logp).max()):.1f})")
    assert logp.shape == ref_logp.shape and err <= tol
    assert (r["pred"].cpu().numpy() == ref_pred).all()
    return r


def _assert_same_result(a, b):
    """two results of ``forward(want_logp=True)`` hold the same bits (ids: up to each row's id_len; behind it they are not written)"""
    for k in ("logp", "pred", "id_len", "enc_len"):
        assert torch.equal(a[k], b[k]), k
    for row, n in enumerate(a["id_len"].cpu().tolist()):
        assert torch.equal(a["ids"][row, :n], b["ids"][row, :n]), ("ids", row)


def test_fused_path_with_masks_matches_the_oracle_on_masked_features(gpu, tiny):
    eng = tiny["eng"]
    x, ln = torch.from_numpy(np.ascontiguousarray(tiny["sig"][:3, :int(tiny["lens"][:3].max())])).to(gpu), \
        torch.from_numpy(tiny["lens"][:3]).to(gpu)
    plain = eng.forward(x, ln, want_logp=True)
    masked = _compare_with_oracle(gpu, tiny, 3, 41, MIXED, "B = 3, cutout + augment")           # (a)
    assert not torch.equal(masked["logp"], plain["logp"])                                        # the masks bite
    # (c) the handle's state is cleared: the next unmasked call returns the unmasked bits
    again = eng.forward(x, ln, want_logp=True)
    torch.cuda.synchronize()
    _assert_same_result(again, plain)
    # (b) draws that are all empty: the same bits as the call without the argument
    from viet_asr_amd import asr
    for empty in (asr.SpectrogramAugmentation(rng=random.Random(1)),
                  asr.SpectrogramAugmentation(freq_masks=3, time_masks=3, freq_width=0, time_width=0, rect_masks=2, rect_time=0,
                                              rect_freq=0, rng=random.Random(2))):
        r = eng.forward(x, ln, want_logp=True, spec_augment=empty)
        _assert_same_result(r, plain)
    # the structural acceptance condition: the fused call gains exactly one launch bracket, in the front end's class
    counts = []
    for aug in (None, asr.SpectrogramAugmentation(rng=random.Random(3), **SHIPPED)):
        eng.handle.profile_begin()
        eng.forward(x, ln, spec_augment=aug)
        counts.append({k: v["launches"] for k, v in eng.handle.profile_end().items()})
    assert counts[1]["frontend"] == counts[0]["frontend"] + 1
    assert all(counts[1][k] == counts[0][k] for k in counts[0] if k != "frontend")


def _frontend_brackets(eng, x, ln, aug):
    eng.handle.profile_begin()
    eng.forward(x, ln, spec_augment=aug)
    return eng.handle.profile_end()["frontend"]["launches"]


def test_fused_path_with_masks_and_two_slices(gpu, tiny):
    """(d) as the issue states it, B = 4 -- which the library runs as ONE slice (a slice keeps at least 8 rows) -- and then a batch
    of 16 that really is cut in two: the second slice owns rows 8 .. 15 and must apply THEIR rectangles (row_begin + 8)."""
    from viet_asr_amd import asr, synth
    eng = tiny["eng"]
    sig, lens = synth.audio_batch(16, 8000, 29, ragged=True)
    x, ln = torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu)
    # the rows of the second slice have rectangles of their own: no row's mask equals the mask of the row 8 before it
    mask = _oracle_masked(tiny, 16, 47, MIXED, (sig, lens))[4]
    assert all((mask[b] != mask[b - 8]).any() for b in range(8, 16))
    unsliced = _frontend_brackets(eng, x, ln, asr.SpectrogramAugmentation(rng=random.Random(47), **MIXED))
    eng.handle.set_slices(2)
    try:
        _compare_with_oracle(gpu, tiny, 4, 43, MIXED, "B = 4, set_slices(2)")
        _compare_with_oracle(gpu, tiny, 16, 47, MIXED, "B = 16, two slices", (sig, lens))
        # the call really was sliced: every slice brackets its own front end and its own mask launch
        assert _frontend_brackets(eng, x, ln, asr.SpectrogramAugmentation(rng=random.Random(47), **MIXED)) == 2 * unsliced
        assert _frontend_brackets(eng, x, ln, None) == unsliced
    finally:
        eng.handle.set_slices(1)


def test_row_independent_rows_equal_batch_1_calls(gpu, tiny):
    from viet_asr_amd import asr
    eng = tiny["eng"]                                                                            # (e)
    lens = tiny["lens"][:3]
    sig = np.ascontiguousarray(tiny["sig"][:3, :int(lens.max())])
    x, ln = torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu)
    for host in (lens.tolist(), None):            # lengths known on the host, and read back from the device
        r = eng.forward(x, ln, row_independent=True, spec_augment=asr.SpectrogramAugmentation(rng=random.Random(9), **MIXED),
                        _lengths_host=host)
        single = asr.SpectrogramAugmentation(rng=random.Random(9), **MIXED)
        ids, n = r["ids"].cpu().numpy(), r["id_len"].cpu().numpy()
        for b in range(3):
            one = eng.forward(x[b:b + 1, :int(lens[b])].contiguous(), ln[b:b + 1], spec_augment=single)
            m = int(one["id_len"][0])
            assert m == n[b] and (one["ids"][0, :m].cpu().numpy() == ids[b, :m]).all(), b


def test_evaluate_manifest_takes_spec_augment(gpu, tmp_path, tiny):
    from viet_asr_amd import audio
    from viet_asr_amd.infer import VietASR
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in tiny["enc_sd"].items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in tiny["dec_sd"].items()}, dec_p)
    asr_ = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy")
    sr = 16000
    rows, lines = [], []
    for i, n in enumerate((9000, 12001)):         # ascending durations: the manifest walk's order is the list's
        path = str(tmp_path / f"a{i}.wav")
        audio.write_wav(path, tiny["sig"][i, :n], sr)
        rows.append(audio.read_wav(path)[0])
        lines.append(dict(audio_filepath=path, duration=n / sr, text=["xin chao", "mot hai"][i]))
    man = str(tmp_path / "manifest.json")
    with open(man, "w") as f:
        f.write("\n".join(json.dumps(e) for e in lines) + "\n")
    aug = asr_.spectrogram_augmentation(rng=random.Random(77))
    assert (aug.spec_cutout.rect_masks, aug.spec_cutout.rect_time, aug.spec_cutout.rect_freq) == (5, 120, 50)
    plain_hyps, plain = asr_.evaluate_manifest(man, batch_size=2)
    hyps, res = asr_.evaluate_manifest(man, batch_size=2, spec_augment=aug)
    assert set(res) == set(plain) and res["ref_words"] == plain["ref_words"] and len(hyps) == 2
    assert hyps == asr_.transcribe_batch(rows, row_independent=True, spec_augment=asr_.spectrogram_augmentation(rng=random.Random(77)))
    assert plain_hyps == asr_.transcribe_batch(rows, row_independent=True)
    # the argument reaches the engine through both calls: with it, the one batch brackets one more launch (the mask's)
    handle = asr_._fused_engine().handle

    def brackets(call, **kw):
        handle.profile_begin()
        call(**kw)
        return handle.profile_end()["frontend"]["launches"]
    for call in (lambda **kw: asr_.evaluate_manifest(man, batch_size=2, **kw),
                 lambda **kw: asr_.transcribe_batch(rows, row_independent=True, **kw)):
        assert brackets(call, spec_augment=asr_.spectrogram_augmentation(rng=random.Random(78))) == brackets(call) + 1
