"""GPU checks of the split at silences (csrc/trim.hip through the C ABI, audio.split_silence / gather_segments and
VietASR.transcribe_long) against the float64 restatement of tests/split_reference.py.  Every frame and every cut of every table
case is decidable (tests/test_split_host.py), so counts and bounds must EQUAL the restatement's; gathered rows are copies,
compared bit for bit."""
import numpy as np
import pytest
import torch

import split_reference as S
import trim_reference as T

pytestmark = pytest.mark.gpu

NP_DTYPE = {"float32": np.float32, "int16": np.int16}
SENTINEL = -7


def _abi(gpu, batch, lens, top_db, fl, hop, m, M, max_segments=None):
    """batch [B, ld_in] numpy (float32 or int16) through vasr_split_silence_* -> (bounds [B, N, 2], count [B]) on the host; the
    outputs are filled with SENTINEL first"""
    from viet_asr_amd import _lib
    L = _lib.lib()
    B, ld_in = batch.shape
    N = 1 + ld_in // hop if max_segments is None else max_segments
    x = torch.from_numpy(batch).to(gpu)
    ln = torch.tensor(lens, dtype=torch.int64, device=gpu)
    bounds = torch.full((B, max(N, 1), 2), SENTINEL, dtype=torch.int64, device=gpu)
    count = torch.full((B,), SENTINEL, dtype=torch.int64, device=gpu)
    need = int(L.vasr_split_silence_workspace_bytes(B, ld_in, fl, hop))
    assert need > 0
    ws = torch.empty(need + 3, dtype=torch.uint8, device=gpu)[3:]          # any address
    entry = L.vasr_split_silence_pcm16 if batch.dtype == np.int16 else L.vasr_split_silence_f32
    _lib.check(entry(x.data_ptr(), ld_in, ln.data_ptr(), B, float(top_db), fl, hop, m, M, bounds.data_ptr(), N, count.data_ptr(),
                     ws.data_ptr(), need, torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize()
    return bounds.cpu().numpy()[:, :N], count.cpu().numpy()


def _collate(rows, ld_in, dtype, poison=False):
    fill = (32767 if dtype == "int16" else np.nan) if poison else 0
    batch = np.full((len(rows), ld_in), fill, dtype=NP_DTYPE[dtype])
    for b, x in enumerate(rows):
        batch[b, : len(x)] = x
    return batch


def _check(want, bounds, count, names):
    """want: per row the restatement's [(start, end)]"""
    N = bounds.shape[1]
    for b, w in enumerate(want):
        assert int(count[b]) == len(w), (names[b], int(count[b]), len(w))
        k = min(len(w), N)
        assert bounds[b, :k].tolist() == [list(p) for p in w[:k]], names[b]
        assert (bounds[b, k:] == SENTINEL).all(), names[b]                 # nothing is written behind the count


def _ld(cases, layout):
    ld_in = max(1, max(c["n"] for c in cases))
    if layout == "odd_ld":
        ld_in += 1 + ld_in % 2                             # odd: every second row starts off the vector alignment
    return ld_in


@pytest.mark.parametrize("layout", ("same", "odd_ld"))
@pytest.mark.parametrize("dtype", S.DTYPES)
def test_the_whole_table_through_the_c_abi(gpu, dtype, layout):
    for (fl, hop, top_db, _), idx in S.groups().items():
        cases = [S.case(i, dtype) for i in idx]
        ld_in = _ld(cases, layout)
        batch = _collate([c["x"] for c in cases], ld_in, dtype)
        for m, M in S.PAIRS:
            bounds, count = _abi(gpu, batch, [c["n"] for c in cases], top_db, fl, hop, m, M)
            _check([S.expected(i, dtype, m, M) for i in idx], bounds, count, [c["name"] for c in cases])
            assert (count <= 1 + np.array([c["n"] for c in cases]) // hop).all()


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_a_table_smaller_than_the_count_reports_the_total(gpu, dtype):
    for (fl, hop, top_db, long_row), idx in S.groups().items():
        if long_row or top_db != 60.0:
            continue
        cases = [S.case(i, dtype) for i in idx]
        batch = _collate([c["x"] for c in cases], _ld(cases, "same"), dtype)
        for (m, M), cap in (((1, 0), 3), ((1, 2), 50), ((3, 7), 1), ((8, 40), 0)):
            want = [S.expected(i, dtype, m, M) for i in idx]
            assert max(len(w) for w in want) > cap
            bounds, count = _abi(gpu, batch, [c["n"] for c in cases], top_db, fl, hop, m, M, max_segments=cap)
            assert bounds.shape[1] == cap
            _check(want, bounds, count, [c["name"] for c in cases])


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_poison_behind_the_lengths_changes_nothing(gpu, dtype):
    for (fl, hop, top_db, long_row), idx in S.groups().items():
        if long_row:
            continue
        cases = [S.case(i, dtype) for i in idx]
        ld_in = _ld(cases, "odd_ld")
        lens = [c["n"] for c in cases]
        for m, M in ((1, 0), (3, 7)):
            dirty = _abi(gpu, _collate([c["x"] for c in cases], ld_in, dtype, poison=True), lens, top_db, fl, hop, m, M)
            _check([S.expected(i, dtype, m, M) for i in idx], *dirty, [c["name"] for c in cases])
        # lengths beyond the row pitch are clamped to it, negative ones to 0
        wild = [10 ** 12 if b % 2 else -5 for b in range(len(cases))]
        zero = _collate([c["x"] for c in cases], ld_in, dtype)
        bounds, count = _abi(gpu, zero, wild, top_db, fl, hop, 3, 7)
        want = [tuple(S.split(zero[b, : ld_in if b % 2 else 0], top_db, fl, hop, 3, 7)) for b in range(len(cases))]
        _check(want, bounds, count, [c["name"] for c in cases])


def test_a_row_gives_the_same_answer_however_it_is_launched(gpu):
    for dtype in S.DTYPES:
        for fl, hop in S.FORMS:
            picks = [i for i, t in enumerate(S.TABLE) if (t[3], t[4]) == (fl, hop) and t[5] == 60.0 and 1000 <= t[2] <= S.LONG
                     and t[1] in ("pauses", "dips", "inner_gap", "zeros", "sil_speech_sil", "below_amin", "click_last")][:10]
            assert len(picks) == 10
            cases = [S.case(i, dtype) for i in picks]
            for m, M in ((1, 0), (8, 40), (1, 2)):
                want = [S.expected(i, dtype, m, M) for i in picks]
                for b, c in enumerate(cases):             # alone, at the row's own pitch
                    _check([want[b]], *_abi(gpu, _collate([c["x"]], c["n"], dtype), [c["n"]], 60.0, fl, hop, m, M), [c["name"]])
                for size, extra in ((2, 3), (5, 1001)):   # batches of 2 and of 5, at other pitches
                    for lo in range(0, len(cases), size):
                        grp = cases[lo : lo + size]
                        ld = max(c["n"] for c in grp) + extra
                        got = _abi(gpu, _collate([c["x"] for c in grp], ld, dtype), [c["n"] for c in grp], 60.0, fl, hop, m, M)
                        _check(want[lo : lo + size], *got, [c["name"] for c in grp])


# ---- the gather ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("dtype", S.DTYPES)
def test_gather_copies_bit_for_bit_and_refuses_what_lies_outside(gpu, dtype):
    from viet_asr_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    B, ld_in, ld_out = 3, 9001, 4200                      # an odd pitch: rows 1 and 2 start off the vector alignment
    if dtype == "int16":
        src = rng.integers(-32768, 32767, (B, ld_in)).astype(np.int16)
    else:
        src = rng.standard_normal((B, ld_in)).astype(np.float32)
        src[1, 17] = np.nan                               # copied as bits
    #        row start len
    good = [(0, 0, 4200), (0, 4, 4097), (1, 1, 4096), (2, 3, 1), (1, 9000, 1), (2, 4801, 4200), (0, 8, 0), (1, 7, 4099),
            (2, 9001, 0), (0, 16, 4096)]
    bad = [(-1, 0, 10), (3, 0, 10), (0, -1, 10), (0, 0, -1), (0, 9000, 2), (1, 0, 4201), (0, 2 ** 62, 2 ** 62), (2 ** 31 - 1, 0, 1)]
    desc = good + bad
    row = torch.tensor([d[0] for d in desc], dtype=torch.int32, device=gpu)
    start = torch.tensor([d[1] for d in desc], dtype=torch.int64, device=gpu)
    ln = torch.tensor([d[2] for d in desc], dtype=torch.int64, device=gpu)
    x = torch.from_numpy(src).to(gpu)
    out = torch.full((len(desc), ld_out), 77 if dtype == "int16" else float("nan"), dtype=x.dtype, device=gpu)
    entry = L.vasr_gather_segments_pcm16 if dtype == "int16" else L.vasr_gather_segments_f32
    _lib.check(entry(x.data_ptr(), ld_in, B, row.data_ptr(), start.data_ptr(), ln.data_ptr(), len(desc), out.data_ptr(), ld_out,
                     torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s, (r, st, n) in enumerate(desc):
        if s >= len(good):
            n = 0
        assert np.array_equal(_bits(got[s, :n]), _bits(np.ascontiguousarray(src[r, st : st + n]))) if n else True, desc[s]
        assert not _bits(got[s, n:]).any(), desc[s]       # zeros, not NaN / 77, up to ld_out
    # audio.gather_segments: the same rows; width=None takes the longest length
    from viet_asr_amd import audio
    a = audio.gather_segments(x, [d[0] for d in good], [d[1] for d in good], [d[2] for d in good])
    assert a.shape == (len(good), 4200) and a.dtype == x.dtype
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(got[: len(good)]))
    wide = audio.gather_segments(x, row[:3], start[:3], ln[:3], width=5000).cpu().numpy()
    assert wide.shape == (3, 5000) and np.array_equal(_bits(wide[:, :4200]), _bits(got[:3])) and not _bits(wide[:, 4200:]).any()
    assert audio.gather_segments(x, [], [], []).shape[0] == 0


def test_audio_split_silence(gpu):
    from viet_asr_amd import audio
    idx = S.groups()[(2048, 512, 60.0, False)]
    for dtype in S.DTYPES:
        cases = [S.case(i, dtype) for i in idx]
        ld = max(c["n"] for c in cases)
        x = torch.from_numpy(_collate([c["x"] for c in cases], ld, dtype)).to(gpu)
        ln = torch.tensor([c["n"] for c in cases], device=gpu)
        for (m, M), kw in (((1, 0), {}), ((8, 40), dict(min_silence_frames=8, max_segment_frames=40))):
            bounds, count = audio.split_silence(x, ln, **kw)
            assert bounds.shape == (len(cases), 1 + ld // 512, 2) and bounds.dtype == count.dtype == torch.int64
            assert bounds.device == count.device == x.device
            bh, ch = bounds.cpu().numpy(), count.cpu().numpy()
            for b, i in enumerate(idx):
                w = S.expected(i, dtype, m, M)
                assert int(ch[b]) == len(w) and bh[b, : len(w)].tolist() == [list(p) for p in w], cases[b]["name"]
            plan, dropped = audio.plan_segments(bounds, count, ln, 0, 0)
            assert plan == [(b, s, e - s) for b, i in enumerate(idx) for s, e in S.expected(i, dtype, m, M) if e > s]
            assert sum(dropped) == sum(1 for i in idx for s, e in S.expected(i, dtype, m, M) if e == s)
        _, count = audio.split_silence(x, ln, max_segments=0)                 # count only
        assert count.cpu().tolist() == [len(S.expected(i, dtype, 1, 0)) for i in idx]


# ---- end to end: VietASR.transcribe_long ------------------------------------------------------------------------------
RATE, HOP, FL = 16000, 512, 2048
MIN_SILENCE, MAX_SECONDS = 0.3, 3.0
M_FRAMES, MAX_FRAMES = 9, 93                              # floor(0.3 * 16000 / 512), floor(3.0 * 16000 / 512)


def _recording(seed, int16=False):
    """noise bursts and pauses at 16 kHz: a lead of silence, bursts of 1 - 2.4 s, pauses of 0.5 s, one pause of 0.1 s (bridged),
    a burst of 5.4 s with two quieter dips (cut twice under max_seconds = 3), a tail"""
    rng = np.random.default_rng(seed)
    parts = [(0.4, T.SILENCE), (1.3, T.SPEECH), (0.5, T.SILENCE), (1.0, T.SPEECH), (0.1, T.SILENCE), (1.1, T.SPEECH),
             (0.5, T.SILENCE), (2.0, T.SPEECH), (0.2, S.DIP), (1.8, T.SPEECH), (0.2, S.DIP), (1.2, T.SPEECH), (0.6, T.SILENCE),
             (2.4, T.SPEECH), (0.7, T.SILENCE)]
    amp = np.concatenate([np.full(int(round(sec * RATE)), a) for sec, a in parts])
    x = (rng.standard_normal(amp.size) * amp).astype(np.float32)
    return T.to_int16(x) if int16 else x


def _plan(x, pad=FL // 2, min_samples=256):
    """the restatement's plan of one recording: decidable frames and cuts asserted, then split -> audio.plan_segments"""
    from viet_asr_amd import audio
    ratio = T.threshold_ratios(T.frame_energies(x, FL, HOP), 60.0)
    assert np.abs(ratio - 1).min() > T.band(FL)
    segs, _, windows, _ = S.split_frames(x, 60.0, FL, HOP, M_FRAMES, MAX_FRAMES)
    exact = S.sums_exact(x, S.frame_flags(x, 60.0, FL, HOP)[1].max())
    assert all(exact or S.cut_margin(w) > S.CUT_MARGIN for w, _ in windows)
    bounds = S.split(x, 60.0, FL, HOP, M_FRAMES, MAX_FRAMES)
    plan, dropped = audio.plan_segments([bounds], [len(bounds)], [len(x)], pad, min_samples)
    return [(s, n) for _, s, n in plan], dropped[0], len(windows)


def _save(tmp_path, enc_sd, dec_sd, tag):
    enc_p, dec_p = str(tmp_path / f"{tag}-JasperEncoder-STEP-1.pt"), str(tmp_path / f"{tag}-JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in enc_sd.items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in dec_sd.items()}, dec_p)
    return enc_p, dec_p


def _as_float(x):
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x


def _check_long(asr, got, x, align=False):
    plan, dropped, _ = _plan(x)
    assert got["dropped"] == dropped and len(got["segments"]) == len(plan)
    xf = _as_float(x)
    slices = [np.ascontiguousarray(xf[s : s + n]) for s, n in plan]
    texts = [asr.transcribe_batch([c], row_independent=True)[0] for c in slices]
    for seg, (s, n), t in zip(got["segments"], plan, texts):
        assert (seg["start"], seg["end"]) == (s / float(RATE), (s + n) / float(RATE)) and seg["text"] == t
    assert got["text"] == " ".join(t for t in texts if t)
    if align:
        for seg, c in zip(got["segments"], slices):
            want = asr.align([c])[0]
            assert seg["text"] == want["text"]
            for key in ("chars", "words"):
                assert len(seg[key]) == len(want[key])
                for a, w in zip(seg[key], want[key]):
                    assert a["start"] == w["start"] + seg["start"] and a["end"] == w["end"] + seg["start"]
                    assert a.get("char") == w.get("char") and a.get("word") == w.get("word")
    return texts


def test_transcribe_long_end_to_end(gpu, tmp_path):
    from conftest import load_golden
    from viet_asr_amd.infer import VietASR
    _, cfg, _, _, enc_sd, dec_sd = load_golden("vi12x1_b1_tiny")
    assert cfg["AudioToMelSpectrogramPreprocessor"]["sample_rate"] == RATE
    asr = VietASR("quartznet12x1_vi", *_save(tmp_path, enc_sd, dec_sd, "vi"), device="gpu", decoder="greedy")
    x, y = _recording(11), _recording(12)[: 9 * RATE + 77]
    plan, dropped, cuts = _plan(x)
    assert len(plan) == 6 and dropped == 0 and cuts == 2   # 1.3 s | 1.0 + 1.1 s bridged | 5.4 s in three | 2.4 s
    one = asr.transcribe_long(x, max_seconds=MAX_SECONDS)
    texts = _check_long(asr, one, x)
    assert sum(bool(t) for t in texts) >= 2                # the join is of more than one text
    both = asr.transcribe_long([x, y], max_seconds=MAX_SECONDS, batch_size=4)   # a list equals the single calls
    assert both[0] == one and both[1] == asr.transcribe_long(y, max_seconds=MAX_SECONDS)
    _check_long(asr, both[1], y)
    aligned = asr.transcribe_long(x, max_seconds=MAX_SECONDS, align=True)
    _check_long(asr, aligned, x, align=True)
    assert [{k: v for k, v in s.items() if k not in ("chars", "words")} for s in aligned["segments"]] == one["segments"]
    x16 = _recording(13, int16=True)                       # int16 stays int16 on the device; the texts are its float conversion's
    _check_long(asr, asr.transcribe_long(x16, max_seconds=MAX_SECONDS), x16)
    with pytest.raises(ValueError):
        asr.transcribe_long(x, decoder="beam")             # only on an instance built with the beam search


def test_transcribe_long_runs_a_squeeze_and_excitation_model(gpu, tmp_path):
    """nothing in transcribe_long depends on a receptive field: a model forward_long refuses runs"""
    import json
    import os
    import yaml
    from viet_asr_amd import configs, synth
    from viet_asr_amd.infer import VietASR
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "se_nores_k11s2_rows3.npz"))
    jas = json.loads(str(g["definition"]))
    assert any(b.get("se") for b in jas)
    cfg = configs.jasper_definition(jas)
    path = str(tmp_path / "se.yaml")
    with open(path, "w", encoding="utf-8") as f:
        yaml.safe_dump(cfg, f)
    seed = int(g["seed"])
    enc_sd = synth.encoder_state_dict(jas, 64, seed)
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, seed)
    asr = VietASR(path, *_save(tmp_path, enc_sd, dec_sd, "se"), device="gpu", decoder="greedy")
    x = _recording(14)
    _check_long(asr, asr.transcribe_long(x, max_seconds=MAX_SECONDS), x)
    with pytest.raises(NotImplementedError):
        asr._fused_engine().forward_long(torch.from_numpy(x).to(gpu))
