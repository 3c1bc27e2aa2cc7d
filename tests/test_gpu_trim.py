"""GPU checks of the silence trim (csrc/trim.hip through the C ABI, audio.trim_silence, the engines and VietASR.align) against
the float64 restatement of tests/trim_reference.py.  Every frame of every table case is decidable (tests/test_trim_host.py),
so start and length must EQUAL the restatement's and the rows are copies: compared bit for bit."""
import numpy as np
import pytest
import torch

import trim_reference as R

pytestmark = pytest.mark.gpu

NP_DTYPE = {"float32": np.float32, "int16": np.int16}


def _abi(gpu, batch, lens, top_db, fl, hop, ld_out=None, want_start=True):
    """batch [B, ld_in] numpy (float32 or int16) through vasr_trim_silence_* -> (out [B, ld_out], len_out, start) on the host"""
    from viet_asr_amd import _lib
    L = _lib.lib()
    B, ld_in = batch.shape
    ld_out = ld_in if ld_out is None else ld_out
    x = torch.from_numpy(batch).to(gpu)
    ln = torch.tensor(lens, dtype=torch.int64, device=gpu)
    fill = 77 if batch.dtype == np.int16 else float("nan")                # every element must be written
    out = torch.full((B, ld_out), fill, dtype=x.dtype, device=gpu)
    len_out = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    start = torch.full((B,), -7, dtype=torch.int64, device=gpu)
    need = int(L.vasr_trim_silence_workspace_bytes(B, ld_in, fl, hop))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    entry = L.vasr_trim_silence_pcm16 if batch.dtype == np.int16 else L.vasr_trim_silence_f32
    _lib.check(entry(x.data_ptr(), ld_in, ln.data_ptr(), B, float(top_db), fl, hop, out.data_ptr(), ld_out, len_out.data_ptr(),
                     start.data_ptr() if want_start else None, ws.data_ptr(), ws.numel(),
                     torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), len_out.cpu().numpy(), start.cpu().numpy()


def _collate(rows, ld_in, dtype, poison=False):
    fill = (32767 if dtype == "int16" else np.nan) if poison else 0
    batch = np.full((len(rows), ld_in), fill, dtype=NP_DTYPE[dtype])
    for b, x in enumerate(rows):
        batch[b, : len(x)] = x
    return batch


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _check_rows(cases, out, len_out, start, ld_out):
    for b, c in enumerate(cases):
        assert (int(start[b]), int(len_out[b])) == (c["start"], c["end"] - c["start"]), c["name"]
        m = c["end"] - c["start"]
        assert np.array_equal(_bits(out[b, :m]), _bits(np.ascontiguousarray(c["x"][c["start"]:c["end"]]))), c["name"]
        assert not out[b, m:ld_out].any() and not np.isnan(out[b, m:ld_out].astype(np.float64)).any(), c["name"]


LAYOUTS = ("same", "wider_out", "odd_ld")


def _ld(cases, layout):
    ld_in = max(1, max(c["n"] for c in cases))
    if layout == "odd_ld":
        ld_in += 1 + ld_in % 2                           # odd: every second row starts off the vector alignment
    return ld_in, ld_in + 37 if layout == "wider_out" else ld_in


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_the_whole_table_through_the_c_abi(gpu, dtype, layout):
    for (fl, hop, top_db, _), idx in R.groups().items():
        cases = [R.case(i, dtype) for i in idx]
        ld_in, ld_out = _ld(cases, layout)
        batch = _collate([c["x"] for c in cases], ld_in, dtype)
        out, len_out, start = _abi(gpu, batch, [c["n"] for c in cases], top_db, fl, hop, ld_out)
        _check_rows(cases, out, len_out, start, ld_out)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_poison_behind_the_lengths_changes_nothing(gpu, dtype):
    for (fl, hop, top_db, long_row), idx in R.groups().items():
        if long_row:
            continue
        cases = [R.case(i, dtype) for i in idx]
        ld_in, ld_out = _ld(cases, "odd_ld")
        lens = [c["n"] for c in cases]
        clean = _abi(gpu, _collate([c["x"] for c in cases], ld_in, dtype), lens, top_db, fl, hop, ld_out)
        dirty = _abi(gpu, _collate([c["x"] for c in cases], ld_in, dtype, poison=True), lens, top_db, fl, hop, ld_out)
        for a, b in zip(clean, dirty):
            assert np.array_equal(_bits(a), _bits(b))
        _check_rows(cases, *dirty, ld_out)
        # lengths beyond the row pitch are clamped to it, negative ones to 0; d_start may be NULL
        wild = [10 ** 12 if b % 2 else -5 for b in range(len(cases))]
        zero = _collate([c["x"] for c in cases], ld_in, dtype)
        out, len_out, start = _abi(gpu, zero, wild, top_db, fl, hop, ld_out, want_start=False)
        assert (start == -7).all()
        for b in range(len(cases)):
            n = ld_in if b % 2 else 0
            s, e = R.trim_bounds(zero[b, :n], top_db, fl, hop)
            assert int(len_out[b]) == e - s and np.array_equal(_bits(out[b, : e - s]), _bits(zero[b, s:e]))


def test_a_row_gives_the_same_answer_however_it_is_launched(gpu):
    picks = [i for i, t in enumerate(R.TABLE) if t[2] in (1000, 18000, 65, 2049) and t[5] == 60.0 and t[3] != 256]
    for dtype in R.DTYPES:
        for fl, hop in ((2048, 512), (64, 16)):
            cases = [R.case(i, dtype) for i in picks if R.TABLE[i][3] == fl][:10]
            assert len(cases) == 10
            for b, c in enumerate(cases):                 # alone, at the row's own pitch
                out, len_out, start = _abi(gpu, _collate([c["x"]], max(1, c["n"]), dtype), [c["n"]], 60.0, fl, hop)
                _check_rows([c], out, len_out, start, max(1, c["n"]))
            for size, extra in ((2, 3), (5, 1001)):       # batches of 2 and of 5, at other pitches
                for lo in range(0, len(cases), size):
                    grp = cases[lo : lo + size]
                    ld = max(c["n"] for c in grp) + extra
                    out, len_out, start = _abi(gpu, _collate([c["x"] for c in grp], ld, dtype), [c["n"] for c in grp], 60.0, fl, hop)
                    _check_rows(grp, out, len_out, start, ld)


def test_audio_trim_silence(gpu):
    from viet_asr_amd import audio
    idx = R.groups()[(2048, 512, 60.0, False)]
    for dtype in R.DTYPES:
        cases = [R.case(i, dtype) for i in idx]
        ld = max(c["n"] for c in cases)
        x = torch.from_numpy(_collate([c["x"] for c in cases], ld, dtype)).to(gpu)
        out, ln, start = audio.trim_silence(x, torch.tensor([c["n"] for c in cases], device=gpu))
        assert out.shape == x.shape and out.dtype == x.dtype and ln.dtype == start.dtype == torch.int64
        _check_rows(cases, out.cpu().numpy(), ln.cpu().numpy(), start.cpu().numpy(), ld)


# ---- end to end: the engines and VietASR ----------------------------------------------------------------------------
def _clips(seed, n_rows=4, int16=False):
    """rows of silence, noise, silence at 16 kHz with ragged lengths and margins; -> (rows, host-trimmed rows, starts)"""
    rng = np.random.default_rng(seed)
    rows, cut, starts = [], [], []
    for b in range(n_rows):
        lead, body, tail = 1500 + 1900 * b, 9000 + 2500 * b, 700 + 1300 * (n_rows - b)
        amp = np.concatenate([np.full(lead, 1e-5), np.full(body, 0.1), np.full(tail, 1e-5)])
        x = (rng.standard_normal(amp.size) * amp).astype(np.float32)
        if int16:
            x = R.to_int16(x)
        mse = R.frame_energies(x)
        assert np.abs(R.threshold_ratios(mse, 60.0) - 1).min() > R.band(2048)       # decidable
        t, s = R.trim(x)
        assert 0 < s and s + len(t) < len(x)
        rows.append(x), cut.append(np.ascontiguousarray(t)), starts.append(s)
    return rows, cut, starts


def _dev(rows, gpu):
    lens = [len(r) for r in rows]
    batch = np.zeros((len(rows), max(lens)), dtype=rows[0].dtype)
    for b, r in enumerate(rows):
        batch[b, : lens[b]] = r
    return torch.from_numpy(batch).to(gpu), torch.tensor(lens, dtype=torch.int64, device=gpu)


@pytest.fixture(scope="module")
def tiny():
    """the tiny 12x1 configuration with synthetic weights, as the vi12x1_b1_tiny fixture builds them"""
    from conftest import load_golden
    _, cfg, _, _, enc_sd, dec_sd = load_golden("vi12x1_b1_tiny")
    return cfg, enc_sd, dec_sd


def test_forward_and_launch_trim_like_the_host(gpu, tiny):
    from viet_asr_amd.engine import QuartzNetCTC
    cfg, enc_sd, dec_sd = tiny
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    rows, cut, starts = _clips(5)
    got = eng.forward(*_dev(rows, gpu), trim_silence=True, row_independent=True, want_logp=True)
    want = eng.forward(*_dev(cut, gpu), row_independent=True, want_logp=True)
    torch.cuda.synchronize()
    assert got["trim_start"].cpu().tolist() == starts
    assert got["length"].cpu().tolist() == [len(c) for c in cut]
    n = want["id_len"].cpu().numpy()
    assert np.array_equal(got["id_len"].cpu().numpy(), n)
    assert np.array_equal(got["enc_len"].cpu().numpy(), want["enc_len"].cpu().numpy())
    gi, wi, gl, wl = (t.cpu().numpy() for t in (got["ids"], want["ids"], got["logp"], want["logp"]))
    for b in range(len(rows)):
        t1 = eng.frames(len(cut[b]))[1]                   # the row's own encoded frames: what a batch-1 call returns
        assert np.array_equal(gi[b, : n[b]], wi[b, : n[b]])
        assert np.array_equal(gl[b, :t1].view(np.int32), wl[b, :t1].view(np.int32))
    texts = eng.texts(want["ids"], want["id_len"])
    assert eng.launch(rows, row_independent=True, trim_silence=True).texts() == texts
    assert eng.transcribe(rows, row_independent=True, trim_silence=True) == texts
    rows16, cut16, _ = _clips(6, int16=True)
    assert eng.launch(rows16, row_independent=True, trim_silence=True).texts() == eng.launch(cut16, row_independent=True).texts()
    assert eng.launch(rows, row_independent=True).texts() == eng.transcribe(rows, row_independent=True)   # the default: untrimmed


def test_frames_of_and_frame_seconds_follow_the_library(gpu, tiny):
    """``frames_of`` -- the frames of trimmed rows, whose lengths exist on the device only -- is the library's own chain
    (vasr_mel_frames, vasr_encoded_frames), and ``frame_seconds`` divides by the same stride product.  No launch beyond the
    engine's construction."""
    from viet_asr_amd import geometry
    from viet_asr_amd.engine import QuartzNetCTC, blocks_from_config
    cfg, enc_sd, dec_sd = tiny
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd, device=gpu)
    ns = [257, 319, 320, 321, 16000, 160077]
    got = eng.frames_of(torch.tensor(ns))
    assert got.dtype == torch.int32
    assert got.tolist() == [eng.handle.encoded_frames(eng.handle.mel_frames(n)) for n in ns]
    pre = cfg["AudioToMelSpectrogramPreprocessor"]
    hop = int(round(pre["window_stride"] * pre["sample_rate"]))
    stride = geometry.stride_product(blocks_from_config(cfg["JasperEncoder"]["jasper"]))
    assert (hop, stride) == (160, 2)
    assert eng.frame_seconds() == hop * stride / pre["sample_rate"]


def test_align_reports_times_of_the_recording_it_was_given(gpu, tiny, tmp_path):
    from viet_asr_amd.infer import VietASR
    cfg, enc_sd, dec_sd = tiny
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in enc_sd.items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in dec_sd.items()}, dec_p)
    asr = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy")
    rows, cut, starts = _clips(7, n_rows=3)
    rate = cfg["AudioToMelSpectrogramPreprocessor"]["sample_rate"]
    got = asr.align(rows, trim_silence=True)
    want = asr.align(cut)
    for b, (g, w) in enumerate(zip(got, want)):
        off = starts[b] / rate
        assert g["offset"] == off and g["text"] == w["text"] and g["score"] == w["score"]
        assert len(g["chars"]) == len(w["chars"]) and len(g["words"]) == len(w["words"])
        for key in ("chars", "words"):
            for a, c in zip(g[key], w[key]):
                assert a["start"] == c["start"] + off and a["end"] == c["end"] + off and a["logp"] == c["logp"]
    assert asr.transcribe_batch(rows, row_independent=True, trim_silence=True) == asr.transcribe_batch(cut, row_independent=True)
    assert asr.score(rows, [w["text"] for w in want], trim_silence=True) == asr.score(cut, [w["text"] for w in want])
    # "config" follows the model definition's data layer section: the 12x1 YAML does not trim
    assert asr.transcribe_batch(rows, row_independent=True, trim_silence="config") == asr.transcribe_batch(rows, row_independent=True)


def test_classifier_trims_like_the_host(gpu, tiny):
    from viet_asr_amd import synth
    from viet_asr_amd.engine import QuartzNetClassifier
    cfg, enc_sd, _ = tiny
    rng = np.random.default_rng(3)
    feat = cfg["JasperEncoder"]["jasper"][-1]["filters"]
    dec_sd = {"decoder_layers.0.weight": (rng.standard_normal((7, feat)) / np.sqrt(feat)).astype(np.float32),
              "decoder_layers.0.bias": rng.standard_normal(7).astype(np.float32)}
    clf = QuartzNetClassifier(cfg, enc_sd, dec_sd, audio_length=256, device=gpu)    # wider than every clip: no random crop
    rows, cut, _ = _clips(8)
    assert clf.classify(rows, row_independent=True, trim_silence=True) == clf.classify(cut, row_independent=True)
    got = clf.classify_topk(rows, 3, row_independent=True, trim_silence=True)
    assert got == clf.classify_topk(cut, 3, row_independent=True)
    x, ln = _dev(rows, gpu)
    a = clf.forward(x, ln, row_independent=True, trim_silence=True)
    b = clf.forward(*_dev(cut, gpu), row_independent=True)
    assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
