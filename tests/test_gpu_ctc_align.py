"""GPU checks of the forced CTC alignment (csrc/ctc_align.hip through stages.ctc_align, the C ABI and VietASR.align) against
the float32 restatement in the kernel's order -- BIT FOR BIT in score, path, spans and token sums --, the float64 restatement
and its bound, and the path validator (tests/ctc_align_reference.py).  Every test checks a value."""
import math
import os
import re

import numpy as np
import pytest
import torch

import ctc_align_reference as AR
import ctc_reference as CR
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _constants():
    src = open(os.path.join(ROOT, "viet-asr_amd", "csrc", "vasr_internal.h")).read()
    return {k: int(v) for k, v in re.findall(r"constexpr int (kCtc\w+) = (\d+);", src)}


K = _constants()
LANES, NARROW_SLOTS, MAX_WIDTH = K["kCtcLossLanes"], K["kCtcLossNarrowSlots"], K["kCtcLossMaxWidth"]
NARROW_MAX_WIDTH = (LANES * NARROW_SLOTS - 1) // 2          # 511: S = 1023
BLOCK_NARROW, BLOCK_WIDE = K["kCtcAlignNarrowBlock"], K["kCtcAlignWideBlock"]   # frames per staged block of the back-trace
KEYS = ("score", "start", "end", "token_logp", "path")


def device_align(gpu, logp, frames, tgt, tgt_len, blank, want_path=True):
    from viet_asr_amd import stages
    out = stages.ctc_align(torch.from_numpy(np.ascontiguousarray(logp)).to(gpu), torch.as_tensor(np.asarray(frames)).to(gpu),
                           torch.from_numpy(np.ascontiguousarray(tgt)).to(gpu), torch.as_tensor(np.asarray(tgt_len)).to(gpu), blank,
                           want_path=want_path)
    assert sorted(out) == sorted(KEYS if want_path else KEYS[:4])
    assert all(v.device.type == "cuda" and not v.requires_grad for v in out.values())
    assert out["score"].dtype == out["token_logp"].dtype == torch.float32 and out["start"].dtype == out["end"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in out.items()}


def log_softmax_rows(rng, shape, scale=1.0):
    """seeded log-softmax rows without subnormal values (the float32 restatement is bit-exact on normal numbers)"""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    logp = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
    assert np.isfinite(logp).all() and (np.abs(logp[logp != 0]) >= np.finfo(np.float32).tiny).all()
    return logp


def make_rows(rng, lengths, C, extra=3, scale=1.0, repeats=0.2, width=None, frames_pad=0):
    """One ragged batch: row b has lengths[b] ids below C - 1 (a share of equal neighbours) and the fewest frames with a path
    + extra (a list gives one per row); finite log-probs and valid ids everywhere."""
    B, W = len(lengths), width or max(max(lengths), 1)
    tgt = rng.integers(0, C - 1, (B, W)).astype(np.int64)
    for b, L in enumerate(lengths):
        for i in range(1, L):
            if rng.random() < repeats:
                tgt[b, i] = tgt[b, i - 1]
            elif tgt[b, i] == tgt[b, i - 1]:
                tgt[b, i] = (tgt[b, i] + 1) % (C - 1)
    extra = extra if isinstance(extra, (list, tuple)) else [extra] * B
    tgt_len = np.array(lengths, dtype=np.int64)
    frames = np.array([AR.min_frames(tgt[b], L) + x for (b, L), x in zip(enumerate(lengths), extra)], dtype=np.int64)
    return log_softmax_rows(rng, (B, int(frames.max()) + frames_pad, C), scale), frames, tgt, tgt_len


def check_rows(got, logp, frames, tgt, tgt_len, blank, tag=None):
    """every row of a device result against the two restatements -> the number of rows that have a path"""
    paths = 0
    for b in range(len(frames)):
        r32 = AR.align32(logp[b], frames[b], tgt[b], tgt_len[b], blank)
        r64 = AR.align64(logp[b], frames[b], tgt[b], tgt_len[b], blank)
        bound = AR.bound(r64)
        print(tag, b, float(got["score"][b]), float(r32["score"]), float(r64["score"]), bound)
        for k in KEYS:
            assert got[k][b].dtype == r32[k].dtype and got[k][b].tobytes() == r32[k].tobytes(), (tag, b, k, got[k][b], r32[k])
        assert AR.close(got["score"][b], r64["score"], bound), (tag, b, float(got["score"][b]), float(r64["score"]), bound)
        if np.isfinite(r64["score"]) and min(int(frames[b]), logp.shape[1]) > 0:
            AR.validate(got["path"][b], got["start"][b], got["end"][b], frames[b], tgt[b], tgt_len[b])
            own = AR.path_score64(logp[b], got["path"][b], frames[b], tgt[b], blank)
            assert own >= float(r64["score"]) - 2 * bound, (tag, b, own, float(r64["score"]), bound)
            paths += 1
        else:
            assert (got["path"][b] == -1).all() and (got["start"][b] == -1).all() and (got["end"][b] == -1).all()
            assert got["token_logp"][b].tobytes() == np.zeros_like(got["token_logp"][b]).tobytes()        # +0.0f
    return paths


def single_path_rows(rng, C, T, y, keep=True):
    """log-probs [T][C] whose -inf entries leave exactly one path of y (every frame has one finite class: a frame labelling
    that collapses to y has one state path), or none (keep=False: one frame is -inf throughout)"""
    L = len(y)
    cuts = np.sort(rng.choice(np.arange(1, T), 2 * L, replace=False)) if L else np.array([], dtype=int)
    lab = np.full(T, C - 1)
    for j in range(L):                                   # token j on [cuts[2j], cuts[2j+1]): a blank before every token
        lab[cuts[2 * j] : cuts[2 * j + 1]] = y[j]
    lp = log_softmax_rows(rng, (T, C))
    mask = np.ones((T, C), dtype=bool)
    mask[np.arange(T), lab] = False
    lp[mask] = -np.inf
    if not keep:
        lp[T // 2] = -np.inf
    return lp, lab


def case_short(rng):
    """T = 1 .. 7, odd and even around the double buffer, with 0, 1 and 2 ids"""
    C = 5
    tgt = np.array([[0, 0], [1, 0], [2, 0], [0, 1], [3, 0], [2, 2], [1, 3], [0, 0], [2, 1], [3, 3], [1, 2]], dtype=np.int64)
    tgt_len = np.array([0, 1, 1, 2, 1, 2, 2, 0, 2, 2, 1], dtype=np.int64)
    frames = np.array([1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7], dtype=np.int64)
    return log_softmax_rows(rng, (len(frames), 7, C)), frames, tgt, tgt_len, C - 1


def case_min_frames(rng):
    """T == min_frames: the unique path, with repeated labels"""
    return make_rows(rng, [5, 40, 130, 2], 6, extra=0, repeats=0.4) + (5,)


def case_empty_targets(rng):
    logp, frames, tgt, tgt_len = make_rows(rng, [0, 0, 0], 4, extra=[1, 7, 70])
    return logp, frames, tgt, tgt_len, 3


def case_lane_wrap(rng):
    """L = 127, 128: S = 255 / 257, the wrap from slot 0 to slot 1, with T = L + 3"""
    return make_rows(rng, [LANES // 2 - 1, LANES // 2], 7, extra=3, repeats=0.0) + (6,)


def case_width_511(rng):
    return make_rows(rng, [NARROW_MAX_WIDTH, 17], 8, extra=3) + (7,)


def case_width_512(rng):
    return make_rows(rng, [NARROW_MAX_WIDTH + 1, 17], 8, extra=3) + (7,)


def case_widest(rng):
    """the wide form at L = 4096, T = 4100, C = 4: state 8192, the one state of slot 32"""
    return make_rows(rng, [MAX_WIDTH], 4, extra=4, repeats=0.0) + (3,)


def case_blocks_narrow(rng):
    """T at one, two and three back-trace blocks and one frame either side"""
    ts = [k * BLOCK_NARROW + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    return make_rows(rng, [20] * len(ts), 6, extra=[t - 20 for t in ts], repeats=0.0) + (5,)


def case_blocks_wide(rng):
    ts = [k * BLOCK_WIDE + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    return make_rows(rng, [9] * len(ts), 6, extra=[t - 9 for t in ts], repeats=0.0, width=NARROW_MAX_WIDTH + 1) + (5,)


def case_ties(rng):
    """all-equal log-probs: the tie-break decides the entire path, in both forms"""
    logp, frames, tgt, tgt_len = make_rows(rng, [5, 12, 0, 1], 5, extra=[15, 3, 9, 30], repeats=0.3)
    logp[:] = np.float32(-math.log(5))
    return logp, frames, tgt, tgt_len, 4


def case_ties_wide(rng):
    logp, frames, tgt, tgt_len = make_rows(rng, [5, 300], 5, extra=[15, 40], repeats=0.3, width=600)
    logp[:] = np.float32(-0.75)
    return logp, frames, tgt, tgt_len, 4


def case_neg_inf(rng):
    """-inf entries that leave exactly one path (rows 0, 1) and none (rows 2, 3)"""
    C, T = 6, 40
    ys = [np.array([0, 1, 1, 2, 4]), np.array([3]), np.array([0, 1, 1, 2, 4]), np.array([], dtype=np.int64)]
    rows = [single_path_rows(rng, C, T, y, keep=b < 2)[0] for b, y in enumerate(ys)]
    tgt = np.zeros((4, 5), dtype=np.int64)
    for b, y in enumerate(ys):
        tgt[b, : len(y)] = y
    return np.stack(rows), np.full(4, T, dtype=np.int64), tgt, np.array([len(y) for y in ys], dtype=np.int64), C - 1


def case_ragged(rng):
    """every convention in one batch: NaN rows, rows without a path, empty rows, next to ordinary ones; frames and tgt_width
    larger than any row needs"""
    C = 6
    logp, frames, tgt, tgt_len = make_rows(rng, [30, 4, 4, 4, 4, 4, 0, 2, 0, 4, 12], C, extra=9, width=40, frames_pad=6)
    T = logp.shape[1]
    tgt[:, :4][1:6] = np.array([0, 1, 1, 2])
    tgt[9, :4] = np.array([0, 1, 1, 2])
    frames = np.array([frames[0], -1, T, T, T, T, 0, 0, 20, 4, 10 ** 6], dtype=np.int64)
    tgt_len = np.array([30, 4, -3, 4, 4, 4, 0, 2, 0, 4, 12], dtype=np.int64)
    tgt[3, 2] = C - 1              # the blank inside the length
    tgt[4, 0] = C                  # out of range
    tgt[5, 3] = -1
    return logp, frames, tgt, tgt_len, C - 1           # row 9: 4 ids with a repeat in 4 frames: no path; row 10: clamped


CASES = {"short": (case_short, 11), "min_frames": (case_min_frames, 4), "empty_targets": (case_empty_targets, 3),
         "lane_wrap": (case_lane_wrap, 2), "width_511": (case_width_511, 2), "width_512": (case_width_512, 2),
         "widest": (case_widest, 1), "blocks_narrow": (case_blocks_narrow, 9), "blocks_wide": (case_blocks_wide, 9),
         "ties": (case_ties, 4), "ties_wide": (case_ties_wide, 2), "neg_inf": (case_neg_inf, 2), "ragged": (case_ragged, 3)}


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_float32_restatement_bit_for_bit(gpu, name):
    make, want_paths = CASES[name]
    logp, frames, tgt, tgt_len, blank = make(np.random.default_rng(len(name) + 100))
    got = device_align(gpu, logp, frames, tgt, tgt_len, blank)
    assert check_rows(got, logp, frames, tgt, tgt_len, blank, name) == want_paths
    if name == "min_frames":                             # the unique path: the best path is the sum over paths
        for b in range(len(frames)):
            l64 = CR.loss64(logp[b], frames[b], tgt[b], tgt_len[b], blank)
            assert abs(float(got["score"][b]) + l64) <= AR.bound(AR.align64(logp[b], frames[b], tgt[b], tgt_len[b], blank)) + 1e-12
    if name == "neg_inf":
        rng = np.random.default_rng(len(name) + 100)
        lab = single_path_rows(rng, 6, 40, np.array([0, 1, 1, 2, 4]))[1]
        emitted = np.where(got["path"][0] & 1, tgt[0][np.minimum(got["path"][0] >> 1, 4)], blank)
        assert (emitted == lab).all() and np.isneginf(got["score"][2:]).all()
    if name == "ragged":
        assert np.isnan(got["score"][[1, 2, 3, 4, 5]]).all() and got["score"][6] == 0.0 and np.isneginf(got["score"][[7, 9]]).all()
        assert (got["path"][8][:20] == 0).all() and (got["path"][8][20:] == -1).all()


def _row_bytes(got, b, T, L):
    return (got["score"][b].tobytes(), got["path"][b][:T].tobytes(), got["start"][b][:L].tobytes(), got["end"][b][:L].tobytes(),
            got["token_logp"][b][:L].tobytes())


def test_a_row_gives_the_same_bits_however_it_is_launched(gpu):
    rng = np.random.default_rng(21)
    C, L = 9, 200
    logp, frames, tgt, tgt_len = make_rows(rng, [L, 3, 50, 0, 77, 120, 9], C, extra=25, width=300)
    T = int(frames[0])
    alone = device_align(gpu, logp[:1, :T], frames[:1], tgt[:1, :L], tgt_len[:1], C - 1)
    assert np.isfinite(alone["score"]).all()
    want = _row_bytes(alone, 0, T, L)
    order = [4, 2, 0, 6, 1, 5, 3]
    batch = device_align(gpu, logp[order], frames[order], tgt[order], tgt_len[order], C - 1)        # inside a batch of 7
    assert _row_bytes(batch, 2, T, L) == want
    long = np.concatenate([logp[:1], log_softmax_rows(rng, (1, 37, C))], axis=1)                     # frames and tgt_width padded
    wider = np.concatenate([tgt[:1], np.full((1, 100), 3, dtype=np.int64)], axis=1)
    assert wider.shape[1] == 400 and _row_bytes(device_align(gpu, long, frames[:1], wider, tgt_len[:1], C - 1), 0, T, L) == want
    wide = np.zeros((1, 600), dtype=np.int64)                                                        # the other instantiation
    wide[:, :300] = tgt[:1]
    assert 2 * 300 + 1 <= LANES * NARROW_SLOTS < 2 * 600 + 1
    assert _row_bytes(device_align(gpu, logp[:1], frames[:1], wide, tgt_len[:1], C - 1), 0, T, L) == want


def raw_align(gpu, logp, frames, tgt, tgt_len, blank, tok=True, path=True, sentinel=-77):
    """the C ABI itself, on outputs pre-filled with a sentinel -> the outputs as numpy arrays"""
    from viet_asr_amd import _lib
    x = torch.from_numpy(np.ascontiguousarray(logp)).to(gpu)
    fr, tl = (torch.as_tensor(np.asarray(v)).to(gpu).to(torch.int32) for v in (frames, tgt_len))
    y = torch.from_numpy(np.ascontiguousarray(tgt)).to(gpu).to(torch.int32)
    B, T, Cn = x.shape
    W = y.shape[1]
    full = lambda shape, dtype: torch.full(shape, sentinel, dtype=dtype, device=gpu)  # noqa: E731
    out = {"score": full((B,), torch.float32), "start": full((B, W), torch.int32), "end": full((B, W), torch.int32)}
    if tok:
        out["token_logp"] = full((B, W), torch.float32)
    if path:
        out["path"] = full((B, T), torch.int32)
    L = _lib.lib()
    n = L.vasr_ctc_align_workspace_bytes(B, T, W)
    ws = torch.empty(n, dtype=torch.uint8, device=gpu)
    with torch.cuda.device(x.device):
        _lib.check(L.vasr_ctc_align_f32(x.data_ptr(), fr.data_ptr(), B, T, Cn, blank, y.data_ptr(), W, tl.data_ptr(),
                                        out["score"].data_ptr(), out["start"].data_ptr(), out["end"].data_ptr(),
                                        out["token_logp"].data_ptr() if tok else None, out["path"].data_ptr() if path else None,
                                        ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_poison_behind_the_lengths_changes_nothing_and_every_element_is_written(gpu):
    rng = np.random.default_rng(22)
    for width in (40, 600):                                             # both forms
        logp, frames, tgt, tgt_len, blank = case_ragged(rng)
        if width > tgt.shape[1]:
            tgt = np.concatenate([tgt, np.zeros((tgt.shape[0], width - tgt.shape[1]), dtype=np.int64)], axis=1)
        clean = raw_align(gpu, logp, frames, tgt, tgt_len, blank)
        for k, v in clean.items():
            assert not (v == -77).any(), k                               # every element of every output was written
        check_rows(clean, logp, frames, tgt, tgt_len, blank, f"clean{width}")
        bad_logp, bad_tgt = logp.copy(), tgt.copy()
        for b in range(len(frames)):
            T, L = min(max(int(frames[b]), 0), logp.shape[1]), min(max(int(tgt_len[b]), 0), tgt.shape[1])
            bad_logp[b, T:] = np.nan
            bad_tgt[b, L:] = (10 ** 6, -7)[b % 2]
        poisoned = raw_align(gpu, bad_logp, frames, bad_tgt, tgt_len, blank)
        for k in KEYS:
            assert poisoned[k].tobytes() == clean[k].tobytes(), (width, k)


def test_optional_outputs_do_not_change_the_others(gpu):
    rng = np.random.default_rng(23)
    logp, frames, tgt, tgt_len, blank = case_ragged(rng)
    full = device_align(gpu, logp, frames, tgt, tgt_len, blank)
    part = device_align(gpu, logp, frames, tgt, tgt_len, blank, want_path=False)
    for k in KEYS[:4]:
        assert part[k].tobytes() == full[k].tobytes(), k
    for tok, path in ((False, True), (False, False)):
        raw = raw_align(gpu, logp, frames, tgt, tgt_len, blank, tok=tok, path=path)
        assert sorted(raw) == sorted(k for k in KEYS if (k != "token_logp" or tok) and (k != "path" or path))
        for k in raw:
            assert raw[k].tobytes() == full[k].tobytes(), (tok, path, k)
    # frames == 0 and tgt_width == 0 are legal shapes
    from viet_asr_amd import stages
    z = stages.ctc_align(torch.zeros(2, 0, 6, device=gpu), torch.tensor([0, 0], device=gpu),
                         torch.zeros(2, 0, dtype=torch.int64, device=gpu), torch.tensor([0, 0], device=gpu), 5, want_path=True)
    assert z["score"].cpu().tolist() == [0.0, 0.0] and z["path"].shape == (2, 0) and z["start"].shape == (2, 0)
    with pytest.raises(NotImplementedError):
        stages.ctc_align(torch.zeros(1, 4, 3, device=gpu), torch.tensor([4], device=gpu),
                         torch.zeros(1, MAX_WIDTH + 1, dtype=torch.int64, device=gpu), torch.tensor([2], device=gpu), 2)


def test_align_end_to_end(gpu, tmp_path):
    """On generated signals and the smallest model (as tests/test_gpu_ctc.py builds them): the alignment of a row's own
    greedy transcript is the run structure of the per-frame argmax, words tile their characters, a given text scores no more
    than ``score``, and a text longer than the frames has no path."""
    from viet_asr_amd import configs, synth
    from viet_asr_amd.infer import VietASR
    cfg = configs.builtin("quartznet12x1_vi")
    labels = cfg["labels"]
    jas = cfg["JasperEncoder"]["jasper"]
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in synth.encoder_state_dict(jas, 64, 3).items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in synth.decoder_state_dict(1024, len(labels) + 1, 3).items()}, dec_p)
    asr = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy")
    rng = np.random.default_rng(8)
    lens = [9000, 31000, 16000, 4000, 25000]
    sigs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    eng = asr._fused_engine()
    sec = eng.frame_seconds()
    assert all(abs(eng.frames(n)[1] * sec - n / 16000.0) <= 2 * sec for n in lens)       # frames x seconds per frame = the audio
    own = asr.transcribe_batch(sigs, row_independent=True)
    rows = asr.align(sigs)
    assert [r["text"] for r in rows] == own
    r, frames = asr._forward_logp(sigs, True)
    logp, frames, blank = r["logp"].cpu().numpy(), frames.cpu().numpy(), len(labels)
    left_out = 0
    for b, row in enumerate(rows):
        T = int(frames[b])
        lp = logp[b, :T]
        top = np.sort(lp, axis=1)
        if not (top[:, -1] > top[:, -2]).all():
            left_out += 1
            continue
        k = lp.argmax(axis=1)
        runs, prev = [], blank                          # (label, first frame, last frame + 1) of every run of a non-blank argmax
        for t, c in enumerate(k):
            if c != blank and c != prev:
                runs.append([int(c), t, t + 1])
            elif c != blank:
                runs[-1][2] = t + 1
            prev = c
        assert "".join(labels[c] for c, _, _ in runs) == row["text"] and len(row["chars"]) == len(runs)
        for ch, (c, t0, t1) in zip(row["chars"], runs):
            assert ch["char"] == labels[c] and ch["start"] == t0 * sec and ch["end"] == t1 * sec
            assert abs(ch["logp"] - float(lp[t0:t1, c].astype(np.float64).sum())) <= CR.U * (t1 - t0) * abs(ch["logp"]) + 1e-12
        ids = np.array([c for c, _, _ in runs] or [0], dtype=np.int64)
        bound = AR.bound(AR.align64(lp, T, ids, len(runs), blank))
        best = float(lp.max(axis=1).astype(np.float64).sum())
        print("row", b, row["score"], best, bound)
        assert abs(row["score"] - best) <= bound
        # words tile their characters
        assert [w["word"] for w in row["words"]] == row["text"].split()
        at = 0
        for w in row["words"]:
            while row["chars"][at]["char"].isspace():
                at += 1
            mine = row["chars"][at : at + len(w["word"])]
            assert "".join(c["char"] for c in mine) == w["word"] and w["start"] == mine[0]["start"] and w["end"] == mine[-1]["end"]
            assert abs(w["logp"] - sum(c["logp"] for c in mine)) <= 1e-9
            at += len(w["word"])
    print("rows left out (an argmax tie in some frame):", left_out, "of", len(rows))
    assert left_out == 0
    # given texts: the best path is no more than the sum over paths
    word = labels[5] + labels[7]
    texts = [(own[0] + " " + word)[:12], word + " " + own[1][2:30], word, word, own[4][:20] + " " + word]
    given, total = asr.align(sigs, texts), asr.score(sigs, texts)
    lab = {c: i for i, c in enumerate(labels)}
    for b, (g, s) in enumerate(zip(given, total)):
        ids = np.array([lab[c] for c in texts[b]], dtype=np.int64)
        T = int(frames[b])
        slack = AR.bound(AR.align64(logp[b], T, ids, len(ids), blank)) + CR.loss_bound(logp[b], T, ids, len(ids), blank)
        print("given", b, g["score"], s, slack)
        assert g["text"] == texts[b] and math.isfinite(g["score"]) and g["score"] <= s + slack
        assert "".join(c["char"] for c in g["chars"]) == texts[b] and all(c["end"] > c["start"] for c in g["chars"])
        assert all(x["end"] <= y["start"] for x, y in zip(g["chars"], g["chars"][1:])) and g["chars"][-1]["end"] <= T * sec
    # a text longer than the frames
    long_text = (word + " ") * eng.frames(lens[3])[1]
    none = asr.align([sigs[3], sigs[0]], [long_text, ""])
    assert none[0]["score"] == -math.inf and none[0]["chars"] == [] and none[0]["words"] == [] and none[0]["text"] == long_text
    assert math.isfinite(none[1]["score"]) and none[1]["chars"] == [] and none[1]["text"] == ""
    with pytest.raises(ValueError):
        asr.align(sigs, texts[:2])
