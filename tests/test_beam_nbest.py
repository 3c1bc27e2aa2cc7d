"""The n-best list of the device beam search (include/vasr.h vasr_beam_search_nbest_f32, viet_asr_amd.beam
BeamSearchDecoder.decode_beams / decode_beams_ids): CPU tests of argument validation; -m gpu tests against the oracle's
decode_beams (oracle/beam_oracle.py), against the top-1 entry, between the two kernel forms, per-row frame counts, long
transcripts and buffer bounds."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import beam_oracle as BO
from test_beam import (LABELS, LM_MODES, WAVE_ROWS, ctc_like_posteriors, make_decoder, oracle_lm, random_posteriors,
                       toy_lm)


def combined_tol(s):
    return 2e-3 * max(1.0, abs(s) / 50)


def logit_tol(s):          # no fixed-point LM term: fp64 sums of the same float32 log-probs
    return 1e-5 * max(1.0, abs(s) / 50)


def norm(t):
    return " ".join(t.split())


def check_against_oracle(got, ref_all, nbest, prune=BO.DEFAULT_BEAM_PRUNE_LOGP):
    """got: the device's list for one row; ref_all: the oracle's whole list (pruned, cut to beam_width).  Membership may
    differ only near the cut (the nbest-th score or the prune threshold), order only between hypotheses within tolerance."""
    ref = ref_all[:nbest]
    texts = [norm(t) for t, _, _ in got]
    assert 1 <= len(got) <= nbest
    assert len(set(texts)) == len(texts), texts                      # distinct texts within a row
    assert all(a[2] >= b[2] for a, b in zip(got, got[1:])), "not best first"
    by_text = {t: (lg, s) for t, lg, s in ref_all}
    thr = ref_all[0][2] + prune
    cut = ref[-1][2]

    def near_cut(s):
        return abs(s - cut) <= combined_tol(cut) or abs(s - thr) <= combined_tol(thr)

    in_ref = {r[0] for r in ref}
    for t, (_, lg, s) in zip(texts, got):
        if t not in in_ref:                                          # beyond the oracle's nbest, or not in its list at all
            assert near_cut(s), ("not in the oracle's list", t, s, ref[-3:])
        if t in by_text:
            rlg, rs = by_text[t]
            assert abs(s - rs) <= combined_tol(rs), (t, s, rs)
            assert abs(lg - rlg) <= logit_tol(rlg), (t, lg, rlg)
    for t, lg, s in ref:
        if t not in texts:
            assert near_cut(s), ("missing", t, s, got[-3:])
    for i in range(len(texts)):
        for j in range(i + 1, len(texts)):
            if texts[i] in by_text and texts[j] in by_text:
                si, sj = by_text[texts[i]][1], by_text[texts[j]][1]
                assert si >= sj - combined_tol(sj), ("order", texts[i], si, texts[j], sj)


# --------------------------------------------------------------------------------------------------------------- CPU
def test_nbest_arguments_are_validated_without_a_gpu():
    from viet_asr_amd import _lib
    from viet_asr_amd.beam import BeamSearchDecoder
    L = _lib.lib()
    fake = C.c_void_p(16)        # never dereferenced: validation returns first
    for nbest in (0, -1, 9):
        rc = L.vasr_beam_search_nbest_f32(fake, None, 2, 10, 29, 0, 8, nbest, -5.0, -10.0, None, fake, fake, fake, fake,
                                          fake, fake, 1 << 20, None)
        assert rc == -1 and b"nbest" in L.vasr_last_error(), nbest
    dec = BeamSearchDecoder(LABELS)
    x = torch.zeros((1, 4, len(LABELS) + 1))
    for nbest in (0, 9):
        with pytest.raises(ValueError, match="nbest"):
            dec.decode_beams_ids(x, 8, nbest)
        with pytest.raises(ValueError, match="nbest"):
            dec.decode_beams(x, 8, nbest=nbest)


# --------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("lm_mode", LM_MODES)
@pytest.mark.parametrize("beam_width,V1,seed", [(8, 29, 1), (32, 29, 2), (128, 29, 3), (20, 91, 4)])
def test_nbest_matches_the_oracle(gpu, tmp_path, lm_mode, beam_width, V1, seed):
    labels = LABELS if V1 == 29 else [" "] + [chr(0x100 + i) for i in range(89)]
    path, _ = toy_lm(str(tmp_path))
    lp = np.stack([random_posteriors(40 + 7 * b, V1, seed * 10 + b)[:40] for b in range(3)])
    dec = make_decoder(labels, path, lm_mode)
    lm = oracle_lm(path, lm_mode)
    refs = [[(norm(t), lg, s) for t, lg, s in BO.decode_beams(np.exp(lp[b].astype(np.float64)), labels, beam_width, lm=lm)]
            for b in range(3)]
    x = torch.from_numpy(lp).to(gpu)
    for nbest in sorted({1, 5, beam_width}):
        got = dec.decode_beams(x, beam_width, nbest)
        assert len(got) == 3
        for b in range(3):
            check_against_oracle(got[b], refs[b], nbest)
    assert dec.decode_beams(x, beam_width) == dec.decode_beams(x, beam_width, beam_width)      # nbest=None: beam_width


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [3, WAVE_ROWS])
@pytest.mark.parametrize("lm_mode", ["none", "arpa"])
def test_nbest_slot_0_is_the_top_1_search(gpu, tmp_path, rows, lm_mode):
    """Slot 0 equals decode_ids bit for bit (ids, length, float32 of the combined score), in both kernel forms (3 rows: four
    wavefronts per utterance, 65: one), with and without per-row frame counts."""
    path, _ = toy_lm(str(tmp_path))
    T = 96
    lp = np.stack([ctc_like_posteriors(T, 29, 1200 + b, p_blank=0.6) if b % 2 else random_posteriors(T, 29, 1300 + b, peaky=2.0)
                   for b in range(rows)])
    x = torch.from_numpy(lp).to(gpu)
    dec = make_decoder(LABELS, path, lm_mode)
    for frames in (None, [T - (7 * b) % T for b in range(rows)]):
        ids, n, score = dec.decode_ids(x, 32, frames=frames)
        nids, nn, count, logit, nscore = dec.decode_beams_ids(x, 32, 5, frames=frames)
        assert nids.shape == (rows, 5, T) and nn.shape == (rows, 5) and count.shape == (rows,)
        assert logit.dtype == nscore.dtype == torch.float64
        assert bool((count >= 1).all()) and bool((count <= 5).all())
        assert torch.equal(nn[:, 0], n)
        for b in range(rows):
            assert torch.equal(nids[b, 0, : n[b]], ids[b, : n[b]]), b
        assert torch.equal(nscore[:, 0].to(torch.float32), score)


_AB_SNIPPET = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch
import viet_asr_amd
import test_beam as T
path, _ = T.toy_lm({tmp!r})
lp = np.stack([T.ctc_like_posteriors(160, 29, 900 + b, p_blank=0.55) for b in range(4)] +
              [T.random_posteriors(160, 29, 950 + b, peaky=k) for b, k in enumerate((0.5, 2.0, 4.0))])
x = torch.from_numpy(lp).cuda()
out = []
for mode in T.LM_MODES:
    dec = T.make_decoder(T.LABELS, path, mode)
    for w, k in ((8, 8), (50, 10), (100, 70), (128, 128)):
        ids, n, count, logit, score = dec.decode_beams_ids(x, w, k)
        n = n.cpu().numpy()
        ids = ids.cpu().numpy()
        ids = np.where(np.arange(ids.shape[2])[None, None, :] < np.maximum(n, 0)[:, :, None], ids, 0)   # ids past the length are not written
        out.append((ids.tobytes(), n.tobytes(), count.cpu().numpy().tobytes(), logit.cpu().numpy().tobytes(),
                    score.cpu().numpy().tobytes()))
np.save({dst!r}, np.array(out, dtype=object), allow_pickle=True)
"""


@pytest.mark.gpu
def test_nbest_wave_kernel_and_group_kernel_agree(gpu, tmp_path):
    """VASR_BEAM_GROUP=0 (one wavefront per utterance) against =4 (four), each in its own process on the devtools build:
    every slot's ids, lengths, counts and both scores identical bit for bit, without an LM and with both LM behaviours,
    nbest up to 128 (two slots per lane)."""
    import subprocess
    import sys
    from conftest import ROOT
    dev = os.path.join(ROOT, "viet-asr_amd", "lib", "libvasr_hip_dev.so")
    res = []
    for tag, extra in (("wave", {"VASR_BEAM_GROUP": "0"}), ("group4", {"VASR_BEAM_GROUP": "4"})):
        dst = str(tmp_path / f"{tag}.npy")
        env = dict(os.environ, VASR_LIB_PATH=dev, **extra)
        r = subprocess.run([sys.executable, "-c", _AB_SNIPPET.format(root=ROOT, tmp=str(tmp_path), dst=dst)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res.append(np.load(dst, allow_pickle=True))
    assert len(res[0]) == len(res[1]) == 12
    for k, (a, b) in enumerate(zip(res[0], res[1])):
        for f in range(5):
            assert a[f] == b[f], (k, ("ids", "id_len", "count", "logit", "score")[f])
    counts = np.concatenate([np.frombuffer(a[2], np.int32) for a in res[0]])
    assert counts.max() > 64                           # the second slot of a lane was exercised


@pytest.mark.gpu
@pytest.mark.parametrize("lm_mode", LM_MODES)
def test_nbest_per_row_frame_counts(gpu, tmp_path, lm_mode):
    """A row searched over its own frame count inside a padded batch gives its batch-1 list bit for bit; 0 frames -> one
    empty hypothesis."""
    path, _ = toy_lm(str(tmp_path))
    T = 90
    lp = np.stack([ctc_like_posteriors(T, 29, 500 + b, p_blank=0.6) for b in range(5)])
    frames = [T, 37, 1, 64, 0]
    dec = make_decoder(LABELS, path, lm_mode)
    x = torch.from_numpy(lp).to(gpu)
    ids, n, count, logit, score = dec.decode_beams_ids(x, 32, 12, frames=frames)
    assert int(count[4]) == 1 and int(n[4, 0]) == 0 and bool((n[4, 1:] == 0).all())
    assert dec.decode_beams(x, 32, 12, frames=frames)[4][0][0] == ""
    for b in range(4):
        one = dec.decode_beams_ids(x[b : b + 1, : frames[b]].contiguous(), 32, 12)
        c = int(count[b])
        assert c == int(one[2][0])
        assert torch.equal(n[b], one[1][0])
        for k in range(c):
            assert torch.equal(ids[b, k, : n[b, k]], one[0][0, k, : n[b, k]]), (b, k)
        assert torch.equal(logit[b], one[3][0]) and torch.equal(score[b], one[4][0])
    with pytest.raises(ValueError):
        dec.decode_beams_ids(x, 32, 4, frames=[1, 2])


@pytest.mark.gpu
def test_nbest_long_recording(gpu):
    """More than kChars (3 072) frames: hypothesis 0 equals decode_ids; the others are distinct, best first."""
    from viet_asr_amd.beam import BeamSearchDecoder
    lp = ctc_like_posteriors(3500, 29, 4242, p_blank=0.7)
    dec = BeamSearchDecoder(LABELS, lm_path=None)
    for T in (3500, 3000):
        x = torch.from_numpy(lp[None, :T].copy()).to(gpu)
        ids, n, score = dec.decode_ids(x, 8)
        nids, nn, count, logit, nscore = dec.decode_beams_ids(x, 8, 8)
        assert int(nn[0, 0]) == int(n[0]) > 200
        assert torch.equal(nids[0, 0, : n[0]], ids[0, : n[0]])
        assert float(nscore[0, 0].to(torch.float32)) == float(score[0])
        got = dec.decode_beams(x, 8, 8)[0]
        assert len({t for t, _, _ in got}) == len(got) == int(count[0])


@pytest.mark.gpu
@pytest.mark.parametrize("beam_width,nbest", [(128, 128), (128, 100), (16, 5)])
def test_nbest_writes_stay_inside_its_buffers(gpu, beam_width, nbest):
    """Workspace and the [B][nbest][T] / [B][nbest] / [B] outputs between sentinel-filled guard regions; slots from the
    count on hold id_len 0 and scores -inf."""
    from viet_asr_amd import _lib
    B, T, V1, G = 3, 77, 29, 1 << 16
    lp = torch.from_numpy(np.stack([random_posteriors(T, V1, 900 + b, peaky=1.5) for b in range(B)])).to(gpu)
    L = _lib.lib()
    sizes = dict(ws=int(L.vasr_beam_workspace_bytes(B, T)), ids=B * nbest * T * 4, n=B * nbest * 4, count=B * 4,
                 logit=B * nbest * 8, score=B * nbest * 8)
    bufs = {k: torch.full((((v + 15) // 16) * 16 + 2 * G,), 0xA5, dtype=torch.uint8, device=gpu) for k, v in sizes.items()}
    p = {k: v[G:].data_ptr() for k, v in bufs.items()}
    _lib.check(L.vasr_beam_search_nbest_f32(lp.data_ptr(), None, B, T, V1, 0, beam_width, nbest, -5.0, -10.0, None, p["ids"],
                                            p["n"], p["count"], p["logit"], p["score"], p["ws"], sizes["ws"],
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, buf in bufs.items():
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + sizes[k]:] == 0xA5).all()), f"write outside {k}"
    count = bufs["count"][G : G + 4 * B].view(torch.int32).cpu().numpy()
    n = bufs["n"][G : G + 4 * B * nbest].view(torch.int32).cpu().numpy().reshape(B, nbest)
    logit = bufs["logit"][G : G + 8 * B * nbest].view(torch.float64).cpu().numpy().reshape(B, nbest)
    score = bufs["score"][G : G + 8 * B * nbest].view(torch.float64).cpu().numpy().reshape(B, nbest)
    assert (count >= 1).all() and (count <= nbest).all()
    for b in range(B):
        c = int(count[b])
        assert (n[b, :c] >= 0).all() and np.isfinite(score[b, :c]).all() and np.isfinite(logit[b, :c]).all()
        assert (n[b, c:] == 0).all()
        assert np.all(score[b, c:] == -math.inf) and np.all(logit[b, c:] == -math.inf)
