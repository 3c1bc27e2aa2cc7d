"""GPU checks of the device WER / CER scoring (vasr_error_counts_i32, stages.error_counts, metrics.ErrorRate,
VietASR.evaluate_manifest): every count equals tests/wer_reference.py exactly -- integers have no tolerance.

Every batch built here is wider than its longest row, and the ids behind each row's length are filled with 2^31 - 1 and
negative values: a kernel that reads past a length cannot produce the expected counts.  The shapes are the smallest at which
the kernel's paths change: 64 lanes per wavefront (word compaction), 256 lanes per workgroup (cells of a diagonal per pass),
the 4096-id limit, and the 64 KB above which the launch opts in to more dynamic LDS."""
import json
import os

import numpy as np
import pytest
import torch

import wer_reference as WR
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

POISON = (2 ** 31 - 1, -1, -(2 ** 31), -7)


def pack(rows, width=None, poison=POISON):
    """Rows of ids -> (padded int32 [B, width], lengths int32 [B]); width defaults to the longest row + 3."""
    longest = max([len(r) for r in rows] + [0])
    width = longest + 3 if width is None else width
    out = np.empty((len(rows), width), dtype=np.int64)
    out[:] = np.resize(np.asarray(poison, dtype=np.int64), width)[None, :]
    for k, r in enumerate(rows):
        out[k, : len(r)] = r
    return out.astype(np.int32), np.array([len(r) for r in rows], dtype=np.int32)


def device_counts(hyp, hyp_len, ref, ref_len, space_ids):
    from viet_asr_amd import stages
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return stages.error_counts(t(hyp), t(hyp_len), t(ref), t(ref_len), space_ids).cpu().numpy()


def check_rows(hyps, refs, space_ids, hyp_width=None, ref_width=None):
    hyp, hn = pack(hyps, hyp_width)
    ref, rn = pack(refs, ref_width)
    got = device_counts(hyp, hn, ref, rn, space_ids)
    want = WR.batch_counts(hyp, hn, ref, rn, space_ids)
    assert got.dtype == np.int32 and got.shape == (len(hyps), 4)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(b), len(hyps[b]), len(refs[b]), got[b].tolist(), want[b].tolist()) for b in bad[:6]]
    return got


def seq(rng, n, symbols):
    return rng.integers(0, symbols, n).tolist()


def test_fixture_of_the_reference_metric(gpu):
    g = np.load(os.path.join(GOLDEN_DIR, "wer_cases.npz"), allow_pickle=False)
    got = device_counts(g["hyp"], g["hyp_len"], g["ref"], g["ref_len"], g["space_ids"].tolist())
    assert got[:, 0].tolist() == g["word_edits"].tolist() and got[:, 1].tolist() == g["ref_words"].tolist()
    assert got[:, 2].tolist() == g["char_edits"].tolist() and got[:, 3].tolist() == g["ref_len"].tolist()
    assert WR.rates(got.astype(np.int64).sum(axis=0)) == (float(g["wer"]), float(g["cer"]))


def test_empty_sides_and_single_ids(gpu):
    a, b = [1, 2, 0, 3], [4, 5, 6, 0, 7, 8]
    hyps = [[], a, [], [1], [1], [0], a, [1, 2, 3, 1], []]
    refs = [a, [], [], [1], [2], [1], a, [4, 5, 6, 4], [0, 0]]
    got = check_rows(hyps, refs, [0])
    assert got[0].tolist() == [2, 2, 4, 4] and got[1].tolist() == [2, 0, 4, 0] and got[2].tolist() == [0, 0, 0, 0]
    assert got[6].tolist() == [0, 2, 0, 4] and got[7].tolist() == [1, 1, 4, 4] and got[8].tolist() == [0, 0, 2, 2]
    # width 0 on either side and on both: [B, 0] tensors
    z = np.zeros((2, 0), dtype=np.int32)
    zl = np.zeros(2, dtype=np.int32)
    ref, rn = pack([a, b])
    assert device_counts(z, zl, ref, rn, [0]).tolist() == [[2, 2, 4, 4], [2, 2, 6, 6]]
    assert device_counts(ref, rn, z, zl, [0]).tolist() == [[2, 0, 4, 0], [2, 0, 6, 0]]
    assert device_counts(z, zl, z, zl, [0]).tolist() == [[0, 0, 0, 0]] * 2
    # lengths beyond the width are clamped to it
    full, _ = pack([a, a], width=4)
    assert device_counts(full, np.array([9, 4], np.int32), full, np.array([4, 1 << 30], np.int32), [0]).tolist() == [[0, 2, 0, 4]] * 2


@pytest.mark.parametrize("symbols", [3, 95])
def test_lengths_around_the_lane_and_workgroup_boundaries(gpu, symbols):
    """3 symbols: most cells tie in the min; 95: few equal cells.  Id 0 is whitespace in both, so the word path sees the same
    lengths (with 3 symbols, words of one or two ids)."""
    rng = np.random.default_rng(symbols)
    edges = [63, 64, 65, 255, 256, 257, 513]
    hyps, refs = [], []
    for L in edges:
        base = seq(rng, L, symbols)
        noisy = [c if rng.random() > 0.1 else int(rng.integers(symbols)) for c in base]
        for h, r in ((base, seq(rng, 5, symbols)), (seq(rng, 5, symbols), base), (base, noisy), (noisy[:-1], base),
                     (base, seq(rng, L + 1, symbols)), (base, base)):
            hyps.append(h); refs.append(r)
    for n, m in ((513, 63), (63, 513), (257, 255), (255, 257), (64, 256), (256, 64), (1, 513), (513, 1)):
        hyps.append(seq(rng, n, symbols)); refs.append(seq(rng, m, symbols))
    check_rows(hyps, refs, [0])
    check_rows(refs, hyps, [0], hyp_width=600, ref_width=517)        # the other order, other strides


def test_the_widest_rows(gpu):
    """4096 ids per side: the launch that needs more than 64 KB of LDS.  One 4096 x 4096 pair, 4096 x 1 and 1 x 4096."""
    rng = np.random.default_rng(4096)
    base = seq(rng, 4096, 3)
    other = [c if rng.random() > 0.15 else int(rng.integers(3)) for c in base]
    got = check_rows([base, base, [2]], [other, [1], base], [0], hyp_width=4096, ref_width=4096)
    assert got[0, 3] == 4096 and 0 < got[0, 2] < 4096 and got[0, 0] > 0


def test_wider_than_4096_is_refused(gpu):
    from viet_asr_amd import stages
    wide = torch.zeros((1, 4097), dtype=torch.int32, device="cuda")
    ok = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    n = torch.ones(1, dtype=torch.int32, device="cuda")
    for h, r in ((wide, ok), (ok, wide)):
        with pytest.raises(NotImplementedError):
            stages.error_counts(h, n, r, n, [0])


def _ids(text, labels):
    return [labels.index(c) for c in text]


def test_words(gpu):
    labels = " abcdefg\t"
    sp = [0, 8]
    long_a, long_b = "abcdefg" * 43, "abcdefg" * 42 + "abcdefa"                     # one word of 301 characters
    pairs = [("  ab cd  ", "ab cd"), ("ab  cd", "ab cd"), ("ab\tcd", "ab cd"), ("ab \t cd", "abcd"), (" \t  ", "ab"),
             ("ab", "\t \t"), (" ", "\t"), ("a b c d e f g", "a b d d e g"), (long_a, long_b), (long_a, long_a),
             ("abcd abce abc", "abce abcd abcd"), ("abc abcd ab", "abcd abc abc"), ("ab ab ab ab", "ab ab ab"),
             ("abcdefg abcdeff", "abcdeff abcdefg abcdef"), ("a", "a "), ("\ta", "a"), ("a\tb", "a b")]
    hyps, refs = [_ids(h, labels) for h, _ in pairs], [_ids(r, labels) for _, r in pairs]
    got = check_rows(hyps, refs, sp)
    assert got[0].tolist()[:2] == [0, 2] and got[4].tolist()[:2] == [1, 1] and got[5].tolist()[:2] == [1, 0]
    assert got[8].tolist() == [1, 1, 1, 301] and got[10].tolist()[:2] == [3, 3] and got[11].tolist()[:2] == [3, 3]
    # only one of the two whitespace ids given: the tab is then part of a word
    one = check_rows(hyps, refs, [0])
    assert one[2].tolist()[:2] == [2, 2] and got[2].tolist()[:2] == [0, 2]
    # n_space = 0: a non-empty row is one word, an empty row has none
    none = check_rows(hyps + [[]], refs + [[1]], [])
    assert none[0].tolist()[:2] == [1, 1] and none[9].tolist()[:2] == [0, 1] and none[-1].tolist()[:2] == [1, 1]
    # more whitespace ids than labels in use, and 8 of them
    check_rows(hyps, refs, [0, 8, 20, 21, 22, 23, 24, 25])


def test_rows_do_not_depend_on_batch_padding_or_neighbours(gpu):
    rng = np.random.default_rng(77)
    rows_h = [seq(rng, int(rng.integers(0, 140)), 5) for _ in range(300)]
    rows_r = [seq(rng, int(rng.integers(0, 140)), 5) for _ in range(300)]
    probe_h, probe_r = seq(rng, 131, 5), seq(rng, 97, 5)
    rows_h[0], rows_r[0] = probe_h, probe_r
    rows_h[299], rows_r[299] = probe_h, probe_r
    got = check_rows(rows_h, rows_r, [0])
    alone = check_rows([probe_h], [probe_r], [0])
    assert got[0].tolist() == got[299].tolist() == alone[0].tolist()
    # other strides and other values behind the lengths: the same counts
    hyp, hn = pack(rows_h, width=257, poison=(-5, 0, 1, 2 ** 31 - 1, 3))
    ref, rn = pack(rows_r, width=140, poison=(0,))
    assert (device_counts(hyp, hn, ref, rn, [0]) == got).all()
    # a permuted batch gives the permuted counts
    perm = rng.permutation(300)
    hyp0, hn0 = pack(rows_h)
    ref0, rn0 = pack(rows_r)
    assert (device_counts(hyp0[perm], hn0[perm], ref0[perm], rn0[perm], [0]) == got[perm]).all()


def test_negative_length_rows_are_reported_not_scored(gpu):
    rng = np.random.default_rng(5)
    hyps, refs = [seq(rng, 40, 4) for _ in range(5)], [seq(rng, 44, 4) for _ in range(5)]
    hyp, hn = pack(hyps)
    ref, rn = pack(refs)
    want = WR.batch_counts(hyp, hn, ref, rn, [0])
    hn2 = hn.copy(); hn2[1] = -1; hn2[4] = -1
    rn2 = rn.copy(); rn2[3] = -1
    got = device_counts(hyp, hn2, ref, rn2, [0])
    assert got[[1, 3, 4]].tolist() == [[-1] * 4] * 3 and (got[[0, 2]] == want[[0, 2]]).all()
    assert (got == WR.batch_counts(hyp, hn2, ref, rn2, [0])).all()


def test_error_rate_accumulates_without_synchronising(gpu):
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import ErrorRate, word_error_rate_ids
    labels = list(" abcd\te")
    rng = np.random.default_rng(12)
    m = ErrorRate(labels)
    assert m.space_ids == [0, 5]
    total = np.zeros(4, dtype=np.int64)
    batches = []
    for B, wh, wr in ((3, 50, 40), (17, 130, 300), (1, 7, 9)):
        hyp, hn = pack([seq(rng, int(rng.integers(0, wh)), 7) for _ in range(B)], width=wh)
        ref, rn = pack([seq(rng, int(rng.integers(0, wr)), 7) for _ in range(B)], width=wr)
        total += WR.batch_counts(hyp, hn, ref, rn, m.space_ids).astype(np.int64).sum(axis=0)
        # the data layer's ports are int64; ids and lengths of the decoders are int32
        batches.append((torch.from_numpy(hyp).cuda(), torch.from_numpy(hn).cuda(),
                        torch.from_numpy(ref.astype(np.int64)).cuda(), torch.from_numpy(rn.astype(np.int64)).cuda()))
    torch.cuda.synchronize()
    # update() must not synchronise: torch raises on any blocking call while the debug mode is "error"
    assert hasattr(torch.cuda, "set_sync_debug_mode"), "sync debug mode missing: update() is then reviewed in the code only"
    torch.cuda.set_sync_debug_mode("error")
    try:
        for b in batches:
            m.update(*b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    r = m.compute()
    assert [r[k] for k in ("word_edits", "ref_words", "char_edits", "ref_chars")] == total.tolist()
    assert (r["wer"], r["cer"]) == WR.rates(total)
    assert m.compute(reduce=True) == r
    one = WR.batch_counts(*[t.cpu().numpy() for t in batches[1]], m.space_ids).astype(np.int64).sum(axis=0)
    assert word_error_rate_ids(*batches[1], labels) == WR.rates(one)[0]
    assert word_error_rate_ids(*batches[1], labels, use_cer=True) == WR.rates(one)[1]
    # a -1 row (the beam search's overflow report) makes compute raise; reset clears it
    hyp, hn, ref, rn = batches[0]
    bad = hn.clone(); bad[2] = -1
    m.update(hyp, bad, ref, rn)
    with pytest.raises(VasrError):
        m.compute()
    m.reset()
    m.update(*batches[2])
    last = WR.batch_counts(*[t.cpu().numpy() for t in batches[2]], m.space_ids)[0]
    assert m.compute()["char_edits"] == int(last[2])


def test_evaluate_manifest_end_to_end(gpu, tmp_path):
    """evaluate_manifest on generated WAVs: the references are the model's own transcripts with edits and one character outside
    the labels.  The returned counts equal the restatement on the returned hyps and the PARSED references;
    transcribe_manifest on the same manifest returns the same transcripts and its raw-text WER."""
    from viet_asr_amd import audio, configs, synth
    from viet_asr_amd.data_layer import word_error_rate
    from viet_asr_amd.infer import VietASR
    cfg = configs.builtin("quartznet12x1_vi")
    labels = cfg["labels"]
    jas = cfg["JasperEncoder"]["jasper"]
    enc_p, dec_p = str(tmp_path / "JasperEncoder-STEP-1.pt"), str(tmp_path / "JasperDecoderForCTC-STEP-1.pt")
    torch.save({k: torch.as_tensor(v) for k, v in synth.encoder_state_dict(jas, 64, 3).items()}, enc_p)
    torch.save({k: torch.as_tensor(v) for k, v in synth.decoder_state_dict(1024, len(labels) + 1, 3).items()}, dec_p)
    asr = VietASR("quartznet12x1_vi", enc_p, dec_p, device="gpu", decoder="greedy")
    rng = np.random.default_rng(8)
    lens = [9000, 31000, 16000, 4000, 25000, 12000, 20000]
    paths = []
    for i, n in enumerate(lens):
        paths.append(str(tmp_path / f"u{i}.wav"))
        audio.write_wav(paths[-1], (0.1 * rng.standard_normal(n)).astype(np.float32), 16000)
    man = str(tmp_path / "plain.json")
    with open(man, "w", encoding="utf-8") as f:
        for p, n in zip(paths, lens):
            f.write(json.dumps({"audio_filepath": p, "duration": n / 16000}) + "\n")
    own, none = asr.transcribe_manifest(man, batch_size=3)
    assert none is None and any(own)
    assert "#" not in labels
    refs = list(own)
    refs[0] = own[0][:3] + "#" + own[0][3:]                   # a character outside the labels: dropped by the parser
    refs[1] = own[1][2:] + " " + labels[5] + labels[7]        # edits at both ends
    refs[2] = "  ".join(own[2].split()) + " "                 # other whitespace, the same words
    refs[4] = own[4][: len(own[4]) // 2]
    refs[5] = None                                            # no text: transcribed, not scored
    man2 = str(tmp_path / "refs.json")
    with open(man2, "w", encoding="utf-8") as f:
        for p, n, t in zip(paths, lens, refs):
            e = {"audio_filepath": p, "duration": n / 16000}
            if t is not None:
                e["text"] = t
            f.write(json.dumps(e, ensure_ascii=False) + "\n")
    hyps, res = asr.evaluate_manifest(man2, batch_size=3)
    assert hyps == own
    sp = [i for i, c in enumerate(labels) if c.isspace()]
    ids = lambda s: [labels.index(c) for c in s if c in labels]  # noqa: E731
    scored = [i for i, t in enumerate(refs) if t]
    total = np.sum([WR.counts(ids(hyps[i]), ids(refs[i]), sp) for i in scored], axis=0)
    assert [res[k] for k in ("word_edits", "ref_words", "char_edits", "ref_chars")] == total.tolist()
    assert (res["wer"], res["cer"]) == WR.rates(total) and res["char_edits"] > 0
    parsed = ["".join(c for c in refs[i] if c in labels) for i in scored]
    assert res["wer"] == word_error_rate([hyps[i] for i in scored], parsed)
    assert res["cer"] == word_error_rate([hyps[i] for i in scored], parsed, use_cer=True)
    hyps2, wer2 = asr.transcribe_manifest(man2, batch_size=3)
    assert hyps2 == own and wer2 == word_error_rate([hyps[i] for i in scored], [refs[i] for i in scored])
