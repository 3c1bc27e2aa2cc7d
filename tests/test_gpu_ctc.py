"""GPU checks of the CTC forward score (csrc/ctc_loss.hip through stages.ctc_loss, asr.CTCLossNM, metrics.CTCEvalLoss, the
evaluation helpers, VietASR.evaluate_manifest(eval_loss=True) and VietASR.score) against the float64 restatement and its
bound (tests/ctc_reference.py) and the fixture of the reference's own functions (tests/golden/ctc_cases.npz).  Every test
checks a value or a return code."""
import json
import math
import os

import numpy as np
import pytest
import torch

import ctc_reference as CR
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# the kernel's mapping (csrc/vasr_internal.h): lane l of 256 owns the states l, l + 256, ...; 4 of them per lane while
# 2 * tgt_width + 1 <= 1024, 33 above; a wavefront has 64 lanes
WAVE, LANES, NARROW_SLOTS, WIDE_SLOTS, MAX_WIDTH = 64, 256, 4, 33, 4096
NARROW_MAX_WIDTH = (LANES * NARROW_SLOTS - 1) // 2          # 511: S = 1023


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "ctc_cases.npz"), allow_pickle=False)


def device_loss(gpu, logp, frames, tgt, tgt_len, blank):
    from viet_asr_amd import stages
    out = stages.ctc_loss(torch.from_numpy(np.ascontiguousarray(logp)).to(gpu), torch.as_tensor(np.asarray(frames)).to(gpu),
                          torch.from_numpy(np.ascontiguousarray(tgt)).to(gpu), torch.as_tensor(np.asarray(tgt_len)).to(gpu), blank)
    assert out.dtype == torch.float32 and out.device.type == "cuda" and not out.requires_grad
    return out.cpu().numpy()


def check(got, l64, bound, tag=None):
    for b in range(len(l64)):
        print(tag, b, float(got[b]), l64[b], abs(float(got[b]) - l64[b]) if np.isfinite(l64[b]) else None, bound[b])
        assert CR.close(got[b], l64[b], bound[b]), (tag, b, float(got[b]), l64[b], bound[b])


def make_rows(rng, lengths, C, extra=3, scale=1.0, repeats=0.2):
    """One ragged batch: row b has lengths[b] ids below C - 1 (a share of equal neighbours) and the fewest frames with a path
    + extra; finite log-probs and valid ids everywhere."""
    B, W = len(lengths), max(max(lengths), 1)
    tgt = rng.integers(0, C - 1, (B, W)).astype(np.int64)
    for b, L in enumerate(lengths):
        for i in range(1, L):
            if rng.random() < repeats:
                tgt[b, i] = tgt[b, i - 1]
    tgt_len = np.array(lengths, dtype=np.int64)
    frames = np.array([CR.min_frames(tgt[b], L) + extra for b, L in enumerate(lengths)], dtype=np.int64)
    x = (rng.standard_normal((B, int(frames.max()), C)) * scale).astype(np.float32)
    logp = torch.log_softmax(torch.from_numpy(x), dim=-1).numpy()
    return logp, frames, tgt, tgt_len


def test_every_fixture_case(gpu, golden):
    g = golden
    for i in range(int(g["cases"])):
        lp, fr, tg, tl = g[f"c{i}_logp"], g[f"c{i}_frames"], g[f"c{i}_tgt"], g[f"c{i}_tgt_len"]
        blank = lp.shape[2] - 1
        l64, bound = CR.batch(lp, fr, tg, tl, blank)
        got = device_loss(gpu, lp, fr, tg, tl, blank)
        check(got, l64, bound, f"c{i}")
        assert (np.isposinf(got) == np.isposinf(g[f"c{i}_loss"])).all()          # +inf where the reference has it


EDGES = {
    # S = 2 L + 1 one below, at and one above a boundary of the mapping, by tgt_width (which picks the instantiation)
    "narrow": (NARROW_MAX_WIDTH, [WAVE // 2 - 1, WAVE // 2, WAVE // 2 + 1,                  # S = 63, 65, 67: a wavefront
                                  LANES // 2 - 1, LANES // 2, LANES // 2 + 1,               # S = 255, 257, 259: the workgroup
                                  LANES - 1, LANES, LANES + 1,                              # S = 511, 513, 515: slot 1 -> 2
                                  3 * LANES // 2 - 1, 3 * LANES // 2,                       # S = 767, 769: slot 2 -> 3
                                  NARROW_MAX_WIDTH - 1, NARROW_MAX_WIDTH]),                 # S = 1021, 1023: the last narrow
    "switch": (NARROW_MAX_WIDTH + 1, [NARROW_MAX_WIDTH, NARROW_MAX_WIDTH + 1, 0, 1]),       # S = 1023, 1025 in the wide kernel
    "wide": (5 * LANES // 2 + 1, [NARROW_MAX_WIDTH + 2, 2 * LANES + LANES // 2 - 1, 2 * LANES + LANES // 2,
                                  5 * LANES // 2 + 1]),                                     # S = 1027, 1279, 1281, 1283
}


@pytest.mark.parametrize("name", list(EDGES))
def test_rows_at_the_edges_of_the_mapping(gpu, name):
    width, lengths = EDGES[name]
    rng = np.random.default_rng(len(name))
    C = 7
    logp, frames, tgt, tgt_len = make_rows(rng, lengths, C)
    pad = np.full((len(lengths), width), C - 2, dtype=np.int64)
    pad[:, : tgt.shape[1]] = tgt
    l64, bound = CR.batch(logp, frames, pad, tgt_len, C - 1)
    assert np.isfinite(l64).all()
    check(device_loss(gpu, logp, frames, pad, tgt_len, C - 1), l64, bound, name)


def test_the_two_instantiations_give_the_same_bits(gpu):
    """The same rows at tgt_width 511 (4 states per lane) and 512 (33): a state's arithmetic does not depend on its place."""
    rng = np.random.default_rng(11)
    logp, frames, tgt, tgt_len = make_rows(rng, [NARROW_MAX_WIDTH, 300, 5, 0], 9)
    wide = np.zeros((4, NARROW_MAX_WIDTH + 1), dtype=np.int64)
    wide[:, : tgt.shape[1]] = tgt
    a = device_loss(gpu, logp, frames, tgt, tgt_len, 8)
    b = device_loss(gpu, logp, frames, wide, tgt_len, 8)
    assert np.isfinite(a).all() and a.tobytes() == b.tobytes()


def test_the_widest_row(gpu):
    """One row at tgt_width 4096 with frames just above feasibility: 8193 states, 33 per lane, 64 KB of LDS."""
    rng = np.random.default_rng(12)
    logp, frames, tgt, tgt_len = make_rows(rng, [MAX_WIDTH], 5, extra=2, repeats=0.05)
    assert tgt.shape[1] == MAX_WIDTH and LANES * WIDE_SLOTS >= 2 * MAX_WIDTH + 1
    l64, bound = CR.batch(logp, frames, tgt, tgt_len, 4)
    assert np.isfinite(l64).all()
    check(device_loss(gpu, logp, frames, tgt, tgt_len, 4), l64, bound, "widest")
    too_few = device_loss(gpu, logp, frames - 3, tgt, tgt_len, 4)
    assert np.isposinf(too_few).all()


def test_wider_than_4096_is_refused(gpu):
    from viet_asr_amd import stages
    z = torch.zeros
    with pytest.raises(NotImplementedError):
        stages.ctc_loss(z(1, 4, 3, device=gpu), torch.tensor([4], device=gpu), z(1, MAX_WIDTH + 1, dtype=torch.int64, device=gpu),
                        torch.tensor([2], device=gpu), 2)
    with pytest.raises(ValueError):
        stages.ctc_loss(z(1, 4, 3, device=gpu), torch.tensor([4], device=gpu), z(1, 2, dtype=torch.int64, device=gpu),
                        torch.tensor([2], device=gpu), 3)                        # blank outside [0, C)


def test_rows_do_not_depend_on_the_batch_or_on_what_lies_behind_their_lengths(gpu):
    rng = np.random.default_rng(13)
    C = 29
    lengths = [40, 0, 129, 7, 64]
    logp, frames, tgt, tgt_len = make_rows(rng, lengths, C, extra=9)
    alone = []
    for b, L in enumerate(lengths):                                 # every row alone, cut to its own lengths
        alone.append(device_loss(gpu, logp[b : b + 1, : frames[b]], frames[b : b + 1], tgt[b : b + 1, : max(L, 1)],
                                 tgt_len[b : b + 1], C - 1)[0])
    alone = np.array(alone, dtype=np.float32)
    # the ragged batch, wider and longer, in another order, NaN log-probs and out-of-range ids behind every length
    order = [3, 0, 4, 2, 1]
    T, W = int(frames.max()) + 5, 600                               # (the wide instantiation)
    big = np.full((5, T, C), np.nan, dtype=np.float32)
    ids = np.full((5, W), 10 ** 6, dtype=np.int64)
    ids[::2] = -7
    for k, b in enumerate(order):
        big[k, : frames[b]] = logp[b, : frames[b]]
        ids[k, : lengths[b]] = tgt[b, : lengths[b]]
    got = device_loss(gpu, big, frames[order], ids, tgt_len[order], C - 1)
    assert np.isfinite(got).all() and got.tobytes() == alone[order].tobytes()
    l64, bound = CR.batch(logp, frames, tgt, tgt_len, C - 1)
    check(alone, l64, bound, "alone")
    # lengths above the tensor's are clamped to it
    clamped = device_loss(gpu, logp[:1, : frames[0]], [10 ** 6], tgt[:1, : lengths[0]], [10 ** 6], C - 1)
    assert clamped.tobytes() == alone[:1].tobytes()


def test_nan_conventions_and_empty_sides(gpu):
    rng = np.random.default_rng(14)
    C = 6
    logp, _, _, _ = make_rows(rng, [3] * 9, C, extra=8)
    T = logp.shape[1]
    tgt = np.tile(np.array([0, 1, 1, 2], dtype=np.int64), (9, 1))
    frames = np.array([T, -1, T, T, T, T, 0, 0, T], dtype=np.int64)
    tgt_len = np.array([4, 4, -3, 4, 4, 4, 0, 2, 0], dtype=np.int64)
    tgt[3, 2] = C - 1              # the blank inside the length
    tgt[4, 0] = C                  # out of range
    tgt[5, 3] = -1
    got = device_loss(gpu, logp, frames, tgt, tgt_len, C - 1)
    assert np.isnan(got[[1, 2, 3, 4, 5]]).all() and np.isfinite(got[[0, 6, 8]]).all()
    assert got[6] == 0.0 and np.isposinf(got[7])                    # no frames: 0 for the empty target, otherwise no path
    l64, bound = CR.batch(logp, frames, tgt, tgt_len, C - 1)
    check(got, l64, bound, "conventions")
    assert abs(l64[8] + logp[8, :, C - 1].astype(np.float64).sum()) < 1e-9     # L == 0: minus the blank's sum
    # float lengths are truncated as .long() truncates them; frames == 0 and tgt_width == 0 are legal shapes
    from viet_asr_amd import stages
    dev = lambda a: torch.as_tensor(a).to(gpu)  # noqa: E731
    f = stages.ctc_loss(dev(logp[:1]), dev(np.array([T - 0.5], dtype=np.float32)), dev(tgt[:1]), dev([4]), C - 1).cpu().numpy()
    assert f.tobytes() == device_loss(gpu, logp[:1], [T - 1], tgt[:1], [4], C - 1).tobytes()
    none = stages.ctc_loss(torch.zeros(2, 0, C, device=gpu), dev([0, 0]), torch.zeros(2, 0, dtype=torch.int64, device=gpu),
                           dev([0, 0]), C - 1).cpu().numpy()
    assert none.tolist() == [0.0, 0.0]
    # a row whose log-probs are all -inf has no path and makes no NaN
    dead = np.full_like(logp[:1], -np.inf)
    assert np.isposinf(device_loss(gpu, dead, [T], tgt[:1], [4], C - 1)).all()


def test_module_metric_and_helpers_reproduce_the_reference_epoch(gpu, golden):
    from viet_asr_amd import asr, helpers
    from viet_asr_amd.metrics import CTCEvalLoss
    g = golden
    dev = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
    # CTCLossNM.forward against every stored batch mean
    for i in range(int(g["cases"])):
        lp, fr, tg, tl = g[f"c{i}_logp"], g[f"c{i}_frames"], g[f"c{i}_tgt"], g[f"c{i}_tgt_len"]
        nm = asr.CTCLossNM(num_classes=lp.shape[2] - 1)
        got = nm(force_pt=True, log_probs=dev(lp), targets=dev(tg), input_length=dev(fr).float(), target_length=dev(tl))
        assert got.dim() == 0 and got.dtype == torch.float32 and got.device.type == "cuda" and not got.requires_grad
        l64, bound = CR.batch(lp, fr, tg, tl, lp.shape[2] - 1)
        want = float(g[f"c{i}_mean"])
        if np.isfinite(l64).all():
            tol = CR.mean_bound(bound, l64.mean())
            print("mean", i, float(got), want, l64.mean(), tol)
            assert abs(float(got) - l64.mean()) <= tol and abs(float(got) - want) <= 2 * tol
        else:
            assert float(got) == want == np.inf
    # the three-batch epoch: CTCEvalLoss, and the helpers on device tensors
    labels = g["epoch_labels"].tolist()
    nm, metric, gv = asr.CTCLossNM(num_classes=len(labels)), CTCEvalLoss(len(labels)), {}
    means64, tols, rows = [], [], 0
    for j in range(3):
        lp, fr, tg, tl = (g[f"epoch{j}_{k}"] for k in ("logp", "frames", "tgt", "tgt_len"))
        metric.update(dev(lp), dev(fr), dev(tg), dev(tl))
        loss = nm(force_pt=True, log_probs=dev(lp), targets=dev(tg), input_length=dev(fr), target_length=dev(tl))
        helpers.process_evaluation_batch({"loss": [loss], "predictions": [dev(g[f"epoch{j}_pred"])], "transcript": [dev(tg)],
                                          "transcript_length": [dev(tl)], "output": [dev(lp)]}, gv, labels)
        assert gv["EvalLoss"][-1].device.type == "cuda"             # nothing came to the host for the loss
        l64, bound = CR.batch(lp, fr, tg, tl, len(labels))
        means64.append(l64.mean()); tols.append(CR.mean_bound(bound, l64.mean())); rows += len(fr)
    tol = float(np.mean(tols)) + CR.U * 4 * float(np.mean(means64))
    want = float(g["epoch_loss"])
    r = metric.compute()
    print("epoch", r, want, np.mean(means64), tol)
    assert abs(r["eval_loss"] - np.mean(means64)) <= tol and abs(r["eval_loss"] - want) <= 2 * tol
    assert r["scored"] == rows == 9 and r["infeasible"] == 0
    every = np.concatenate([g[f"epoch{j}_loss"] for j in range(3)]).astype(np.float64)
    assert abs(r["loss_sum"] - every.sum()) <= 9 * max(tols) + CR.U * 10 * every.sum()
    assert abs(r["loss_sum"] / r["scored"] - r["eval_loss"]) > 1e-2     # the mean of means is not the sample mean
    assert gv["predictions"] == g["epoch_predictions"].tolist() and gv["transcripts"] == g["epoch_transcripts"].tolist()
    logs = helpers.process_evaluation_epoch(gv, eval_metric="WER")
    assert sorted(logs) == ["Evaluation_Loss", "Evaluation_Valid_CER", "Evaluation_Valid_WER"]
    assert logs["Evaluation_Valid_WER"] == float(g["epoch_wer"]) and logs["Evaluation_Valid_CER"] == float(g["epoch_cer"])
    assert abs(logs["Evaluation_Loss"] - want) <= 2 * tol
    assert list(helpers.process_evaluation_epoch(gv, tag="dev"))[0] == "Evaluation_Loss_dev"
    # a NaN row is reported, not averaged
    from viet_asr_amd._lib import VasrError
    metric.update(dev(g["epoch2_logp"]), dev(np.array([-1])), dev(g["epoch2_tgt"]), dev(g["epoch2_tgt_len"]))
    with pytest.raises(VasrError):
        metric.compute()


def test_evaluate_manifest_with_eval_loss_and_score(gpu, tmp_path):
    """On generated WAVs and the smallest model: the loss form returns the plain call's transcripts and rates, loss_sum is the
    sum of -score(...) over the scored rows, and a text with no path scores -inf."""
    from viet_asr_amd import audio, configs, synth
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
    paths = []
    for i, n in enumerate(lens):
        paths.append(str(tmp_path / f"u{i}.wav"))
        audio.write_wav(paths[-1], (0.1 * rng.standard_normal(n)).astype(np.float32), 16000)
    own = asr.transcribe_batch([audio.read_wav(p)[0] for p in paths], row_independent=True)
    word = labels[5] + labels[7]
    refs = [(own[0] + " " + word)[:12], word + " " + own[1][2:30], None, word, (own[4][:20] + " " + word)]
    man = str(tmp_path / "refs.json")
    with open(man, "w", encoding="utf-8") as f:
        for p, n, t in zip(paths, lens, refs):
            e = {"audio_filepath": p, "duration": n / 16000}
            if t is not None:
                e["text"] = t
            f.write(json.dumps(e, ensure_ascii=False) + "\n")
    hyps, plain = asr.evaluate_manifest(man, batch_size=2)
    for bs in (2, 8):
        hyps2, res = asr.evaluate_manifest(man, batch_size=bs, eval_loss=True)
        assert hyps2 == hyps and all(res[k] == v for k, v in plain.items())
        assert res["scored"] == 4 and res["infeasible"] == 0 and math.isfinite(res["eval_loss"]) and res["loss_sum"] > 0
        if bs == 2:
            per_batch = res
    # one batch of all five, as batch_size 8 cut it (sorted by duration): the same forward pass, hence the same rows
    order = sorted(range(5), key=lambda i: lens[i])
    sigs = [audio.read_wav(paths[i])[0] for i in order]
    scores = asr.score(sigs, [refs[i] or word for i in order])
    assert all(isinstance(s, float) and math.isfinite(s) and s < 0 for s in scores)
    total = -sum(s for s, i in zip(scores, order) if refs[i])
    print("loss_sum", res["loss_sum"], total, per_batch["loss_sum"], res["eval_loss"], per_batch["eval_loss"])
    assert abs(res["loss_sum"] - total) <= CR.U * 8 * total
    # batch_size 2 cut [o0, o1], [o2, o3], [o4]: the same sum from the same batches, and another mean of batch means
    chunk_scores, chunk_means = [], []
    for lo in range(0, 5, 2):
        idx = order[lo : lo + 2]
        sc = asr.score([audio.read_wav(paths[i])[0] for i in idx], [refs[i] or word for i in idx])
        kept = [-v for v, i in zip(sc, idx) if refs[i]]
        chunk_scores += kept
        if kept:
            chunk_means.append(sum(kept) / len(kept))
    assert abs(per_batch["loss_sum"] - sum(chunk_scores)) <= CR.U * 8 * total
    assert abs(per_batch["eval_loss"] - sum(chunk_means) / len(chunk_means)) <= CR.U * 8 * total
    assert abs(res["eval_loss"] - total / 4) <= CR.U * 8 * total
    # a text with no path through its audio: more characters than the 4000-sample signal has frames
    frames = asr._fused_engine().frames(lens[3])[1]
    long_text = (word + " ") * frames
    s = asr.score([audio.read_wav(paths[3])[0], audio.read_wav(paths[0])[0]], [long_text, ""])
    assert s[0] == -math.inf and math.isfinite(s[1]) and s[1] < 0
    hyps3, res3 = asr.evaluate_manifest(_one_line(tmp_path, paths[3], lens[3], long_text), eval_loss=True)
    assert res3["infeasible"] == 1 and res3["scored"] == 0 and res3["eval_loss"] == math.inf and res3["loss_sum"] == 0.0
    with pytest.raises(ValueError):
        asr.evaluate_manifest(man, eval_loss=True, nbest=2)


def _one_line(tmp_path, path, n, text):
    man = str(tmp_path / "one.json")
    with open(man, "w", encoding="utf-8") as f:
        f.write(json.dumps({"audio_filepath": path, "duration": n / 16000, "text": text}) + "\n")
    return man
