"""vasr_class_scores_f32 on the device (csrc/cls_eval.hip) and what is built on it, against the fixture of the reference's own
functions (tests/golden/cls_eval_cases.npz) and the float64 / integer restatement (tests/cls_eval_reference.py): ranks and
top-k indices exactly, top-k values bit for bit, losses and probabilities inside the bound derived there; then the edges of a
lane-strided kernel (C around 64, 128 and 512 -- the accumulators' second round --, B around the four rows of a workgroup,
k = C and k = 16), rows built to tie, NaN and infinities, out-of-range targets, every combination of NULL outputs, row
independence, and ``QuartzNetClassifier.evaluate_manifest`` / ``classify_topk`` end to end."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import cls_eval_reference as ER
import cls_reference as CR
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "cls_eval_cases.npz"), allow_pickle=False)


def _scores(gpu, x, t=None, k=0, want_prob=False):
    from viet_asr_amd import stages
    out = stages.classification_scores(torch.from_numpy(np.ascontiguousarray(x)).to(gpu),
                                       None if t is None else torch.from_numpy(np.asarray(t, dtype=np.int64)).to(gpu), k, want_prob)
    return {name: v.cpu().numpy() for name, v in out.items()}


def _check(tag, x, t, out, k, loss_rows=None):
    """Every output of one call against the restatement: integers exactly, values bit for bit, loss / probs inside the bound
    on the rows of loss_rows (default: all)."""
    rank, top, loss = ER.batch(x, t, k)
    assert out["rank"].dtype == np.int32 and out["rank"].tolist() == rank.tolist(), tag
    if k:
        assert out["indices"].dtype == np.int32 and out["indices"].tolist() == top.tolist(), tag
        want = np.take_along_axis(x, top, axis=1)
        assert out["values"].view(np.int32).tolist() == want.view(np.int32).tolist(), tag
    for b in (range(len(t)) if loss_rows is None else loss_rows):
        if rank[b] < 0:
            assert out["loss"][b] == 0.0 and not np.signbit(out["loss"][b]), (tag, b)
            continue
        bound = ER.loss_bound(x[b], t[b])
        err = abs(float(out["loss"][b]) - loss[b])
        print(f"{tag} row {b}: loss {out['loss'][b]:.9g} f64 {loss[b]:.12g} err {err:.3g} bound {bound:.3g}")
        assert err <= bound, (tag, b, float(out["loss"][b]), loss[b], bound)
        if k and "probs" in out:
            p, pb = ER.prob64(x[b], top[b]), ER.prob_bound(x[b], top[b])
            assert (np.abs(out["probs"][b].astype(np.float64) - p) <= pb).all(), (tag, b, out["probs"][b], p, pb)


def test_every_fixture_case(gpu, golden):
    from viet_asr_amd.metrics import classification_accuracy
    g = golden
    for i in range(int(g["cases"])):
        x, t = g[f"c{i}_logits"], g[f"c{i}_targets"]
        k = min(5, x.shape[1])
        out = _scores(gpu, x, t, k, want_prob=True)
        assert out["indices"].tolist() == g[f"c{i}_top5"].tolist(), i                # the reference's own topk
        _check(f"case {i} {x.shape}", x, t, out, k)
        for j in range(3):
            ks = g[f"c{i}_acc{j}_k"].tolist()
            got = classification_accuracy(torch.from_numpy(x).to(gpu), torch.from_numpy(t).to(gpu), top_k=ks)
            assert [float(a) for a in got] == g[f"c{i}_acc{j}"].tolist(), (i, ks)       # the reference's floats
    x, t = torch.from_numpy(g["c0_logits"]).to(gpu), torch.from_numpy(g["c0_targets"]).to(gpu)
    assert [float(a) for a in classification_accuracy(x, t)] == g["c0_acc0"].tolist()  # top_k=None: [1]


def test_epoch_through_the_metric_and_the_helpers(gpu, golden):
    from viet_asr_amd import helpers
    from viet_asr_amd.metrics import TopKAccuracy
    g = golden
    ks = g["epoch_top_k"].tolist()                                                       # [5, 1]: unsorted
    m, gv = TopKAccuracy(ks), {}
    sizes, bounds, means, hits = [], [], [], {k: 0 for k in ks}
    for j in range(3):
        x, t = g[f"epoch{j}_logits"], g[f"epoch{j}_targets"]
        xd, td = torch.from_numpy(x).to(gpu), torch.from_numpy(t).to(gpu)
        m.update(xd, td)
        helpers.process_classification_evaluation_batch({"logits": [xd], "labels": [td]}, gv, top_k=ks)
        rank, _, loss = ER.batch(x, t, 0)
        sizes.append(len(t)); means.append(loss.mean()); bounds.append([ER.loss_bound(r, tt) for r, tt in zip(x, t)])
        for k in ks:
            hits[k] += ER.hits(rank, k)
    bound = ER.mean_of_means_bound(sizes, bounds, means)
    ref_loss = float(g["epoch_loss"])
    # the reference's own float32 epoch loss lies inside the same bound of the float64 mean of means
    assert abs(ref_loss - np.mean(means)) <= bound
    r = m.compute()
    assert r["samples"] == 73 and r["correct"] == hits and r["accuracy"] == {k: hits[k] / 73 for k in ks}
    print(f"eval_loss {r['eval_loss']:.9g} f64 {np.mean(means):.12g} reference {ref_loss:.9g} bound {bound:.3g}")
    assert abs(r["eval_loss"] - np.mean(means)) <= bound
    logs = m.logs("t")
    assert sorted(logs) == ["Evaluation_Accuracy_Top@1 t", "Evaluation_Accuracy_Top@5 t", "Evaluation_Loss t"]
    for k in ks:
        # the reference rounds hits / (k B) x B per batch in float32, the metric divides the exact totals once
        assert abs(logs[f"Evaluation_Accuracy_Top@{k} t"] - float(g[f"epoch_acc{k}"])) <= 100.0 * 8 * ER.EPS
    # the helpers keep the reference's per-batch float32 entries: the same numbers
    assert gv["batchsize"] == sizes and all(v.device.type == "cuda" for k in ks for v in gv[f"CorrectCount@{k}"])
    assert all(v.device.type == "cuda" for v in gv["EvalLoss"])
    for k in ks:
        assert [float(v) for v in gv[f"CorrectCount@{k}"]] == g[f"epoch_counts{k}"].tolist()
    hl = helpers.process_classification_evaluation_epoch(gv, eval_metric=ks, tag="t")
    assert sorted(hl) == sorted(logs)
    for k in ks:
        assert float(hl[f"Evaluation_Accuracy_Top@{k} t"]) == float(g[f"epoch_acc{k}"])
    assert abs(hl["Evaluation_Loss t"] - np.mean(means)) <= bound
    # a caller's own loss tensors are gathered as the reference gathers them
    gv2 = {}
    helpers.process_classification_evaluation_batch(
        {"loss": [torch.tensor(2.0, device=gpu), torch.tensor(4.0, device=gpu)], "logits": [xd], "labels": [td]}, gv2, top_k=1)
    assert float(gv2["EvalLoss"][0]) == 3.0 and sorted(gv2) == ["CorrectCount@1", "EvalLoss", "batchsize"]
    # the training monitor hands the logger classification_accuracy's figures (the fixture's, for the unsorted [5, 1, 3])
    class Board:
        def __init__(self):
            self.scalars = []

        def add_scalar(self, name, value):
            self.scalars.append((name, float(value)))
    i = next(i for i in range(int(g["cases"])) if g[f"c{i}_logits"].shape == (67, 35))
    xd, td = torch.from_numpy(g[f"c{i}_logits"]).to(gpu), torch.from_numpy(g[f"c{i}_targets"]).to(gpu)
    board = Board()
    assert helpers.monitor_classification_training_progress([torch.tensor(1.0), xd, td], g[f"c{i}_acc2_k"].tolist(), board) is None
    assert board.scalars == [(f"training_batch_top@{k}", a) for k, a in zip(g[f"c{i}_acc2_k"].tolist(), g[f"c{i}_acc2"].tolist())]
    board = Board()
    helpers.monitor_classification_training_progress([torch.tensor(1.0), xd, td], tb_logger=board)
    assert board.scalars == [("training_batch_top@1", float(g[f"c{i}_acc0"][0]))]


EDGE_C = (1, 2, 16, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025)


@pytest.mark.parametrize("C", EDGE_C)
def test_lane_and_accumulator_edges(gpu, C):
    rng = np.random.default_rng(100 + C)
    for B in (1, 3, 4, 5):
        x = (rng.standard_normal((B, C)) * (1.0, 0.01, 30.0)[B % 3]).astype(np.float32)
        t = rng.integers(0, C, B)
        t[0] = C - 1                                            # the last class
        if B > 1:
            t[1] = 0
            x[1, 0] = x[1].max() + 1.0                          # class 0 the best
        if B > 3:
            x[3, C - 1] = x[3].max() + 1.0                      # the last class the best
        k = min(C, 16)                                          # k = C up to 16; k = 16 at C = 16
        _check(f"C {C} B {B} k {k}", x, t, _scores(gpu, x, t, k, want_prob=True), k)
        probs = _scores(gpu, x, None, k, want_prob=True)["probs"].astype(np.float64)      # without targets: the same bits
        assert probs.tobytes() == _scores(gpu, x, t, k, want_prob=True)["probs"].astype(np.float64).tobytes()
        if k == C:                                              # all classes: the probabilities sum to one
            for b in range(B):
                assert abs(probs[b].sum() - 1.0) <= ER.prob_bound(x[b], ER.topk(x[b], k)).sum(), (C, B, b)


def test_ties_follow_the_lower_index_rule(gpu):
    """Checked against the restatement's rule, not against torch.topk, which leaves the order of equal values open."""
    C = 70
    x = np.zeros((6, C), dtype=np.float32)
    x[0] = 2.5                                                   # all equal
    x[1] = np.linspace(-1, 1, C); x[1, 5] = x[1, 40] = 3.0       # target 40 tied with an EARLIER class
    x[2] = np.linspace(1, -1, C); x[2, 7] = x[2, 66] = 3.0       # target 7 tied with a LATER class
    x[3] = 1.0; x[3, 64:] = 1.0; x[3, 10] = 0.0                  # ties across the lane-stride boundary
    x[4, ::2] = 0.0; x[4, 1::2] = -0.0                           # -0 == +0: all equal
    x[5, 3] = x[5, 67] = x[5, 68] = 9.0
    t = np.array([33, 40, 7, 69, 69, 68])
    out = _scores(gpu, x, t, 16)
    _check("ties", x, t, out, 16)
    assert out["rank"].tolist() == [33, 1, 0, 68, 69, 2]
    assert out["indices"][0].tolist() == list(range(16)) and out["indices"][1, :2].tolist() == [5, 40]
    assert out["indices"][3].tolist() == [c for c in range(17) if c != 10] and out["indices"][5, :3].tolist() == [3, 67, 68]
    assert out["values"][4].view(np.int32).tolist() == x[4, :16].view(np.int32).tolist()        # the signs of the zeros survive
    y = np.array([[1, 3, 3, 2, 3]], dtype=np.float32)            # the header's example
    assert _scores(gpu, y, None, 3)["indices"].tolist() == [[1, 2, 4]]


def test_nan_and_infinities_follow_the_documented_order(gpu):
    nan, inf = np.float32("nan"), np.float32("inf")
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 130)).astype(np.float32)
    x[0, 100] = nan; x[0, 3] = nan; x[0, 64] = inf
    x[1, 129] = -inf; x[1, 0] = -inf
    x[2, :] = nan
    x[3, 70] = inf; x[3, 6] = inf; x[3, 7] = -nan
    t = np.array([64, 129, 77, 6, 5])
    out = _scores(gpu, x, t, 8)
    rank, top, _ = ER.batch(x, t, 8)
    assert out["rank"].tolist() == rank.tolist() and out["indices"].tolist() == top.tolist()
    assert out["rank"][:4].tolist() == [2, 129, 77, 1] and out["indices"][0, :3].tolist() == [3, 100, 64]
    assert out["indices"][3, :3].tolist() == [7, 6, 70] and out["indices"][2].tolist() == list(range(8))
    want = np.take_along_axis(x, top, axis=1)
    assert out["values"].view(np.int32).tolist() == want.view(np.int32).tolist()                 # NaN payloads included
    _check("finite neighbour", x, t, out, 8, loss_rows=[4])      # the loss of the rows with specials is not asserted


def test_out_of_range_targets(gpu):
    rng = np.random.default_rng(11)
    C = 65
    x = rng.standard_normal((6, C)).astype(np.float32)
    t = np.array([3, -1, 64, C, 0, -(2 ** 40)])
    out = _scores(gpu, x, t, 4, want_prob=True)
    _check("out of range", x, t, out, 4)
    assert out["rank"][[1, 3, 5]].tolist() == [-1, -1, -1] and (out["rank"][[0, 2, 4]] >= 0).all()
    assert out["loss"][[1, 3, 5]].view(np.int32).tolist() == [0, 0, 0]                           # +0.0f
    ok = _scores(gpu, x[[0, 2, 4]], t[[0, 2, 4]], 4, want_prob=True)                            # the neighbours, alone
    for name in ("rank", "loss", "indices", "values", "probs"):
        assert out[name][[0, 2, 4]].tobytes() == ok[name].tobytes(), name
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import TopKAccuracy
    m = TopKAccuracy((1,))
    m.update(torch.from_numpy(x).to(gpu), torch.from_numpy(t).to(gpu))
    with pytest.raises(VasrError):
        m.compute()


def test_null_outputs_in_each_combination(gpu):
    """Straight through the C ABI: every subset of the five outputs that the argument checks admit gives the bits of the full
    call, and a buffer that was not passed is never written (it is not there)."""
    from viet_asr_amd import _lib
    rng = np.random.default_rng(13)
    B, C, k = 5, 129, 7
    x = torch.from_numpy(rng.standard_normal((B, C)).astype(np.float32)).to(gpu)
    t = torch.from_numpy(rng.integers(0, C, B)).to(gpu)
    names = ("indices", "values", "probs", "rank", "loss")

    def run(want, with_targets=True, kk=k):
        buf = dict(indices=torch.full((B, kk), -7, dtype=torch.int32, device=gpu), values=torch.full((B, kk), -7.0, device=gpu),
                   probs=torch.full((B, kk), -7.0, device=gpu), rank=torch.full((B,), -7, dtype=torch.int32, device=gpu),
                   loss=torch.full((B,), -7.0, device=gpu))
        ptr = [buf[n].data_ptr() if n in want else None for n in names]
        rc = _lib.lib().vasr_class_scores_f32(x.data_ptr(), B, C, t.data_ptr() if with_targets else None, kk, *ptr,
                                              torch.cuda.current_stream().cuda_stream)
        _lib.check(rc)
        return {n: buf[n].cpu().numpy() for n in want}

    full = run(names)
    _check("full", x.cpu().numpy(), t.cpu().numpy(), full, k)
    count = 0
    for r in range(1, 5):
        for want in itertools.combinations(names, r):
            topk = any(n in want for n in names[:3])
            got = run(want, kk=k if topk else 0)
            for n in want:
                assert got[n].tobytes() == full[n].tobytes(), (want, n)
            count += 1
            if not ("rank" in want or "loss" in want):          # without targets as well
                got = run(want, with_targets=False)
                for n in want:
                    assert got[n].tobytes() == full[n].tobytes(), (want, n, "no targets")
    assert count == 30


def test_a_row_does_not_depend_on_its_batch(gpu, golden):
    g = golden
    i = next(i for i in range(int(g["cases"])) if g[f"c{i}_logits"].shape == (67, 257))
    x, t = g[f"c{i}_logits"], g[f"c{i}_targets"]
    big = _scores(gpu, x, t, 5, want_prob=True)
    for r in (0, 1, 2, 3, 4, 33, 63, 64, 65, 66):
        one = _scores(gpu, x[r : r + 1], t[r : r + 1], 5, want_prob=True)
        for name, v in one.items():
            assert v.tobytes() == big[name][r : r + 1].tobytes(), (r, name)
    sub = _scores(gpu, x[60:], t[60:], 5, want_prob=True)        # another position inside the workgroup
    for name, v in sub.items():
        assert v.tobytes() == big[name][60:].tobytes(), name


def test_stage_argument_checks(gpu):
    from viet_asr_amd import stages
    x = torch.zeros((2, 3), device=gpu)
    t = torch.zeros(2, dtype=torch.int64, device=gpu)
    for bad in (lambda: stages.classification_scores(x), lambda: stages.classification_scores(x[0], t),
                lambda: stages.classification_scores(x, t[:1]), lambda: stages.classification_scores(x, t.float()),
                lambda: stages.classification_scores(x, k=4), lambda: stages.classification_scores(x, k=17),
                lambda: stages.classification_scores(x, t, want_prob=True), lambda: stages.classification_scores(x.long(), t),
                lambda: stages.classification_scores(x[:0], t[:0])):
        with pytest.raises(ValueError):
            bad()
    # a strided view and other dtypes are made contiguous float32 / int64 on the device
    y = torch.arange(12, device=gpu, dtype=torch.float64).reshape(3, 4).t()          # [4, 3], not contiguous
    out = stages.classification_scores(y, torch.tensor([2, 2, 0, 1], dtype=torch.int32, device=gpu), k=1)
    assert out["indices"].view(-1).tolist() == [2, 2, 2, 2] and out["rank"].tolist() == [0, 0, 2, 1]
    assert sorted(stages.classification_scores(x, k=2)) == ["indices", "values"]
    assert sorted(stages.classification_scores(x, t)) == ["loss", "rank"]
    assert sorted(stages.classification_scores(x, t, want_loss=False)) == ["rank"]


def test_engine_evaluate_manifest_and_classify_topk(gpu, tmp_path):
    from viet_asr_amd import audio
    from viet_asr_amd.data_layer import AudioToSpeechLabelDataLayer
    from viet_asr_amd.engine import QuartzNetClassifier
    g, cfg, jas = CR.load("cls_pad_avg_rows3")                   # 35 classes; every clip below stays under audio_length frames
    enc_sd, dec_sd = CR.fixture_weights(g, jas)
    sig, lens = CR.signals(g["lens"], int(g["seed"]))
    names = [f"word{i}" for i in range(int(g["num_classes"]))]
    eng = QuartzNetClassifier(cfg, enc_sd, dec_sd, int(g["audio_length"]), labels=names, pooling_type=str(g["pooling_type"]),
                              gemm="fp32")
    cuts = [(0, 16000), (1, 9011), (2, 12503), (0, 11000), (1, 7000), (2, 9500), (0, 13777)]
    targets = [(5 * i + 3) % len(names) for i in range(len(cuts))]
    clips, lines = [], []
    for i, (row, n) in enumerate(cuts):
        path = str(tmp_path / f"clip{i}.wav")
        audio.write_wav(path, sig[row, :n], 16000)
        clips.append(audio.read_wav(path)[0])
        lines.append({"audio_filepath": path, "duration": n / 16000.0, "label": names[targets[i]]})
    man = str(tmp_path / "manifest.json")
    with open(man, "w", encoding="utf-8") as f:
        f.write("\n".join(json.dumps(e) for e in lines) + "\n")

    preds, res = eng.evaluate_manifest(man, batch_size=3, top_k=(1, 3), row_independent=True)
    assert preds == eng.classify(clips, row_independent=True)
    # the host's answer from forward's logits: rows are bit-equal alone and in any batch (row_independent)
    logits = eng.forward(*eng._collate(clips, True), row_independent=True).cpu().numpy()
    rank, top, loss = ER.batch(logits, targets, 3)
    assert preds == [names[c] for c in top[:, 0]]
    assert res["samples"] == 7 and res["correct"] == {1: ER.hits(rank, 1), 3: ER.hits(rank, 3)}
    assert res["accuracy"] == {k: res["correct"][k] / 7 for k in (1, 3)}
    order = AudioToSpeechLabelDataLayer(man, names, 3).utterance_order()
    batches = [order[0:3], order[3:6], order[6:7]]
    means = [loss[b].mean() for b in batches]
    bounds = [[ER.loss_bound(logits[i], targets[i]) for i in b] for b in batches]
    assert abs(res["eval_loss"] - np.mean(means)) <= ER.mean_of_means_bound([3, 3, 1], bounds, means)

    best = eng.classify_topk(clips, 3, row_independent=True)
    assert [b[0][0] for b in best] == preds and all(len(b) == 3 for b in best)
    for r, b in enumerate(best):
        assert [n for n, _ in b] == [names[c] for c in top[r]]
        p = np.array([q for _, q in b])
        assert (np.abs(p - ER.prob64(logits[r], top[r])) <= ER.prob_bound(logits[r], top[r])).all()
        assert p.sum() <= 1.0
    with pytest.raises(ValueError):
        eng.classify_topk(clips, 0)
    with pytest.raises(ValueError):
        eng.classify_topk(clips, 17)
