"""CPU checks of the CTC evaluation loss: the float64 and float32 restatements (tests/ctc_reference.py) against the fixture
the reference's own CTCLossNM and evaluation helpers wrote (tests/golden/ctc_cases.npz, make_golden_ctc.py) -- every +inf
exactly, every loss inside the bound, and the bound not vacuous: each rule of the recursion, broken in turn, moves a fixture
row by more than ten bounds --, the exported symbol / signature / header declaration with the ABI still 8, every refusal of
vasr_ctc_loss_f32 before a device is touched, the evaluation helpers on host tensors, and the host arithmetic of
``CTCEvalLoss.compute``."""
import math
import os

import numpy as np
import pytest
import torch

import ctc_reference as CR
from conftest import GOLDEN_DIR, ROOT

INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "ctc_cases.npz"), allow_pickle=False)


def cases(g):
    for i in range(int(g["cases"])):
        yield i, g[f"c{i}_logp"], g[f"c{i}_frames"], g[f"c{i}_tgt"], g[f"c{i}_tgt_len"]


@pytest.fixture(scope="module")
def restated(golden):
    """(loss64 [B], bound [B]) of every fixture case, computed once"""
    return {i: CR.batch(lp, fr, tg, tl, lp.shape[2] - 1) for i, lp, fr, tg, tl in cases(golden)}


def test_fixture_covers_the_cases_the_issue_names(golden):
    g = golden
    classes, batches, lengths, kinds, scales = set(), set(), set(), set(), set()
    repeats = {False: 0, True: 0}
    neg_inf_rows = 0
    for i, lp, fr, tg, tl in cases(g):
        assert lp.dtype == np.float32 and tg.dtype == fr.dtype == tl.dtype == np.int64 and not np.isnan(lp).any()
        assert lp.shape[1] > fr.max() and tg.shape[1] > tl.max()          # something real sits behind every length
        classes.add(lp.shape[2]); batches.add(lp.shape[0]); scales.add(float(g[f"c{i}_scale"]))
        lengths |= set(tl.tolist()); kinds |= set(g[f"c{i}_kinds"].tolist())
        for b in range(len(fr)):
            y = tg[b, : tl[b]]
            if len(y) > 1:
                repeats[bool((y[1:] == y[:-1]).any())] += 1
            neg_inf_rows += bool(np.isneginf(lp[b, : fr[b]]).any())
            assert not np.isnan(g[f"c{i}_loss"][b])                        # the reference is defined on every row
    assert classes == {2, 5, 29, 96} and batches == {1, 3, 5} and lengths == {0, 1, 2, 31, 32, 33}
    assert kinds == {0, 1, 2, 3} and scales == {0.1, 8.0} and repeats[False] and repeats[True] and neg_inf_rows == 1
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "ctc_cases.npz")) < 600 * 1000


def test_float64_restatement_has_every_inf_and_the_reference_lies_inside_the_bound(golden, restated):
    g = golden
    infs = finite = single_path = 0
    for i, lp, fr, tg, tl in cases(g):
        l64, bound = restated[i]
        ref32 = g[f"c{i}_loss"]
        assert ref32.dtype == np.float32
        for b in range(len(fr)):
            need = CR.min_frames(tg[b], tl[b])
            if fr[b] < need:
                assert ref32[b] == np.inf and l64[b] == np.inf, (i, b)        # exactly, from both
                infs += 1
            elif np.isfinite(l64[b]):
                finite += 1
                single_path += int(fr[b] == need and tl[b] > 0)
            assert CR.close(ref32[b], l64[b], bound[b]), (i, b, float(ref32[b]), l64[b], bound[b])
        # the batch mean of CTCLossNM._loss: torch.mean of the rows
        if np.isfinite(l64).all():
            assert abs(float(g[f"c{i}_mean"]) - l64.mean()) <= CR.mean_bound(bound, l64.mean()), i
        else:
            assert float(g[f"c{i}_mean"]) == np.inf
    assert infs >= 5 and finite >= 20 and single_path >= 3


def test_float32_restatement_lies_inside_the_bound(golden, restated):
    for i, lp, fr, tg, tl in cases(golden):
        l64, bound = restated[i]
        for b in range(len(fr)):
            got = CR.loss32(lp[b], fr[b], tg[b], tl[b], lp.shape[2] - 1)
            assert got.dtype == np.float32 and CR.close(got, l64[b], bound[b]), (i, b, float(got), l64[b], bound[b])


@pytest.mark.parametrize("rule", CR.BROKEN)
def test_bound_is_not_vacuous(golden, restated, rule):
    """Each rule of the recursion, broken in the float64 restatement, moves at least one fixture row by more than 10 x that
    row's bound."""
    moved = []
    for i, lp, fr, tg, tl in cases(golden):
        l64, bound = restated[i]
        for b in range(len(fr)):
            v = CR.loss64(lp[b], fr[b], tg[b], tl[b], lp.shape[2] - 1, broken=rule)
            if bound[b] > 0 and np.isfinite(l64[b]) and np.isfinite(v) and abs(v - l64[b]) > 10 * bound[b]:
                moved.append((i, b, abs(v - l64[b]) / bound[b]))
    assert moved, rule


def test_restatement_conventions_and_the_cases_torch_defines():
    rng = np.random.default_rng(3)
    lp = np.log(rng.dirichlet(np.ones(4), size=6)).astype(np.float32)         # [6][4], blank 3
    tgt = np.array([0, 1, 1, 2])
    nan, inf = math.isnan, float("inf")
    assert nan(CR.loss64(lp, -1, tgt, 2, 3)) and nan(CR.loss64(lp, 3, tgt, -2, 3))
    assert nan(CR.loss64(lp, 6, np.array([0, 3, 1]), 3, 3)) and nan(CR.loss64(lp, 6, np.array([0, 4]), 2, 3))
    assert nan(CR.loss64(lp, 6, np.array([-1, 0]), 2, 3))
    assert not nan(CR.loss64(lp, 6, np.array([0, 3, 9, -5]), 1, 3))           # ids behind the length are not looked at
    assert CR.loss64(lp, 0, tgt, 0, 3) == 0.0 and CR.loss64(lp, 0, tgt, 1, 3) == inf
    assert CR.loss64(lp, 4, tgt, 4, 3) == inf and CR.loss64(lp, 3, tgt, 4, 3) == inf       # 4 ids, one repeat: 5 frames
    assert abs(CR.loss64(lp, 5, tgt, 4, 3) + float(lp[[0, 1, 2, 3, 4], [0, 1, 3, 1, 2]].astype(np.float64).sum())) < 1e-12
    assert abs(CR.loss64(lp, 4, tgt, 0, 3) + float(lp[:4, 3].astype(np.float64).sum())) < 1e-12   # L == 0: the blank's sum
    assert CR.loss64(lp, 99, tgt, 2, 3) == CR.loss64(lp, 6, tgt, 2, 3)        # lengths are clamped
    assert CR.loss64(lp, 6, tgt, 99, 3) == CR.loss64(lp, 6, tgt, 4, 3)
    # against torch's own float64 loss
    want = torch.nn.functional.ctc_loss(torch.from_numpy(lp).double()[:, None], torch.from_numpy(tgt)[None], torch.tensor([6]),
                                        torch.tensor([4]), blank=3, reduction="none")
    assert abs(CR.loss64(lp, 6, tgt, 4, 3) - float(want)) < 1e-12
    # a -inf log-prob never makes a NaN
    lp2 = lp.copy()
    lp2[:, 3] = -np.inf
    assert CR.loss64(lp2, 6, tgt, 4, 3) == inf and np.isposinf(CR.loss32(lp2, 6, tgt, 4, 3))
    assert math.isfinite(CR.loss64(lp2, 3, np.array([0, 1, 2]), 3, 3))


def test_new_symbol_is_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    n = "vasr_ctc_loss_f32"
    assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert len(_lib.SIGNATURES[n][1]) == 11
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    decl = header[header.index(f" {n}("):]
    decl = decl[: decl.index(";")]
    assert decl.count(",") == 10 and "quiet NaN" in header and "bit-identical whatever batch" in header


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f = L.vasr_ctc_loss_f32
    p = 4096
    ok = dict(x=p, fr=p, b=2, t=10, c=5, blank=4, tgt=p, w=3, tl=p, loss=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["fr"], a["b"], a["t"], a["c"], a["blank"], a["tgt"], a["w"], a["tl"], a["loss"], None)

    for name in ("x", "fr", "tgt", "tl", "loss"):
        assert call(**{name: None}) == INVALID, name
    assert call(b=0) == INVALID and call(b=-3) == INVALID and call(t=-1) == INVALID and call(w=-1) == INVALID
    assert call(c=1, blank=0) == INVALID and call(c=0, blank=0) == INVALID
    assert call(blank=-1) == INVALID and call(blank=5) == INVALID
    assert call(w=4097) == UNSUPPORTED and call(w=1 << 40) == UNSUPPORTED
    assert b"4096" in L.vasr_last_error()
    assert call(w=4097, b=0) == INVALID                          # an argument error wins over the size limit
    with pytest.raises(NotImplementedError):
        _lib.check(call(w=5000), L)
    with pytest.raises(ValueError):
        _lib.check(call(b=0), L)


def test_stage_refuses_host_tensors_and_bad_shapes():
    from viet_asr_amd import stages
    from viet_asr_amd._lib import VasrError
    i64 = torch.int64
    with pytest.raises(VasrError):
        stages.ctc_loss(torch.zeros(2, 3, 4), torch.tensor([3, 3]), torch.zeros(2, 1, dtype=i64), torch.tensor([1, 1]), 3)


def test_module_ports():
    from viet_asr_amd import asr
    m = asr.CTCLossNM(num_classes=28)
    assert sorted(m.input_ports) == ["input_length", "log_probs", "target_length", "targets"] and list(m.output_ports) == ["loss"]
    assert m._blank == 28 and "CTCLossNM" in asr.__all__ and "training stays out of scope" in " ".join(asr.CTCLossNM.__doc__.split())


def _epoch_tensors(g, j):
    return {"loss": [torch.tensor(g["epoch_batch_losses"][j], dtype=torch.float32)], "predictions": [],
            "transcript": [torch.from_numpy(g[f"epoch{j}_tgt"])], "transcript_length": [torch.from_numpy(g[f"epoch{j}_tgt_len"])],
            "output": [torch.from_numpy(g[f"epoch{j}_logp"])]}


def test_helpers_reproduce_the_stored_epoch_from_host_tensors(golden):
    """What needs no device: the losses, the transcripts and the epoch's figures.  (The predictions are collapsed on the
    device: tests/test_gpu_ctc.py; here the reference's own strings stand in for them.)"""
    from viet_asr_amd import helpers
    g = golden
    labels = g["epoch_labels"].tolist()
    gv = {}
    for j in range(3):
        helpers.process_evaluation_batch(_epoch_tensors(g, j), gv, labels)
    assert sorted(gv) == ["EvalLoss", "logits", "predictions", "transcripts"]
    assert gv["transcripts"] == g["epoch_transcripts"].tolist() and gv["predictions"] == [] and len(gv["logits"]) == 3
    assert [float(v) for v in gv["EvalLoss"]] == g["epoch_batch_losses"].tolist()
    both = [torch.from_numpy(g[f"epoch{j}_tgt"]) for j in range(3)], [torch.from_numpy(g[f"epoch{j}_tgt_len"]) for j in range(3)]
    assert helpers.post_process_transcripts(*both, labels) == g["epoch_transcripts"].tolist()
    gv["predictions"] = g["epoch_predictions"].tolist()
    logs = helpers.process_evaluation_epoch(gv)
    assert logs == {"Evaluation_Loss": float(g["epoch_loss"]), "Evaluation_Valid_WER": float(g["epoch_wer"]),
                    "Evaluation_Valid_CER": float(g["epoch_cer"])}
    tagged = helpers.process_evaluation_epoch(gv, eval_metric="cer", tag="dev")
    assert sorted(tagged) == ["Evaluation_Loss_dev", "Evaluation_Valid_CER", "Evaluation_Valid_WER"]
    assert tagged["Evaluation_Loss_dev"] == logs["Evaluation_Loss"] and tagged["Evaluation_Valid_WER"] == logs["Evaluation_Valid_WER"]
    with pytest.raises(ValueError, match="eval_metric must be 'WER' or 'CER'"):
        helpers.process_evaluation_epoch(gv, eval_metric="PER")
    with pytest.raises(ValueError):
        helpers.process_evaluation_batch({"loss": [torch.tensor(1.0)]}, {}, labels)
    # the mean of the batch means is not the mean over the utterances
    rows = np.concatenate([g[f"epoch{j}_loss"] for j in range(3)]).astype(np.float64)
    assert abs(rows.mean() - logs["Evaluation_Loss"]) > 1e-2


def test_ctc_eval_loss_host_arithmetic():
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import CTCEvalLoss
    m = CTCEvalLoss(28)
    assert m.blank == 28
    r = m.compute()
    assert math.isnan(r["eval_loss"]) and r["loss_sum"] == 0.0 and r["scored"] == 0 and r["infeasible"] == 0
    f32, inf, nan = torch.float32, float("inf"), float("nan")
    m.add_losses(torch.tensor([1, 2, 3, 4, 5, 6], dtype=f32))          # mean 3.5
    m.add_losses(torch.tensor([0.5], dtype=f32))                       # mean 0.5
    r = m.compute()
    assert r == dict(eval_loss=2.0, loss_sum=21.5, scored=7, infeasible=0)                   # NOT 21.5 / 7
    assert m.compute(reduce=True) == r                                                       # no process group
    m.add_losses(torch.tensor([2.0, inf, 4.0], dtype=f32))
    r = m.compute()
    assert r == dict(eval_loss=inf, loss_sum=27.5, scored=9, infeasible=1)                   # the reference's mean is inf too
    m.add_losses(torch.tensor([1.0, nan], dtype=f32))
    with pytest.raises(VasrError):
        m.compute()
    m.reset()
    m.add_losses(torch.tensor([7.0], dtype=f32))
    assert m.compute() == dict(eval_loss=7.0, loss_sum=7.0, scored=1, infeasible=0)
