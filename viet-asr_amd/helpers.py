"""Greedy CTC post-processing: counterpart of nemo/collections/asr/helpers.py:7-33, 207-208.

The reference collapses predictions in a Python loop over every frame of every utterance; here the
collapse runs on the device (vasr_ctc_collapse: ballot + popcount compaction, one wavefront per
utterance) and only the id -> label join happens on the host.  Like the reference it walks ALL T'
frames, including padded ones (quirk Q4).

Evaluation of the CTC path (helpers.py:128-212): ``process_evaluation_batch`` / ``process_evaluation_epoch`` /
``post_process_transcripts`` keep the reference's signatures, ``global_vars`` keys and returned dict.  The batch's loss is what
``asr.CTCLossNM`` (or ``stages.ctc_loss``) computed on the device; it stays a device scalar until the epoch function.

Classification (helpers.py:81-113, 215-288): the three functions keep the reference's signatures and ``global_vars`` keys
and take their top-k hits from ``stages.classification_scores``; the per-batch entries stay device tensors until the epoch
function, which is the one place that synchronises.
"""
import logging

import torch

from . import stages
from .metrics import top_k_hits


def ctc_decoder_predictions_tensor(tensor, labels):
    """[B, T'] predictions -> list of B strings (helpers.py:7-33)."""
    blank_id = len(labels)
    t = torch.as_tensor(tensor).long()
    if t.device.type != "cuda":
        if not torch.cuda.is_available():
            from ._lib import VasrError
            raise VasrError("viet-asr_amd needs a HIP device; there is no CPU fallback for this path")
        t = t.cuda()
    ids, n = stages.ctc_collapse(t, blank_id)
    ids, n = ids.cpu().numpy(), n.cpu().numpy()
    return ["".join(labels[c] for c in ids[b, : n[b]]) for b in range(ids.shape[0])]


def post_process_predictions(predictions, labels):
    """helpers.py:207-208 -> __gather_predictions (:120-125): list of [B,T'] tensors -> flat list of strings."""
    results = []
    for prediction in predictions:
        results += ctc_decoder_predictions_tensor(prediction, labels=labels)
    return results


def post_process_transcripts(transcript_list, transcript_len_list, labels):
    """helpers.py:211-212 -> __gather_transcripts (:128-143): lists of [B,T] id tensors and [B] lengths (any device) -> flat
    list of strings, every row over its own length.  One host copy per tensor."""
    results = []
    for t, ln in zip(transcript_list, transcript_len_list):
        ids, n = torch.as_tensor(t).long().cpu().numpy(), torch.as_tensor(ln).long().cpu().numpy()
        results += ["".join(labels[c] for c in ids[b, : n[b]]) for b in range(ids.shape[0])]
    return results


def process_evaluation_batch(tensors, global_vars, labels):
    """Counterpart of helpers.py:146-172: one batch into the running lists of ``global_vars`` -- ``EvalLoss`` (the mean of
    the batch's loss tensors), ``predictions`` and ``transcripts`` (strings) and ``logits``.  tensors: lists of tensors under
    keys matched by prefix, in the reference's order of precedence: ``loss*`` (what ``asr.CTCLossNM`` returned), ``predictions*``
    ([B,T'] greedy predictions, collapsed on the device), ``transcript_length*``, ``transcript*`` and ``output*``.  The loss
    entry stays a device scalar: nothing synchronises on it before the epoch function."""
    for key in ("EvalLoss", "predictions", "transcripts", "logits"):
        global_vars.setdefault(key, [])
    transcript_list = transcript_len_list = None
    for kv, v in tensors.items():
        if kv.startswith("loss"):
            global_vars["EvalLoss"] += [torch.mean(torch.stack([torch.as_tensor(x) for x in v]))]
        elif kv.startswith("predictions"):
            global_vars["predictions"] += post_process_predictions(v, labels)
        elif kv.startswith("transcript_length"):
            transcript_len_list = v
        elif kv.startswith("transcript"):
            transcript_list = v
        elif kv.startswith("output"):
            global_vars["logits"] += list(v)
    if transcript_list is None or transcript_len_list is None:
        raise ValueError("tensors must hold the transcripts and their lengths (keys starting with 'transcript' and "
                         "'transcript_length')")
    global_vars["transcripts"] += post_process_transcripts(transcript_list, transcript_len_list, labels)


def process_evaluation_epoch(global_vars, eval_metric="WER", tag=None):
    """Counterpart of helpers.py:175-204: ``Evaluation_Loss`` (``Evaluation_Loss_{tag}`` with a tag) -- the float32 mean of
    the batch means in ``EvalLoss`` --, ``Evaluation_Valid_WER`` and ``Evaluation_Valid_CER`` over the gathered strings.  Both
    rates are always returned; eval_metric is only checked ('WER' or 'CER', ValueError otherwise), as there.  The one place
    that synchronises on the losses."""
    from .data_layer import word_error_rate
    eloss = torch.stack([torch.as_tensor(v, dtype=torch.float32).cpu() for v in global_vars["EvalLoss"]]).mean().item()
    hypotheses, references = global_vars["predictions"], global_vars["transcripts"]
    eval_metric = eval_metric.upper()
    if eval_metric not in {"WER", "CER"}:
        raise ValueError("eval_metric must be 'WER' or 'CER'")
    wer = word_error_rate(hypotheses, references, use_cer=False)
    cer = word_error_rate(hypotheses, references, use_cer=True)
    logging.info("==========>>>>>>Evaluation Loss%s: %s", "" if tag is None else f" {tag}", eloss)
    logging.info("==========>>>>>>Evaluation Valid WER: %5.2f%%", wer * 100)
    logging.info("==========>>>>>>Evaluation Valid CER: %5.2f%%", cer * 100)
    return {"Evaluation_Loss" if tag is None else f"Evaluation_Loss_{tag}": eloss, "Evaluation_Valid_WER": wer,
            "Evaluation_Valid_CER": cer}


def _k_list(eval_metric):
    if eval_metric is None:
        return [1]
    return list(eval_metric) if isinstance(eval_metric, (list, tuple)) else [eval_metric]


def _reference_accuracy(rank, top_k):
    """Per k of top_k, the figure the reference's classification_accuracy returns (metrics.classification_accuracy: hits /
    (k * B)) as a float32 device scalar."""
    hits = top_k_hits(rank, top_k).to(torch.float32)
    rows = int(rank.shape[0])
    # tensor / tensor: a correctly rounded float32 division, as the reference's mean (a scalar divisor may be turned into a
    # multiplication by its reciprocal)
    return [hits[i] / torch.full((), float(k * rows), dtype=torch.float32, device=rank.device) for i, k in enumerate(top_k)]


def monitor_classification_training_progress(tensors, eval_metric=None, tb_logger=None):
    """Counterpart of helpers.py:81-113.  tensors: [loss, logits, targets]; eval_metric: a k or a list of them (default
    [1]).  Logs the loss and, per k, ``training_batch_top@k`` in percent; ``tb_logger.add_scalar`` gets the same tag with the
    fraction.  The figures come back from the device in one copy."""
    top_k = _k_list(eval_metric)
    loss, logits, targets = tensors
    rank = stages.classification_scores(logits, targets, want_loss=False)["rank"]
    accs = torch.stack(_reference_accuracy(rank, [int(k) for k in top_k])).cpu().numpy()
    logging.info("Loss: %s", loss)
    for k, acc in zip(top_k, accs):
        name = f"training_batch_top@{k}"
        if tb_logger is not None:
            tb_logger.add_scalar(name, acc)
        logging.info("%s: %.4f", name, acc * 100.0)


def process_classification_evaluation_batch(tensors, global_vars, top_k=1):
    """Counterpart of helpers.py:215-253: one batch into the running lists of ``global_vars`` -- ``EvalLoss`` (the batch's
    mean loss), ``batchsize`` and, per k of the sorted top_k, ``CorrectCount@k`` (``classification_accuracy`` x batch size).
    tensors: lists of tensors under keys starting with ``logits`` and ``label`` (concatenated), optionally the batch's loss
    tensors under a key starting with ``loss``; without one the loss is the stage's, the mean cross entropy of the batch,
    and only then does the launch compute it.  Everything appended but the batch size is a device scalar; nothing
    synchronises."""
    ks = sorted([top_k] if isinstance(top_k, int) else top_k)
    own_loss = [v for name, v in tensors.items() if name.startswith("loss")]
    logits = torch.cat(list(next(v for name, v in tensors.items() if name.startswith("logits"))), 0)
    labels = torch.cat(list(next(v for name, v in tensors.items() if name.startswith("label"))), 0)
    scores = stages.classification_scores(logits, labels, want_loss=not own_loss)
    rows = int(labels.shape[0])
    batch_losses = [torch.stack(list(v)).mean() for v in own_loss] or [scores["loss"].mean()]
    global_vars.setdefault("EvalLoss", []).extend(batch_losses)
    global_vars.setdefault("batchsize", []).append(rows)
    for k, acc in zip(ks, _reference_accuracy(scores["rank"], ks)):
        global_vars.setdefault(f"CorrectCount@{k}", []).append(acc * rows)


def process_classification_evaluation_epoch(global_vars, eval_metric=None, tag=None):
    """Counterpart of helpers.py:256-288: the epoch's dict from what the batch function gathered -- ``Evaluation_Loss {tag}``,
    the mean of the batch means, and per k of eval_metric ``Evaluation_Accuracy_Top@{k} {tag}`` in percent (a float32
    tensor, as there).  The one place that synchronises: the entries are copied to the host and reduced there in float32."""
    tag = "" if tag is None else tag
    host = lambda entries: torch.stack([torch.as_tensor(v, dtype=torch.float32) for v in entries]).cpu()  # noqa: E731
    samples = torch.tensor(global_vars["batchsize"]).sum().float()
    logs = {f"Evaluation_Loss {tag}": host(global_vars["EvalLoss"]).mean().item()}
    for k in _k_list(eval_metric):
        logs[f"Evaluation_Accuracy_Top@{k} {tag}"] = host(global_vars[f"CorrectCount@{k}"]).sum() / samples * 100.0
    for name, value in logs.items():
        logging.info("%s: %s", name, float(value))
    return logs
