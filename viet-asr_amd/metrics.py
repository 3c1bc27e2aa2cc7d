"""Word and character error rate on device id sequences; top-k accuracy and evaluation loss on classification logits.

Reference: nemo/collections/asr/metrics.py:30-63 (``word_error_rate``, both ``use_cer`` settings) as
``process_evaluation_epoch`` reports them (helpers.py:188-189), scored on the parsed token tensors the data layer delivers
(``__gather_transcripts``, helpers.py:128-143) -- not on raw manifest text.  The edit distances are computed per row by
``stages.error_counts`` (vasr_error_counts_i32, csrc/metrics.hip); this module only sums four integers on the device and
divides them once on the host.  ``data_layer.word_error_rate`` is the same metric on host strings; the two differ only
where a reference holds characters outside the labels, which the character parser drops before the tokens are made.
``ErrorBreakdown`` splits the edits into substitutions, deletions and insertions (``stages.error_ops``, vasr_error_ops_i32),
``word_alignment`` / ``confusion_pairs`` report which words were confused, and ``OracleErrorRate`` scores the best hypothesis
of the beam search's n-best list (``stages.nbest_error_counts``, vasr_nbest_error_counts_i32).

``classification_accuracy`` (metrics.py:66-99) and ``TopKAccuracy`` (the running form of
process_classification_evaluation_batch / _epoch, helpers.py:215-288) rest on ``stages.classification_scores``
(vasr_class_scores_f32, csrc/cls_eval.hip): the target's rank among the row's classes and its cross-entropy loss per row.

``CTCEvalLoss`` is the ``Evaluation_Loss`` of the ASR path (helpers.py:146-204 with CTCLossNM, losses.py): the running mean
of the batch means of ``stages.ctc_loss`` (vasr_ctc_loss_f32, csrc/ctc_loss.hip), with the per-utterance sums beside it.
"""
import torch

from . import _lib, dist, stages


def space_ids(labels):
    """The label ids ``str.split()`` separates on.  Raises NotImplementedError for labels that are not single characters:
    an id row is then no longer ``list(text)``."""
    labels = list(labels)
    multi = [c for c in labels if not isinstance(c, str) or len(c) != 1]
    if multi:
        raise NotImplementedError(f"labels must be single characters (an id row has to equal list(text)); got {multi[:4]!r}")
    ids = [i for i, c in enumerate(labels) if c.isspace()]
    if len(ids) > 8:
        raise NotImplementedError(f"{len(ids)} whitespace labels; vasr_error_counts_i32 takes at most 8")
    return ids


def _rates(totals):
    """[word_edits, ref_words, char_edits, ref_chars] (host integers) -> the result dict; a zero denominator gives
    float('inf'), as metrics.py:59-62 does."""
    we, rw, ce, rc = (int(v) for v in totals)
    return dict(wer=1.0 * we / rw if rw else float("inf"), cer=1.0 * ce / rc if rc else float("inf"),
                word_edits=we, ref_words=rw, char_edits=ce, ref_chars=rc)


class ErrorRate:
    """Running WER / CER over batches.  ``update`` enqueues and never synchronises; ``compute`` is the one sync."""

    def __init__(self, labels):
        self.space_ids = space_ids(labels)
        self._acc = None          # int64 [5]: the four sums + the number of rows that came back as -1

    def update(self, ids, id_len, transcripts, transcript_length):
        """ids [B,T'] / id_len [B]: collapsed hypothesis ids (``engine.forward``, the beam search); transcripts [B,T] /
        transcript_length [B]: the data layer's ports.  All on the device; enqueued on the current stream."""
        self._add(stages.error_counts(ids, id_len, transcripts, transcript_length, self.space_ids))

    def _add(self, counts):
        """counts [B,4] i32 of ``stages.error_counts`` -> the accumulator, without a host round trip."""
        # a row is either four counts >= 0 or four -1 (vasr.h): clamping drops the reported rows from the sums
        sums = counts.clamp_min(0).sum(dim=0, dtype=torch.int64)
        row = torch.cat([sums, (counts[:, 0] < 0).sum(dtype=torch.int64).reshape(1)])
        self._acc = row if self._acc is None else self._acc + row

    def reset(self):
        self._acc = None

    def compute(self, reduce=False, group=None):
        """-> {"wer", "cer", "word_edits", "ref_words", "char_edits", "ref_chars"}.  reduce=True sums over the process
        group first (``dist.all_reduce_counts``).  Raises VasrError when a row reported the beam search's overflow
        (a length of -1)."""
        acc = self._acc if self._acc is not None else torch.zeros(5, dtype=torch.int64)
        if reduce:
            acc = dist.all_reduce_counts(acc, group)
        host = acc.cpu().tolist()
        if host[4]:
            raise _lib.VasrError(f"{host[4]} scored rows carried a negative length (the beam search's id_len = -1 overflow "
                                 "report): no error rate is returned for them")
        return _rates(host[:4])


OPS_KEYS = ("word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del", "char_ins", "char_hits")


class ErrorBreakdown:
    """``ErrorRate`` with the edits split into substitutions, deletions and insertions, and the hits, at both levels
    (``stages.error_ops``, the alignment rule of include/vasr.h).  ``update`` enqueues and never synchronises; ``compute`` is
    the one sync.  The six keys it shares with ``ErrorRate`` carry the same values: edits = sub + del + ins, reference
    count = hits + sub + del."""

    def __init__(self, labels):
        self.space_ids = space_ids(labels)
        self._acc = None          # int64 [9]: the eight sums + the number of rows that came back as -1

    def update(self, ids, id_len, transcripts, transcript_length):
        """Arguments as ``ErrorRate.update``; all on the device, enqueued on the current stream."""
        self._add(stages.error_ops(ids, id_len, transcripts, transcript_length, self.space_ids))

    def _add(self, ops):
        """ops [B,8] i32 of ``stages.error_ops`` -> the accumulator, without a host round trip."""
        sums = ops.clamp_min(0).sum(dim=0, dtype=torch.int64)
        row = torch.cat([sums, (ops[:, 0] < 0).sum(dtype=torch.int64).reshape(1)])
        self._acc = row if self._acc is None else self._acc + row

    def reset(self):
        self._acc = None

    def compute(self, reduce=False, group=None):
        """-> ``ErrorRate.compute``'s six keys + "word_sub", "word_del", "word_ins", "word_hits", "char_sub", "char_del",
        "char_ins", "char_hits".  reduce=True sums over the process group first.  Raises VasrError on -1 rows."""
        acc = self._acc if self._acc is not None else torch.zeros(9, dtype=torch.int64)
        if reduce:
            acc = dist.all_reduce_counts(acc, group)
        host = [int(v) for v in acc.cpu().tolist()]
        if host[8]:
            raise _lib.VasrError(f"{host[8]} scored rows carried a negative length (the beam search's id_len = -1 overflow "
                                 "report): no error rate is returned for them")
        ws, wd, wi, wh, cs, cd, ci, ch = host[:8]
        out = _rates([ws + wd + wi, wh + ws + wd, cs + cd + ci, ch + cs + cd])
        out.update(zip(OPS_KEYS, host[:8]))
        return out


class OracleErrorRate:
    """Running oracle WER / CER of n-best lists: per utterance the hypothesis with the fewest word edits, and (independently)
    the one with the fewest character edits, among the slots the search filled (``stages.nbest_error_counts``).  The gap to
    the 1-best ``ErrorRate`` is what rescoring the list could gain at most.  ``update`` enqueues and never synchronises."""

    def __init__(self, labels):
        self.space_ids = space_ids(labels)
        self._acc = None          # as ErrorRate's

    def update(self, nbest_ids, nbest_len, count, transcripts, transcript_length):
        """nbest_ids [B,N,T] / nbest_len [B,N] / count [B]: ``DeviceBeamDecoder.decode_beams_ids``' first three results;
        transcripts [B,Tr] / transcript_length [B].  All on the device; enqueued on the current stream."""
        self._add(stages.nbest_error_counts(nbest_ids, nbest_len, count, transcripts, transcript_length, self.space_ids)["counts"])

    _add = ErrorRate._add
    reset = ErrorRate.reset

    def compute(self, reduce=False, group=None):
        """-> {"oracle_wer", "oracle_cer", "word_edits", "ref_words", "char_edits", "ref_chars"} (the edits are the minima's
        sums).  Raises VasrError when a row could not be scored (a negative length, no filled slot)."""
        r = ErrorRate.compute(self, reduce, group)
        return dict(oracle_wer=r["wer"], oracle_cer=r["cer"], word_edits=r["word_edits"], ref_words=r["ref_words"],
                    char_edits=r["char_edits"], ref_chars=r["ref_chars"])


OP_NAMES = ("hit", "sub", "del", "ins")


def word_alignment(ids, id_len, transcripts, transcript_length, labels):
    """The word alignment of every (hypothesis, reference) row: per row a list of (op, hyp_word | None, ref_word | None), op
    in "hit", "sub", "del", "ins", first word to last, by the alignment rule of include/vasr.h (``stages.error_ops`` with
    script=True: rows of at most 1024 ids).  Words are strings over ``labels``.  For reporting: this call synchronises (the
    scripts and the ids are copied to the host).  Raises VasrError for a row with a negative length."""
    labels = list(labels)
    sp = space_ids(labels)
    _, script, script_len = stages.error_ops(ids, id_len, transcripts, transcript_length, sp, script=True)
    script, script_len = script.cpu().numpy(), script_len.cpu().numpy()
    if (script_len < 0).any():
        raise _lib.VasrError("rows %s carried a negative length (the beam search's id_len = -1 overflow report): no alignment "
                             "is returned for them" % (script_len < 0).nonzero()[0].tolist())
    hyp, hyp_n = ids.cpu().numpy(), id_len.cpu().numpy()
    ref, ref_n = transcripts.cpu().numpy(), transcript_length.cpu().numpy()
    rows = []
    for b in range(script.shape[0]):
        h = "".join(labels[c] for c in hyp[b, : hyp_n[b]].tolist()).split()
        r = "".join(labels[c] for c in ref[b, : ref_n[b]].tolist()).split()
        i = j = 0
        row = []
        for code in script[b, : script_len[b]].tolist():
            hw = rw = None
            if code != 2:
                hw, i = h[i], i + 1
            if code != 3:
                rw, j = r[j], j + 1
            row.append((OP_NAMES[code], hw, rw))
        assert i == len(h) and j == len(r), (b, i, len(h), j, len(r))
        rows.append(row)
    return rows


def confusion_pairs(alignments):
    """``word_alignment``'s rows -> collections.Counter of (ref_word, hyp_word) over the substitutions."""
    from collections import Counter
    return Counter((rw, hw) for row in alignments for op, hw, rw in row if op == "sub")


def word_error_rate_ids(ids, id_len, transcripts, transcript_length, labels, use_cer=False):
    """One-shot functional form: ``word_error_rate`` of one batch of device id rows (metrics.py:30-63)."""
    m = ErrorRate(labels)
    m.update(ids, id_len, transcripts, transcript_length)
    return m.compute()["cer" if use_cer else "wer"]


def _top_k_list(top_k):
    ks = [int(k) for k in ([top_k] if isinstance(top_k, int) else top_k)]
    if not ks or min(ks) < 1:
        raise ValueError(f"top_k must hold integers >= 1, got {top_k!r}")
    return ks


def top_k_hits(rank, top_k):
    """rank [B] i32 of ``stages.classification_scores`` -> int64 [len(top_k)] on its device: the rows with 0 <= rank < k,
    per k.  The k are kernel arguments: nothing is copied from the host."""
    valid = rank >= 0
    return torch.stack([(valid & (rank < int(k))).sum(dtype=torch.int64) for k in top_k])


def classification_accuracy(logits, targets, top_k=None):
    """metrics.py:66-99 for device tensors: one float32 per entry of ``top_k`` (default [1]), in the order given.  The
    reference takes ``logits.topk(max(top_k))`` and compares; here a row is top-k correct iff its target's rank
    (``stages.classification_scores``) is below k.  One synchronisation.

    The RESULT is the reference's, as written there: ``correct[:k].view(-1).float().mean()`` averages over the k x B
    comparison matrix, of which at most one entry per row is true, so the value is hits / (k * B) -- the top-k accuracy
    divided by k (equal to it for k = 1).  ``TopKAccuracy.compute()["accuracy"]`` is hits / B.  Where a row's values tie at
    the target, torch.topk's order is unspecified and this library puts the lower class index first."""
    import numpy as np
    ks = _top_k_list([1] if top_k is None else top_k)
    rank = stages.classification_scores(logits, targets, want_loss=False)["rank"]
    n = int(rank.shape[0])
    # float32 division of two integers below 2^24, as torch's mean of a float32 tensor of zeros and ones
    return [np.float32(c) / np.float32(k * n) for c, k in zip(top_k_hits(rank, ks).cpu().tolist(), ks)]


class TopKAccuracy:
    """Running top-k accuracy and evaluation loss over batches of logits: process_classification_evaluation_batch / _epoch
    (helpers.py:215-288) without their per-batch host round trips.  ``update`` enqueues and never synchronises; ``compute``
    is the one sync.  The loss is kept as the reference keeps it -- one float32 batch mean per ``update``, and ``eval_loss``
    the mean of those batch means (EvalLoss), not the mean over the samples."""

    def __init__(self, top_k=(1,)):
        self.top_k = sorted(set(_top_k_list(top_k)))
        self._acc = None          # int64 [len(top_k) + 2]: correct rows per k, rows, rows whose target was out of range
        self._loss = None         # float32 [2]: the sum of the batch means, the number of batches

    def update(self, logits, targets):
        """logits [B,C] / targets [B] on the device; enqueued on the current stream."""
        out = stages.classification_scores(logits, targets)
        self.add_scores(out["rank"], out["loss"])

    def add_scores(self, rank, loss):
        """One batch as ``stages.classification_scores`` scored it -- rank [B] i32, loss [B] f32 -- for callers that made
        that launch themselves (``QuartzNetClassifier.evaluate_manifest`` takes its top-1 from the same one).  No host
        round trip."""
        n = torch.full((1,), rank.shape[0], dtype=torch.int64, device=rank.device)
        row = torch.cat([top_k_hits(rank, self.top_k), n, (rank < 0).sum(dtype=torch.int64).reshape(1)])
        pair = torch.stack([loss.mean(dtype=torch.float32), torch.ones((), dtype=torch.float32, device=loss.device)])
        self._acc = row if self._acc is None else self._acc + row
        self._loss = pair if self._loss is None else self._loss + pair

    def reset(self):
        self._acc = self._loss = None

    def compute(self, reduce=False, group=None):
        """-> {"accuracy": {k: correct / samples}, "correct": {k: int}, "samples": int, "eval_loss": float}.  reduce=True sums
        the integers (``dist.all_reduce_counts``) and the (sum of batch means, batches) pair (one float all-reduce) over the
        process group first.  The division of the loss pair is done here, in float64 on the host.  No sample gives NaN.
        Raises VasrError when a target was outside [0, num_classes)."""
        nk = len(self.top_k)
        acc = self._acc if self._acc is not None else torch.zeros(nk + 2, dtype=torch.int64)
        pair = self._loss if self._loss is not None else torch.zeros(2, dtype=torch.float32)
        if reduce:
            acc, pair = dist.all_reduce_counts(acc, group), dist.all_reduce_counts(pair, group)
        host, (loss_sum, batches) = acc.cpu().tolist(), pair.cpu().tolist()
        samples, bad = host[nk], host[nk + 1]
        if bad:
            raise _lib.VasrError(f"{bad} scored rows carried a target outside [0, num_classes): no accuracy or loss is "
                                 "returned for them")
        nan = float("nan")
        return dict(accuracy={k: host[i] / samples if samples else nan for i, k in enumerate(self.top_k)},
                    correct={k: host[i] for i, k in enumerate(self.top_k)}, samples=samples,
                    eval_loss=float(loss_sum) / float(batches) if batches else nan)

    def logs(self, tag=None, reduce=False, group=None):
        """process_classification_evaluation_epoch's dict (helpers.py:256-288): ``Evaluation_Loss {tag}`` and
        ``Evaluation_Accuracy_Top@{k} {tag}``, in percent.  The reference's figure, as its batch function accumulates it:
        CorrectCount@k holds ``classification_accuracy`` x batch size = hits / k, so the logged value is 100 x hits /
        (k x samples) -- the accuracy of ``compute`` divided by k (see ``classification_accuracy``)."""
        r = self.compute(reduce, group)
        tag = "" if tag is None else tag
        out = {f"Evaluation_Loss {tag}": r["eval_loss"]}
        for k in self.top_k:
            out[f"Evaluation_Accuracy_Top@{k} {tag}"] = r["accuracy"][k] / k * 100.0
        return out


class CTCEvalLoss:
    """Running CTC evaluation loss over batches of log-probs: ``Evaluation_Loss`` of process_evaluation_batch / _epoch
    (helpers.py:146-204) with ``CTCLossNM`` (losses.py) without their per-batch host round trips.  ``update`` enqueues and
    never synchronises; ``compute`` is the one sync.  The loss is kept as the reference keeps it -- one float32 batch mean
    per ``update`` (``torch.mean`` of the per-row losses, not divided by the target lengths), and ``eval_loss`` the mean of
    those batch means, which depends on how the utterances were cut into batches; ``loss_sum`` / ``scored`` does not."""

    def __init__(self, num_classes):
        self.blank = int(num_classes)         # CTCLossNM: the blank follows the labels
        self._acc = None          # int64 [3]: finite rows, +inf rows (no path), NaN rows (a length or an id the kernel refused)
        self._loss = None         # float32 [2]: the sum of the batch means, the number of batches
        self._sums = []           # float32 [] per batch: the sum of its finite per-row losses (added up in float64 on the host)

    def update(self, log_probs, input_length, targets, target_length):
        """log_probs [B,T',C] / input_length [B] / targets [B,W] / target_length [B] on the device (``stages.ctc_loss``);
        enqueued on the current stream."""
        self.add_losses(stages.ctc_loss(log_probs, input_length, targets, target_length, self.blank))

    def add_losses(self, loss):
        """One batch as ``stages.ctc_loss`` scored it -- loss [B] f32 -- for callers that made that launch themselves.  No
        host round trip."""
        finite = torch.isfinite(loss)
        row = torch.stack([finite.sum(dtype=torch.int64), torch.isinf(loss).sum(dtype=torch.int64),
                           torch.isnan(loss).sum(dtype=torch.int64)])
        pair = torch.stack([loss.mean(dtype=torch.float32), torch.ones((), dtype=torch.float32, device=loss.device)])
        self._sums.append(torch.where(finite, loss, torch.zeros_like(loss)).sum(dtype=torch.float32))
        self._acc = row if self._acc is None else self._acc + row
        self._loss = pair if self._loss is None else self._loss + pair

    def reset(self):
        self._acc, self._loss, self._sums = None, None, []

    def compute(self, reduce=False, group=None):
        """-> {"eval_loss": the mean of the float32 batch means (inf once a batch held a row without a path, as the
        reference's), "loss_sum": the sum of the finite per-row losses, "scored": the rows counted in it, "infeasible":
        the rows that came back +inf}.  reduce=True sums the accumulators over the process group first
        (``dist.all_reduce_counts``).  No batch gives eval_loss NaN.  Raises VasrError when a row came back NaN (a negative
        length, or a target id inside its length that is out of range or the blank)."""
        acc = self._acc if self._acc is not None else torch.zeros(3, dtype=torch.int64)
        pair = self._loss if self._loss is not None else torch.zeros(2, dtype=torch.float32)
        total = torch.stack(self._sums).cpu().to(torch.float64).sum().reshape(1) if self._sums else torch.zeros(1, dtype=torch.float64)
        if reduce:
            acc, pair = dist.all_reduce_counts(acc, group), dist.all_reduce_counts(pair, group)
            total = dist.all_reduce_counts(total, group)
        (scored, infeasible, bad), (mean_sum, batches) = acc.cpu().tolist(), pair.cpu().tolist()
        if bad:
            raise _lib.VasrError(f"{bad} scored rows came back NaN (a negative length, or a target id inside the row's length "
                                 "that is out of range or the blank): no loss is returned for them")
        return dict(eval_loss=float(mean_sum) / float(batches) if batches else float("nan"), loss_sum=float(total.cpu()[0]),
                    scored=int(scored), infeasible=int(infeasible))
