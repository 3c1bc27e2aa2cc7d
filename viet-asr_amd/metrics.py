"""Word and character error rate on device id sequences.

Reference: nemo/collections/asr/metrics.py:30-63 (``word_error_rate``, both ``use_cer`` settings) as
``process_evaluation_epoch`` reports them (helpers.py:188-189), scored on the parsed token tensors the data layer delivers
(``__gather_transcripts``, helpers.py:128-143) -- not on raw manifest text.  The edit distances are computed per row by
``stages.error_counts`` (vasr_error_counts_i32, csrc/metrics.hip); this module only sums four integers on the device and
divides them once on the host.  ``data_layer.word_error_rate`` is the same metric on host strings; the two differ only
where a reference holds characters outside the labels, which the character parser drops before the tokens are made.
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


def word_error_rate_ids(ids, id_len, transcripts, transcript_length, labels, use_cer=False):
    """One-shot functional form: ``word_error_rate`` of one batch of device id rows (metrics.py:30-63)."""
    m = ErrorRate(labels)
    m.update(ids, id_len, transcripts, transcript_length)
    return m.compute()["cer" if use_cer else "wer"]
