"""Batched manifest-driven data layers: counterparts of ``AudioToTextDataLayer`` and ``AudioToSpeechLabelDataLayer`` for
inference / evaluation.

Reference: nemo/collections/asr/data_layer.py:42-190 (ports, manifest arguments),
parts/manifest.py:21-94 (JSON-lines entries with ``audio_filepath``, ``duration``, ``text``),
parts/dataset.py:14-53 (``seq_collate_fn``: zero-pad signals and tokens to the batch maximum),
parts/parsers.py (character parser: unknown characters dropped).  Decoding is PCM-WAV only (audio.py); files at
another rate are resampled on the device by the caller (``VietASR`` / ``audio.resample``), so this layer tags
every batch with its source rate.  With ``AllGpu`` placement the utterance list is sharded by rank: by default in
duration-balanced length buckets (``dist.balanced_shards``; ``shard_by="count"`` keeps contiguous equal-count shards
in manifest order -- the reference shards with a DistributedSampler, data_layer.py:161-165, equal counts too).
"""
import json
import os

import numpy as np
import torch

from .audio import read_wav
from .core import AudioSignal, DataLayerNM, DeviceType, LengthsType, NeuralType
from .dist import balanced_shards, shard_range


class ChannelIndexType(LengthsType):
    pass


class _ManifestBatches:
    """What the manifest-driven layers share: the cut of the kept items (path, duration, target) into this rank's batches
    -- sharding, length buckets, ``drop_last`` -- and the iteration protocol over them (``_BatchIter``)."""

    def _plan(self, items, batch_size, bucket_by_length, drop_last, shard_by):
        if shard_by not in ("duration", "count"):
            raise ValueError(f"shard_by must be 'duration' or 'count', got {shard_by!r}")
        self.manifest_index = list(range(len(items)))        # position of every kept item in the (filtered) manifest
        batches = None
        if self.placement == DeviceType.AllGpu and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
            # duration-balanced dealing fixes the batch composition (length buckets), so it is only taken when the caller did
            # not ask for something it cannot honour: shuffle=True (the reference's DistributedSampler shuffles
            # utterances, actions.py:669-693) and bucket_by_length=False fall back to equal-count contiguous shards
            if shard_by == "duration" and all(it[1] > 0 for it in items) and bucket_by_length and not self._shuffle:
                # length buckets of batch_size utterances dealt heaviest-first to the least loaded rank: the ranks'
                # padded work (rows x longest row, summed over batches) ends up within a few percent of each other
                batches = [sorted(b, key=lambda i: (items[i][1], i)) for b in balanced_shards([it[1] for it in items], world, batch_size)[rank]]
                batches.sort(key=lambda b: items[b[0]][1])
            else:
                lo, hi = shard_range(len(items), rank, world)
                self.manifest_index = self.manifest_index[lo:hi]
                items = items[lo:hi]
        order = list(range(len(items)))
        if bucket_by_length and not self._shuffle:
            order.sort(key=lambda i: items[i][1])    # similar lengths share a batch: less padding work
        self._items, self._order = items, order
        self._batches = batches if batches is not None else [order[i:i + batch_size] for i in range(0, len(order), batch_size)]
        if drop_last:     # (the duration-balanced path sorts its batches by length: the short one is not the last)
            self._batches = [b for b in self._batches if len(b) == batch_size]

    def __len__(self):
        return len(self._batches)

    @property
    def dataset(self):
        return None

    @property
    def data_iterator(self):
        return _BatchIter(self)

    def utterance_order(self):
        """Indices into the (duration-filtered) manifest, in the order the batches deliver them."""
        return [self.manifest_index[i] for b in self._batches for i in b]


class AudioToTextDataLayer(_ManifestBatches, DataLayerNM):
    @property
    def output_ports(self):
        return {"audio_signal": NeuralType(("B", "T"), AudioSignal(freq=self._sample_rate)),
                "a_sig_length": NeuralType(tuple("B"), LengthsType()),
                "transcripts": NeuralType(("B", "T"), ChannelIndexType()),
                "transcript_length": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, manifest_filepath, labels, batch_size, sample_rate=16000, min_duration=0.1, max_duration=None,
                 shuffle=False, bucket_by_length=True, drop_last=False, pad_id=None, shard_by="duration", **_unused):
        """``trim_silence`` (among the reference's options taken and not used here) does not act in this layer: it hands out
        host tensors, and the trim (librosa.effects.trim) runs on the device in the engine call that consumes them --
        ``VietASR.evaluate_manifest(..., trim_silence="config")`` follows the YAML's value, ``audio.trim_silence`` is the call."""
        super().__init__()
        self._sample_rate, self._batch_size, self._shuffle = sample_rate, batch_size, shuffle
        self.labels = list(labels)
        self._lab = {c: i for i, c in enumerate(self.labels)}
        self.pad_id = len(self.labels) if pad_id is None else pad_id
        items = []
        for path in str(manifest_filepath).split(","):
            with open(path, encoding="utf-8") as f:
                for line in f:
                    if not line.strip():
                        continue
                    e = json.loads(line)
                    d = float(e.get("duration", 0.0))
                    if (min_duration and d and d < min_duration) or (max_duration and d > max_duration):
                        continue                       # manifest.py filters by duration the same way
                    items.append((e["audio_filepath"], d, e.get("text", "")))
        self._plan(items, batch_size, bucket_by_length, drop_last, shard_by)

    def tokens(self, text):
        return [self._lab[c] for c in text if c in self._lab]

    def _targets(self, texts):
        """seq_collate_fn's token half: pad_id-padded token rows and their lengths."""
        toks = [self.tokens(t) for t in texts]
        t_len = torch.tensor([len(t) for t in toks], dtype=torch.int64)
        tokens = torch.full((len(toks), max(int(t_len.max()), 1)), self.pad_id, dtype=torch.int64)
        for k, t in enumerate(toks):
            tokens[k, : len(t)] = torch.tensor(t, dtype=torch.int64)
        return tokens, t_len


class SpeechLabelsType(ChannelIndexType):
    pass


class AudioToSpeechLabelDataLayer(_ManifestBatches, DataLayerNM):
    """Counterpart of ``AudioToSpeechLabelDataLayer`` (data_layer.py:449-620) for evaluation: clips with one target class
    each.  Manifest lines as ``ASRSpeechLabel.__parse_item`` reads them (parts/collections.py:242-277): the audio under
    ``audio_filename`` or ``audio_filepath`` (through ``expanduser``), a required ``duration``, the label under ``command``,
    ``target`` or ``label`` in that precedence; ``offset`` is ignored, as ``AudioLabelDataset.__getitem__`` ignores it
    (parts/dataset.py:380-391).  Duration filtering as ``SpeechLabel`` (collections.py:195-203).  Labels are mapped by
    ``label2id``; an unknown one raises KeyError (here when the manifest is read, in the reference when the item is).
    Batches: signals zero padded to the batch maximum (seq_collate_fn), ``label`` [B] int64, ``label_length`` [B] int64, all
    ones.  PCM WAV only; ``trim_silence`` and ``augmentor`` are not implemented HERE: the layer hands out host tensors, and the
    trim (librosa.effects.trim) runs on the device, in the engine call that consumes them
    (``engine.QuartzNetClassifier.evaluate_manifest(..., trim_silence=True)``, ``audio.trim_silence``), as the perturbations do
    (``perturb.AudioAugmentor``, the ``augmentor`` argument of ``engine.QuartzNetCTC`` and ``VietASR``'s batch calls).  Sharding, length buckets and
    ``utterance_order`` as in ``AudioToTextDataLayer``, whose defaults (no shuffle) it shares."""

    @property
    def output_ports(self):
        return {"audio_signal": NeuralType(("B", "T"), AudioSignal(freq=self._sample_rate)),
                "a_sig_length": NeuralType(tuple("B"), LengthsType()),
                "label": NeuralType(tuple("B"), SpeechLabelsType()),
                "label_length": NeuralType(tuple("B"), LengthsType())}

    def __init__(self, manifest_filepath, labels, batch_size, sample_rate=16000, int_values=False, num_workers=0,
                 shuffle=False, min_duration=0.1, max_duration=None, trim_silence=False, drop_last=False, load_audio=True,
                 augmentor=None, bucket_by_length=True, shard_by="duration"):
        super().__init__()
        if trim_silence:
            raise NotImplementedError("trim_silence=True (librosa.effects.trim) is not implemented")
        if augmentor is not None:
            raise NotImplementedError("audio augmentors are not applied in the data layer: pass the perturb.AudioAugmentor to the "
                                      "engine call that consumes the batches (augmentor=...)")
        if not load_audio:
            raise NotImplementedError("load_audio=False is not implemented")
        self._sample_rate, self._batch_size, self._shuffle = sample_rate, batch_size, shuffle
        self.labels = list(labels)
        self.label2id = {label: i for i, label in enumerate(self.labels)}
        self.id2label = dict(enumerate(self.labels))
        items = []
        for path in str(manifest_filepath).split(","):
            with open(path, encoding="utf-8") as f:
                for line in f:
                    if not line.strip():
                        continue
                    audio_file, duration, label = self._parse_item(line)
                    if (min_duration is not None and duration < min_duration) or \
                            (max_duration is not None and duration > max_duration):
                        continue
                    items.append((audio_file, duration, self.label2id[label]))
        self._plan(items, batch_size, bucket_by_length, drop_last, shard_by)

    _AUDIO_KEYS, _LABEL_KEYS = ("audio_filename", "audio_filepath"), ("command", "target", "label")

    @classmethod
    def _parse_item(cls, line):
        """One manifest line -> (path, duration, label); the first key present wins, in the reference's precedence."""
        entry = json.loads(line)
        first = lambda keys: next((entry[k] for k in keys if k in entry), None)  # noqa: E731
        found = (("audio file", first(cls._AUDIO_KEYS)), ("duration", entry.get("duration")), ("label", first(cls._LABEL_KEYS)))
        for what, value in found:
            if value is None:
                raise ValueError(f"Manifest file has invalid json line structure: {line} without proper {what} key.")
        return os.path.expanduser(found[0][1]), found[1][1], found[2][1]

    def _targets(self, labels):
        return torch.tensor(labels, dtype=torch.int64), torch.ones(len(labels), dtype=torch.int64)


class _BatchIter:
    def __init__(self, layer):
        self.layer, self.i = layer, 0
        if layer._shuffle:
            np.random.shuffle(layer._batches)

    def __len__(self):
        return len(self.layer._batches)

    def __iter__(self):
        return self

    def __next__(self):
        L = self.layer
        if self.i >= len(L._batches):
            raise StopIteration
        idx = L._batches[self.i]
        self.i += 1
        sigs, targets = [], []
        for j in idx:
            path, _, target = L._items[j]
            x, sr = read_wav(path)
            if sr != L._sample_rate:
                raise ValueError(f"{path}: sample rate {sr} != {L._sample_rate}; resample first (audio.resample)")
            sigs.append(x)
            targets.append(target)
        a_len = torch.tensor([len(s) for s in sigs], dtype=torch.int64)
        audio = torch.zeros((len(sigs), int(a_len.max())), dtype=torch.float32)
        for k, s in enumerate(sigs):
            audio[k, : len(s)] = torch.from_numpy(s)
        return (audio, a_len) + tuple(L._targets(targets))


def word_error_rate(hypotheses, references, use_cer=False):
    """nemo/collections/asr/metrics.py:30-63: summed Levenshtein distance / summed reference length, on host strings.
    ``metrics.ErrorRate`` (``VietASR.evaluate_manifest``) computes the same two rates on the device from the parsed token
    ids; on raw manifest text this one differs from it only where a reference contains characters outside the labels."""
    def lev(a, b):
        prev = list(range(len(b) + 1))
        for i, x in enumerate(a, 1):
            cur = [i]
            for j, y in enumerate(b, 1):
                cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
            prev = cur
        return prev[-1]
    if len(hypotheses) != len(references):
        raise ValueError("In word error rate calculation, hypotheses and reference lists must have the same number of "
                         f"elements. But I got: {len(hypotheses)} and {len(references)} correspondingly")
    scores = words = 0
    for h, r in zip(hypotheses, references):
        h_list, r_list = (list(h), list(r)) if use_cer else (h.split(), r.split())
        words += len(r_list)
        scores += lev(h_list, r_list)
    return 1.0 * scores / words if words else float("inf")
