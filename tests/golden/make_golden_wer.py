#!/usr/bin/env python3
"""Generate tests/golden/wer_cases.npz by running the REAL reference metric (nemo/collections/asr/metrics.py) on the CPU --
dev container only.

    python tests/golden/make_golden_wer.py     # needs the reference checkout

Stored: the labels (one string; two of them are whitespace), their whitespace ids, up to 64 (hypothesis, reference) pairs
of at most 300 label ids as padded int32 batches with lengths, and for every pair the reference's ``__levenshtein`` on
``list(s)`` and on ``s.split()``, ``len(r.split())``; and ``word_error_rate`` over the whole list with use_cer False and True.
The pairs: seeded random text with about 10 % substitutions, insertions and deletions, plus the edges of ``str.split()``
(empty strings, whitespace only, leading / trailing / doubled / mixed whitespace, one-character words, one long word, words
that differ in their last character or are prefixes of each other)."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
LABELS = " abcdefghijklm\tnopq'"
MAX_IDS = 300


def reference_metrics():
    spec = importlib.util.spec_from_file_location("ref_asr_metrics", os.path.join(REF, "nemo", "collections", "asr", "metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_pairs(rng, count):
    letters = [c for c in LABELS if not c.isspace()]
    pairs = []
    for k in range(count):
        n = int(rng.integers(1, MAX_IDS - 40))
        space_p = (0.0, 0.1, 0.17, 0.4)[k % 4]
        ref = "".join(" " if rng.random() < space_p else ("\t" if rng.random() < 0.02 else letters[int(rng.integers(len(letters)))])
                      for _ in range(n))
        hyp = []
        for c in ref:
            u = rng.random()
            if u < 0.035:
                continue                                                    # deletion
            hyp.append(LABELS[int(rng.integers(len(LABELS)))] if u < 0.07 else c)  # substitution
            if u > 0.965:
                hyp.append(LABELS[int(rng.integers(len(LABELS)))])          # insertion
        pairs.append(("".join(hyp)[:MAX_IDS], ref))
    return pairs


EDGES = [
    ("", ""), ("", "abc de"), ("abc de", ""), ("   ", "abc"), ("abc", " \t "), (" \t ", "\t  "),
    ("a", "a"), ("a", "b"), ("a", " "), ("  abc  de ", "abc de"), ("abc\tde", "abc de"), ("abc \t de", "abcde"),
    ("a b c d e f g", "a b d d e g"), ("abcdefghijklmnopq" * 17, "abcdefghijklmnopq" * 16 + "abcdefghijklmnopa"),
    ("abcd abce abc", "abce abcd abcd"), ("abc abcd ab", "abcd abc abc"), ("ab ab ab ab", "ab ab ab"),
    ("no ho 'a", "no  ho 'a "), ("abcabcabc", "cbacbacba"), ("aaaa aaaa", "aaaa aaab"),
]


def main():
    M = reference_metrics()
    lev = getattr(M, "__levenshtein")
    rng = np.random.default_rng(20261018)
    pairs = EDGES + random_pairs(rng, 64 - len(EDGES))
    assert len(pairs) <= 64 and all(len(h) <= MAX_IDS and len(r) <= MAX_IDS for h, r in pairs)
    lab = {c: i for i, c in enumerate(LABELS)}
    width = max(1, max(max(len(h), len(r)) for h, r in pairs))
    hyp = np.zeros((len(pairs), width), dtype=np.int32)
    ref = np.zeros((len(pairs), width), dtype=np.int32)
    for k, (h, r) in enumerate(pairs):
        hyp[k, : len(h)] = [lab[c] for c in h]
        ref[k, : len(r)] = [lab[c] for c in r]
    hyps, refs = [h for h, _ in pairs], [r for _, r in pairs]
    fixture = dict(
        labels=LABELS, space_ids=np.array([i for i, c in enumerate(LABELS) if c.isspace()], dtype=np.int32),
        hyp=hyp, hyp_len=np.array([len(h) for h in hyps], dtype=np.int32),
        ref=ref, ref_len=np.array([len(r) for r in refs], dtype=np.int32),
        char_edits=np.array([lev(list(h), list(r)) for h, r in pairs], dtype=np.int64),
        word_edits=np.array([lev(h.split(), r.split()) for h, r in pairs], dtype=np.int64),
        ref_words=np.array([len(r.split()) for r in refs], dtype=np.int64),
        wer=np.float64(M.word_error_rate(hyps, refs, use_cer=False)),
        cer=np.float64(M.word_error_rate(hyps, refs, use_cer=True)))
    path = os.path.join(HERE, "wer_cases.npz")
    np.savez_compressed(path, **fixture)
    print(f"wer_cases: {len(pairs)} pairs, width {width}, wer {float(fixture['wer']):.6f} cer {float(fixture['cer']):.6f}, "
          f"bytes={os.path.getsize(path)}")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
