"""CPU checks of the device WER / CER scoring: the NumPy restatement (tests/wer_reference.py) against the fixture the
reference's own metrics module wrote (tests/golden/wer_cases.npz, make_golden_wer.py) -- integer for integer, the two rates
bit for bit --, the exported symbol / signature / header declaration with the ABI still 8, every refusal of
vasr_error_counts_i32 before a device is touched, ErrorRate's constructor and the host arithmetic of ``compute`` (fed CPU
counts through ``_add``), and all_reduce_counts over a gloo world of 2."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import wer_reference as WR
from conftest import GOLDEN_DIR, ROOT

INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "wer_cases.npz"), allow_pickle=False)


def test_restatement_equals_the_reference_metric(golden):
    g = golden
    labels = str(g["labels"])
    assert g["space_ids"].tolist() == [i for i, c in enumerate(labels) if c.isspace()] and len(g["space_ids"]) == 2
    assert len(g["hyp_len"]) <= 64 and int(max(g["hyp_len"].max(), g["ref_len"].max())) <= 300
    got = WR.batch_counts(g["hyp"], g["hyp_len"], g["ref"], g["ref_len"], g["space_ids"].tolist())
    assert got[:, 0].tolist() == g["word_edits"].tolist()
    assert got[:, 1].tolist() == g["ref_words"].tolist()
    assert got[:, 2].tolist() == g["char_edits"].tolist()
    assert got[:, 3].tolist() == g["ref_len"].tolist()
    wer, cer = WR.rates(got.astype(np.int64).sum(axis=0))
    assert wer == float(g["wer"]) and cer == float(g["cer"])          # bit for bit: the same two integers divided
    # the host scorer of the parent commit, on the same pairs as strings
    from viet_asr_amd.data_layer import word_error_rate
    text = lambda rows, lens: ["".join(labels[c] for c in r[:n]) for r, n in zip(rows, lens)]  # noqa: E731
    hyps, refs = text(g["hyp"], g["hyp_len"]), text(g["ref"], g["ref_len"])
    assert word_error_rate(hyps, refs) == wer and word_error_rate(hyps, refs, use_cer=True) == cer


def test_restatement_split_semantics_and_a_wide_pair():
    sp = [0, 5]
    assert WR.split_ids([0, 0, 1, 2, 5, 0, 3, 0], sp) == [(1, 2), (3,)]
    assert WR.split_ids([0, 5, 0], sp) == [] and WR.split_ids([], sp) == [] and WR.split_ids([0, 1], []) == [(0, 1)]
    assert WR.counts([1, 2, 0, 3], [1, 2, 0, 4, 0, 0], sp) == [1, 2, 3, 6]
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 3, 4096), rng.integers(0, 3, 4096)
    d = WR.levenshtein(a, b)
    assert 0 < d <= 4096 and WR.levenshtein(a, a) == 0 and WR.levenshtein(a, b[:1]) in (4095, 4096)
    # against the plain cell-by-cell recurrence on a small pair
    x, y = rng.integers(0, 3, 37).tolist(), rng.integers(0, 3, 23).tolist()
    prev = list(range(len(y) + 1))
    for i, u in enumerate(x, 1):
        cur = [i]
        for j, v in enumerate(y, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (u != v)))
        prev = cur
    assert WR.levenshtein(x, y) == prev[-1]


def test_new_symbol_is_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    n = "vasr_error_counts_i32"
    assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f = L.vasr_error_counts_i32
    p = 4096                                   # a non-NULL, 16-byte aligned "device pointer"
    sp = (C.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 7)
    ok = dict(hyp=p, hw=16, hl=p, ref=p, rw=16, rl=p, batch=2, sp=sp, ns=1, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["hyp"], a["hw"], a["hl"], a["ref"], a["rw"], a["rl"], a["batch"], a["sp"], a["ns"], a["out"], None)

    for name in ("hyp", "hl", "ref", "rl", "out"):
        assert call(**{name: None}) == INVALID, name
    assert call(batch=0) == INVALID and call(batch=-3) == INVALID
    assert call(hw=-1) == INVALID and call(rw=-1) == INVALID
    assert call(ns=-1) == INVALID and call(ns=9) == INVALID and call(sp=None, ns=1) == INVALID
    assert call(out=p + 4) == INVALID          # the counts are stored as one 16-byte vector per row
    assert call(hw=4097) == UNSUPPORTED and call(rw=4097) == UNSUPPORTED and call(hw=1 << 40) == UNSUPPORTED
    assert b"4096" in L.vasr_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(rw=5000), L)
    with pytest.raises(ValueError):
        _lib.check(call(batch=0), L)


def test_error_rate_refuses_multi_character_labels():
    from viet_asr_amd.metrics import ErrorRate, space_ids
    with pytest.raises(NotImplementedError):
        ErrorRate([" ", "a", "ch", "b"])
    with pytest.raises(NotImplementedError):
        ErrorRate([" ", "a", ""])
    assert ErrorRate(list(" ab\tc")).space_ids == [0, 3] and space_ids("abc") == []
    with pytest.raises(NotImplementedError):
        space_ids(" \t\n\r\x0b\x0c\x1c\x1d\x1ea")          # nine whitespace labels: the entry point takes eight


def test_compute_host_arithmetic():
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import ErrorRate
    m = ErrorRate(list(" abc"))
    assert m.compute() == dict(wer=float("inf"), cer=float("inf"), word_edits=0, ref_words=0, char_edits=0, ref_chars=0)
    m._add(torch.tensor([[1, 0, 3, 0], [2, 0, 1, 0]], dtype=torch.int32))      # hypotheses against empty references
    r = m.compute()
    assert r["wer"] == float("inf") and r["cer"] == float("inf") and r["word_edits"] == 3 and r["char_edits"] == 4
    m._add(torch.tensor([[1, 3, 2, 7]], dtype=torch.int32))
    m._add(torch.tensor([[0, 4, 1, 9], [2, 0, 5, 5]], dtype=torch.int32))
    r = m.compute()
    assert r == dict(wer=6 / 7, cer=12 / 21, word_edits=6, ref_words=7, char_edits=12, ref_chars=21)
    assert m.compute(reduce=True) == r                                          # no process group: the identity
    m._add(torch.tensor([[5, 5, 5, 5], [-1, -1, -1, -1]], dtype=torch.int32))
    with pytest.raises(VasrError):
        m.compute()
    m.reset()
    m._add(torch.tensor([[0, 2, 0, 5]], dtype=torch.int32))
    assert m.compute() == dict(wer=0.0, cer=0.0, word_edits=0, ref_words=2, char_edits=0, ref_chars=5)
    big = torch.full((3, 4), 2 ** 30, dtype=torch.int32)                        # the sums are 64-bit
    m.reset(); m._add(big)
    assert m.compute()["ref_chars"] == 3 * 2 ** 30


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reduce_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import viet_asr_amd  # noqa: F401
    from viet_asr_amd import dist as vdist
    from viet_asr_amd.metrics import ErrorRate
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mine = torch.tensor([1 + rank, 10 + rank, 100 + rank, 1000 + rank, 0], dtype=torch.int64)
        total = vdist.all_reduce_counts(mine)
        assert total.tolist() == [3, 21, 201, 2001, 0] and mine.tolist()[0] == 1 + rank     # the input is left alone
        m = ErrorRate(list(" ab"))
        m._add(torch.tensor([[1 + rank, 4, 2, 8 + rank]], dtype=torch.int32))
        assert m.compute()["ref_chars"] == 8 + rank
        r = m.compute(reduce=True)
        assert r == dict(wer=3 / 8, cer=4 / 17, word_edits=3, ref_words=8, char_edits=4, ref_chars=17), r
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_all_reduce_counts_gloo():
    from viet_asr_amd import dist as vdist
    x = torch.tensor([1, 2, 3, 4, 0])
    assert vdist.all_reduce_counts(x) is x                  # no process group: the identity
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=100) for _ in procs)
    for p in procs:
        p.join(30)
    assert res == {r: "ok" for r in range(world)}, res
