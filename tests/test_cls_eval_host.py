"""CPU checks of the classification scoring: the float64 / integer restatement (tests/cls_eval_reference.py) against the
fixture the reference's own functions wrote (tests/golden/cls_eval_cases.npz, make_golden_cls_eval.py) -- every integer
exactly, every loss inside the bound, the reference's float32 losses inside it too --, the exported symbol / signature /
header declaration with the ABI still 8, every refusal of vasr_class_scores_f32 before a device is touched, the host
arithmetic of ``TopKAccuracy.compute`` / ``logs`` (fed CPU ranks and losses through ``add_scores``), its reduction over a
gloo world of 2, and ``AudioToSpeechLabelDataLayer`` on temporary WAV files."""
import ctypes as C
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import cls_eval_reference as ER
from conftest import GOLDEN_DIR, ROOT

INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN_DIR, "cls_eval_cases.npz"), allow_pickle=False)


def cases(g):
    for i in range(int(g["cases"])):
        yield i, g[f"c{i}_logits"], g[f"c{i}_targets"]


def test_fixture_covers_the_shapes_and_holds_no_tie(golden):
    g = golden
    shapes = {(x.shape[1], x.shape[0]) for _, x, _ in cases(g)}
    assert {c for c, _ in shapes} == {1, 2, 35, 64, 65, 257, 1000} and {b for _, b in shapes} == {1, 3, 4, 5, 67}
    assert {float(g[f"c{i}_scale"]) for i in range(int(g["cases"]))} == {0.01, 1.0, 100.0}
    for _, x, t in cases(g):
        assert x.dtype == np.float32 and t.dtype == np.int64 and np.isfinite(x).all()
        for row, tt in zip(x, t):
            top = np.sort(row)[::-1][: min(6, row.size)]
            assert len(set(top.tolist())) == top.size and int((row == row[tt]).sum()) == 1     # no row is excused


def test_restatement_reproduces_every_fixture_integer_and_loss(golden):
    g = golden
    for i, x, t in cases(g):
        k = min(5, x.shape[1])
        rank, top, loss = ER.batch(x, t, k)
        assert (top == g[f"c{i}_top5"]).all(), i
        # the rank against the reference's own top-5: inside it at the same position, outside it >= 5
        for b in range(len(t)):
            where = np.nonzero(g[f"c{i}_top5"][b] == t[b])[0]
            assert (rank[b] == where[0]) if where.size else (rank[b] >= k), (i, b)
        for j in range(3):
            ks = g[f"c{i}_acc{j}_k"].tolist()
            assert [float(a) for a in ER.reference_accuracy(rank, ks)] == g[f"c{i}_acc{j}"].tolist(), (i, j)
        ref32 = g[f"c{i}_loss"]
        assert ref32.dtype == np.float32
        for b in range(len(t)):
            bound = ER.loss_bound(x[b], t[b])
            assert abs(float(ref32[b]) - loss[b]) <= bound, (i, b, float(ref32[b]), loss[b], bound)   # the reference, in float32


def test_restatement_epoch(golden):
    g = golden
    ks = g["epoch_top_k"].tolist()
    assert ks == [5, 1]
    sizes, means, hits = [], [], {k: 0 for k in ks}
    for j in range(3):
        x, t = g[f"epoch{j}_logits"], g[f"epoch{j}_targets"]
        rank, _, loss = ER.batch(x, t, 0)
        sizes.append(len(t))
        means.append(loss.mean())
        assert abs(means[-1] - g["epoch_batch_losses"][j]) <= np.mean([ER.loss_bound(r, tt) for r, tt in zip(x, t)]) + ER.EPS * (len(t) + 1) * means[-1]
        for k in ks:
            hits[k] += ER.hits(rank, k)
            # CorrectCount@k: accuracy x batch size = hits / k, through two float32 roundings
            assert abs(g[f"epoch_counts{k}"][j] - ER.hits(rank, k) / k) <= 4 * ER.EPS * len(t)
    assert sizes == [67, 5, 1]
    for k in ks:
        assert abs(float(g[f"epoch_acc{k}"]) - 100.0 * hits[k] / (k * 73)) <= 100.0 * 8 * ER.EPS
    assert abs(float(g["epoch_loss"]) - np.mean(means)) <= 1e-5


def test_restatement_order_ties_and_specials():
    nan, inf = float("nan"), float("inf")
    assert ER.order([1, 3, 3, 2, 3]).tolist() == [1, 2, 4, 3, 0]            # lower index first (torch.topk: 2, 4, 1)
    assert ER.order([0.0, -0.0, 0.0]).tolist() == [0, 1, 2]                  # -0 == +0
    assert ER.order([1.0, nan, inf, nan, -inf]).tolist() == [1, 3, 2, 0, 4]  # NaN above every number, NaNs by index
    assert ER.rank([5.0, 5.0, 5.0], 2) == 2 and ER.rank([5.0, 5.0, 5.0], 0) == 0
    assert ER.rank([1.0, 2.0], -1) == -1 and ER.rank([1.0, 2.0], 2) == -1 and ER.loss64([1.0, 2.0], 2) == 0.0
    assert abs(ER.loss64([0.0, 0.0], 1) - math.log(2)) < 1e-15 and ER.loss64([3.0], 0) == 0.0


def test_summation_depth_constant():
    """K(C) of the kernel's order never exceeds the issue's tree constant up to C = 1536, and the first sizes where it does."""
    for c in range(1, 1537):
        assert ER.kernel_roundings(c) <= ER.tree_roundings(c), c
        assert ER.sum_roundings(c) == ER.tree_roundings(c)
    assert [ER.kernel_roundings(c) for c in (1, 2, 3, 64, 65, 129, 257, 512, 513, 1000, 1536)] == [0, 1, 2, 6, 7, 8, 9, 9, 10, 10, 11]
    assert ER.kernel_roundings(1537) == 12 and ER.tree_roundings(1537) == 11 and ER.sum_roundings(65536) == 136


def test_new_symbol_is_exported_and_the_abi_is_still_8():
    from viet_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "vasr.h")).read()
    n = "vasr_class_scores_f32"
    assert n in _lib.SIGNATURES and hasattr(_lib.lib(), n) and hasattr(_lib.dev_lib(), n) and f" {n}(" in header
    assert _lib.lib().vasr_abi_version() == _lib.ABI_VERSION == 8 and "#define VASR_ABI_VERSION 8" in header
    assert "lower class index" in header.lower() or "LOWER class index" in header     # the tie rule is stated as the library's own


@pytest.mark.parametrize("which", ["lib", "dev_lib"])
def test_refusals_come_before_a_device_is_touched(which):
    """Pointers that are never dereferenced stand in for device memory: every call below has to return from its argument
    checks."""
    from viet_asr_amd import _lib
    L = getattr(_lib, which)()
    f = L.vasr_class_scores_f32
    p = 4096
    ok = dict(x=p, b=2, c=10, t=p, k=3, idx=p, val=p, prob=p, rank=p, loss=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["b"], a["c"], a["t"], a["k"], a["idx"], a["val"], a["prob"], a["rank"], a["loss"], None)

    assert call(x=None) == INVALID
    assert call(b=0) == INVALID and call(b=-2) == INVALID and call(c=0) == INVALID and call(c=-1) == INVALID
    assert call(k=-1) == INVALID and call(k=17, c=100) == INVALID and call(k=11) == INVALID and call(k=2, c=1) == INVALID
    assert call(t=None) == INVALID and call(t=None, loss=None) == INVALID and call(t=None, rank=None) == INVALID
    assert call(k=0, rank=None, loss=None) == INVALID and call(k=0, t=None, rank=None, loss=None) == INVALID
    assert call(idx=None, val=None, prob=None) == INVALID
    assert call(c=65537) == UNSUPPORTED and call(c=1 << 30, k=16) == UNSUPPORTED
    assert b"65536" in L.vasr_last_error()
    assert call(c=65537, k=17) == INVALID                       # an argument error wins over the size limit
    with pytest.raises(NotImplementedError):
        _lib.check(call(c=70000), L)
    with pytest.raises(ValueError):
        _lib.check(call(b=0), L)


def test_stage_refuses_host_tensors_and_bad_shapes():
    from viet_asr_amd import stages
    from viet_asr_amd._lib import VasrError
    with pytest.raises(VasrError):
        stages.classification_scores(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))


def test_compute_and_logs_host_arithmetic():
    from viet_asr_amd._lib import VasrError
    from viet_asr_amd.metrics import TopKAccuracy
    m = TopKAccuracy((5, 1, 5))
    assert m.top_k == [1, 5]
    r = m.compute()
    assert r["samples"] == 0 and r["correct"] == {1: 0, 5: 0} and math.isnan(r["eval_loss"]) and math.isnan(r["accuracy"][1])
    i32, f32 = torch.int32, torch.float32
    m.add_scores(torch.tensor([0, 4, 5, 2, 0, 9], dtype=i32), torch.tensor([1, 2, 3, 4, 5, 6], dtype=f32))     # mean 3.5
    m.add_scores(torch.tensor([1], dtype=i32), torch.tensor([0.5], dtype=f32))                                 # mean 0.5
    r = m.compute()
    assert r == dict(accuracy={1: 2 / 7, 5: 5 / 7}, correct={1: 2, 5: 5}, samples=7, eval_loss=2.0)      # NOT 22 / 7
    assert m.compute(reduce=True) == r                                                                   # no process group
    logs = m.logs("dev")
    assert sorted(logs) == ["Evaluation_Accuracy_Top@1 dev", "Evaluation_Accuracy_Top@5 dev", "Evaluation_Loss dev"]
    # the reference's figure: hits / (k x samples), in percent
    assert logs["Evaluation_Loss dev"] == 2.0 and logs["Evaluation_Accuracy_Top@1 dev"] == 2 / 7 * 100.0
    assert logs["Evaluation_Accuracy_Top@5 dev"] == 5 / 7 / 5 * 100.0
    assert sorted(m.logs()) == ["Evaluation_Accuracy_Top@1 ", "Evaluation_Accuracy_Top@5 ", "Evaluation_Loss "]
    m.add_scores(torch.tensor([0, -1], dtype=i32), torch.tensor([1.0, 0.0], dtype=f32))
    with pytest.raises(VasrError):
        m.compute()
    with pytest.raises(VasrError):
        m.logs()
    m.reset()
    m.add_scores(torch.tensor([3], dtype=i32), torch.tensor([7.0], dtype=f32))
    assert m.compute() == dict(accuracy={1: 0.0, 5: 1.0}, correct={1: 0, 5: 1}, samples=1, eval_loss=7.0)
    with pytest.raises(ValueError):
        TopKAccuracy((0,))
    with pytest.raises(ValueError):
        TopKAccuracy(())


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
    from viet_asr_amd.metrics import TopKAccuracy
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = TopKAccuracy((1, 3))
        # rank 0: two batches (means 2 and 4), rank 1: one batch (mean 0.25)
        if rank == 0:
            m.add_scores(torch.tensor([0, 2, 7], dtype=torch.int32), torch.tensor([1.0, 2.0, 3.0]))
            m.add_scores(torch.tensor([1], dtype=torch.int32), torch.tensor([4.0]))
        else:
            m.add_scores(torch.tensor([0, 0], dtype=torch.int32), torch.tensor([0.25, 0.25]))
        own = m.compute()
        assert own["samples"] == (4 if rank == 0 else 2) and own["eval_loss"] == (3.0 if rank == 0 else 0.25)
        r = m.compute(reduce=True)
        assert r == dict(accuracy={1: 3 / 6, 3: 5 / 6}, correct={1: 3, 3: 5}, samples=6, eval_loss=6.25 / 3), r
        assert m.compute() == own                                    # the accumulators are left alone
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_top_k_accuracy_reduces_over_gloo():
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


# ---- AudioToSpeechLabelDataLayer ----
LABELS = ["yes", "no", "up", "down"]


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """Five 16 kHz clips of different lengths -> (directory, [(path, samples)])."""
    from viet_asr_amd import audio
    d = tmp_path_factory.mktemp("cls_clips")
    rng = np.random.default_rng(5)
    out = []
    for i, n in enumerate([4000, 1600, 8000, 2400, 800]):
        x = (rng.standard_normal(n) * 0.1).astype(np.float32)
        path = str(d / f"clip{i}.wav")
        audio.write_wav(path, x, 16000)
        out.append((path, audio.read_wav(path)[0]))
    return d, out


def _manifest(d, name, lines):
    path = str(d / name)
    with open(path, "w", encoding="utf-8") as f:
        for e in lines:
            f.write(json.dumps(e) + "\n")
    return path


def test_data_layer_keys_precedence_ports_and_padding(clips):
    from viet_asr_amd.data_layer import AudioToSpeechLabelDataLayer
    d, c = clips
    man = _manifest(d, "keys.json", [
        {"audio_filepath": c[0][0], "duration": 0.25, "label": "yes"},
        {"audio_filename": c[1][0], "duration": 0.10, "target": "no", "label": "yes"},                  # target before label
        {"audio_filepath": c[2][0], "duration": 0.50, "command": "up", "target": "no", "label": "yes", "offset": 0.2},
        {"audio_filename": c[3][0], "audio_filepath": "/nowhere.wav", "duration": 0.15, "label": "down"},  # filename first
        {"audio_filepath": c[4][0], "duration": 0.05, "label": "yes"},                                   # below min_duration
    ])
    layer = AudioToSpeechLabelDataLayer(man, LABELS, batch_size=3)
    assert sorted(layer.output_ports) == ["a_sig_length", "audio_signal", "label", "label_length"]
    assert len(layer) == 2 and layer.label2id == {"yes": 0, "no": 1, "up": 2, "down": 3}
    order = layer.utterance_order()
    assert order == [1, 3, 0, 2]                                    # four kept entries, by duration
    got = list(layer.data_iterator)
    assert [b[0].shape[0] for b in got] == [3, 1]
    want_label = {0: 0, 1: 1, 2: 2, 3: 3}
    pos = 0
    for audio_t, a_len, label, label_len in got:
        B = audio_t.shape[0]
        assert audio_t.dtype == torch.float32 and a_len.dtype == label.dtype == label_len.dtype == torch.int64
        assert a_len.shape == label.shape == label_len.shape == (B,) and label_len.tolist() == [1] * B
        assert audio_t.shape[1] == int(a_len.max())
        for r in range(B):
            i = order[pos + r]
            x = c[i][1]
            assert int(a_len[r]) == len(x) and label[r].item() == want_label[i]
            assert np.array_equal(audio_t[r, : len(x)].numpy(), x) and not audio_t[r, len(x):].any()   # offset ignored, zero padded
        pos += B
    # no bucketing: manifest order; the filters of SpeechLabel
    flat = AudioToSpeechLabelDataLayer(man, LABELS, batch_size=2, bucket_by_length=False, min_duration=None)
    assert flat.utterance_order() == [0, 1, 2, 3, 4] and len(flat) == 3
    assert AudioToSpeechLabelDataLayer(man, LABELS, 2, min_duration=0.1, max_duration=0.25).utterance_order() == [1, 2, 0]
    assert AudioToSpeechLabelDataLayer(man, LABELS, 2, min_duration=0.10001).utterance_order() == [2, 0, 1]   # entry 1 dropped
    assert AudioToSpeechLabelDataLayer(man, LABELS, 2, drop_last=True, min_duration=None).utterance_order() == [4, 1, 3, 0]
    both = AudioToSpeechLabelDataLayer(man + "," + man, LABELS, batch_size=8)                                  # comma-separated
    assert len(both.utterance_order()) == 8


def test_data_layer_refusals(clips, monkeypatch):
    from viet_asr_amd.data_layer import AudioToSpeechLabelDataLayer
    d, c = clips
    ok = {"audio_filepath": c[0][0], "duration": 0.25, "label": "yes"}
    for drop, word in (("audio_filepath", "audio file key"), ("duration", "duration key"), ("label", "label key")):
        e = {k: v for k, v in ok.items() if k != drop}
        with pytest.raises(ValueError, match=f"without proper {word}"):
            AudioToSpeechLabelDataLayer(_manifest(d, f"no_{drop}.json", [e]), LABELS, 2)
    with pytest.raises(KeyError):
        AudioToSpeechLabelDataLayer(_manifest(d, "unknown.json", [dict(ok, label="left")]), LABELS, 2)
    man = _manifest(d, "ok.json", [ok])
    with pytest.raises(NotImplementedError):
        AudioToSpeechLabelDataLayer(man, LABELS, 2, trim_silence=True)
    with pytest.raises(NotImplementedError):
        AudioToSpeechLabelDataLayer(man, LABELS, 2, augmentor={"white_noise": {"prob": 0.5}})
    with pytest.raises(ValueError, match="sample rate"):
        next(AudioToSpeechLabelDataLayer(man, LABELS, 2, sample_rate=8000).data_iterator)
    with pytest.raises(ValueError):
        AudioToSpeechLabelDataLayer(man, LABELS, 2, shard_by="rows")
    # the path goes through expanduser
    monkeypatch.setenv("HOME", str(d))
    home = _manifest(d, "home.json", [dict(ok, audio_filepath="~/" + os.path.basename(c[0][0]))])
    audio_t, a_len, label, _ = next(AudioToSpeechLabelDataLayer(home, LABELS, 2).data_iterator)
    assert int(a_len[0]) == len(c[0][1]) and label.tolist() == [0]
