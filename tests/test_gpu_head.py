"""-m gpu: the CTC head (1x1 conv with bias -> log-softmax -> arg-max, frame-major; csrc/decode.hip behind the head's GEMM)
against float64 at every class count and in every GEMM form (tests/head_reference.py: reference, elementwise bound, the
restated kernel choice, the case tables; tests/test_head_host.py holds the bound to honest float32 and to nine defects).

The epilogue alone, through vasr_bench_ctc_head: log-probs inside the epilogue's bound, the prediction bit-for-bit the first
maximum of the device's own log-probs and equal to float64's wherever the top-2 gap decides it, NaN in the logits' padding
columns leaving no trace, guard bands and sentinels around both outputs, either output alone equal to the call that asked for
both, ties at the quarter edges of all four instantiations, non-finite logits as torch.log_softmax + argmax treat them.
GEMM + epilogue, through _lib.Handle(dec_feat_in, num_classes) + stages.decoder in f16x2, bf16x3 and fp32: inside the full
bound, every row a log-distribution, the arg-max against float64.  Then the bit equalities (forced tiles and the chunked kernel
against the product's choice; rows of a large batch against the same rows alone) and the two shipped class counts no other
test puts on a GPU, end to end.

Largest |logp - ref| / bound seen on an MI355X (256 compute units).  The epilogue alone, by instantiation (in brackets: the
same error against the cruder u (d + V + 2 + 2 |lp|) the calibration of head_reference.py is stated against, where the CPU's
float32 restatement reaches 0.62):
    <32>    0.839 (0.571)   v31_t64_b1_span170          Gaussian logits by gain:  1: 0.238 (0.273)
    <64>    0.811 (0.562)   v63_t64_b1_gauss60                                    8: 0.610 (0.465)
    <96>    0.828 (0.584)   v96_t130_b3_gauss60                                  60: 0.828 (0.584)
    <128>   0.821 (0.580)   v98_t65_b3_span170
    planted: ties 0.149 ... 0.335, all classes equal 0.035, the finite frames of the non-finite cases 0.477
No near-tie frame on any Gaussian epilogue case.  The device's expf / logf stay inside the assumed 2 ulps each: C_E = C_L = 4
stand as they started (the worst ratios sit where |z - max| and |lp| are in the hundreds and the terms u |z - max|, u |lp| -- one
rounding each, no library function -- make up the bound; at gain 1, where the library terms dominate it, the ratio is 0.24).
GEMM + epilogue, by kernel and row-block state (worst |logp - ref| / bound | worst |logsumexp| / the row's largest bound):
    kernel    row blocks       f16x2              bf16x3             fp32
    128x64    full             0.035 | 0.014      0.045 | 0.018
    128x64    partial          0.042 | 0.019      0.050 | 0.021
    64x32     full+full        0.006 | 0.001      0.013 | 0.001
    64x32     full+partial     0.033 | 0.017      0.045 | 0.014
    64x32     full+empty       0.022 | 0.008      0.035 | 0.010
    64x32     partial+empty    0.028 | 0.007      0.034 | 0.010
    latency   full             0.004 | 0.001
    latency   partial          0.007 | 0.002
    128x128   full                                                   0.041 | 0.017
    128x128   partial                                                0.047 | 0.021
The largest figures are the K = 64 cases (the large batch among them): the accumulation term K u A_acc is a worst case that grows
with K while the kernels' error grows with its root, so the bound is 20 times what they do at K = 64 and 300 times at K = 1024.
It is the net for what is structurally wrong -- a row not stored, a wrong stride, a dropped chunk or bias, each at 29 times the
bound or more on every case (test_head_host.py) -- and the bit equalities below are what sees a lost low-order product.  Near-tie
frames left out of the arg-max comparison: 2.0 % at worst (v98_k1024_b3_t33, then 1.6 % on v65_k512_b1_t64; the cap is 3 %).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import head_reference as H
from test_gpu_parity import _oracle, _record, logp_tol

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.mark.parametrize("case", H.EPI_CASES, ids=repr)
def test_epilogue_alone_against_float64(gpu, case):
    got = H.device_epilogue(case, gpu)
    r = H.check_epilogue(case, got)
    print(f"{case} vmax {H.vmax_of(case.V)}: worst |logp - ref| / bound = {r['ratio']:.4f} (of the crude bound: {r['crude']:.4f}), "
          f"near-tie frames {r['excluded']:.2%}")
    _record("head_epilogue_f64", case=case.name, vmax=H.vmax_of(case.V), ratio=r["ratio"], crude=r["crude"], excluded=r["excluded"])
    assert not r["failures"], r["failures"]
    # either output alone: the same bits as in the call that asked for both, and the other buffer untouched
    only_p = H.device_epilogue(case, gpu, want_logp=False)
    only_l = H.device_epilogue(case, gpu, want_pred=False)
    assert not only_p["bad"] and not only_l["bad"], (only_p["bad"], only_l["bad"])
    assert np.array_equal(only_p["pred"], got["pred"])
    assert np.array_equal(only_l["logp"].view(np.uint32), got["logp"].view(np.uint32))


@pytest.mark.parametrize("case", H.GEMM_CASES, ids=repr)
def test_head_against_float64_in_the_form_the_product_picks(gpu, case):
    got = H.device_head(case, gpu)
    r = H.check_head(case, got, _cus(gpu))
    for a in got:
        print(f"{case} {a} {r['forms'][a]}: worst |logp - ref| / bound = {r['ratios'][a]:.4f}, |logsumexp| / bound "
              f"{r['lse'].get(a, float('nan')):.4f}, near-tie frames {r['excluded'].get(a, float('nan')):.2%}")
        _record("head_gemm_f64", case=case.name, gemm=a, form=r["forms"][a], ratio=r["ratios"][a], lse=r["lse"].get(a),
                excluded=r["excluded"].get(a))
    assert not r["failures"], r["failures"]


def test_tables_reach_every_form_on_this_device(gpu):
    """The coverage test_head_host.py computes for 256 compute units, on the count of the device the cases really ran on (the
    head's tile choice does not depend on it: 128 rows never reach the 512-row rule that does)."""
    cus = _cus(gpu)
    seen = {a: {(p["kernel"], p["blocks"]) for c in H.GEMM_CASES for p in [H.head_plan(c.V, c.K, c.B, c.T, a, cus)]} for a in H.ARITHS}
    _record("head_forms", cus=cus, forms={a: sorted(f"{k}:{'+'.join(b)}" for k, b in s) for a, s in seen.items()})
    for a in ("f16x2", "bf16x3"):
        assert {("128x64", ("full",)), ("128x64", ("partial",)), ("64x32", ("full", "full")), ("64x32", ("full", "empty")),
                ("64x32", ("full", "partial")), ("64x32", ("partial", "empty"))} <= seen[a], (a, seen[a])
    assert {("lat", ("full",)), ("lat", ("partial",))} <= seen["f16x2"]
    assert seen["fp32"] == {("fp32", ("full",)), ("fp32", ("partial",))}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_rows_of_a_large_batch_equal_the_same_rows_alone(gpu):
    """The 128 x 64 tile the large batch takes against the 64 x 32 tile (f16x2 at K = 64: no latency shape) of three of its rows
    run as a batch of their own, V = 98 (partial row block) and V = 128 (full): the same bits in both split arithmetics -- no
    reduction order depends on the tile, and the f16x2 scale is the utterance's own."""
    rows = [0, 1, H.BIG[0] - 1]
    for V in (98, 128):
        case = H.BY_NAME[H.GemmCase(V, 64, *H.BIG).name]
        cus = _cus(gpu)
        assert H.head_plan(V, 64, case.B, case.T, "bf16x3", cus)["kernel"] == "128x64"
        assert H.head_plan(V, 64, len(rows), case.T, "bf16x3", cus)["kernel"] == "64x32"
        whole = H.device_head(case, gpu, ("f16x2", "bf16x3"))
        alone = H.device_head(case, gpu, ("f16x2", "bf16x3"), rows=rows)
        for a in whole:
            same = _same_bits(whole[a][rows], alone[a])
            _record("head_bits", case=case.name, what=f"{a}: rows {rows} alone", same=same)
            assert same, (case.name, a)


def test_forced_tiles_and_the_chunked_kernel_give_the_products_bits(gpu, tmp_path):
    """VASR_PW3_TILE=3, VASR_PW3_TILE=4 and VASR_PW_LAT=0 (devtools build, one child process per setting, each under its own
    time limit; a child that fails is not started again): the bits of the product's own choice in f16x2 and bf16x3, V in
    {29, 64, 65, 128} at K = 256 and 1024."""
    from viet_asr_amd import _lib
    names = [c.name for c in H.BITS_CASES]
    base = {f"{c.name}/{a}": y for c in H.BITS_CASES for a, y in H.device_head(c, gpu, ("f16x2", "bf16x3")).items()}
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    for env in H.BITS_SETTINGS:
        tag = "_".join(f"{k}{v}" for k, v in env.items())
        path = str(tmp_path / f"{tag}.npz")
        out = subprocess.run([sys.executable, os.path.join(HERE, "head_child.py"), path] + names,
                             env={**os.environ, "VASR_LIB_PATH": dev, **env}, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "HEAD_CHILD_OK" in out.stdout, (env, out.stdout[-2000:], out.stderr[-2000:])
        forced = dict(np.load(path))
        for key, y in base.items():
            same = _same_bits(forced[key], y)
            _record("head_bits", case=key, what=tag, same=same)
            assert same, (env, key)


@pytest.mark.parametrize("n_labels", [97, 63], ids=["98_classes", "64_classes"])
def test_shipped_class_counts_end_to_end(gpu, n_labels):
    """The builtin quartznet12x1 (LABELS_VI_DIGITS: 98 classes with the blank, the <128> epilogue) with synthetic weights, and
    the same with the label list cut to 63 symbols (64 classes, <64>): 2 x 1 s through QuartzNetCTC.forward."""
    from viet_asr_amd import configs, synth
    from viet_asr_amd.engine import QuartzNetCTC
    from oracle import quartznet_oracle as O
    cfg = configs.builtin("quartznet12x1")
    assert len(cfg["labels"]) == 97
    cfg["labels"] = cfg["labels"][:n_labels]
    V = n_labels + 1
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd, dec_sd = synth.encoder_state_dict(jas, 64, 31), synth.decoder_state_dict(1024, V, 31)
    sig, lens = synth.audio_batch(2, 16000, 31, ragged=True)
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd)
    r = eng.forward(torch.from_numpy(sig).to(gpu), torch.from_numpy(lens).to(gpu), want_logp=True)
    torch.cuda.synchronize()
    ref = _oracle(cfg, sig, lens, enc_sd, dec_sd)
    logp, pred = r["logp"].cpu().numpy(), r["pred"].cpu().numpy()
    assert logp.shape == tuple(ref["logp"].shape) and logp.shape[-1] == V
    assert np.array_equal(pred, H.first_argmax(logp))
    ids, n = r["ids"].cpu().numpy(), r["id_len"].cpu().numpy()
    for b in range(2):
        assert ids[b, :n[b]].tolist() == O.ctc_collapse_ids(pred[b], V - 1)
    err = float(np.abs(logp - ref["logp"].numpy()).max())
    _record("head_engine", classes=V, err=err, scale=float(ref["logp"].abs().max()))
    assert err <= logp_tol(ref["logp"]), err
