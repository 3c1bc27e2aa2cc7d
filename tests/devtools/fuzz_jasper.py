#!/usr/bin/env python3
"""Randomised whole-path comparison of JASPER layouts against the oracle (dev tool, GPU):

    python tests/devtools/fuzz_jasper.py [n_cases] [seed0] [max_seconds] [se]

The Jasper counterpart of fuzz_encoder.py.  Each case draws a layout the reference can run: a non-separable prologue (strided
or not), ONE contiguous dense run of 1-4 blocks (every one residual and dense; its pane buffer and dense-residual GEMMs),
optionally a plain residual block after the run (its residual comes from pane 0, the run's input) and a 1x1 epilogue block --
filters 128-384 (the library refuses widths that are not multiples of 128), kernels 1-29, dilation 1 or 2, repeats 1-3.  Batches
of 1-5 / 6-20 / 21-72 rows of short clips with one very short row, so that the product's own choice of CONV tile is
exercised, in a randomly drawn GEMM arithmetic.  Checks against oracle.quartznet_oracle (which runs dense residuals):
log-probs within the goldens' tolerance, encoded lengths equal, predictions equal wherever the oracle's margin exceeds twice
the tolerance, everything finite.  A fourth argument "se" adds squeeze-and-excitation draws (draw_se: flag, ratio and
excitation regime per case, from streams of their own, so the layouts stay those of the plain run).  Prints one summary line."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402
from oracle import quartznet_oracle as O  # noqa: E402  (checker only)

STATS = {"cases": 0, "rows": 0, "worst_err_over_tol": 0.0, "by_batch_class": [0, 0, 0], "dense_blocks": 0, "se_blocks": 0}
SE_REGIMES = ("synthetic", "mixed", "strong")
FLOP_BUDGET = 1.5e10            # per case, for the oracle's float32 convolutions on the CPU


def _blk(rng, filters, residual, dense=False, stride=1, k=None):
    k = int(rng.choice(np.arange(1, 30, 2))) if k is None else k
    dil = 2 if stride == 1 and k > 1 and rng.random() < 0.25 else 1
    d = dict(filters=int(filters), repeat=int(rng.integers(1, 4)) if stride == 1 else 1, kernel=[k], stride=[stride],
             dilation=[dil], dropout=0.0, residual=bool(residual))
    if dense:
        d["residual_dense"] = True
    return d


def random_jasper_layout(rng):
    width = lambda: int(128 * rng.integers(1, 4))                          # 128 ... 384 (vasr_create: multiples of 128)
    stride = int(rng.choice([1, 2]))
    pro = _blk(rng, width(), False, stride=stride, k=int(rng.choice([1, 3, 5, 7, 11])) if stride == 2 else None)
    jas = [pro]
    for _ in range(int(rng.integers(1, 5))):
        jas.append(_blk(rng, width(), True, dense=True))
    if rng.random() < 0.5:          # plain residual block after the run: its input width must be the run's input width
        jas[-1]["filters"] = pro["filters"]
        jas.append(_blk(rng, width(), True))
    if rng.random() < 0.5:
        jas.append(_blk(rng, width(), False, k=1))
    return jas


def draw_se(jas, case):
    """Opt-in squeeze-and-excitation draws, from a stream of their own (the layout's draws are untouched): each block gets SE
    with probability 0.6 and a ratio leaving 1 ... filters hidden units; one excitation regime per case.  -> regime."""
    rng = np.random.default_rng(920000 + case)
    for b in jas:
        if rng.random() < 0.6:
            b["se"] = True
            b["se_reduction_ratio"] = int(rng.choice([1, 2, 5, 8, 16, 48, b["filters"]]))
    return str(rng.choice(SE_REGIMES))


def apply_se_regime(sd, regime, case):
    """synthetic: synth's own SE weights (s close to 1); mixed: W1 ~ N(0, 1/C), W2 ~ N(0, 9/h) (s across (0, 1)); strong:
    W2 ~ -|N(6, 3)| / sqrt(h) (most s far below 1 -- the republished fp16-split maxima carry the next layer)."""
    rng = np.random.default_rng(930000 + case)
    for k in sorted(sd):
        if regime == "mixed" and k.endswith(".fc.0.weight"):
            h, c = sd[k].shape
            sd[k] = rng.normal(0, 1 / np.sqrt(c), (h, c)).astype(np.float32)
        elif regime in ("mixed", "strong") and k.endswith(".fc.2.weight"):
            c, h = sd[k].shape
            w = rng.normal(0, 3, (c, h)) if regime == "mixed" else -np.abs(rng.normal(6, 3, (c, h)))
            sd[k] = (w / np.sqrt(h)).astype(np.float32)


def _flops(jas, T):
    c, f = 64, 0.0
    for b in jas:
        f += 2.0 * T * b["repeat"] * b["kernel"][0] * c * b["filters"] + 2.0 * T * c * b["filters"] * (len(jas))
        c = b["filters"]
    return f


def jasper_case(case, se=False):
    """se=True: SE drawn on top of the case's layout (draw_se / apply_se_regime); se=False draws exactly what it always did."""
    rng = np.random.default_rng(910000 + case)
    cls = int(rng.integers(0, 3))
    B = int(rng.integers(1, 6)) if cls == 0 else int(rng.integers(6, 21)) if cls == 1 else int(rng.integers(21, 73))
    L = int(rng.integers(1500, 30000)) if cls == 0 else int(rng.integers(1500, 12000)) if cls == 1 else int(rng.integers(1500, 6000))
    while True:
        jas = random_jasper_layout(rng)
        if _flops(jas, B * (1 + L // 160)) <= FLOP_BUDGET:
            break
    regime = draw_se(jas, case) if se else None
    cfg = configs.jasper_definition(jas)
    enc_sd = synth.encoder_state_dict(jas, 64, case)
    if se:
        apply_se_regime(enc_sd, regime, case)
        STATS["se_blocks"] += sum(1 for b in jas if b.get("se"))
    dec_sd = synth.decoder_state_dict(jas[-1]["filters"], len(cfg["labels"]) + 1, case)
    gemm = str(rng.choice(["f16x2", "f16x2", "bf16x3", "fp32"]))
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd, gemm=gemm)
    sig, lens = synth.audio_batch(B, L, case, ragged=True)
    lens[int(rng.integers(0, B))] = L
    lens[int(rng.integers(0, B))] = max(300, int(lens.min()) // 3)
    for b in range(B):
        sig[b, lens[b]:] = 0
    ref = O.forward_all(sig, lens, enc_sd, dec_sd, jas)
    r = eng.forward(torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda(), want_logp=True)
    torch.cuda.synchronize()
    lp, want = r["logp"].cpu(), ref["logp"]
    tol = max(5e-4, 2e-5 * float(want.abs().max()))
    err = float((lp - want).abs().max()) if lp.shape == want.shape else float("inf")
    top2 = want.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 2 * tol
    STATS["cases"] += 1
    STATS["rows"] += B
    STATS["by_batch_class"][cls] += 1
    STATS["dense_blocks"] += sum(1 for b in jas if b.get("residual_dense"))
    STATS["worst_err_over_tol"] = max(STATS["worst_err_over_tol"], err / tol)
    ok = (err <= tol and bool(torch.isfinite(r["logp"]).all()) and r["enc_len"].cpu().tolist() == ref["enc_len"].tolist()
          and bool((r["pred"].cpu()[clear] == ref["pred"][clear]).all()))
    if ok:
        return None
    return (f"jasper case {case}: gemm {gemm} B {B} L {L} err {err:.3e} tol {tol:.3e} se {regime} blocks "
            f"{[(b['filters'], b['kernel'][0], b['repeat'], b['stride'][0], b['dilation'][0], b['residual'], b.get('residual_dense', False), b.get('se_reduction_ratio', 0) if b.get('se') else 0) for b in jas]}")


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    S0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    LIMIT = float(sys.argv[3]) if len(sys.argv) > 3 else 1e9
    SE = len(sys.argv) > 4 and sys.argv[4] == "se"
    t0, bad = time.time(), 0
    for case in range(S0, S0 + N):
        if time.time() - t0 > LIMIT:
            break
        msg = jasper_case(case, se=SE)
        if msg:
            bad += 1
            print("MISMATCH", msg, flush=True)
    print(f"{STATS['cases']} Jasper cases from {S0} ({STATS['rows']} rows; batches of 1-5 / 6-20 / 21-72 rows: {STATS['by_batch_class']}; "
          f"{STATS['dense_blocks']} dense blocks, {STATS['se_blocks']} SE blocks), {bad} mismatches, worst error {STATS['worst_err_over_tol']:.2f} x the tolerance, "
          f"{time.time() - t0:.0f} s")
