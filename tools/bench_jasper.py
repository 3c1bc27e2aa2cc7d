"""Jasper10x5DR on the fused path: ms per batch and x real time at 64 x 10 s and 1 x 10 s in the f16x2 and fp32 arithmetics,
the GEMM class's algorithmic TFLOP/s as a fraction of the box's own sustained f16x2 MFMA rate (tools/mfma_sustained.py's
stream), and the same encoder + head as torch float32 conv1d on the same GPU (the reference's arithmetic) -- one JSON line.

    python tools/bench_jasper.py [--steps 5] [--warmup 2]

`--one-pass` runs the 64 x 10 s batch once in f16x2 (after one warm-up pass) and prints the split-GEMM layer list of a pass in
launch order, for `tools/jasper_layers.py`, which matches it with the dispatches of a `rocprofv3 --kernel-trace` run and of a
separate `rocprofv3 --pmc FETCH_SIZE` run: per-layer time, fraction of the sustained rate and weight-pack traffic.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import _lib, configs, stages, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def sustained_f16x2_tflops():
    L = _lib.dev_lib()
    sink, fl = torch.zeros(16, device="cuda"), ctypes.c_double()
    st = torch.cuda.current_stream().cuda_stream
    run = lambda: _lib.check(L.vasr_bench_mfma_sustained(3, 256, 8000, sink.data_ptr(), ctypes.byref(fl), st), L)
    ms = _time(run, 3, 1)
    return fl.value / (ms * 1e-3) / 1e12


def torch_reference(jas, enc_sd, dec_sd, mel, seq):
    """JasperEncoder + head in eval mode as plain float32 conv1d / batch_norm (masking as MaskedConv1d)."""
    t = lambda k: enc_sd[k]
    bn = lambda x, p: F.batch_norm(x, t(p + ".running_mean"), t(p + ".running_var"), t(p + ".weight"), t(p + ".bias"),
                                   False, 0.1, 1e-3)

    def mconv(x, lens, w, stride=1, pad=0, dil=1):
        x = x.masked_fill(torch.arange(x.shape[2], device=x.device)[None, None, :] >= lens[:, None, None], 0)
        k = w.shape[2]
        return F.conv1d(x, w, None, stride, pad, dil), (lens + 2 * pad - dil * (k - 1) - 1) // stride + 1

    xs, lens = [mel], seq
    for i, l in enumerate(jas):
        k, s, d = synth.kernel_of(l), synth.first(l["stride"]), synth.first(l["dilation"])
        pad = (d * k) // 2 - 1 if d > 1 else k // 2
        out, ln, j = xs[-1], lens, 0
        for r in range(l["repeat"]):
            out, ln = mconv(out, ln, t(f"encoder.{i}.mconv.{j}.conv.weight"), s, pad, d)
            out = bn(out, f"encoder.{i}.mconv.{j + 1}")
            j += 2
            if r != l["repeat"] - 1:
                out = F.relu(out)
                j += 2
        if l["residual"]:
            for q in range(len(xs) if l.get("residual_dense") else 1):
                res, _ = mconv(xs[q], lens, t(f"encoder.{i}.res.{q}.0.conv.weight"))   # (a plain residual block: xs[0] too)
                out = out + bn(res, f"encoder.{i}.res.{q}.1")
        out = F.relu(out)
        xs = xs + [out] if (l.get("residual_dense") and l["residual"]) else [out]
        lens = ln
    y = F.conv1d(xs[-1], dec_sd["decoder_layers.0.weight"], dec_sd["decoder_layers.0.bias"])
    return F.log_softmax(y.transpose(1, 2), dim=-1)


def gemm_layers(jas, feat_in, batch, T, n_classes):
    """The split-GEMM launches of one fused pass, in launch order: per block the residual GEMM (dense: over all panes), then
    the sub-block convolutions; then the CTC head.  T = mel frames."""
    out, c, panes, t = [], feat_in, [], T
    add = lambda kind, i, m, k, taps, frames: out.append(dict(
        kind=kind, block=i, M=m, K=k, taps=taps, flops=2.0 * m * k * frames * batch,
        w16_bytes=4 * ((m + 127) // 128 * 128) * k))
    for i, l in enumerate(jas):
        k, s, d = synth.kernel_of(l), synth.first(l["stride"]), synth.first(l["dilation"])
        pad = (d * k) // 2 - 1 if d > 1 else k // 2
        t_out = (t + 2 * pad - d * (k - 1) - 1) // s + 1
        dense = l.get("residual_dense", False)
        if dense:
            panes.append(c)
        if l["residual"]:
            add("residual", i, l["filters"], sum(panes) if dense else c, 1, t)
        ci = c
        for _ in range(l["repeat"]):
            add("conv" if k > 1 or s > 1 else "1x1", i, l["filters"], k * ci, k, t_out)
            ci = l["filters"]
        if not (dense and l["residual"]):
            panes = []
        c, t = l["filters"], t_out
    add("head", len(jas), n_classes, c, 1, t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--one-pass", action="store_true")
    args = ap.parse_args()
    cfg = configs.builtin("jasper10x5dr")
    jas = cfg["JasperEncoder"]["jasper"]
    enc_sd = synth.encoder_state_dict(jas, 64, 0)
    dec_sd = synth.decoder_state_dict(1024, len(cfg["labels"]) + 1, 0)
    eng = QuartzNetCTC(cfg, enc_sd, dec_sd)
    if args.one_pass:
        sig, lens = synth.audio_batch(64, 160000, 0)
        x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
        for _ in range(2):
            eng.forward(x, n)
        torch.cuda.synchronize()
        print(json.dumps(dict(layers=gemm_layers(jas, 64, 64, eng.handle.mel_frames(160000), len(cfg["labels"]) + 1))))
        return
    peak = sustained_f16x2_tflops()
    dev_enc = {k: torch.as_tensor(v).cuda() for k, v in enc_sd.items() if np.asarray(v).dtype.kind == "f"}
    dev_dec = {k: torch.as_tensor(v).cuda() for k, v in dec_sd.items()}
    out = dict(model="jasper10x5dr", sustained_f16x2_tflops=round(peak, 1), runs=[])
    for batch in (64, 1):
        sig, lens = synth.audio_batch(batch, 160000, 0)
        x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
        work = eng.handle.algorithmic_work(batch, 160000)
        for gemm in ("f16x2", "fp32"):
            eng.handle.set_gemm_mode(gemm)
            ms = _time(lambda: eng.forward(x, n), args.steps, args.warmup)
            eng.handle.profile_begin()
            eng.forward(x, n)
            torch.cuda.synchronize()
            prof = eng.handle.profile_end()["pointwise"]
            tf = prof["flops"] / (prof["ms"] * 1e-3) / 1e12 if prof["ms"] else 0.0
            out["runs"].append(dict(batch=batch, gemm=gemm, ms_per_batch=round(ms, 2), x_real_time=round(batch * 10.0 / (ms * 1e-3), 1),
                                    gemm_ms=round(prof["ms"], 2), gemm_tflops=round(tf, 1),
                                    gemm_fraction_of_sustained=round(3 * tf / peak, 3) if gemm == "f16x2" else None,
                                    algorithmic_tflop=round(work["pointwise_flops"] / 1e12, 2)))
        eng.handle.set_gemm_mode("f16x2")
        mel, seq = stages.melspec(eng.handle, x, n)
        with torch.no_grad():
            ms = _time(lambda: torch_reference(jas, dev_enc, dev_dec, mel, seq), max(1, args.steps // 2), 1)
        out["runs"].append(dict(batch=batch, gemm="torch_fp32_conv1d", ms_per_batch=round(ms, 2),
                                x_real_time=round(batch * 10.0 / (ms * 1e-3), 1)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
