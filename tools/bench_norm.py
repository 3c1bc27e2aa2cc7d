"""Cost of GroupNorm: QuartzNet15x5 on the fused path with BatchNorm (folded into the GEMM epilogues) and with
normalization_mode "group" (norm_groups 32), "layer" and "instance", at 64 x 10 s and 1 x 10 s, f16x2 (the default
arithmetic): ms per batch and the per-class profile of one pass (vasr_profile_end; the GroupNorm passes -- row statistics,
group merge, apply -- are counted in the depthwise class, "depthwise_and_norm") -- one JSON line.

    python tools/bench_norm.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, engine, synth  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    base = configs.builtin("quartznet15x5")
    out = dict(model="quartznet15x5", gemm="f16x2", runs=[])
    jas = base["JasperEncoder"]["jasper"]
    modes = (("batch", -1), ("group", 32), ("layer", -1), ("instance", -1))
    for mode, ng in modes:
        cfg = configs.jasper_definition(jas, base["labels"])
        cfg["JasperEncoder"].update(normalization_mode=mode, norm_groups=ng)
        norm = engine.norm_from_config(cfg["JasperEncoder"], jas)
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0, norm=norm),
                           synth.decoder_state_dict(1024, len(base["labels"]) + 1, 0))
        for batch in (64, 1):
            sig, lens = synth.audio_batch(batch, 160000, 0)
            x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
            ms = _time(lambda: eng.forward(x, n), args.steps, args.warmup)
            eng.handle.profile_begin()
            eng.forward(x, n)
            torch.cuda.synchronize()
            prof = eng.handle.profile_end()
            cls = {("depthwise_and_norm" if k == "depthwise" else k): dict(ms=round(v["ms"], 3), launches=v["launches"])
                   for k, v in prof.items()}
            out["runs"].append(dict(mode=mode, norm_groups=ng, batch=batch, ms_per_batch=round(ms, 3), classes=cls))
        del eng
    for mode, _ng in modes[1:]:
        for batch in (64, 1):
            a, b = (next(r for r in out["runs"] if r["mode"] == m and r["batch"] == batch) for m in ("batch", mode))
            out[f"{mode}_cost_ms_b{batch}"] = round(b["ms_per_batch"] - a["ms_per_batch"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
