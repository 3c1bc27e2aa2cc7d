"""Cost of the encoder activation and residual_mode: QuartzNet15x5 on the fused path with relu / add (the default), hardtanh /
add, selu / add, relu / max and selu / max, at 64 x 10 s and 1 x 10 s, f16x2 (the default arithmetic): ms per batch and the
per-class profile of one pass (vasr_profile_end) -- one JSON line.  Max runs its residual as a GEMM of its own (never folded
into the main GEMM), so its cost is the unfolded residual plus the general epilogue.

    python tools/bench_act.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, synth  # noqa: E402
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
    variants = (("relu", "add"), ("hardtanh", "add"), ("selu", "add"), ("relu", "max"), ("selu", "max"))
    for act, mode in variants:
        cfg = configs.jasper_definition(jas, base["labels"])
        cfg["JasperEncoder"].update(activation=act, residual_mode=mode)
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(base["labels"]) + 1, 0))
        for batch in (64, 1):
            sig, lens = synth.audio_batch(batch, 160000, 0)
            x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
            ms = _time(lambda: eng.forward(x, n), args.steps, args.warmup)
            eng.handle.profile_begin()
            eng.forward(x, n)
            torch.cuda.synchronize()
            prof = eng.handle.profile_end()
            cls = {k: dict(ms=round(v["ms"], 3), launches=v["launches"]) for k, v in prof.items()}
            out["runs"].append(dict(activation=act, residual_mode=mode, batch=batch, ms_per_batch=round(ms, 3), classes=cls))
        del eng
    for act, mode in variants[1:]:
        for batch in (64, 1):
            a, b = (next(r for r in out["runs"] if (r["activation"], r["residual_mode"], r["batch"]) == (x, m, batch))
                    for x, m in (("relu", "add"), (act, mode)))
            out[f"{act}_{mode}_cost_ms_b{batch}"] = round(b["ms_per_batch"] - a["ms_per_batch"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
