"""Cost of grouped JasperBlocks: QuartzNet15x5 with ``groups`` = 1, 2, 4, 8 on every block on the fused path, at 64 x 10 s and
1 x 10 s, f16x2 (the default arithmetic): ms per batch and the per-class profile of one pass (vasr_profile_end) -- for the
product path, and for the block-diagonal form of every grouped layer (VASR_NO_GROUPED=1: the devtools library, in a child
process, since the switch is read once per process) -- one JSON line.

    python tools/bench_groups.py [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import viet_asr_amd  # noqa: E402,F401
from viet_asr_amd import configs, synth  # noqa: E402
from viet_asr_amd.engine import QuartzNetCTC  # noqa: E402

GROUPS = (1, 2, 4, 8)


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


def runs(steps, warmup):
    base = configs.builtin("quartznet15x5")
    out = []
    for G in GROUPS:
        jas = [dict(b, groups=G) for b in base["JasperEncoder"]["jasper"]]
        cfg = configs.jasper_definition(jas, base["labels"])
        eng = QuartzNetCTC(cfg, synth.encoder_state_dict(jas, 64, 0), synth.decoder_state_dict(1024, len(base["labels"]) + 1, 0))
        for batch in (64, 1):
            sig, lens = synth.audio_batch(batch, 160000, 0)
            x, n = torch.from_numpy(sig).cuda(), torch.from_numpy(lens).cuda()
            ms = _time(lambda: eng.forward(x, n), steps, warmup)
            eng.handle.profile_begin()
            eng.forward(x, n)
            torch.cuda.synchronize()
            prof = eng.handle.profile_end()
            cls = {k: dict(ms=round(v["ms"], 3), launches=v["launches"]) for k, v in prof.items()}
            out.append(dict(groups=G, batch=batch, ms_per_batch=round(ms, 3), classes=cls))
        del eng
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RUNS " + json.dumps(runs(args.steps, args.warmup)))
        return
    out = dict(model="quartznet15x5", gemm="f16x2", product=runs(args.steps, args.warmup))
    dev = os.path.join(ROOT, "viet-asr_amd", "lib", "libvasr_hip_dev.so")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup)],
                       env={**os.environ, "VASR_LIB_PATH": dev, "VASR_NO_GROUPED": "1"}, capture_output=True, text=True,
                       timeout=1200)
    line = next((l for l in r.stdout.splitlines() if l.startswith("RUNS ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"block-diagonal child failed (exit {r.returncode})")
    out["block_diagonal"] = json.loads(line[5:])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
