#!/usr/bin/env python3
"""Per-layer table of one Jasper10x5DR pass (64 x 10 s, f16x2) from two rocprofv3 runs of `tools/bench_jasper.py --one-pass`:

    rocprofv3 --kernel-trace --output-format csv -d DIR/trace -- python tools/bench_jasper.py --one-pass > DIR/layers.json
    rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d DIR/fetch -- python tools/bench_jasper.py --one-pass
    python tools/jasper_layers.py DIR/layers.json DIR/trace DIR/fetch SUSTAINED_TFLOPS

The split GEMM dispatches of the last pass are matched, in launch order, with the layer list the tool printed (kind, M, K, taps,
algorithmic flops, bytes of the f16x2 weight pack).  Per layer: kernel µs, algorithmic TFLOP/s, its fraction of the sustained
f16x2 stream (3 products per multiply), FETCH_SIZE (KiB as rocprofv3 reports it; on gfx950 it under-reports wide coalesced
reads by up to 2 x, MI355X_MICROARCH.md) against the weight pack.  One JSON object on stdout.
"""
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    out = []
    for p in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        out += list(csv.DictReader(open(p)))
    return out


def main(layers_json, trace_dir, fetch_dir, sustained):
    layers = json.load(open(layers_json))["layers"]
    n = len(layers)
    tr = [r for r in rows(trace_dir, "kernel_trace.csv") if "pw_gemm_split_kernel" in r["Kernel_Name"]]
    tr.sort(key=lambda r: int(r["Start_Timestamp"]))
    tr = tr[-n:]
    fetch = {}
    for r in rows(fetch_dir, "counter_collection.csv"):
        if "pw_gemm_split_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "FETCH_SIZE":
            fetch[int(r["Dispatch_Id"])] = fetch.get(int(r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
    fv = [fetch[k] for k in sorted(fetch)][-n:]
    out, tot_us, tot_fl = [], 0.0, 0.0
    for i, L in enumerate(layers):
        us = (int(tr[i]["End_Timestamp"]) - int(tr[i]["Start_Timestamp"])) / 1e3
        tf = L["flops"] / (us * 1e-6) / 1e12
        tot_us += us
        tot_fl += L["flops"]
        rec = dict(L, us=round(us, 1), tflops=round(tf, 1), fraction_of_sustained=round(3 * tf / sustained, 3),
                   kernel="pw_gemm_split_kernel" + tr[i]["Kernel_Name"].split("pw_gemm_split_kernel")[1].split(">")[0] + ">")
        if len(fv) == n:
            rec["fetch_mb"] = round(fv[i] * 1024 / 1e6, 1)
            rec["fetch_over_weight_pack"] = round(fv[i] * 1024 / L["w16_bytes"], 2)
        out.append(rec)
    tf = tot_fl / (tot_us * 1e-6) / 1e12
    print(json.dumps(dict(sustained_f16x2_tflops=sustained, gemm_us=round(tot_us, 1), gemm_tflops=round(tf, 1),
                          gemm_fraction_of_sustained=round(3 * tf / sustained, 3), layers=out)))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], float(sys.argv[4]))
