"""What tests/test_rotation_host.py and tests/test_gpu_rotation.py share with their child processes, and the child itself (one
per VASR_BUF_ROTATE value: the devtools build reads its switches once per process).

The models are the smallest that reach every aliasing case of run_encoder's buffer rotation (csrc/vasr_host.h BufRotation),
all at repeat 3 behind a stride-2 leading block, so that 2 s of audio are 201 mel frames and 101 encoder frames -- one
128-column tile:

  c512      two 512-channel K = 51 residual blocks: the two-kernel separable path, residual folded into the last GEMM
  c256_512  a 256-channel K = 33 block (the fused depthwise + pointwise kernel, which reads the current tensor) followed by
            a 512-channel one
  max, se, gn   the same with residual_mode "max", with squeeze-and-excitation, with group normalization: the residual
            branch runs on its own and its result R is live across all sub-blocks
  dense     a two-block Jasper dense-residual run, K = 11: non-separable K-tap GEMMs that read the current tensor, panes
  stride2   a non-separable stride-2 first block: the GEMM's output pitch differs from its input's

As a script:  rotation_child.py plan OUT.json   -> the buffer plans (vasr_plan_buffers; no GPU)
              rotation_child.py run OUT.npz     -> every GPU case's outputs
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SEED = 23
RATE = 16000
CLIP = 2 * RATE                                   # 2.0 s: 201 mel frames, 101 encoder frames
RAGGED = (CLIP, int(1.3 * RATE), int(0.6 * RATE))


def blk(filters, repeat, kernel, stride=1, residual=True, separable=True, dense=False, se=False):
    d = dict(filters=filters, repeat=repeat, kernel=[kernel], stride=[stride], dilation=[1], dropout=0.0, residual=residual)
    if separable:
        d["separable"] = True
    if dense:
        d["residual_dense"] = True
    if se:
        d["se"] = True
    return d


LEAD = blk(256, 1, 33, stride=2, residual=False)
JLEAD = blk(256, 1, 11, stride=2, residual=False, separable=False)
TRAIL = blk(512, 1, 1, residual=False, separable=False)
_B256_512 = [LEAD, blk(256, 3, 33), blk(512, 3, 51), TRAIL]
# name -> (JasperEncoder options, block list)
MODELS = {
    "c512": ({}, [LEAD, blk(512, 3, 51), blk(512, 3, 51), TRAIL]),
    "c256_512": ({}, _B256_512),
    "max": ({"residual_mode": "max"}, _B256_512),
    "se": ({}, [LEAD, blk(256, 3, 33, se=True), blk(512, 3, 51, se=True), TRAIL]),
    "gn": ({"normalization_mode": "group", "norm_groups": 8}, _B256_512),
    "dense": ({}, [JLEAD, blk(256, 3, 11, separable=False, dense=True), blk(256, 3, 11, separable=False, dense=True), TRAIL]),
    "stride2": ({}, [JLEAD, blk(512, 3, 51), TRAIL]),
}
BUILTIN = ("quartznet15x5", "quartznet12x1_vi")
# GPU cases: name -> (model, batch, row_independent, slices)
GPU_CASES = {f"{m}_b{b}": (m, b, False, 1) for m in MODELS for b in (6, 3)}
GPU_CASES["row_independent"] = ("c256_512", 6, True, 1)
GPU_CASES["slices"] = ("c512", 16, False, 2)       # (a slice has at least 8 rows: vasr_set_slices)
GPU_CASES["b64"] = ("c256_512", 64, False, 1)      # 64 x 2 s: the 512 x 128 GEMM tile, the fused kernel's 16-wavefront form


def definition(name):
    """-> the model definition dict of a model above or of a built-in one."""
    from viet_asr_amd import configs
    if name in BUILTIN:
        return configs.builtin(name)
    opts, jas = MODELS[name]
    d = configs.jasper_definition(jas)
    d["JasperEncoder"].update(opts)
    return d


def weights(d):
    from viet_asr_amd import engine, synth
    enc, jas = d["JasperEncoder"], d["JasperEncoder"]["jasper"]
    norm = engine.norm_from_config(enc, jas)
    return (synth.encoder_state_dict(jas, 64, SEED, norm=norm),
            synth.decoder_state_dict(jas[-1]["filters"], len(d["labels"]) + 1, SEED))


def host_handle(name):
    """An UNFINALIZED handle of the model with its weights loaded: nothing here touches a device."""
    from viet_asr_amd import _lib, engine
    from viet_asr_amd.frontend_tables import frontend_description
    d = definition(name)
    h = _lib.Handle(frontend=frontend_description(dict(d["AudioToMelSpectrogramPreprocessor"])),
                    dec_feat_in=d["JasperEncoder"]["jasper"][-1]["filters"], num_classes=len(d["labels"]) + 1,
                    **engine.handle_arguments(d["JasperEncoder"], 64))
    for sd in weights(d):
        h.load_state_dict(sd)
    return h


def plan(h, batch, samples=0, mel_frames=0):
    """-> [[kind, dst, src, src2, res], ...] of one encoder pass (include/vasr_devtools.h vasr_plan_buffers)."""
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    cap = 1024
    out = (C.c_int32 * (5 * cap))()
    n = L.vasr_plan_buffers(h.h, batch, samples, mel_frames, out, cap)
    if n < 0:
        _lib.check(n, L)
    assert n <= cap
    return [list(out[5 * i:5 * i + 5]) for i in range(n)]


def plans():
    out = {}
    for name in BUILTIN:
        h = host_handle(name)
        out[name] = plan(h, 64, samples=10 * RATE)                      # the benchmark's shape
        h.close()
    for name in MODELS:
        h = host_handle(name)
        out[name] = plan(h, 6, samples=CLIP)
        out[name + "/b64"] = plan(h, 64, samples=CLIP)
        out[name + "/module"] = plan(h, 6, mel_frames=201)              # vasr_encoder_f32
        if name in ("c512", "c256_512"):
            h.set_row_independent(True)
            out[name + "/row_independent"] = plan(h, 6, samples=CLIP)
            h.set_row_independent(False)
            h.set_slices(2)
            out[name + "/slices"] = plan(h, 16, samples=CLIP)
        h.close()
    return out


def audio(batch):
    """-> (wav [batch, CLIP] float32, zero past each row's length; lengths int64): clips of 2.0 / 1.3 / 0.6 s in turn."""
    from viet_asr_amd import synth
    wav, _ = synth.audio_batch(batch, CLIP, SEED)
    lens = np.array([RAGGED[b % 3] for b in range(batch)], dtype=np.int64)
    for b, n in enumerate(lens):
        wav[b, n:] = 0
    return np.ascontiguousarray(wav, dtype=np.float32), lens


def run(engines, case, device):
    import torch
    from viet_asr_amd import stages
    from viet_asr_amd.engine import QuartzNetCTC
    model, batch, row_independent, slices = GPU_CASES[case]
    if model not in engines:
        d = definition(model)
        engines[model] = (QuartzNetCTC(d, *weights(d), device="cuda:0", gemm="f16x2"), d)
    eng, d = engines[model]
    eng.handle.set_slices(slices)
    wav, lens = audio(batch)
    wd, ld = torch.from_numpy(wav).to(device), torch.from_numpy(lens).to(device)
    eng._workspace(batch, CLIP).fill_(0xFF)                              # every float of the workspace a NaN
    r = eng.forward(wd, ld, want_logp=True, row_independent=row_independent)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in ("logp", "enc_len", "ids", "id_len", "pred")}
    eng.handle.set_row_independent(False)
    eng._row_independent = False
    eng.handle.set_slices(1)
    # the per-module entry points: vasr_melspec_f32, then vasr_encoder_f32 on the port tensor
    mel, seq = stages.melspec(eng.handle, wd, ld)
    c_out = d["JasperEncoder"]["jasper"][-1]["filters"]
    stages._workspace(wd.device, eng.handle.workspace_bytes(batch, mel_frames=mel.shape[2])).fill_(0xFF)
    enc, enc_len = stages.encoder(eng.handle, mel, seq, c_out)
    torch.cuda.synchronize()
    out["enc"], out["enc_len_module"] = enc.cpu().numpy(), enc_len.cpu().numpy()
    return out


def main():
    import viet_asr_amd  # noqa: F401
    mode, path = sys.argv[1], sys.argv[2]
    if mode == "plan":
        with open(path, "w") as f:
            json.dump(plans(), f)
    else:
        import torch
        engines, out = {}, {}
        for case in GPU_CASES:
            for k, v in run(engines, case, torch.device("cuda:0")).items():
                out[f"{case}/{k}"] = v
        np.savez(path, **out)
    print("ROTATION_CHILD_OK")


if __name__ == "__main__":
    main()
