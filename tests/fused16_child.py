"""What tests/test_gpu_fused16.py shares with its child processes, and the child itself (one per VASR_FUSED_WAVES setting:
the devtools build reads its switches once per process).

The cases are the smallest at which the fused depthwise + pointwise kernel's 128-frame tile can go wrong: a 64 -> 256 leading
1x1 block, ONE 256-channel separable block of two sub-layers (K = 33 / 39, with and without the residual, which the last
sub-layer then folds in as a second K range) and the identity trailing block of tests/sep_reference.py, so that both sub-layers
are interior ones (both fused) and a GEMM consumes the maxima the last one published.  Batch 3 at 200 frames (pitch 256: two
tiles a row) with lengths 200 / 129 / 37: a full row, a row that ends one frame into its second tile, a row whose second tile
is dead and whose first tile masks in the middle of a producer lane's segment.  Every column past a row's length is NaN.

As a script: fused16_child.py OUT.npz NAME[:ACTIVATION] ... -> per item the encoder output "y", the leading block's output run
alone "lead", the encoded lengths "lens" and the (fused, depthwise, pointwise) launch counts "counts", in f16x2.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sep_reference as SEP  # noqa: E402

B, T = 3, 200
LENS = np.array([200, 129, 37], dtype=np.int64)
CASES = {f"k{k}{'_res' if res else ''}": SEP.Case(f"fused16_k{k}{'_res' if res else ''}", 64,
                                                  [SEP.LEAD(256), SEP.blk(256, k, 2, res), SEP.TRAIL(256)], 1, B, T)
         for k in (33, 39) for res in (False, True)}


def inputs(case):
    """-> (x [3, 64, 200] float32 with NaN past each row's length, lens)."""
    rng = np.random.default_rng(case.seed)
    x = rng.standard_normal((B, case.feat_in, T)).astype(np.float32)
    x[1] *= np.float32(37.5)
    for b, n in enumerate(LENS):
        x[b, :, n:] = np.nan
    return x, LENS.copy()


def run(case, activation, device):
    import torch
    from viet_asr_amd import asr
    sd = SEP.weights(case)
    x, lens = inputs(case)
    xd, ld = torch.from_numpy(x).to(device), torch.from_numpy(lens).to(device)

    def encoder(blocks, weights):
        enc = asr.JasperEncoder(jasper=blocks, activation=activation, feat_in=case.feat_in)
        enc.load_state_dict({k: torch.as_tensor(v) for k, v in weights.items()})
        enc._get_handle().set_gemm_mode("f16x2")
        return enc

    full = encoder(case.blocks, sd)
    h = full._get_handle()
    h.profile_begin()
    y, yl = full.forward(xd, ld)
    torch.cuda.synchronize()
    p = h.profile_end()
    counts = [int(p[k]["launches"]) for k in ("fused", "depthwise", "pointwise")]
    lead = encoder(case.blocks[:1], SEP.sub_state_dict(sd, 1)).forward(xd, ld)[0]
    return dict(y=y.cpu().numpy(), lead=lead.cpu().numpy(), lens=yl.cpu().numpy(), counts=np.asarray(counts))


def main():
    import torch
    import viet_asr_amd  # noqa: F401
    path, items = sys.argv[1], sys.argv[2:]
    out = {}
    for item in items:
        name, _, act = item.partition(":")
        for k, v in run(CASES[name], act or "relu", torch.device("cuda:0")).items():
            out[f"{item}/{k}"] = v
    np.savez(path, **out)
    print("FUSED16_CHILD_OK")


if __name__ == "__main__":
    main()
