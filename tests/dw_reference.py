"""What the depthwise tests share (tests/test_gpu_dw.py, tests/test_dw_host.py): a plain float64 restatement of one masked
depthwise layer (reference jasper.py:113-132: mask the input at t >= lens, conv1d with groups == channels and the "same" padding
of jasper.py:60-65; the following MaskedConv1d masks with the new lengths, so the kernels store zeros there), the error bound
of a K-term float32 FMA chain, the test inputs, and the runner that puts one case through vasr_bench_depthwise_layer
(csrc/encoder_dw.hip launch_depthwise with its full argument list) and lists what it finds wrong.

Run as a script it takes the ONE_ROW cases through the library it is given and prints one JSON line: VASR_DW_PAIR is read once
per process, so the one-row kernel needs a process of its own (VASR_LIB_PATH = the devtools build, VASR_DW_PAIR=0)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

EPS = 2.0 ** -24          # unit round-off of float32
TINY = 2.0 ** -126        # so that exact zeros compare


def same_padding(K, stride, dil):
    """get_same_padding (jasper.py:60-65)."""
    if stride > 1 and dil > 1:
        raise ValueError("Only stride OR dilation may be greater than 1")
    return (dil * K) // 2 - 1 if dil > 1 else K // 2


def out_frames(T, K, stride, dil):
    """Columns conv1d gives for T input columns."""
    return (T + 2 * same_padding(K, stride, dil) - dil * (K - 1) - 1) // stride + 1


def lens_out(lens, K, stride, dil):
    """MaskedConv1d.get_seq_len (jasper.py:108-111) followed by the next layer's .to(long): a float division, then truncation."""
    lens = np.asarray(lens, dtype=np.int64)
    lf = (lens + 2 * same_padding(K, stride, dil) - dil * (K - 1) - 1).astype(np.float32) / np.float32(stride) + np.float32(1)
    return np.trunc(lf).astype(np.int32)


def padded(T):
    """vasr_padded_frames without the library (the GPU test confirms it against the library's)."""
    return (T + 127) // 128 * 128


def inputs(K, stride, dil, C, B, T, lens, seed=0):
    """x [B][C][padded(T)] float32: randn with row 1 % B at 300 times the level, FINITE garbage (1e6 randn) in
    lens[b] <= t < T and NaN in every padding column t >= T -- neither may be consumed; taps [C][K] = randn / sqrt(K) with
    channel 3 a thousand times smaller."""
    g = torch.Generator().manual_seed(1000003 * K + 8191 * stride + 131 * dil + 17 * T + B + seed)
    ld = padded(T)
    x = torch.randn(B, C, ld, generator=g)
    x[1 % B] *= 300.0
    junk = 1e6 * torch.randn(B, C, ld, generator=g)
    t = torch.arange(ld)
    past = t[None, :] >= torch.as_tensor(np.asarray(lens, dtype=np.int64))[:, None]
    x = torch.where(past[:, None, :], junk, x)
    x[:, :, T:] = float("nan")
    w = torch.randn(C, K, generator=g) / K ** 0.5
    if C > 3:
        w[3] *= 1e-3
    return x.contiguous(), w.contiguous()


def reference(x, w, lens_in, lens_o, T, stride, dil):
    """-> (ref, bound), float64 [B][C][t_out], on the CPU.  ref: mask at t >= lens_in, conv1d(groups = C), zero at
    t >= lens_o.  bound = K 2^-24 (|w| * |x masked|) + 2^-126: the first-order worst case of K float32 fused multiply-adds
    whatever their order or the number of partial accumulators -- derived, per element, not measured."""
    B, C, _ = x.shape
    K = w.shape[1]
    pad = same_padding(K, stride, dil)
    t = torch.arange(T)
    live = (t[None, :] < torch.as_tensor(np.asarray(lens_in, dtype=np.int64))[:, None])[:, None, :]
    xm = torch.where(live, x[:, :, :T].double(), torch.zeros((), dtype=torch.float64))
    w64 = w.double()[:, None, :]
    ref = torch.nn.functional.conv1d(xm, w64, None, stride, pad, dil, C)
    mag = torch.nn.functional.conv1d(xm.abs(), w64.abs(), None, stride, pad, dil, C)
    t_out = ref.shape[-1]
    assert t_out == out_frames(T, K, stride, dil)
    keep = (torch.arange(t_out)[None, :] < torch.as_tensor(np.asarray(lens_o, dtype=np.int64))[:, None])[:, None, :]
    ref = torch.where(keep, ref, torch.zeros((), dtype=torch.float64))
    return ref, K * EPS * mag + TINY


def ragged(B, T, zero_row=False, floor=0):
    """Row lengths of a ragged batch: T first (every column is somebody's), then half, 1, the values around a 512-frame
    tile edge where T allows, T - 1, 2, 130; B = 1: T - 3.  zero_row: row 2 has length 0.  floor: the least length allowed."""
    if B == 1:
        return [max(T - 3, 1)]
    cand = [v for v in (T, T // 2 + 1, 1, 513, 512, 511, T - 1, 2, 130) if floor <= v <= T]
    lens = [cand[i % len(cand)] for i in range(B)]
    if zero_row:
        lens[2] = 0
    return lens


class Case:
    def __init__(self, K, stride, dil, C, B, T, lens="ragged", offset=0):
        self.K, self.stride, self.dil, self.C, self.B, self.T, self.offset = K, stride, dil, C, B, T, offset
        self.kind = lens
        assert lens in ("full", "ragged", "zero")
        self.lens_in = [T] * B if lens == "full" else ragged(B, T, zero_row=lens == "zero", floor=1 if stride > 1 else 0)

    def __repr__(self):
        off = f"-x+{self.offset}" if self.offset else ""
        return f"K{self.K}s{self.stride}d{self.dil}-C{self.C}-B{self.B}-T{self.T}-{self.kind}{off}"


def run_case(L, case, device):
    """One case through vasr_bench_depthwise_layer on `device` -> dict(failures=[...], ratio=worst |y - ref| / bound,
    digest=sha1 of y).  Checked: the bound elementwise below t_out, exact zeros from lens_out[b] to the row pitch, no NaN
    anywhere in y (y starts as NaN: an unwritten column shows; x holds NaN in its padding: a consumed column shows), the
    published maxima reduced over the slots bit-equal to max |y[b]| of the stored tensor, and the same y without a table."""
    from viet_asr_amd import _lib
    c = case
    bad = []
    ldx, t_out = int(L.vasr_padded_frames(c.T)), out_frames(c.T, c.K, c.stride, c.dil)
    ldy = int(L.vasr_padded_frames(t_out))
    assert ldx == padded(c.T) and ldy == padded(t_out)
    lo = lens_out(c.lens_in, c.K, c.stride, c.dil)
    assert int(lo.max()) <= t_out and int(lo.min()) >= 0
    x, w = inputs(c.K, c.stride, c.dil, c.C, c.B, c.T, c.lens_in)
    ref, bound = reference(x, w, c.lens_in, lo, c.T, c.stride, c.dil)
    flat = torch.empty(x.numel() + c.offset, device=device)         # offset: an x that is not 16-byte aligned
    xd = flat[c.offset:].view(x.shape)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == (4 * c.offset) % 16
    wd = w.to(device)
    li = torch.tensor(c.lens_in, dtype=torch.int32, device=device)
    lod = torch.from_numpy(lo).to(device)
    slots = c.C * ((ldy + 255) // 256) * 4
    st = torch.cuda.current_stream().cuda_stream
    ys = []
    for table in (True, False):
        y = torch.full((c.B, c.C, ldy), float("nan"), device=device)
        amax = torch.full((c.B, slots), -1, dtype=torch.int32, device=device)      # 0xffffffff: a slot below n left unwritten shows
        _lib.check(L.vasr_bench_depthwise_layer(xd.data_ptr(), wd.data_ptr(), li.data_ptr(), lod.data_ptr(), c.B, c.C, c.T, c.K,
                                                c.stride, c.dil, y.data_ptr(), amax.data_ptr() if table else None, slots, st), L)
        torch.cuda.synchronize()
        ys.append((y.cpu(), amax.cpu()))
    (y, amax), (y_bare, _) = ys
    if bool(torch.isnan(y).any()):
        bad.append(f"{int(torch.isnan(y).sum())} NaN in y (a column not written, or padding consumed)")
    err = (y[:, :, :t_out].double() - ref).abs()
    ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max())
    if not bool((err <= bound).all()):
        b, ch, t = np.unravel_index(int(torch.nan_to_num(err / bound, nan=float("inf")).argmax()), err.shape)
        bad.append(f"|y - ref| = {float(err[b, ch, t]):.3e} > bound {float(bound[b, ch, t]):.3e} at b={b} c={ch} t={t} "
                   f"({int((~(err <= bound)).sum())} elements outside)")
    for b in range(c.B):
        tail = y[b, :, int(lo[b]):]
        if tail.numel() and not bool((tail == 0).all()):
            bad.append(f"row {b}: {int((tail != 0).sum())} columns past lens_out = {int(lo[b])} are not zero")
    got = amax.numpy().view(np.uint32).max(-1)
    want = y.abs().amax((1, 2)).numpy().view(np.uint32)
    if not np.array_equal(got, want):
        bad.append(f"published maxima {got.tolist()} != max|y[b]| {want.tolist()} (fp32 bits)")
    if not np.array_equal(y_bare.numpy().view(np.uint32), y.numpy().view(np.uint32)):
        bad.append("y differs without a maxima table")
    return dict(failures=[f"{c!r}: {m}" for m in bad], ratio=ratio, digest=hashlib.sha1(y.numpy().tobytes()).hexdigest())


# (K, dilation) of every launch_dw_pair<K, DIL> / dw_conv_kernel<K, 1, DIL> instantiation
TILED = ((33, 1), (39, 1), (51, 1), (63, 1), (75, 1), (87, 2))
# dw_conv_kernel<K, 1> x 5 and dw_conv_kernel<87, 1, 2>: a 256-column pitch (one tile, its second group of 256 outputs past
# the pitch), 640 (a second tile of which 128 columns exist) and 1152 (three tiles); B = 1 and an odd ragged batch
ONE_ROW = [Case(K, 1, dil, 8, B, T, "ragged" if (B, T) != (1, 516) else "full")
           for K, dil in TILED for B in (1, 3) for T in (200, 516, 1030)]


def main():
    """The ONE_ROW cases on the library VASR_LIB_PATH names, with the switches of this process's environment."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import viet_asr_amd  # noqa: F401
    from viet_asr_amd import _lib
    L = _lib.dev_lib()
    dev = torch.device("cuda:0")
    out = dict(failures=[], ratios={}, digests={}, dw_pair=os.environ.get("VASR_DW_PAIR"))
    for c in ONE_ROW:
        r = run_case(L, c, dev)
        out["failures"] += r["failures"]
        out["ratios"][repr(c)] = r["ratio"]
        out["digests"][repr(c)] = r["digest"]
    print("DW_ONE_ROW " + json.dumps(out))


if __name__ == "__main__":
    main()
