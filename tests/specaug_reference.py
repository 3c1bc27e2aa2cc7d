"""What the SpecAugment / SpecCutout tests share: a numpy rasteriser from (rects, row_begin) to a mask -- the statement
vasr_spec_mask_f32 is held to, clipping and empty lists included --, the table of golden cases (tests/golden/
make_golden_specaug.py runs the REAL reference on them and stores its masks and draws), and the hand-made rectangle tables of
the kernel tests.  No GPU, no reference checkout needed."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the kernel's own tiling (viet-asr_amd/csrc/vasr_internal.h: kSpecTile, kSpecRows, kSpecChunk; 16-byte vectors of 4 cells): the
# GPU tests put one width just below, at and just above each, a feature count across the row tile, and a row list longer than
# one LDS chunk
TIME_TILE, ROW_TILE, RECT_CHUNK, VEC = 1024, 8, 256, 4

# (B, D, T, ld): the issue's shapes, then the widths around the vector width and the time tile (D = 9: across the row tile;
# ld = 1027: rows that leave the 16-byte grid, which takes the dword path)
KERNEL_SHAPES = [(1, 1, 1, 1), (2, 3, 5, 5), (3, 64, 37, 37), (2, 64, 37, 48), (2, 80, 130, 130),
                 (1, 2, VEC - 1, VEC - 1), (1, 2, VEC, VEC), (1, 2, TIME_TILE - 1, TIME_TILE - 1), (1, 9, TIME_TILE, TIME_TILE),
                 (2, 9, TIME_TILE + 1, TIME_TILE + 3),
                 # 16-byte pitches with more than one time tile: the out-of-place form's vector path in its second and third tile
                 (1, 9, TIME_TILE + 8, TIME_TILE + 8), (2, 9, 2 * TIME_TILE + 4, 2 * TIME_TILE + 8)]

# kind: which reference class runs; args: its constructor arguments (everything else: the reference's defaults)
CASES = [
    dict(name="augment_3x64x37", kind="augment", args=dict(freq_masks=2, time_masks=2), seed=101, shape=(3, 64, 37)),
    dict(name="augment_time_width_over_T", kind="augment", args=dict(freq_masks=2, time_masks=3, time_width=10), seed=102,
         shape=(2, 64, 7)),
    dict(name="augment_freq_width_over_D", kind="augment", args=dict(freq_masks=3, time_masks=2, freq_width=10), seed=103,
         shape=(1, 5, 130)),
    dict(name="cutout_shipped_2x64x7", kind="cutout", args=dict(rect_masks=5, rect_time=120, rect_freq=50), seed=104,
         shape=(2, 64, 7)),
    dict(name="cutout_shipped_3x64x300", kind="cutout", args=dict(rect_masks=5, rect_time=120, rect_freq=50), seed=105,
         shape=(3, 64, 300)),
    dict(name="cutout_default_widths_2x64x37", kind="cutout", args=dict(rect_masks=3), seed=106, shape=(2, 64, 37)),
    dict(name="both_shared_rng_4x80x257", kind="both",
         args=dict(freq_masks=2, time_masks=2, freq_width=15, time_width=25, rect_masks=5, rect_time=120, rect_freq=50),
         seed=107, shape=(4, 80, 257)),
]


def rasterise(rects, row_begin, B, D, T):
    """-> bool [B, D, T]: True where a rectangle of the row covers the cell.  Rectangles are clipped to [0, D) x [0, T); lo >= hi,
    a non-increasing row_begin pair and a negative row_begin[b] are empty -- the kernel's rules."""
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    row_begin = np.asarray(row_begin, dtype=np.int64)
    assert row_begin.shape == (B + 1,)
    mask = np.zeros((B, D, T), dtype=bool)
    for b in range(B):
        lo, hi = int(row_begin[b]), int(row_begin[b + 1])
        if lo < 0 or hi <= lo:
            continue
        for f0, f1, t0, t1 in rects[lo:hi]:
            f0, f1, t0, t1 = max(f0, 0), min(f1, D), max(t0, 0), min(t1, T)
            if f0 < f1 and t0 < t1:
                mask[b, f0:f1, t0:t1] = True
    return mask


def csr(rows):
    """per-row lists of (f0, f1, t0, t1) -> (rects int32 [n, 4], row_begin int32 [B + 1]); nothing is dropped or clipped"""
    begin = np.zeros(len(rows) + 1, dtype=np.int32)
    begin[1:] = np.cumsum([len(r) for r in rows])
    return np.asarray([r for row in rows for r in row], dtype=np.int32).reshape(-1, 4), begin


def load_cases():
    """-> [(case dict with "draws", mask bool [B, D, T])] from tests/golden/specaug_cases.{json,npz}"""
    with open(os.path.join(GOLDEN, "specaug_cases.json")) as f:
        meta = json.load(f)
    packed = np.load(os.path.join(GOLDEN, "specaug_cases.npz"))
    out = []
    for c in meta["cases"]:
        B, D, T = c["shape"]
        out.append((c, np.unpackbits(packed[c["name"]])[: B * D * T].astype(bool).reshape(B, D, T)))
    return out


def rect_tables(B, D, T, slack=8):
    """The hand-made tables of the kernel tests for a [B, D, T] tensor -> {name: (rects, row_begin)}.  A rectangle may reach up
    to `slack` cells past the tensor (the kernel clips it), never further."""
    far_t, far_f = T + slack, D + slack
    tabs = {}
    # every t0 mod 4 x width 0 .. 9, one feature row high, spread over the rows and the width
    rows = [[] for _ in range(B)]
    for k in range(40):
        w, t0 = k // 4, min(4 * ((5 * k) % max(T // 4, 1)) + k % 4, far_t)
        f = (3 * k) % D
        rows[k % B].append((f, f + 1, t0, min(t0 + w, far_t)))
    tabs["starts_mod_4_x_widths_0_to_9"] = csr(rows)
    # full rows and full columns: the last feature row, the first and last frame, a whole batch row
    rows = [[(D - 1, D, 0, T), (0, D, T - 1, T), (0, D, 0, 1)]] + [[] for _ in range(B - 1)]
    if B > 1:
        rows[B - 1] = [(0, D, 0, T)]
    tabs["full_rows_and_columns"] = csr(rows)
    # overlapping pairs on row 0; every other row has no rectangle
    tabs["overlapping_pairs"] = csr([[(0, D // 2 + 1, 0, T // 2 + 1), (D // 3, D, T // 3, T), (D // 3, D // 2 + 1, 0, T)]]
                                    + [[] for _ in range(B - 1)])
    tabs["no_rectangles"] = csr([[] for _ in range(B)])
    tabs["last_cell"] = csr([[] for _ in range(B - 1)] + [[(D - 1, D, T - 1, T)]])
    # across the kernel's own seams: the 8-row feature tile, the 1024-frame tile, a 16-byte vector
    rows = [[(ROW_TILE - 2, min(ROW_TILE + 3, far_f), 1, min(VEC + 2, far_t)),
             (0, min(2 * ROW_TILE + 1, far_f), min(TIME_TILE - 3, far_t), min(TIME_TILE + 2, far_t)),
             (min(ROW_TILE - 1, far_f), min(ROW_TILE + 1, far_f), 0, far_t)] for _ in range(B)]
    tabs["across_tile_seams"] = csr(rows)
    # a row list longer than one LDS chunk: single cells and short runs
    rng = np.random.RandomState(B * 1000003 + D * 1009 + T)
    rows = [[] for _ in range(B)]
    for _ in range(RECT_CHUNK + 44):
        f, t = int(rng.randint(0, D)), int(rng.randint(0, T))
        rows[0].append((f, f + 1, t, min(t + int(rng.randint(1, 4)), far_t)))
    tabs["more_than_one_chunk"] = csr(rows)
    return tabs


def special_bits(n, seed):
    """n random 32-bit patterns (int32) with NaN, +inf, -inf and -0.0 planted every few cells, so that they fall inside and
    outside any rectangle"""
    rng = np.random.RandomState(seed)
    bits = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00001, 0x7f800000, 0xff800000, 0x80000000, 0xffc12345], dtype=np.uint32)
    idx = np.arange(0, n, 3)
    bits[idx] = special[(idx // 3) % len(special)]
    return bits.view(np.int32)
