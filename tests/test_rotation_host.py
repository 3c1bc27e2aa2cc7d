"""No GPU: where run_encoder puts its tensors (csrc/vasr_host.h BufRotation), read through the devtools getter
vasr_plan_buffers -- run_encoder's own dry form on a host-side shadow of an unfinalized handle, pure host arithmetic.  One
child process per VASR_BUF_ROTATE value (the devtools build reads its switches once per process) plans the built-in 15x5 and
12x1_vi at the benchmark's shape and every model of tests/rotation_child.py at batch 6 and 64, through the transcribe path, the
per-module encoder, row-independent mode and two slices.

A plan record is (kind, dst, src, src2, res); kinds: 0 pane copy, 1 depthwise -> D, 2 sub-block GEMM, 3 fused depthwise +
pointwise, 4 residual-branch GEMM, 5 SE, 6 GroupNorm; buffers 0-3 rotate, 4 = D, 5 = panes, 6 = encoder input, 7 = output.
"""
import json
import os
import subprocess
import sys

import pytest

import rotation_child as RC

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("pingpong", "inplace")
COPY, DW, GEMM, FUSED, RES, SE, NORM = range(7)
D, PANE, IN, OUT = 4, 5, 6, 7

# The parent commit's assignment for QuartzNet15x5 at 64 x 10 s, taken from its run_encoder: per block, sub-block outputs
# alternate between the first two of (bufP, bufQ, bufR, bufS) that are not the block input, in that order.  One entry per
# block: (block input, destinations of its sub-blocks' GEMM / fused launches).
PARENT_15X5 = ([(IN, [0])] +
               [(0, [1, 2, 1, 2, 1]), (1, [0, 2, 0, 2, 0])] * 7 + [(0, [1, 2, 1, 2, 1])] +
               [(1, [0]), (0, [OUT])])


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    from viet_asr_amd import _lib
    dev = os.path.join(os.path.dirname(_lib.LIB_PATH), "libvasr_hip_dev.so")
    tmp = tmp_path_factory.mktemp("rotation")
    got = {}
    for mode in MODES + (None,):
        env = {k: v for k, v in os.environ.items() if not k.startswith("VASR_")}
        env["VASR_LIB_PATH"] = dev
        if mode:
            env["VASR_BUF_ROTATE"] = mode
        path = str(tmp / f"{mode}.json")
        p = subprocess.run([sys.executable, os.path.join(HERE, "rotation_child.py"), "plan", path], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "ROTATION_CHILD_OK" in p.stdout, (mode, p.stdout[-2000:], p.stderr[-2000:])
        with open(path) as f:
            got[mode] = json.load(f)
    return got


def _repeats(key):
    name = key.split("/")[0]
    return [int(b["repeat"]) for b in RC.definition(name)["JasperEncoder"]["jasper"]]


def _passes(key, plan):
    """The plan cut into encoder passes (one per slice): a pass ends with the launch that writes the encoder output."""
    out, at = [], 0
    for i, rec in enumerate(plan):
        if rec[0] == GEMM and rec[1] == OUT:
            while i + 1 < len(plan) and plan[i + 1][0] in (SE, NORM):       # its in-place passes
                i += 1
            out.append(plan[at:i + 1])
            at = i + 1
    assert at == len(plan) and len(out) == (2 if key.endswith("/slices") else 1), (key, len(out))
    return out


def _blocks(key, one_pass):
    """One pass cut into blocks: a sub-block ends with its GEMM or fused launch and the SE / GroupNorm passes behind it."""
    out, at = [], 0
    for rep in _repeats(key):
        n, i = 0, at
        while i < len(one_pass) and (n < rep or one_pass[i][0] in (SE, NORM)):
            n += one_pass[i][0] in (GEMM, FUSED)
            i += 1
        assert n == rep, (key, rep, n)
        out.append(one_pass[at:i])
        at = i
    assert at == len(one_pass), (key, at, len(one_pass))
    return out


ALL_KEYS = list(RC.BUILTIN) + [m + v for m in RC.MODELS for v in ("", "/b64", "/module")] + \
    [m + v for m in ("c512", "c256_512") for v in ("/row_independent", "/slices")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ALL_KEYS)
def test_no_launch_stores_over_a_source_or_a_live_tensor(plans, mode, key):
    plan = plans[mode][key]
    assert plan
    for one_pass in _passes(key, plan):
        cur = IN
        for block in _blocks(key, one_pass):
            blk_in, live_r = cur, None
            for kind, dst, src, src2, res in block:
                rec = (key, mode, kind, dst, src, src2, res)
                assert dst != -1 and src != -1, rec
                if kind in (DW, GEMM, FUSED):
                    assert dst not in (src, src2, res), rec
                if kind in (COPY, RES):
                    assert dst not in (src, src2), rec
                assert dst != blk_in and dst != IN, rec                  # the block input is live until the block ends
                assert (dst == PANE) == (kind == COPY), rec              # pane sources: written by their copy alone
                if kind == RES and dst < 4:
                    live_r = dst                                         # R: live from the residual branch to the block's end
                if kind in (DW, GEMM, FUSED):
                    assert dst != live_r, rec
                    assert (dst == D) == (kind == DW), rec
                if kind in (DW, FUSED):
                    assert src == cur, rec                               # both read the current tensor
                if kind in (GEMM, FUSED):
                    assert src in (cur, D) and src2 in (-1, blk_in), rec
                    cur = dst
            assert cur != blk_in


@pytest.mark.parametrize("key", ["c512", "c256_512", "max", "se", "gn", "stride2"])
def test_inplace_stores_over_the_current_tensor_only_behind_a_depthwise_kernel(plans, key):
    """In place = the GEMM's destination is the buffer the depthwise kernel in front of it has just read; a block's first
    sub-block, the fused kernel and GEMMs that read the current tensor never do that."""
    seen_in_place = 0
    for block in _blocks(key, _passes(key, plans["inplace"][key])[0]):
        first = True
        for i, (kind, dst, src, src2, res) in enumerate(block):
            if kind not in (GEMM, FUSED):
                continue
            behind_dw = kind == GEMM and i > 0 and block[i - 1][0] == DW and src == D
            if behind_dw and not first and dst != OUT:
                assert dst == block[i - 1][2], (key, i, block[i - 1], block[i])       # over the depthwise kernel's input
                seen_in_place += 1
            first = False
    assert seen_in_place >= 2, key


def test_inplace_15x5_512_channel_blocks_touch_three_buffers(plans):
    jas = RC.definition("quartznet15x5")["JasperEncoder"]["jasper"]
    blocks = _blocks("quartznet15x5", _passes("quartznet15x5", plans["inplace"]["quartznet15x5"])[0])
    n = 0
    for cfg, block in zip(jas, blocks):
        if cfg["filters"] != 512 or not cfg["residual"]:
            continue
        bufs = {b for rec in block for b in rec[1:] if b != -1}
        assert len(bufs) == 3 and D in bufs, (cfg, sorted(bufs))
        n += 1
    assert n == 9
    # the same blocks in the parent's rotation: block input, two alternating outputs and D
    for cfg, block in zip(jas, _blocks("quartznet15x5", _passes("quartznet15x5", plans["pingpong"]["quartznet15x5"])[0])):
        if cfg["filters"] == 512 and cfg["residual"]:
            assert len({b for rec in block for b in rec[1:] if b != -1}) == 4


def test_inplace_first_sub_block_takes_the_previous_block_input(plans):
    """A block's first output goes to a dead buffer that the previous block's last launch has just read or written."""
    for key in ("quartznet15x5", "quartznet12x1_vi", "c512"):
        blocks = _blocks(key, _passes(key, plans["inplace"][key])[0])
        for prev, block in zip(blocks[1:], blocks[2:]):
            last = prev[-1]
            first = next(rec for rec in block if rec[0] in (GEMM, FUSED))
            if first[1] != OUT:
                assert first[1] in last[1:], (key, last, first)


def test_pingpong_is_the_parent_assignment_on_15x5(plans):
    plan = plans["pingpong"]["quartznet15x5"]
    blocks = _blocks("quartznet15x5", _passes("quartznet15x5", plan)[0])
    assert len(blocks) == len(PARENT_15X5) == 18
    for i, (block, (blk_in, dsts)) in enumerate(zip(blocks, PARENT_15X5)):
        assert [rec[1] for rec in block if rec[0] in (GEMM, FUSED)] == dsts, i
        last = [rec for rec in block if rec[0] in (GEMM, FUSED)][-1]
        if len(dsts) == 5:
            assert last[3] == blk_in, (i, last)                         # the folded residual reads the block input
        assert all(rec[1] == D and rec[0] == DW for rec in block if rec[0] not in (GEMM, FUSED)), i
    # blocks 1-6 (256 channels) take the fused kernel, every other separable block two kernels
    kinds = [sorted({rec[0] for rec in block}) for block in blocks]
    assert kinds == [[DW, GEMM]] + [[FUSED]] * 6 + [[DW, GEMM]] * 10 + [[GEMM]]


@pytest.mark.parametrize("key", ALL_KEYS)
def test_pingpong_is_the_parent_rule_everywhere(plans, key):
    """The parent's rule restated: free = the rotation buffers that are not the block input, in index order; sub-block
    outputs alternate between free[0] and free[1] from free[0] on, an unfused residual result takes free[2]."""
    for one_pass in _passes(key, plans["pingpong"][key]):
        cur = IN
        for block in _blocks(key, one_pass):
            free = [b for b in range(4) if b != cur][:3]
            flip = 0
            for kind, dst, src, src2, res in block:
                if kind in (GEMM, FUSED):
                    assert dst in (free[flip], OUT), (key, block)
                    flip ^= 1
                    cur = dst
                if kind == RES:
                    assert dst in (free[2], D), (key, block)


def test_default_is_documented(plans):
    """The product default (no switch set) is the in-place rotation."""
    assert plans[None] == plans["inplace"]
    assert plans["inplace"]["quartznet15x5"] != plans["pingpong"]["quartznet15x5"]
