"""No GPU: how many wavefronts a workgroup of the fused depthwise + pointwise kernel gets (csrc/encoder_fused.hip
fused_waves_choice, through the devtools getter vasr_fused_waves_choice: pure host arithmetic).  The documented default
 with no switch set, VASR_FUSED_WAVES where it is set, and the 64-frame tile's one form whatever is set.
One child process per setting: the devtools build reads its switches once per process."""
import os
import subprocess
import sys

import pytest

# (depthwise kernel, folded residual) -> wavefronts per workgroup of the 128-frame tile, as DESIGN section 4 states them
DEFAULT_WAVES = {(33, 0): 16, (33, 1): 16, (39, 0): 16, (39, 1): 16}

CODE = """
import viet_asr_amd
from viet_asr_amd import _lib
L = _lib.dev_lib()
print(*[L.vasr_fused_waves_choice(k, d, t) for t in (128, 64) for k in (33, 39) for d in (0, 1)])
"""


def _choices(setting):
    env = {k: v for k, v in os.environ.items() if k != "VASR_FUSED_WAVES" and k != "VASR_LIB_PATH"}
    if setting:
        env["VASR_FUSED_WAVES"] = setting
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", CODE], env=env, cwd=root, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (setting, p.stdout[-1000:], p.stderr[-1000:])
    v = [int(t) for t in p.stdout.split()]
    keys = [(t, k, d) for t in (128, 64) for k in (33, 39) for d in (0, 1)]
    return dict(zip(keys, v))


def test_default_is_the_documented_form():
    got = _choices(None)
    for (k, d), w in DEFAULT_WAVES.items():
        assert got[(128, k, d)] == w, (k, d, got)
        assert got[(64, k, d)] == 8


@pytest.mark.parametrize("setting", ["8", "16"])
def test_switch_pins_the_128_frame_tile_only(setting):
    got = _choices(setting)
    for (t, k, d), w in got.items():
        assert w == (int(setting) if t == 128 else 8), (setting, t, k, d, w)
