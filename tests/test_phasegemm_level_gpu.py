"""The tile boundary of the phase-staggered kernel (csrc/phasegemm_kernel.h): both wave rows are levelled by one extra barrier
before a tile's epilogue and staggered again by one behind it.  Blocks that walk four, three, two and one output tiles at one,
two and three K-tiles per tile, and K-block-table launches whose tiles differ in K: every first launch against fp64 with the
criteria of tools/check_tapgemm_matrix.py, seven further launches bit-identical to it.  One child process per configuration
(the library reads L2S_PHASE_SLOTS once per process): tools/check_phasegemm_level.py."""
import os
import subprocess
import sys

import pytest

from tests import _tapgemm_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 135   # seconds, as tests/test_tapgemm_matrix_gpu.py: a barrier-count mismatch is a hang, not a wrong result
PART_ENV = {"walk": dict(L2S_PHASEGEMM="2", L2S_PHASE_SLOTS="2"), "uneven": dict(L2S_PHASEGEMM="2", L2S_PHASE_SLOTS="1"),
            "ktab": dict(L2S_PHASE_SLOTS="1")}


def _run(part, *args):
    env = {k: v for k, v in os.environ.items() if k not in tc.SWITCHES}
    env.update(PART_ENV[part])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_phasegemm_level.py"), part, *args], env=env,
                       capture_output=True, text=True, timeout=TIMEOUT)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]


@pytest.mark.parametrize("K", [64, 192])
def test_walk_across_tile_boundaries(K):
    """7 x 7 tiles, M, N = 1576, 1784, two slots per XCD: blocks walk four and three tiles; none, gelu+mask, stream32,
    res16post+dual+mask and x32+accum+dual+mask in fp16 and bf16."""
    _run("walk", str(K))


def test_uneven_blocks():
    """3 x 3 tiles, M, N = 744, 760, one slot per XCD, chunk 2: four blocks walk two tiles, one block one tile, three none;
    K = 64 and 128, none and stream32."""
    _run("uneven")


def test_ktab_walk():
    """ktab_conv3x3(3, 3, 64, 1), 256 output channels, 520 images: 27 tiles of 4, 6 or 9 K-blocks, four per block; with and
    without the 16-bit residual, against conv2d in fp64."""
    _run("ktab")
