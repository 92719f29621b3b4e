"""Every instantiation of the lip front end's kernels - the fused BasicBlocks of csrc/basicblock.hip and csrc/basicblock_phase.hip
(padded-position, phase CH = 64 / 128, TAIL), the stem kernels, the pools and preprocess_frames of csrc/frontend.hip - against the
operation in fp64, on guarded outputs: every admitted map up to the launcher's limits and the refusals just past them, non-square
maps, one to four blocks with distinct weights, image counts around the 256-block grid, blocks that walk three tiles, exact coded
data, every stem input kind and activation at clip lengths around the chunk boundaries, grid-stride loops past the capped grid.  One
child process per environment: the launchers read their switches once per process.  Cases: tests/_frontend_cases.py
(tests/test_frontend_matrix_cpu.py proves the coverage), checks: tools/check_frontend_kernels.py, measured ratios and child run
times: profiles/frontend_matrix.md."""
import functools
import os
import subprocess
import sys

import pytest

from tests import _frontend_cases as fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 100   # seconds: ten times the slowest child measured on MI355X (default-gridtail-bf16, 9.9 s with start-up, profiles/frontend_matrix.md)


@functools.lru_cache(maxsize=None)
def _child(env_name):
    env = {k: v for k, v in os.environ.items() if k not in fc.SWITCHES}
    env.update(fc.ENVS[env_name])
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_frontend_kernels.py"), env_name], env=env,
                          capture_output=True, text=True, timeout=TIMEOUT)


@pytest.mark.parametrize("env_name", list(fc.ENVS))
def test_frontend_matrix(env_name):
    r = _child(env_name)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]


def test_stem_digests_equal_across_chunkings():
    """The frames per block only decide which block computes a frame: every stem case gives the same output bytes under
    L2S_STEM_FT = 25, 1, 3 and under the launcher's own choice (the children above, run once)."""
    digests = []
    for e in fc.STEM_ENVS:
        lines = [ln.split() for dt in fc.DTYPES for ln in _child(f"{e}-{dt}").stdout.splitlines() if ln.startswith("DIGEST ")]
        digests.append({(ln[1], ln[2]): ln[3] for ln in lines})
    want = {(c["dt"], c["name"]) for c in fc.stem_cases("stem")}
    assert set(digests[0]) == want
    for e, d in zip(fc.STEM_ENVS[1:], digests[1:]):
        assert set(d) == want, e
        diff = sorted(k for k in want if d[k] != digests[0][k])
        assert not diff, (e, diff[:10])
