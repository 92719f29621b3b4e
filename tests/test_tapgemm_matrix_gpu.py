"""Every (tile, type, mode, tap path, epilogue family) instantiation of csrc/tapgemm_kernel.h against the oracle op in fp64, on
guarded operands; a block walking three output tiles on every tile; a short last band.  One child process per (tile, part):
the library reads L2S_FORCE_TILE / L2S_BAND once per process.  The same checks on the phase-staggered kernel (csrc/phasegemm_kernel.h)
and the LDS-patch kernel (csrc/patchconv.hip): every instantiation, blocks walking three and four output tiles under a slot cap,
and two tiles on the kernels' real grids.  Cases: tests/_tapgemm_cases.py (tests/test_tapgemm_matrix_cpu.py
proves the coverage), checks: tools/check_tapgemm_matrix.py, measured ratios and child run times: profiles/tapgemm_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _tapgemm_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 135   # seconds: ten times the slowest child measured on MI355X (phase-walk, 13.5 s, profiles/tapgemm_matrix.md)


def _run(tile, part, **extra):
    env = dict(os.environ, L2S_FORCE_TILE=str(tile), L2S_PHASEGEMM="0", L2S_NO_PATCHCONV="1", **extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_tapgemm_matrix.py"), part], env=env,
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]


@pytest.mark.parametrize("part", ["families", "schedule"])
@pytest.mark.parametrize("tile", sorted(tc.TILES))
def test_matrix(tile, part):
    _run(tile, part)


def test_short_last_band():
    _run(tc.BAND_TILE, "band", L2S_BAND=str(tc.BAND))


@pytest.mark.parametrize("part,kernel", [(part, k) for part in tc.PART_ENV for k in tc.PART_KERNELS[part]])
def test_special_kernels(part, kernel):
    env = {k: v for k, v in os.environ.items() if k not in tc.SWITCHES}
    env.update(tc.PART_ENV[part])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_tapgemm_matrix.py"), part, str(kernel)], env=env,
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
