"""Every instantiation of the attention, LayerNorm, split-K LayerNorm and GLU / depthwise-conv kernels against the operation in
fp64, on guarded operands: both resident and all eight tiled attention kernels across the resident / tiled boundary, ragged, empty
and clamped lengths, a position table that is a column window; the rows, generic and split-K LayerNorm kernels with every
(x, y) type pair, second output, zero prefix and the rows kernel's two fallbacks; both tiles of the conv kernel at every tile edge.
One child process per environment: the launchers read their switches once per process.  Cases: tests/_seq_cases.py
(tests/test_seq_matrix_cpu.py proves the coverage), checks: tools/check_seq_kernels.py, measured ratios and child run times:
profiles/seq_kernels_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _seq_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 60    # seconds: ten times the slowest child measured on MI355X (default, 6.0 s, profiles/seq_kernels_matrix.md)


@pytest.mark.parametrize("env_name", list(sc.ENVS))
def test_seq_matrix(env_name):
    env = {k: v for k, v in os.environ.items() if k not in sc.SWITCHES}
    env.update(sc.ENVS[env_name])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_seq_kernels.py"), env_name], env=env,
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
