"""Every instantiation of the vocoder's fused convolution kernels - the conv pairs of csrc/respair.hip and csrc/respair_phase.hip,
respair_final, the ResBlock and stage kernels of csrc/resblock.hip, conv_post - against the operation in fp64, on guarded outputs:
every admitted geometry up to the launchers' limits, tile edges, ragged, empty and clamped lengths, lens = NULL, len_mul = 4, all
four kinds of pair launch, blocks that walk three tiles in both tile orders, exact tap-coded data, saturated samples.  One child
process per environment: the launchers read their switches once per process.  Cases: tests/_vocconv_cases.py
(tests/test_vocconv_matrix_cpu.py proves the coverage), checks: tools/check_vocoder_convs.py, measured ratios and child run times:
profiles/vocoder_conv_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _vocconv_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 60    # seconds: ten times the slowest child measured on MI355X (default, 5.1 s + start-up, profiles/vocoder_conv_matrix.md)


@pytest.mark.parametrize("env_name", list(vc.ENVS))
def test_vocconv_matrix(env_name):
    env = {k: v for k, v in os.environ.items() if k not in vc.SWITCHES}
    env.update(vc.ENVS[env_name])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_vocoder_convs.py"), env_name], env=env,
                       capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
