"""Every kernel between the model families - the unit decoders of csrc/decode.hip, the framewise and label-repeat kernels of
csrc/ctc.hip, the casts, repeats, broadcasts, transposes, look-ups, lens_from_mask, split_hi_lo, splitk_reduce and conv_post_tanh of
csrc/misc.hip and rows_f32_kernel of csrc/f32_kernels.hip - against the operation in fp64 (bit for bit where the operation is exact),
on operands that are windows of canary-filled device buffers: every instantiation, the shapes at which a kernel takes another path
(the second trip of every grid-stride loop, of the score loop and of the 64-lane loops, V = 256, beam = V - 4, both tile edges), every
refusal by its code, every launch twice.  One child process per part; the parts split the work by run time only.  Cases:
tests/_glue_cases.py (tests/test_glue_matrix_cpu.py proves the coverage), checks: tools/check_glue_kernels.py, measured ratios and
child run times: profiles/glue_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _glue_cases as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 40    # seconds: ten times the slowest child measured on MI355X (split, 3.8 s with start-up, profiles/glue_matrix.md)


@pytest.mark.parametrize("part", list(gc.PARTS))
def test_glue_matrix(part):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_glue_kernels.py"), part], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
