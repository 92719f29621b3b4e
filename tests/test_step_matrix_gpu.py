"""The kernels that decide tokens - l2s_kv_attention, l2s_vocab_argmax and l2s_whisper_advance (csrc/whisper_decode.hip), l2s_beam_attention,
l2s_beam_select and l2s_beam_advance (csrc/s2s_decode.hip), l2s_ctc_beam_search (csrc/ctc.hip) - against the operation in fp64 (bit for bit where the operation is exact), on
operands that are windows of canary-filled device buffers: padded leading dimensions, cache rows that must not be read filled with NaN,
valid lengths and positions at every load / iteration edge, positions at and past the cache, ancestor entries and live counts outside the
beam, every B / d / V switch of the argmax, planted maxima and bit-exact ties in every wave, lane group and tile, every mask, scripted
candidate lists, the no-room rule, 70 clips in one launch, every refusal by its code, every launch twice, every clip alone, and the three
beam kernels chained on device state for 12 steps.  One child process per part; the parts split the work by run time only.  Cases:
tests/_step_cases.py (tests/test_step_matrix_cpu.py proves the coverage and the decisiveness of every case), reference:
tests/_step_reference.py, checks: tools/check_step_kernels.py, measured ratios and child run times: profiles/step_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _step_cases as sc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 51    # seconds: ten times the slowest child measured on MI355X (wadv, 5.1 s under pytest, profiles/step_matrix.md)


@pytest.mark.parametrize("part", list(sc.PARTS))
def test_step_matrix(part):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_step_kernels.py"), part], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
