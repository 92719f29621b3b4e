"""Every kernel that turns a waveform into features or scores - l2s_stft_mel at (640, 160) and (1024, 256) with l2s_mel_spectrogram
(csrc/melspec.hip), l2s_stft_mel_power and l2s_wav_gain (csrc/spkemb.hip), l2s_whisper_logmel (csrc/whisper_logmel.hip), l2s_wave_stem
(csrc/wavestem.hip) and the four stages of csrc/stoi.hip - against the operation in fp64 (bit for bit where the operation is exact), on
operands that are windows of canary-filled device buffers: padded leading dimensions, every pad, T_rows below a clip's frame count,
n_samples NULL / past S / zero / negative, the short-clip edges of every frame rule, every tile edge, 70 clips in one launch, every
refusal by its code, every launch twice, every clip alone, int16 against fp32 input.  One child process per part; the parts split the
work by run time only.  Cases: tests/_wave_cases.py (tests/test_wave_matrix_cpu.py proves the coverage), reference:
tests/_wave_reference.py, checks: tools/check_wave_kernels.py, measured ratios and child run times: profiles/wave_matrix.md."""
import os
import subprocess
import sys

import pytest

from tests import _wave_cases as wc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 47    # seconds: ten times the slowest child measured on MI355X (whisper, 4.7 s with start-up, profiles/wave_matrix.md)


@pytest.mark.parametrize("part", list(wc.PARTS))
def test_wave_matrix(part):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_wave_kernels.py"), part], capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
