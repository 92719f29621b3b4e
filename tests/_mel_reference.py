"""Test-side yardsticks for the log-mel analysis, independent of the product's tables (lip2speech_unit_amd/audio.py):

  mel_f64   the recipe restated in float64 on torch.stft (reflect pad 320, periodic Hann 640, 321 bins, magnitude), with this
            file's own Slaney filterbank, log(clamp(., 1e-5));
  mel_f32   the same recipe evaluated in float32 on the CPU the way TacotronSTFT itself evaluates it: F.conv1d of the
            reflect-padded signal with the dense windowed Fourier basis (np.fft.fft(np.eye(n)) rows, window multiplied in fp32),
            sqrt(re^2 + im^2), torch.matmul with the fp32 filterbank.  Its distance from mel_f64 is what float32 costs the
            reference's own arithmetic on a given signal, which is the unit the GPU gates are stated in.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

N_FFT, HOP, N_MELS, SR, FMIN, FMAX, FLOOR = 640, 160, 80, 16000, 0.0, 8000.0, 1e-5


def _mel_of_hz(f):
    return f * 3.0 / 200.0 if f < 1000.0 else 15.0 + 27.0 * np.log(f / 1000.0) / np.log(6.4)


def _hz_of_mel(m):
    return m * 200.0 / 3.0 if m < 15.0 else 1000.0 * 6.4 ** ((m - 15.0) / 27.0)


def slaney_filterbank():
    """float64 [80, 321], written as loops over bands and bins on purpose (nothing shared with audio.mel_filterbank)."""
    nbin = N_FFT // 2 + 1
    lo, hi = _mel_of_hz(FMIN), _mel_of_hz(FMAX)
    edge = [_hz_of_mel(lo + (hi - lo) * i / (N_MELS + 1)) for i in range(N_MELS + 2)]
    fb = np.zeros((N_MELS, nbin))
    for j in range(N_MELS):
        left, mid, right = edge[j], edge[j + 1], edge[j + 2]
        for k in range(nbin):
            f = k * SR / N_FFT
            up, down = (f - left) / (mid - left), (right - f) / (right - mid)
            fb[j, k] = max(0.0, min(up, down)) * 2.0 / (right - left)
    return fb


_FB = None


def _fb():
    global _FB
    if _FB is None:
        _FB = slaney_filterbank()
    return _FB


def linear_mel_f64(x):
    """float64 [T, 80] mel energies before the clamp and the log; x: 1-d samples in (-1, 1) (any float / int16 -> / 32768)."""
    x = as_float64(x)
    spec = torch.stft(torch.from_numpy(x), N_FFT, hop_length=HOP, win_length=N_FFT,
                      window=torch.hann_window(N_FFT, periodic=True, dtype=torch.float64), center=True, pad_mode="reflect",
                      return_complex=True)
    return (torch.from_numpy(_fb()) @ spec.abs()).t().numpy()


def mel_f64(x):
    return np.log(np.maximum(linear_mel_f64(x), FLOOR))


def mel_f32(x):
    """float32 [T, 80]: TacotronSTFT's own float32 arithmetic on the CPU (see the module docstring)."""
    x = torch.from_numpy(as_float64(x).astype(np.float32))
    cutoff = N_FFT // 2 + 1
    fourier = np.fft.fft(np.eye(N_FFT))
    basis = torch.FloatTensor(np.vstack([np.real(fourier[:cutoff]), np.imag(fourier[:cutoff])])[:, None, :])
    basis = basis * torch.hann_window(N_FFT, periodic=True, dtype=torch.float32)
    padded = F.pad(x[None, None], (N_FFT // 2, N_FFT // 2), mode="reflect")
    y = F.conv1d(padded, basis, stride=HOP)[0]
    mag = torch.sqrt(y[:cutoff] ** 2 + y[cutoff:] ** 2)
    mel = torch.matmul(torch.from_numpy(_fb().astype(np.float32)), mag)
    return torch.log(torch.clamp(mel, min=FLOOR)).t().numpy()


def as_float64(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32768.0
    return x.astype(np.float64)


def load_fixture(golden_dir):
    """[(clip, pcm int16 [n], mel float32 [T, 80], spk float32 [256])] for the five clips of lrs3_sample/test.tsv."""
    a = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    m = np.load(os.path.join(golden_dir, "mel_lrs3.npz"))
    assert list(a["clips"]) == list(m["clips"])
    return [(str(c), a[f"c{i}_pcm"], m[f"c{i}_mel"], m[f"c{i}_spk"]) for i, c in enumerate(m["clips"])]


def synthetic_clip(seed=20240, n=30000):
    """int16 PCM: three tones plus noise, with a stretch of digital silence long enough for whole frames to sit on the clamp floor."""
    rng = np.random.RandomState(seed)
    t = np.arange(n) / SR
    x = 0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 1333.0 * t + 0.5) + 0.05 * np.sin(2 * np.pi * 6100.0 * t)
    x += 0.02 * rng.randn(n)
    x[12000:16000] = 0.0
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def materialise_audio_dataset(root, golden_dir, with_mel):
    """The five fixture clips as a data set in the reference's layout (label/, audio/ with the REAL wavs, spk_emb/, and mel/
    only on request).  Returns (label_dir, fixture)."""
    import shutil
    import wave
    fx = load_fixture(golden_dir)
    src = os.path.join(golden_dir, "lrs3_sample")
    lab = os.path.join(root, "label")
    os.makedirs(lab, exist_ok=True)
    rows = open(os.path.join(src, "test.tsv")).read().splitlines()[1:]
    with open(os.path.join(lab, "test.tsv"), "w") as f:
        f.write(root + "\n" + "\n".join(rows) + "\n")
    for fn in ("test.unt", "dict.unt.txt"):
        shutil.copyfile(os.path.join(src, fn), os.path.join(lab, fn))
    for clip, pcm, mel, spk in fx:
        for kind in ("audio", "spk_emb") + (("mel",) if with_mel else ()):
            os.makedirs(os.path.join(root, kind, os.path.dirname(clip)), exist_ok=True)
        with wave.open(os.path.join(root, "audio", clip + ".wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(SR)
            w.writeframes(pcm.astype("<i2").tobytes())
        np.save(os.path.join(root, "spk_emb", clip + ".npy"), spk)
        if with_mel:
            np.save(os.path.join(root, "mel", clip + ".npy"), mel)
    return lab, fx
