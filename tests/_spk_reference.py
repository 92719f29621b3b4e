"""The speaker-embedding recipe restated for the tests, independent of lip2speech_unit_amd:
RTVC's preprocess_wav (without the webrtcvad trimming) and embed_utterance, i.e. what helpers.py:185-198 returns.

  partial_slices  the partial windows of a clip of n samples and the padded length
  gain            the increase-only volume normalisation to -30 dBFS
  mel_power       librosa 0.8's melspectrogram(sr 16000, n_fft 400, hop 160, n_mels 40): centred reflect padding, periodic Hann,
                  power spectrum, Slaney filterbank with Slaney norm, no log; time-major [T, 40]
  lstm            3-layer LSTM(256), torch gate order i, f, g, o, from zero state
  head            relu(W h + b) / (norm + 1e-5) per window, mean over windows, / norm
  embed           the whole path for one clip

Everything takes `dtype`: float64 is the yardstick; float32 evaluates the same recipe in float32 on the CPU (dense DFT and
filterbank as torch matmuls, the LSTM cell as written below) - its distance from float64 is what float32 costs the recipe, and
the device path is gated at a small multiple of it.

Two points the published code leaves open, decided the same way here and on the device:
  * a clip without energy (mean square 0) has no level: its gain is 1 (the published code would take log10(0));
  * a clip whose every window has an all-zero ReLU output has the mean embedding 0: the final division by its norm would be
    0 / 0 = NaN in the published code; here the result is the zero vector.
"""
import math

import numpy as np
import torch

SR, N_FFT, HOP, N_MELS, PARTIAL, HIDDEN = 16000, 400, 160, 40, 160, 256


def partial_slices(n, rate=1.3, min_coverage=0.75):
    """(starts, n_padded): mel-frame starts of the 160-frame windows and the zero-extended length."""
    samples_per_frame = SR * 10 // 1000
    n_frames = int(np.ceil((n + 1) / samples_per_frame))
    frame_step = max(int(np.round(SR / rate / samples_per_frame)), 1)
    steps = max(1, n_frames - PARTIAL + frame_step + 1)
    starts = [i for i in range(0, steps, frame_step)]
    last_wave_start = starts[-1] * samples_per_frame
    coverage = (n - last_wave_start) / (PARTIAL * samples_per_frame)
    if coverage < min_coverage and len(starts) > 1:
        starts = starts[:-1]
    return starts, max(n, (starts[-1] + PARTIAL) * samples_per_frame)


def gain(wav):
    """The factor normalize_volume(wav, -30, increase_only=True) multiplies by (float64)."""
    wav = np.asarray(wav, dtype=np.float64)
    ms = float(np.mean(wav ** 2)) if wav.size else 0.0
    if ms == 0.0:
        return 1.0
    change = -30.0 - 10.0 * math.log10(ms)
    return 10.0 ** (change / 20.0) if change > 0 else 1.0


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) / 27.0 * (m - 15.0)), m * 200.0 / 3.0)


def filterbank(n_mels=N_MELS, n_fft=N_FFT, sr=SR):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin=0, fmax=sr/2, htk=False, norm='slaney'): float64 [n_mels, n_fft/2 + 1]."""
    fft_f = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        w[i] = np.maximum(0.0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def _dft():
    n = np.arange(N_FFT)
    k = np.arange(N_FFT // 2 + 1)
    ang = 2.0 * np.pi * ((n[:, None] * k[None, :]) % N_FFT) / N_FFT
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
    return np.cos(ang) * w[:, None], -np.sin(ang) * w[:, None]


def mel_power(wav, dtype=torch.float64):
    """wav: float array of n > 200 samples (already scaled and zero-extended).  Returns numpy [1 + n // 160, 40] of `dtype`."""
    wav = np.asarray(wav, dtype=np.float64)
    n = wav.shape[0]
    assert n > N_FFT // 2
    x = torch.from_numpy(np.pad(wav, N_FFT // 2, mode="reflect")).to(dtype)
    frames = x.unfold(0, N_FFT, HOP)                                  # [T, 400]
    c, s = (torch.from_numpy(t).to(dtype) for t in _dft())
    re, im = frames @ c, frames @ s
    power = re * re + im * im
    return (power @ torch.from_numpy(filterbank()).to(dtype).t()).numpy()


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh):
    """x [S, T, in] -> h [S, T, H], from zero state; parameters in torch's layout and gate order, dtype of x."""
    S, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(S, H)
    c = x.new_zeros(S, H)
    out = []
    for t in range(T):
        g = x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out, dim=1)


def lstm(x, sd, layers=3):
    for l in range(layers):
        x = lstm_layer(x, *(sd[f"lstm.{n}_l{l}"].to(x.dtype) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
    return x


def head(h, w, b):
    """h [P, 256] final hidden states of one clip's windows -> [256]."""
    e = torch.relu(h @ w.to(h.dtype).t() + b.to(h.dtype))
    e = e / (torch.linalg.norm(e, dim=1, keepdim=True) + 1e-5)
    v = e.mean(dim=0)
    nrm = torch.linalg.norm(v)
    return v / nrm if float(nrm) > 0.0 else torch.zeros_like(v)


def embed(wav, sd, dtype=torch.float64):
    """wav: float array in (-1, 1) at 16 kHz (int16 PCM: value / 32768).  Returns numpy [256] of `dtype`."""
    wav = np.asarray(wav, dtype=np.float64)
    n = wav.shape[0]
    g = gain(wav)
    if dtype == torch.float32:                                        # float32 flavour: the factor and the product rounded once each
        wav = (wav.astype(np.float32) * np.float32(g)).astype(np.float64)
    else:
        wav = wav * g
    starts, n_pad = partial_slices(n)
    wav = np.concatenate([wav, np.zeros(n_pad - n)])
    mel = torch.from_numpy(mel_power(wav, dtype))
    x = torch.stack([mel[s:s + PARTIAL] for s in starts])
    h = lstm(x, sd)[:, -1]
    return head(h, sd["linear.weight"], sd["linear.bias"]).numpy()
