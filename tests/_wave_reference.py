"""Float64 reference of the waveform analysis kernels' matrix (tests/_wave_cases.py, tools/check_wave_kernels.py), in one generic form:

  framed_spectrum   a clip of analysis length n, reflected ONCE at either end by `pad`, zeros from n_valid on; frames of K every hop,
                    times the window, np.fft.rfft, then the power re^2 + im^2 or the magnitude sqrt(re^2 + im^2 + mag_eps)
  mel_bands         a dense filterbank applied to it; log_floor / whisper_post: what each entry documents behind the bands
  wave_stem         Conv1d(1 -> C, k 10, stride 5), per-clip biased GroupNorm, erf GELU
  gain              the increase-only volume factor
  stoi_*            the four STOI stages; resample, kept frames and the scores are tests/_stoi_reference.py's where that has the
                    arguments (the bands take a kept list with indices the clip does not have, and a frame count cap)

Window and filterbank are arguments - never the packed device tables.  Every function takes `dtype`: np.float64 is the yardstick,
np.float32 evaluates the same steps in float32 on the CPU (torch's float32 FFT); its distance from float64 is the unit e32 of the
matrix's bound.  `dense=True` is the second float32 evaluation order the bound's factor F is derived from: the spectrum as a matrix
product with the dense windowed Fourier basis - the k-ordered chain the kernels run - instead of the FFT.
tests/test_wave_matrix_cpu.py pins all of this to the restatements the project already trusts."""
import math

import numpy as np
import torch
from scipy.special import erf

from tests import _stoi_reference as st

F64, F32 = np.float64, np.float32


# ---- frame rules -----------------------------------------------------------------------------------------------------------------------------
def reflect_frames(n, pad, K, hop):
    """frames of a clip of n samples with `pad` reflected on each side: none unless the reflection is valid and a whole frame fits"""
    return (n + 2 * pad - K) // hop + 1 if (n > pad and n + 2 * pad >= K) else 0


def stem_frames(n):
    return (n - 10) // 5 + 1 if n >= 10 else 0


def len10k(n):
    return (5 * n + 7) // 8


def stoi_frames_of(length):
    return (length - 256 - 1) // 128 + 1 if length > 256 else 0


# ---- the framed analysis ------------------------------------------------------------------------------------------------------------------------
def padded_clip(x, n, n_valid, pad):
    """float64 [n + 2 pad]: positions -pad .. n + pad - 1 of the clip, reflected once against n; zeros from n_valid on"""
    x = np.asarray(x, F64)
    p = np.arange(-pad, n + pad)
    p = np.where(p < 0, -p, p)
    p = np.where(p >= n, 2 * (n - 1) - p, p)
    ok = (p >= 0) & (p < min(n_valid, len(x)))
    out = np.zeros(len(p))
    out[ok] = x[p[ok]]
    return out


_DENSE = {}


def dense_basis(K):
    """(cos, -sin) float64 [K, K/2 + 1], the phase reduced mod K before the division"""
    if K not in _DENSE:
        ang = 2.0 * np.pi * ((np.arange(K)[:, None] * np.arange(K // 2 + 1)[None, :]) % K) / K
        _DENSE[K] = (np.cos(ang), -np.sin(ang))
    return _DENSE[K]


def framed_spectrum(x, n, n_valid, pad, K, hop, window, power, mag_eps=0.0, dtype=F64, dense=False, T=None):
    """[T, K/2 + 1] of `dtype`.  T: the frame count (default: reflect_frames; Whisper keeps 3000 of its 3001)."""
    T = reflect_frames(n, pad, K, hop) if T is None else T
    if T == 0:
        return np.zeros((0, K // 2 + 1), dtype)
    xp = padded_clip(x, n, n_valid, pad).astype(dtype)
    frames = xp[hop * np.arange(T)[:, None] + np.arange(K)[None, :]] * np.asarray(window, F64).astype(dtype)
    if dense:
        c, s = (t.astype(dtype) for t in dense_basis(K))
        re, im = frames @ c, frames @ s
    elif dtype == F64:
        spec = np.fft.rfft(frames, axis=1)
        re, im = spec.real, spec.imag
    else:
        spec = torch.view_as_real(torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames)), dim=1)).numpy()
        re, im = spec[..., 0], spec[..., 1]
    p = re * re + im * im
    assert p.dtype == dtype
    return p if power else np.sqrt(p + dtype(mag_eps))


def mel_bands(spec, fb, dtype=F64):
    return spec @ np.asarray(fb, F64).astype(dtype).T


def log_floor(m, floor, dtype=F64):
    return np.log(np.maximum(m, dtype(floor)))


def whisper_post(m, dtype=F64):
    """log10(max(., 1e-10)), the clamp 8 below the CLIP's maximum, (x + 4) / 4"""
    x = np.log10(np.maximum(m, dtype(1e-10)))
    x = np.maximum(x, x.max() - dtype(8.0))
    return (x + dtype(4.0)) / dtype(4.0)


def stft_mel(x, n, pad, K, hop, window, fb, mag_eps, floor, dtype=F64, dense=False):
    """l2s_stft_mel on one clip: [T_b, n_mels]"""
    return log_floor(mel_bands(framed_spectrum(x, n, n, pad, K, hop, window, False, mag_eps, dtype, dense), fb, dtype), floor, dtype)


def stft_mel_power(x, n, n_valid, pad, window, fb, dtype=F64, dense=False):
    """l2s_stft_mel_power on one clip (already scaled): [T_b, 40]"""
    return mel_bands(framed_spectrum(x, n, n_valid, pad, 400, 160, window, True, 0.0, dtype, dense), fb, dtype)


def whisper_logmel(x, n_valid, window, fb, dtype=F64, dense=False):
    """l2s_whisper_logmel on one clip: [3000, 80]"""
    return whisper_post(mel_bands(framed_spectrum(x, 480000, n_valid, 200, 400, 160, window, True, 0.0, dtype, dense, T=3000), fb, dtype), dtype)


def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


# ---- wave stem and gain ---------------------------------------------------------------------------------------------------------------------------
def wave_stem(x, w, gamma, beta, eps, dtype=F64):
    """x [n] -> [L0, C]: taps w [C, 10], statistics over the clip's own frames, biased variance"""
    L0 = stem_frames(len(x))
    w, gamma, beta = (np.asarray(t, F64).astype(dtype) for t in (w, gamma, beta))
    if L0 == 0:
        return np.zeros((0, w.shape[0]), dtype)
    frames = np.asarray(x, F64).astype(dtype)[5 * np.arange(L0)[:, None] + np.arange(10)[None, :]]
    y = frames @ w.T
    mean = y.mean(0, dtype=dtype)
    d = y - mean
    var = (d * d).mean(0, dtype=dtype)
    v = d / np.sqrt(var + dtype(eps)) * gamma + beta
    out = dtype(0.5) * v * (dtype(1.0) + erf(v * dtype(math.sqrt(0.5))))
    assert out.dtype == dtype
    return out


def gelu(v):
    v = np.asarray(v, F64)
    return 0.5 * v * (1.0 + erf(v * math.sqrt(0.5)))


def gain(x, target_dbfs, dtype=F64):
    """10^(change / 20) if change = target - 10 log10(mean(x^2)) > 0, else 1; 1 for a clip without samples or of zeros only"""
    x = np.asarray(x, F64).astype(dtype)
    if x.size == 0:
        return 1.0
    ms = (x * x).sum(dtype=dtype) / dtype(x.size)
    if ms == 0:
        return 1.0
    change = dtype(target_dbfs) - dtype(10.0) * np.log10(ms)
    return float(dtype(10.0) ** (change / dtype(20.0))) if change > 0 else 1.0


def level_db(x):
    x = np.asarray(x, F64)
    return 10.0 * math.log10(float((x * x).mean()))


# ---- STOI ---------------------------------------------------------------------------------------------------------------------------------------------
def stoi_resample(x, dtype=F64):
    """[ceil(5 n / 8)]: float64 is st.resample; float32 the polyphase chain out[m] = sum_q taps[p][q] x[(8 m + 290 - p) / 5 - q] in float32"""
    x = np.asarray(x, F64)
    if dtype == F64:
        return st.resample(x) if len(x) else np.zeros(0)
    n, R = len(x), len10k(len(x))
    w = st.resample_taps()
    taps = np.zeros((5, 117))
    for p in range(5):
        taps[p, : len(w[p::5])] = 5.0 * w[p::5]
    taps, xf = taps.astype(F32), x.astype(F32)
    m = np.arange(R)
    p = (3 * m) % 5
    base = (8 * m + 290 - p) // 5
    acc = np.zeros(R, F32)
    for q in range(117):
        i = base - q
        ok = (i >= 0) & (i < n)
        acc = acc + taps[p, q] * np.where(ok, xf[np.clip(i, 0, max(n - 1, 0))] if n else F32(0), F32(0))
    return acc


def stoi_kept(x10k):
    """(kept indices, margin in dB) of a resampled clean clip: st.kept_frames"""
    return st.kept_frames(np.asarray(x10k, F64))


def stoi_kept_exact(x10k, window):
    """The header's rule  norm_j + 2^-52 > (max_j norm_j + 2^-52) / 100  in exact rational arithmetic, for signals whose frames hold at
    most one non-zero sample each (the norm is then |window x| exactly): the yardstick of a tie, which no floating-point log can decide."""
    from fractions import Fraction
    x, w = np.asarray(x10k, F64), np.asarray(window, F64)
    norms = []
    for i in range(0, len(x) - st.N_FRAME, st.HOP):
        v = [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, x[i:i + st.N_FRAME]) if a != 0 and b != 0]
        assert len(v) <= 1
        norms.append(abs(v[0]) if v else Fraction(0))
    eps = Fraction(1, 2 ** 52)
    thr = (max(norms) + eps) / 100 if norms else None
    return np.array([j for j, nj in enumerate(norms) if nj + eps > thr], dtype=np.int64), [nj + eps - thr for nj in norms]


def stoi_bands(x10k, kept, n_frames, dtype=F64):
    """[15, max(K - 1, 0)]: the kept windowed frames overlap-added at hop 128 (a kept index outside [0, n_frames) contributes a frame
    of zeros in its place), then windowed 512-point spectra of the compacted signal's frames, third-octave band magnitudes"""
    K = len(kept)
    if K < 2:
        return np.zeros((st.NUMBAND, 0), dtype)
    w = st.window().astype(dtype)
    x = np.asarray(x10k, F64).astype(dtype)
    z = np.zeros((K - 1) * st.HOP + st.N_FRAME, dtype)
    for k, j in enumerate(kept):
        if 0 <= j < n_frames:
            z[k * st.HOP:k * st.HOP + st.N_FRAME] += w * x[j * st.HOP:j * st.HOP + st.N_FRAME]
    frames = z[st.HOP * np.arange(K - 1)[:, None] + np.arange(st.N_FRAME)[None, :]] * w
    if dtype == F64:
        spec = np.fft.rfft(frames, st.NFFT, axis=1)
        re, im = spec.real, spec.imag
    else:
        spec = torch.view_as_real(torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames)), st.NFFT, dim=1)).numpy()
        re, im = spec[..., 0], spec[..., 1]
    p = (re * re + im * im).T
    e = st.band_edges()
    out = np.sqrt(np.stack([p[e[i]:e[i + 1]].sum(0, dtype=dtype) for i in range(st.NUMBAND)]))
    assert out.dtype == dtype
    return out


def _row_col_normalize(s, eps):
    s = s - s.mean(-1, keepdims=True)
    s = s / (np.linalg.norm(s, axis=-1, keepdims=True) + eps)
    s = s - s.mean(-2, keepdims=True)
    return s / (np.linalg.norm(s, axis=-2, keepdims=True) + eps)


def stoi_scores(X, Y, dtype=F64):
    """(stoi, estoi, n_segments) of two [15, F] band matrices; float64 is st.scores_from_bands, float32 the same steps in float32"""
    if dtype == F64:
        return st.scores_from_bands(np.asarray(X, F64), np.asarray(Y, F64))
    X, Y = np.asarray(X, F64).astype(dtype), np.asarray(Y, F64).astype(dtype)
    F, N = X.shape[1], st.N
    if F < N:
        return 1e-5, 1e-5, 0
    eps = dtype(st.EPS)
    Xs = np.array([X[:, m - N:m] for m in range(N, F + 1)])
    Ys = np.array([Y[:, m - N:m] for m in range(N, F + 1)])
    M = Xs.shape[0]
    c = np.linalg.norm(Xs, axis=2, keepdims=True) / (np.linalg.norm(Ys, axis=2, keepdims=True) + eps)
    Yp = np.minimum(c * Ys, Xs * dtype(1.0 + 10.0 ** (-st.BETA / 20.0)))
    xh = Xs - Xs.mean(2, keepdims=True)
    yh = Yp - Yp.mean(2, keepdims=True)
    xh = xh / (np.linalg.norm(xh, axis=2, keepdims=True) + eps)
    yh = yh / (np.linalg.norm(yh, axis=2, keepdims=True) + eps)
    assert xh.dtype == dtype and yh.dtype == dtype
    d_stoi = float((xh * yh).astype(F64).sum() / (st.NUMBAND * M))
    d_estoi = float((_row_col_normalize(Xs, eps) * _row_col_normalize(Ys, eps)).astype(F64).sum() / N / M)
    return d_stoi, d_estoi, M
