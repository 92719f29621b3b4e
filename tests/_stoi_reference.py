"""Float64 restatement of STOI (Taal, Hendriks, Heusdens, Jensen: "An algorithm for intelligibility prediction of time-frequency
weighted noisy speech", IEEE TASL 19(7), 2011) and ESTOI (Jensen, Taal: "An algorithm for predicting the intelligibility of speech
masked by modulated noise maskers", IEEE/ACM TASLP 24(11), 2016) - the yardstick of the device path.

Everything is numpy float64; the resampler is scipy.signal.resample_poly with the Octave-compatible Kaiser taps, the spectrum is
np.fft.rfft.  Every stage is a function of its own so that the device's stages can be compared one by one.
"""
import numpy as np
from scipy.signal import resample_poly

FS = 10000
N_FRAME, HOP, NFFT = 256, 128, 512
NUMBAND, MINFREQ = 15, 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(np.float64).eps          # 2^-52


def resample_taps(up=5, down=8):
    fc = 1.0 / max(up, down) / 2.0                         # 1/16
    half = int(np.ceil(52.0 / (28.714 * (fc / 10.0))))     # 290
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2.0 * up * fc * np.sinc(2.0 * fc * t))
    return h / h.sum()


def resample(x):
    return resample_poly(np.asarray(x, dtype=np.float64), 5, 8, window=resample_taps())


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_energies_db(x):
    """e_j of every analysis frame of the (resampled) clean signal; frames start while i < len - 256."""
    w = window()
    starts = range(0, len(x) - N_FRAME, HOP)
    return np.array([20.0 * np.log10(np.linalg.norm(w * x[i:i + N_FRAME]) + EPS) for i in starts])


def kept_frames(x):
    """(indices of the kept frames, margin = min |e_j - threshold| in dB) of the resampled clean signal."""
    e = frame_energies_db(x)
    if e.size == 0:
        return np.zeros(0, dtype=np.int64), np.inf
    thr = e.max() - DYN_RANGE
    return np.nonzero(e > thr)[0], float(np.abs(e - thr).min())


def compact(x, kept):
    """Overlap-add of the kept windowed frames at hop 128."""
    w = window()
    if len(kept) == 0:
        return np.zeros(0)
    out = np.zeros((len(kept) - 1) * HOP + N_FRAME)
    for k, j in enumerate(kept):
        out[k * HOP:k * HOP + N_FRAME] += w * x[j * HOP:j * HOP + N_FRAME]
    return out


def band_edges():
    """int [16]: band i sums bins [edges[i], edges[i + 1])."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    k = np.arange(NUMBAND)
    lo = np.array([np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i - 1) / 6.0))) for i in k])
    hi = np.array([np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i + 1) / 6.0))) for i in k])
    assert (lo[1:] == hi[:-1]).all()
    return np.concatenate([lo, hi[-1:]])


def band_matrix(z):
    """[15, F] third-octave band magnitudes of a compacted signal."""
    w = window()
    starts = range(0, len(z) - N_FRAME, HOP)
    e = band_edges()
    if len(starts) == 0:
        return np.zeros((NUMBAND, 0))
    spec = np.array([np.fft.rfft(w * z[i:i + N_FRAME], NFFT) for i in starts]).T          # [257, F]
    p = np.abs(spec) ** 2
    return np.sqrt(np.array([p[e[i]:e[i + 1]].sum(0) for i in range(NUMBAND)]))


def _row_col_normalize(s):
    s = s - s.mean(-1, keepdims=True)
    s = s / (np.linalg.norm(s, axis=-1, keepdims=True) + EPS)
    s = s - s.mean(-2, keepdims=True)
    return s / (np.linalg.norm(s, axis=-2, keepdims=True) + EPS)


def scores_from_bands(X, Y):
    """(stoi, estoi, n_segments) of two [15, F] band matrices."""
    F = X.shape[1]
    if F < N:
        return 1e-5, 1e-5, 0
    Xs = np.array([X[:, m - N:m] for m in range(N, F + 1)])                                # [M, 15, 30]
    Ys = np.array([Y[:, m - N:m] for m in range(N, F + 1)])
    M = Xs.shape[0]
    c = np.linalg.norm(Xs, axis=2, keepdims=True) / (np.linalg.norm(Ys, axis=2, keepdims=True) + EPS)
    Yp = np.minimum(c * Ys, Xs * (1.0 + 10.0 ** (-BETA / 20.0)))
    xh = Xs - Xs.mean(2, keepdims=True)
    yh = Yp - Yp.mean(2, keepdims=True)
    xh = xh / (np.linalg.norm(xh, axis=2, keepdims=True) + EPS)
    yh = yh / (np.linalg.norm(yh, axis=2, keepdims=True) + EPS)
    d_stoi = float((xh * yh).sum() / (NUMBAND * M))
    d_estoi = float((_row_col_normalize(Xs) * _row_col_normalize(Ys) / N).sum() / M)
    return d_stoi, d_estoi, M


def stages(x, y):
    """Every observable of one clip pair (16 kHz, equal length): dict of xr, yr, kept, margin_db, X, Y, stoi, estoi, n_segments."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    xr, yr = resample(x), resample(y)
    kept, margin = kept_frames(xr)
    X, Y = band_matrix(compact(xr, kept)), band_matrix(compact(yr, kept))
    s, e, m = scores_from_bands(X, Y)
    return {"xr": xr, "yr": yr, "n_frames": len(range(0, len(xr) - N_FRAME, HOP)), "kept": kept, "margin_db": margin, "X": X, "Y": Y,
            "stoi": s, "estoi": e, "n_segments": m}


def stoi(x, y, extended=False):
    r = stages(x, y)
    return r["estoi"] if extended else r["stoi"]


def add_noise(x, snr_db, seed):
    """x + white Gaussian noise at snr_db (seeded; float64)."""
    x = np.asarray(x, dtype=np.float64)
    g = np.random.default_rng(seed).standard_normal(x.shape)
    return x + g * np.sqrt((x ** 2).mean() / (g ** 2).mean() * 10.0 ** (-snr_db / 10.0))
