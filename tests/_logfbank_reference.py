"""numpy restatement of the audio features of AV-HuBERT (avhubert/hubert_dataset.py:299-315,370-372): the published algorithm of
python_speech_features.logfbank(wav, samplerate=16000) at that library's defaults, then the stacker, the alignment to the video's
frame count and F.layer_norm.  `dtype` is a parameter: float64 is the reference, float32 the same arithmetic class as the kernel
(dense DFT matrix products, not an FFT), whose error against float64 is the yardstick of tests/test_logfbank_gpu.py.

The library is not a dependency; nothing here is taken from a run of it."""
import numpy as np

SR, N_FRAME, HOP, N_DFT, NFILT, PREEMPH = 16000, 400, 160, 512, 26, 0.97
EDGES = [0, 2, 4, 7, 10, 13, 16, 20, 24, 29, 34, 40, 46, 53, 60, 68, 77, 87, 97, 109, 122, 136, 152, 169, 188, 209, 231, 256]
EPS = 2.220446049250313e-16     # numpy.finfo(float).eps


def hz2mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel2hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def edges():
    return np.floor((N_DFT + 1) * mel2hz(np.linspace(0.0, hz2mel(SR / 2.0), NFILT + 2)) / SR).astype(np.int64)


def filterbank():
    """float64 [26, 257]."""
    b = edges()
    fb = np.zeros((NFILT, N_DFT // 2 + 1))
    for j in range(NFILT):
        for i in range(int(b[j]), int(b[j + 1])):
            fb[j, i] = (i - b[j]) / (b[j + 1] - b[j])
        for i in range(int(b[j + 1]), int(b[j + 2])):
            fb[j, i] = (b[j + 2] - i) / (b[j + 2] - b[j + 1])
    return fb


def n_frames(n):
    return 1 if n <= N_FRAME else 1 + int(np.ceil((n - N_FRAME) / HOP))


def frames(x, dtype=np.float64):
    """Pre-emphasis over the whole clip, then frames of 400 every 160 with zeros past the end: [n_frames, 400]."""
    x = np.asarray(x).astype(dtype)
    y = np.append(x[:1], x[1:] - dtype(PREEMPH) * x[:-1])
    nf = n_frames(len(y))
    y = np.concatenate([y, np.zeros((nf - 1) * HOP + N_FRAME - len(y), dtype=dtype)])
    idx = np.arange(N_FRAME)[None, :] + HOP * np.arange(nf)[:, None]
    return y[idx]


def dft_tables():
    """float64 cos and -sin [400, 257]: the dense 512-point DFT over the 400 samples of a frame (phase reduced mod 512)."""
    ang = 2.0 * np.pi * ((np.arange(N_FRAME)[:, None] * np.arange(N_DFT // 2 + 1)[None, :]) % N_DFT) / N_DFT
    return np.cos(ang), -np.sin(ang)


_TABLES = {}


def _tables(dtype):
    if dtype not in _TABLES:
        c, s = dft_tables()
        _TABLES[dtype] = (c.astype(dtype), s.astype(dtype), filterbank().astype(dtype))
    return _TABLES[dtype]


def logfbank(x, dtype=np.float64):
    """[n_frames, 26] of `dtype`: log of the filterbank energies of the power spectrum / 512, a zero energy taken as EPS."""
    c, s, fb = _tables(dtype)
    fr = frames(x, dtype)
    re, im = fr @ c, fr @ s
    pspec = (re * re + im * im) * dtype(1.0 / N_DFT)
    e = pspec @ fb.T
    return np.log(np.where(e == 0, dtype(EPS), e)).astype(dtype)


def logfbank_fft(x):
    """The library's own route in float64: numpy.fft.rfft of the frames."""
    fr = frames(x, np.float64)
    e = (np.abs(np.fft.rfft(fr, N_DFT)) ** 2 / N_DFT) @ filterbank().T
    return np.log(np.where(e == 0, EPS, e))


def stacker(feats, stack):
    """hubert_dataset.py stacker: zero rows (0.0, after the log) up to a multiple of `stack`, then `stack` frames per row."""
    if len(feats) % stack:
        feats = np.concatenate([feats, np.zeros((stack - len(feats) % stack, feats.shape[1]), dtype=feats.dtype)])
    return feats.reshape(-1, stack * feats.shape[1])


def align(feats, n_rows):
    """hubert_dataset.py:309-314: zero rows up to, or trimmed to, the video's frame count."""
    if n_rows is None:
        return feats
    diff = len(feats) - n_rows
    if diff < 0:
        return np.concatenate([feats, np.zeros((-diff, feats.shape[1]), dtype=feats.dtype)])
    return feats[:n_rows]


def layer_norm(x, eps=1e-5):
    """F.layer_norm over the row: biased variance, no affine, two passes in x's dtype."""
    dt = x.dtype.type
    mean = x.mean(axis=1, keepdims=True, dtype=x.dtype)
    d = x - mean
    var = (d * d).mean(axis=1, keepdims=True, dtype=x.dtype)
    return d / np.sqrt(var + dt(eps))


def audio_rows(x, stack=4, n_rows=None, normalize=True, dtype=np.float64):
    """The whole chain: [rows, 26 * stack] of `dtype`."""
    f = align(stacker(logfbank(x, dtype), stack), n_rows)
    return layer_norm(f) if normalize else f


# ---- the signals of the GPU test, at int16 scale (rounded to integers, so int16 and float input hold the same values)
def signal(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        x = rng.normal(0.0, 3000.0, n)
    elif kind == "tone":
        x = 8000.0 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / SR) + rng.normal(0.0, 3.0, n)
    elif kind == "walk":
        x = np.cumsum(rng.normal(0.0, 40.0, n))
    elif kind == "zero":
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
