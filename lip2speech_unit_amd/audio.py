"""Log-mel analysis of waveforms on the device: the vocoder's mel conditioning made from audio.

create_dataset.py:62-75 (extract_mel_spec) calls fairseq's tacotron2 `TacotronSTFT(...).mel_spectrogram(audio)` with the sizes
of config.py:21-27; that class is third-party and not part of the reference tree.  Its recipe - reflect pad n_fft/2, periodic
Hann window, a dense Fourier basis applied as F.conv1d in fp32, magnitude, Slaney mel filterbank, log(clamp(., 1e-5)) - is
restated here as two fp32 tables built in numpy float64 (rounded once) and one HIP launch (csrc/melspec.hip).  There is no
CPU path: host tensors raise L2SError like every other op.
"""
import numpy as np
import torch

from . import ops
from ._lib import L2SError


def _hz_to_mel(f):
    """Slaney's auditory-toolbox scale: linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_filterbank(sr=16000, n_fft=640, n_mels=80, fmin=0.0, fmax=8000.0):
    """Triangular filters on the Slaney scale, each normalised to unit area (`norm='slaney'`): float64 [n_mels, n_fft/2 + 1]."""
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    fb = np.maximum(0.0, np.minimum(lower, upper))
    return fb * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def packed_bins(c):
    """(bin, part) of column c of a packed basis: tile q = c // 32, lane l = c % 32, bin 32 (q // 2) + l; part 0 (even tiles) is
    w cos, part 1 (odd tiles) is -w sin - the column map of csrc/frame_dft.h."""
    c = np.asarray(c)
    return 32 * (c // 64) + c % 32, (c % 64) // 32


def dft_basis(n_frame, n_dft, k, part, window):
    """float64 [n_frame, len(k)]: column c is the window times cos (part[c] = 0) or -sin (part[c] = 1) of bin k[c] of an
    n_dft-point DFT, over the samples of a frame; the phase is the exact integer n k reduced mod n_dft before the division."""
    n = np.arange(n_frame)
    ang = 2.0 * np.pi * ((n[:, None] * np.asarray(k)[None, :]) % n_dft) / n_dft
    return np.where((np.asarray(part) == 0)[None, :], np.cos(ang), -np.sin(ang)) * np.asarray(window, dtype=np.float64)[:, None]


def packed_basis(n_fft=640, window=None):
    """The windowed real DFT as the [n_fft, n_fft] matrix of l2s_mel_spectrogram (include/lip2speech_hip.h): row = sample,
    columns by packed_bins, and column 32 (the imaginary part of bin 0) holds the real part of bin n_fft/2.  float64."""
    if n_fft % 64:
        raise ValueError("n_fft must be a multiple of 64")
    k, part = packed_bins(np.arange(n_fft))
    k[32], part[32] = n_fft // 2, 0
    return dft_basis(n_fft, n_fft, k, part, hann_periodic(n_fft) if window is None else window)


def unpack_spectrum(y, n_fft=640):
    """(re, im) [..., n_fft/2 + 1] of a product x @ packed_basis [..., n_fft] - the column map read backwards."""
    y = np.asarray(y)
    t = y.reshape(y.shape[:-1] + (n_fft // 64, 2, 32))
    re = np.concatenate([t[..., 0, :].reshape(y.shape[:-1] + (n_fft // 2,)), y[..., 32:33]], axis=-1)
    im = np.concatenate([t[..., 1, :].reshape(y.shape[:-1] + (n_fft // 2,)), np.zeros_like(y[..., :1])], axis=-1).copy()
    im[..., 0] = 0.0
    return re, im


def num_frames(n_samples, hop=160):
    return 1 + n_samples // hop


def band_ranges(fb):
    """int32 [n_mels, 2]: [first, past-last) bin of each band's non-zero weights (0, 0 for an empty band)."""
    nz = fb != 0
    return np.stack([np.where(nz.any(1), nz.argmax(1), 0), np.where(nz.any(1), fb.shape[1] - nz[:, ::-1].argmax(1), 0)],
                    axis=1).astype(np.int32)


class _DeviceTables:
    """The float32 / int32 numpy arrays named by TABLES on the instance (and a dict `_dev`), uploaded once per device."""
    TABLES = ("basis", "fb", "fb_range")

    def tables(self, device):
        """The TABLES arrays on `device`, in that order, uploaded once per device."""
        device = torch.device(device)
        if device.type != "cuda":
            raise L2SError(f"{type(self).__name__} needs a HIP device (there is no CPU path)")
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(getattr(self, t)).to(device) for t in self.TABLES)
        return self._dev[key]

    def _lengths(self, wav, n_samples, least):
        """n_samples of mel_rows -> None or an int32 device tensor [B]; a host sequence is checked: least < n <= S."""
        B, S = wav.shape
        if n_samples is None:
            if S <= least:
                raise ValueError(f"reflect padding needs more than {least} samples, got {S}")
            return None
        if isinstance(n_samples, torch.Tensor) and n_samples.is_cuda:
            if n_samples.dtype != torch.int32 or n_samples.shape != (B,):
                raise ValueError("n_samples: int32 [B]")
            return n_samples.contiguous()
        ns = [int(v) for v in (n_samples.tolist() if hasattr(n_samples, "tolist") else n_samples)]
        if len(ns) != B:
            raise ValueError("n_samples: one length per clip")
        if any(v <= least or v > S for v in ns):
            raise ValueError(f"n_samples: every clip needs {least} < n <= {S} samples, got {ns}")
        return torch.tensor(ns, dtype=torch.int32).to(wav.device)


class TacotronSTFT(_DeviceTables):
    """`TacotronSTFT(...).mel_spectrogram(audio)` of extract_mel_spec, on the device; defaults from config.py:21-27."""

    def __init__(self, filter_length=640, hop_length=160, win_length=640, n_mel_channels=80, sampling_rate=16000, mel_fmin=0.0,
                 mel_fmax=8000.0, floor=1e-5):
        if win_length != filter_length:
            raise ValueError("win_length must equal filter_length")
        self.n_fft, self.hop, self.n_mels, self.sr, self.floor = filter_length, hop_length, n_mel_channels, sampling_rate, floor
        self.basis = packed_basis(filter_length).astype(np.float32)
        fb = mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin, mel_fmax)
        self.fb = fb.astype(np.float32)
        self.fb_range = band_ranges(self.fb)
        self._dev = {}

    def mel_rows(self, wav, n_samples=None):
        """wav: device tensor [B, S], fp32 in (-1, 1) or int16 PCM.  n_samples: clip lengths - None (all S), a host sequence
        (checked: n_fft/2 < n <= S) or an int32 device tensor (not read on the host; a clip of <= n_fft/2 samples gives zero rows).
        Returns fp32 [B, 1 + S // hop, n_mel]; clip b's rows past 1 + n_b // hop are zeros."""
        if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
            raise L2SError("mel_rows: expected a device tensor (there is no CPU path)")
        if wav.dim() != 2:
            raise ValueError("wav: [B, S]")
        B, S = wav.shape
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        n_samples = self._lengths(wav, n_samples, self.n_fft // 2)
        basis, fb, fb_range = self.tables(wav.device)
        T = num_frames(S, self.hop)
        mel = torch.empty(B, T, self.n_mels, device=wav.device, dtype=torch.float32)
        ops.mel_spectrogram(wav, mel, basis, fb, fb_range, B=B, S=S, T_rows=T, n_samples=n_samples, ldw=wav.stride(0) if B > 1 else S,
                            n_fft=self.n_fft, hop=self.hop, n_mels=self.n_mels, floor=self.floor)
        return mel

    def mel_spectrogram(self, audio):
        """audio [B, S] in (-1, 1) -> [B, n_mel, T], the call extract_mel_spec makes."""
        return self.mel_rows(audio).transpose(1, 2)


class MelSpectrogram(_DeviceTables):
    """The HiFi-GAN `mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False)` of the
    vocoder's loss (speech-resynthesis/dataset.py:44-67; train.py:152,224 and dataset_multi_input.py:275 call it with the sizes of
    configs/lrs3/multi_input.json and fmax = fmax_for_loss = null, i.e. sr/2), on the device: reflect pad (n_fft - hop_size) // 2 on
    each side, periodic Hann window, torch.stft(center=False), sqrt(re^2 + im^2 + 1e-9), the Slaney filterbank, log(clamp(., 1e-5)).
    Tables are float64, rounded to float32 once, uploaded once per device.  There is no CPU path."""

    def __init__(self, n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=256, win_size=1024, fmin=0, fmax=None):
        if win_size != n_fft:
            raise ValueError("win_size must equal n_fft")
        self.n_fft, self.hop, self.n_mels, self.sr = n_fft, hop_size, num_mels, sampling_rate
        self.pad, self.mag_eps, self.floor = (n_fft - hop_size) // 2, 1e-9, 1e-5
        self.basis = packed_basis(n_fft).astype(np.float32)
        fmax = sampling_rate / 2.0 if fmax is None else fmax
        self.fb = mel_filterbank(sampling_rate, n_fft, num_mels, float(fmin), float(fmax)).astype(np.float32)
        self.fb_range = band_ranges(self.fb)
        self._dev = {}

    def num_frames(self, n_samples):
        """Frames of a clip of n_samples: 0 unless the reflection is valid (n > pad) and one whole frame fits."""
        n = int(n_samples)
        return (n + 2 * self.pad - self.n_fft) // self.hop + 1 if n > self.pad and n + 2 * self.pad >= self.n_fft else 0

    def mel_rows(self, wav, n_samples=None):
        """wav: device tensor [B, S], fp32 in (-1, 1) or int16 PCM.  n_samples: clip lengths - None (all S), a host sequence
        (checked: pad < n <= S) or an int32 device tensor (not read on the host).  Returns fp32 [B, num_frames(S), n_mel]; clip
        b's rows past num_frames(n_b) are zeros."""
        if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
            raise L2SError("mel_rows: expected a device tensor (there is no CPU path)")
        if wav.dim() != 2:
            raise ValueError("wav: [B, S]")
        B, S = wav.shape
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        T = self.num_frames(S)
        if T <= 0:
            raise ValueError(f"no frame fits: {S} samples with n_fft {self.n_fft} and {self.pad} reflected on each side")
        n_samples = self._lengths(wav, n_samples, self.pad)
        basis, fb, fb_range = self.tables(wav.device)
        mel = torch.empty(B, T, self.n_mels, device=wav.device, dtype=torch.float32)
        ops.stft_mel(wav, mel, basis, fb, fb_range, B=B, S=S, T_rows=T, n_samples=n_samples, ldw=wav.stride(0) if B > 1 else S,
                     n_fft=self.n_fft, hop=self.hop, n_mels=self.n_mels, pad=self.pad, mag_eps=self.mag_eps, floor=self.floor)
        return mel

    def __call__(self, y):
        """y [B, S] in (-1, 1) -> [B, n_mel, T], the call the reference makes."""
        return self.mel_rows(y).transpose(1, 2)


def logfbank_filterbank(nfilt=26, nfft=512, sr=16000):
    """python_speech_features.get_filterbanks at its defaults: triangular filters between the bin edges
    floor((nfft + 1) mel2hz(linspace(0, hz2mel(sr / 2), nfilt + 2)) / sr), hz2mel(f) = 2595 log10(1 + f / 700); float64
    [nfilt, nfft / 2 + 1].  The last edge is nfft / 2 exactly, so bin nfft / 2 has weight 0 in every filter."""
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + (sr / 2.0) / 700.0), nfilt + 2)
    edges = np.floor((nfft + 1) * (700.0 * (10.0 ** (mel / 2595.0) - 1.0)) / sr).astype(np.int64)
    fb = np.zeros((nfilt, nfft // 2 + 1))
    for j in range(nfilt):
        lo, mid, hi = int(edges[j]), int(edges[j + 1]), int(edges[j + 2])
        i = np.arange(lo, mid)
        fb[j, i] = (i - lo) / (mid - lo)
        i = np.arange(mid, hi)
        fb[j, i] = (hi - i) / (hi - mid)
    return fb, edges


def logfbank_frames(n, frame=400, hop=160):
    """Frames python_speech_features.framesig makes of n samples: 1 if n <= frame, else 1 + ceil((n - frame) / hop)."""
    n = int(n)
    return 1 if n <= frame else 1 + -((frame - n) // hop)


def logfbank_rows(n, stack=4):
    """Rows of the stacker (hubert_dataset.py:299-304): ceil(frames / stack)."""
    return -(-logfbank_frames(n) // int(stack))


class LogFbank(_DeviceTables):
    """The audio features of AV-HuBERT (hubert_dataset.py:299-315,370-372) on the device: python_speech_features.logfbank at 16 kHz
    with that library's defaults (pre-emphasis 0.97, 400-sample frames every 160, no window, 512-point power spectrum / 512, 26
    triangular filters, log with a zero energy taken as float eps), `stack` frames per row, rows padded or trimmed to the video's
    frame count, and the per-row layer norm.  Tables are float64, rounded to float32 once, uploaded once per device (the basis is
    [400, 512] in the column order of csrc/frame_dft.h).  There is no CPU path."""
    N_FRAME, HOP, N_DFT, NFILT = 400, 160, 512, 26

    def __init__(self, stack=4, normalize=True):
        if stack not in (1, 4):
            raise ValueError(f"stack_order_audio = {stack}: 1 and 4 are built")
        self.stack, self.normalize = int(stack), bool(normalize)
        k, part = packed_bins(np.arange(self.N_DFT))
        self.basis = dft_basis(self.N_FRAME, self.N_DFT, k, part, np.ones(self.N_FRAME)).astype(np.float32)
        fb, self.edges = logfbank_filterbank(self.NFILT, self.N_DFT)
        self.fb = fb.astype(np.float32)
        self.fb_range = band_ranges(self.fb)
        self._dev = {}

    @property
    def width(self):
        return self.NFILT * self.stack

    def rows(self, wav, n_samples=None, n_rows=None, T_rows=None, out=None, dtype=torch.float32):
        """wav: device tensor [B, S], int16 PCM or float AT INT16 SCALE.  n_samples: clip lengths - None (all S), a host sequence
        (checked: 0 < n <= S) or an int32 device tensor (not read on the host).  n_rows: the video's frame counts in the same
        forms, or None for the audio's own row counts.  Returns `out`, [B, T_rows, 26 * stack] of `dtype` (default T_rows: the
        largest n_rows when it is a host sequence, else logfbank_rows(S)); clip b's rows past min(its rows, n_rows[b]) are zeros."""
        if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
            raise L2SError("LogFbank.rows: expected a device tensor (there is no CPU path)")
        if wav.dim() != 2:
            raise ValueError("wav: [B, S]")
        B, S = wav.shape
        if wav.stride(1) != 1:
            wav = wav.contiguous()

        def lengths(v, name, hi):
            if v is None or (isinstance(v, torch.Tensor) and v.is_cuda):
                if v is not None and (v.dtype != torch.int32 or v.shape != (B,)):
                    raise ValueError(f"{name}: int32 [B]")
                return v if v is None else v.contiguous(), None
            host = [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
            if len(host) != B:
                raise ValueError(f"{name}: one value per clip")
            if any(x <= 0 or (hi is not None and x > hi) for x in host):
                raise ValueError(f"{name}: every clip needs 0 < n" + (f" <= {hi}" if hi is not None else "") + f", got {host}")
            return torch.tensor(host, dtype=torch.int32).to(wav.device), host
        n_samples, _ = lengths(n_samples, "n_samples", S)
        n_rows, host_rows = lengths(n_rows, "n_rows", None)
        if T_rows is None:
            T_rows = out.shape[1] if out is not None else (max(host_rows) if host_rows else logfbank_rows(S, self.stack))
        if out is None:
            out = torch.empty(B, T_rows, self.width, device=wav.device, dtype=dtype)
        basis, fb, fb_range = self.tables(wav.device)
        ops.logfbank(wav, out, basis, fb, fb_range, B=B, S=S, T_rows=T_rows, stack=self.stack, normalize=self.normalize,
                     n_samples=n_samples, n_rows=n_rows, ldw=wav.stride(0) if B > 1 else S, ldo=out.stride(-2))
        return out


_default = None


def default_stft():
    global _default
    if _default is None:
        _default = TacotronSTFT()
    return _default


def read_wav_s16(path, sampling_rate=16000):
    """int16 PCM of a 16 kHz mono s16 wav (stdlib `wave`; anything else is refused)."""
    import wave
    with wave.open(path, "rb") as w:
        if w.getnchannels() != 1 or w.getsampwidth() != 2 or w.getframerate() != sampling_rate or w.getcomptype() != "NONE":
            raise ValueError(f"{path}: expected {sampling_rate} Hz mono s16 PCM")
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
