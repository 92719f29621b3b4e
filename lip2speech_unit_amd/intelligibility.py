"""STOI and ESTOI of processed speech against its clean original, on the device - the end-to-end numbers the reference publishes
(README.md:103-122).  The algorithms are the published ones:

  STOI:  C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An algorithm for intelligibility prediction of time-frequency weighted
         noisy speech", IEEE Trans. Audio, Speech, Language Process. 19(7), 2011;
  ESTOI: J. Jensen, C. H. Taal, "An algorithm for predicting the intelligibility of speech masked by modulated noise maskers",
         IEEE/ACM Trans. Audio, Speech, Language Process. 24(11), 2016,

restated in DESIGN.md section 17: resample to 10 kHz with the Octave-compatible 581-tap Kaiser filter, drop the frames of the clean
signal more than 40 dB below its loudest, third-octave band magnitudes of both signals over the kept frames, and the two
correlation measures over every 30-frame segment.  The tables are numpy float64 rounded to fp32 once; the work is four HIP entries
(csrc/stoi.hip).  There is no CPU path: host tensors raise L2SError like every other op.
"""
import numpy as np
import torch

from . import audio, ops
from ._lib import L2SError

FS = 10000
N_FRAME, HOP, NFFT, NUMBAND, MINFREQ, N_SEG = 256, 128, 512, 15, 150, 30
BIN0 = 7                       # the first bin any band reads; the basis holds bins 7 .. 262 (219 and above as zeros)


def resample_taps(up=5, down=8):
    """The 581 normalised taps w of the 16 kHz -> 10 kHz low-pass (Octave's resample): float64."""
    fc = 1.0 / max(up, down) / 2.0
    half = int(np.ceil(52.0 / (28.714 * (fc / 10.0))))
    t = np.arange(-half, half + 1)
    h = np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7)) * (2.0 * up * fc * np.sinc(2.0 * fc * t))
    return h / h.sum()


def polyphase_taps(w=None, up=5):
    """float64 [5, 117]: taps[p, q] = 5 w[p + 5 q], zero where p + 5 q runs past the filter (l2s_stoi_resample's table)."""
    w = resample_taps() if w is None else np.asarray(w, dtype=np.float64)
    nq = (len(w) + up - 1) // up
    t = np.zeros((up, nq))
    for p in range(up):
        ph = w[p::up]
        t[p, :len(ph)] = up * ph
    return t


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def band_edges():
    """int32 [16]: band i sums the bins [edges[i], edges[i + 1]) of the 512-point spectrum at 10 kHz."""
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    lo = [int(np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i - 1) / 6.0)))) for i in range(NUMBAND)]
    hi = [int(np.argmin(np.abs(f - MINFREQ * 2.0 ** ((2 * i + 1) / 6.0)))) for i in range(NUMBAND)]
    if lo[1:] != hi[:-1]:
        raise ValueError("third-octave bands do not tile the spectrum")
    return np.array(lo + hi[-1:], dtype=np.int32)


def basis_bin(c):
    """(bin, part) of column c of the packed basis: part 0 = cos, 1 = -sin (the column map of l2s_stoi_bands)."""
    k, part = audio.packed_bins(c)
    return BIN0 + k, part


def packed_basis():
    """float64 [256, 512]: row n = sample of a frame with the analysis window folded in, columns by basis_bin; bins the bands do
    not read (219 and above) are zeros."""
    k, part = basis_bin(np.arange(2 * N_FRAME))
    b = audio.dft_basis(N_FRAME, NFFT, k, part, window())
    b[:, k >= band_edges()[-1]] = 0.0
    return b


class STOI(audio._DeviceTables):
    """Scores batches of clip pairs on the device; the tables are built once and uploaded once per device."""
    TABLES = ("taps", "window", "basis", "band_edges")

    def __init__(self, sampling_rate=16000):
        if sampling_rate != 16000:
            raise ValueError(f"STOI is built for 16 kHz clips only, got {sampling_rate}")
        self.sampling_rate = sampling_rate
        self.taps = polyphase_taps().astype(np.float32)
        self.window = window().astype(np.float32)
        self.basis = packed_basis().astype(np.float32)
        self.band_edges = band_edges()
        self._dev = {}

    def stages(self, clean, processed, n_samples=None):
        """Everything the four entries produce for device tensors clean / processed [B, S] (fp32 in (-1, 1) or int16 PCM, one dtype)
        and clip lengths n_samples (None, a host sequence or an int32 device tensor [B]): dict of resampled [B, 2, R], kept [B, Kmax],
        n_kept [B], bands [B, 2, 15, Fmax], seg [B, 2, Mmax] float64, stoi / estoi [B] fp32, n_segments [B] int32."""
        for t, name in ((clean, "clean"), (processed, "processed")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise L2SError(f"{name}: expected a device tensor (there is no CPU path)")
        if clean.dim() != 2 or clean.shape != processed.shape or clean.dtype != processed.dtype:
            raise ValueError("clean and processed: [B, S] of one shape and dtype (truncate both to the shorter first)")
        B, S = clean.shape
        if B == 0 or S == 0:
            raise ValueError("clean and processed: empty batch")
        clean, processed = (t if t.stride(1) == 1 else t.contiguous() for t in (clean, processed))
        dev = clean.device
        if n_samples is not None and not (isinstance(n_samples, torch.Tensor) and n_samples.is_cuda):
            ns = [int(v) for v in (n_samples.tolist() if hasattr(n_samples, "tolist") else n_samples)]
            if len(ns) != B or any(v < 0 or v > S for v in ns):
                raise ValueError(f"n_samples: one length 0 <= n <= {S} per clip")
            n_samples = torch.tensor(ns, dtype=torch.int32).to(dev)
        elif n_samples is not None and (n_samples.dtype != torch.int32 or n_samples.shape != (B,)):
            raise ValueError("n_samples: int32 [B]")
        taps, win, basis, edges = self.tables(dev)
        R = ops.stoi_len10k(S)
        Kmax = max(ops.stoi_frames_of(R), 1)
        Fmax, Mmax = max(Kmax - 1, 1), max(Kmax - N_SEG, 1)
        res = torch.empty(B, 2, R, device=dev, dtype=torch.float32)
        for i, wav in enumerate((clean, processed)):
            ops.stoi_resample(wav, taps, res[:, i], B=B, S=S, R=R, n_samples=n_samples, ldw=wav.stride(0) if B > 1 else S, ldo=2 * R)
        kept = torch.empty(B, Kmax, device=dev, dtype=torch.int32)
        n_kept = torch.empty(B, device=dev, dtype=torch.int32)
        ops.stoi_frames(res[:, 0], win, kept, n_kept, B=B, S=S, n_samples=n_samples, ldx=2 * R, ldk=Kmax)
        bands = torch.empty(B, 2, NUMBAND, Fmax, device=dev, dtype=torch.float32)
        ops.stoi_bands(res[:, 0], res[:, 1], kept, n_kept, win, basis, edges, bands, B=B, S=S, ldf=Fmax, n_samples=n_samples,
                       ldx=2 * R, ldk=Kmax)
        seg = torch.empty(B, 2, Mmax, device=dev, dtype=torch.float64)
        stoi_, estoi_ = (torch.empty(B, device=dev, dtype=torch.float32) for _ in range(2))
        n_seg = torch.empty(B, device=dev, dtype=torch.int32)
        ops.stoi_scores(bands, n_kept, seg, stoi_, estoi_, n_seg, B=B, ldf=Fmax, lds=Mmax)
        return {"resampled": res, "kept": kept, "n_kept": n_kept, "bands": bands, "seg": seg, "stoi": stoi_, "estoi": estoi_,
                "n_segments": n_seg}

    def scores(self, clean, processed, n_samples=None):
        """{"stoi", "estoi": fp32 [B], "n_segments": int32 [B]} on the device.  A clip with fewer than 30 frames after the silent
        ones are dropped has no segment: both scores are 1e-5 and n_segments is 0, as the published code returns."""
        r = self.stages(clean, processed, n_samples)
        return {k: r[k] for k in ("stoi", "estoi", "n_segments")}


_default = None


def default_stoi():
    global _default
    if _default is None:
        _default = STOI()
    return _default


def stoi(clean, processed, n_samples=None, sampling_rate=16000):
    """STOI of device tensors [B, S] (or [S]): fp32 [B] (or a 0-d tensor)."""
    return _one("stoi", clean, processed, n_samples, sampling_rate)


def estoi(clean, processed, n_samples=None, sampling_rate=16000):
    """ESTOI of device tensors [B, S] (or [S]): fp32 [B] (or a 0-d tensor)."""
    return _one("estoi", clean, processed, n_samples, sampling_rate)


def _one(key, clean, processed, n_samples, sampling_rate):
    if sampling_rate != 16000:
        raise ValueError(f"STOI is built for 16 kHz clips only, got {sampling_rate}")
    flat = isinstance(clean, torch.Tensor) and clean.dim() == 1
    if flat:
        clean, processed = clean.unsqueeze(0), processed.unsqueeze(0)
    out = default_stoi().scores(clean, processed, n_samples)[key]
    return out[0] if flat else out
