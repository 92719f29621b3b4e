"""Speaker embeddings from audio on the device: the 256-d vector every model here takes as `spk_emb`.

helpers.py:185-198 (_get_speaker_embedding) calls sv2s.utils.get_speaker_embedding, which ends in the GE2E speaker encoder of
Real-Time-Voice-Cloning (encoder/inference.py: preprocess_wav, embed_utterance); none of that is in the reference tree.  Its
recipe is restated in DESIGN.md section 18 and runs here as

  l2s_wav_gain         increase-only volume normalisation to -30 dBFS (a per-clip factor, folded into the mel kernel's input)
  l2s_stft_mel_power   40-band power mel, 400-sample frames every 160 samples, reflect-centred
  l2s_tapgemm (fp32)   the LSTM input projections: layer 0 once per mel frame, layers 1-2 once per sequence row
  l2s_lstm_layer       the recurrence over 160-frame partial windows, gathered from the clip's projection rows by offset
  l2s_spk_embed_head   Linear + ReLU + L2 norm per window, the mean over a clip's windows, the final L2 norm

RTVC trims long silences with webrtcvad when that package imports; it is not installed here and the trimming is NOT built: the
embedding is that of the untrimmed clip (what RTVC itself computes without webrtcvad).  Input is 16 kHz; there is no resampler.
There is no CPU path: host tensors raise L2SError like every other op.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import audio, ops, weights
from ._lib import L2SError
from .packing import PackedState

SAMPLING_RATE = 16000
MEL_N_FFT, MEL_HOP, MEL_N_CHANNELS = 400, 160, 40      # 25 ms window, 10 ms step
PARTIAL_FRAMES = 160                                   # 1.6 s
TARGET_DBFS = -30.0
HIDDEN, LAYERS, EMBED = 256, 3, 256
BASIS_COLS = 448                                       # 7 tile pairs of 32 bins: bins 0 .. 223, zero past bin 200


def compute_partial_slices(n_samples, rate=1.3, min_coverage=0.75):
    """RTVC's compute_partial_slices: (starts, n_padded) - partial i covers mel frames [starts[i], starts[i] + 160), and the clip
    is zero-extended to n_padded = max(n_samples, 160 * (starts[-1] + 160)) samples before the mel analysis."""
    n = int(n_samples)
    if n < 1:
        raise ValueError("a clip needs at least one sample")
    n_frames = int(math.ceil((n + 1) / MEL_HOP))
    step = max(int(round(SAMPLING_RATE / rate / MEL_HOP)), 1)
    starts = list(range(0, max(1, n_frames - PARTIAL_FRAMES + step + 1), step))
    coverage = (n - MEL_HOP * starts[-1]) / (MEL_HOP * PARTIAL_FRAMES)
    if coverage < min_coverage and len(starts) > 1:
        starts = starts[:-1]
    return starts, max(n, MEL_HOP * (starts[-1] + PARTIAL_FRAMES))


def power_basis(n_fft=MEL_N_FFT, cols=BASIS_COLS):
    """The windowed real DFT as the [n_fft, cols] table of l2s_stft_mel_power (include/lip2speech_hip.h): columns by
    audio.packed_bins; zero columns past bin n_fft/2 and for the imaginary parts of bins 0 and n_fft/2.  float64."""
    k, part = audio.packed_bins(np.arange(cols))
    basis = audio.dft_basis(n_fft, n_fft, k, part, audio.hann_periodic(n_fft))
    basis[:, (k > n_fft // 2) | ((part == 1) & ((k == 0) | (k == n_fft // 2)))] = 0.0
    return basis


class PowerMel(audio._DeviceTables):
    """librosa 0.8's melspectrogram(wav, 16000, n_fft=400, hop_length=160, n_mels=40) as RTVC calls it (center=True, reflect
    padding, periodic Hann, power 2, Slaney filterbank and norm, no log), on the device.  Tables are float64 rounded once."""

    def __init__(self):
        self.basis = power_basis().astype(np.float32)
        self.fb = audio.mel_filterbank(SAMPLING_RATE, MEL_N_FFT, MEL_N_CHANNELS, 0.0, SAMPLING_RATE / 2.0).astype(np.float32)
        self.fb_range = audio.band_ranges(self.fb)
        self._dev = {}

    def mel_rows(self, wav, n_samples=None, n_valid=None, scale=None, T_rows=None):
        """wav: device tensor [B, S] fp32 or int16.  n_samples / n_valid / scale: int32 / int32 / fp32 device tensors [B] or None
        (see ops.stft_mel_power).  Returns fp32 [B, T_rows, 40] (default 1 + S // 160 rows), zeros past each clip's frames."""
        if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
            raise L2SError("mel_rows: expected a device tensor (there is no CPU path)")
        if wav.dim() != 2:
            raise ValueError("wav: [B, S]")
        B, S = wav.shape
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        basis, fb, fb_range = self.tables(wav.device)
        T = T_rows if T_rows is not None else 1 + S // MEL_HOP
        mel = torch.empty(B, T, MEL_N_CHANNELS, device=wav.device, dtype=torch.float32)
        ops.stft_mel_power(wav, mel, basis, fb, fb_range, B=B, S=S, T_rows=T, n_samples=n_samples, n_valid=n_valid, scale=scale,
                           ldw=wav.stride(0) if B > 1 else S)
        return mel


def pack_lstm_layer(w_ih, w_hh, b_ih, b_hh):
    """torch's LSTM layer parameters -> the operands of the device path, gate axis innermost (include/lip2speech_hip.h,
    l2s_lstm_layer): (w_ih_p [4H, in] with row 4 u + g = w_ih[g H + u], bias_p [4H] = (b_ih + b_hh) in that order,
    w_hh_p [H k, H u, 4 g] = w_hh[g H + u, k]).  fp32, contiguous, on the parameters' device."""
    H = w_hh.shape[1]
    if w_hh.shape != (4 * H, H) or w_ih.shape[0] != 4 * H or b_ih.shape != (4 * H,) or b_hh.shape != (4 * H,):
        raise ValueError("LSTM layer: w_ih [4H, in], w_hh [4H, H], b_ih / b_hh [4H]")
    w_ih, w_hh, b = w_ih.detach().float(), w_hh.detach().float(), (b_ih.detach().float() + b_hh.detach().float())
    w_ih_p = w_ih.view(4, H, -1).permute(1, 0, 2).reshape(4 * H, -1).contiguous()
    bias_p = b.view(4, H).t().reshape(4 * H).contiguous()
    w_hh_p = w_hh.view(4, H, H).permute(2, 1, 0).contiguous()
    return w_ih_p, bias_p, w_hh_p


def input_projection(x, w_ih_p, bias_p):
    """x fp32 [M, in] -> fp32 [M, 4H] = x w_ih_p^T + bias_p, one launch of the fp32 tap-GEMM."""
    M, K = x.shape
    N = w_ih_p.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    ops.tapgemm(x, w_ih_p, y, M=M, N=N, Cin=K, lda=x.stride(0), bias=bias_p, dtype=ops.F32)
    return y


def synthetic_state_dict(seed=0):
    """Build-owned weights for tests and --synthetic_weights: uniform in +-3/16 (default initialisation, +-1/16, leaves every
    gate in its linear range), drawn from the parameter name like weights.synth_tensor."""
    sd = {}
    for name, p in SpeakerEncoder().state_dict().items():
        r = weights._rng("speaker_encoder." + name, seed)
        sd[name] = torch.from_numpy(r.uniform(-3.0 / 16.0, 3.0 / 16.0, size=tuple(p.shape)).astype(np.float32))
    return sd


class SpeakerEncoder(nn.Module, PackedState):
    """Parameter holder with RTVC's state dict names (lstm.*, linear.*, similarity_weight / similarity_bias are accepted and
    ignored); `embed` runs the device path."""

    def __init__(self):
        super().__init__()
        self.lstm = nn.LSTM(MEL_N_CHANNELS, HIDDEN, LAYERS, batch_first=True)
        self.linear = nn.Linear(HIDDEN, EMBED)
        self.mel = PowerMel()
        self._init_packed()

    def load_state_dict(self, sd, strict=True):
        sd = {k: v for k, v in sd.items() if k not in ("similarity_weight", "similarity_bias")}
        w = sd.get("lstm.weight_hh_l0")
        if w is not None and tuple(w.shape) != (4 * HIDDEN, HIDDEN):
            raise ValueError(f"speaker encoder: hidden size {w.shape[-1]} is not supported (the device path is built for {HIDDEN})")
        return super().load_state_dict(sd, strict=strict)

    def load_checkpoint(self, path):
        """An RTVC encoder checkpoint: {"model_state": state dict, ...} or a bare state dict."""
        ck = torch.load(path, map_location="cpu")
        self.load_state_dict(ck["model_state"] if isinstance(ck, dict) and "model_state" in ck else ck)
        return self

    def pack(self, dev):
        """The device operands, built once per device (derived state keyed by the device index, so a process that alternates
        devices keeps both sets): [(w_ih_p, bias_p, w_hh_p)] * 3, linear weight transposed, linear bias."""
        dev = torch.device(dev)
        if dev.type != "cuda":
            raise L2SError("the speaker encoder needs a HIP device (there is no CPU path)")

        def build():
            layers = []
            for l in range(LAYERS):
                ps = [getattr(self.lstm, f"{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                layers.append(tuple(t.to(dev) for t in pack_lstm_layer(*[p.detach().cpu() for p in ps])))
            return (layers, self.linear.weight.detach().float().t().contiguous().to(dev),
                    self.linear.bias.detach().float().contiguous().to(dev))
        return self.derived(dev.index if dev.index is not None else torch.cuda.current_device(), build)

    def hidden_last(self, xproj0, row_off, packed_layers, max_seqs=2560):
        """Final hidden state of layer 2 for the sequences row_off (int32 host array: first row of each 160-step window in
        xproj0, the layer-0 projection of every mel frame): fp32 [P, 256].  Sequences run in chunks of max_seqs."""
        dev = xproj0.device
        P, T = len(row_off), PARTIAL_FRAMES
        h_last = torch.empty(P, HIDDEN, device=dev, dtype=torch.float32)
        ro_dev = torch.as_tensor(np.asarray(row_off, dtype=np.int32)).to(dev)
        for p0 in range(0, P, max_seqs):
            n = min(max_seqs, P - p0)
            own = torch.arange(n, dtype=torch.int32, device=dev) * T
            h_seq = torch.empty(n, T, HIDDEN, device=dev, dtype=torch.float32)
            ops.lstm_layer(xproj0, ro_dev[p0:p0 + n], packed_layers[0][2], S=n, T=T, h_seq=h_seq)
            xp = input_projection(h_seq.view(n * T, HIDDEN), packed_layers[1][0], packed_layers[1][1])
            ops.lstm_layer(xp, own, packed_layers[1][2], S=n, T=T, h_seq=h_seq)      # xp is computed: h_seq may be overwritten
            xp = input_projection(h_seq.view(n * T, HIDDEN), packed_layers[2][0], packed_layers[2][1])
            ops.lstm_layer(xp, own, packed_layers[2][2], S=n, T=T, h_last=h_last[p0:p0 + n])
        return h_last

    def embed(self, wavs, n_samples, max_seqs=2560):
        """wavs: device tensor [B, S], fp32 in (-1, 1) or int16 PCM at 16 kHz; n_samples: the B clip lengths (host ints, each in
        [1, S]).  Returns fp32 [B, 256] unit vectors; clip b's vector does not depend on its batch mates."""
        if not isinstance(wavs, torch.Tensor) or not wavs.is_cuda:
            raise L2SError("embed: expected a device tensor (there is no CPU path)")
        if wavs.dim() != 2:
            raise ValueError("wavs: [B, S]")
        B, S = wavs.shape
        ns = [int(v) for v in (n_samples.tolist() if hasattr(n_samples, "tolist") else n_samples)]
        if len(ns) != B or any(v < 1 or v > S for v in ns):
            raise ValueError(f"n_samples: one length in [1, {S}] per clip, got {ns}")
        if wavs.stride(1) != 1:
            wavs = wavs.contiguous()
        dev = wavs.device
        layers, lin_wt, lin_b = self.pack(dev)
        slices = [compute_partial_slices(v) for v in ns]
        T_rows = 1 + max(npad for _, npad in slices) // MEL_HOP
        i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)   # noqa: E731
        n_valid, n_pad = i32(ns), i32([npad for _, npad in slices])
        gain = torch.empty(B, device=dev, dtype=torch.float32)
        ops.wav_gain(wavs, gain, B=B, S=S, n_samples=n_valid, ldw=wavs.stride(0) if B > 1 else S, target_dbfs=TARGET_DBFS)
        mel = self.mel.mel_rows(wavs, n_samples=n_pad, n_valid=n_valid, scale=gain, T_rows=T_rows)
        xproj0 = input_projection(mel.view(B * T_rows, MEL_N_CHANNELS), layers[0][0], layers[0][1])
        row_off = [b * T_rows + s for b, (starts, _) in enumerate(slices) for s in starts]
        count = [len(starts) for starts, _ in slices]
        first = np.concatenate([[0], np.cumsum(count)[:-1]]).tolist()
        h_last = self.hidden_last(xproj0, row_off, layers, max_seqs)
        out = torch.empty(B, EMBED, device=dev, dtype=torch.float32)
        ops.spk_embed_head(h_last, i32(first), i32(count), lin_wt, lin_b, out, B=B, n_rows=h_last.shape[0])
        return out

    def embed_file(self, path):
        """float32 (256,) of one 16 kHz mono s16 wav - what _get_speaker_embedding returns for it."""
        pcm = audio.read_wav_s16(path, SAMPLING_RATE)
        if pcm.shape[0] < 1:
            raise ValueError(f"{path}: empty clip")
        return self.embed(torch.from_numpy(pcm).unsqueeze(0).cuda(), [pcm.shape[0]])[0].cpu().numpy()
