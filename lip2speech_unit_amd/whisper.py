"""Whisper speech recognition on gfx950: the recogniser the reference runs on every synthesis request (its `server.py:48`
`WhisperASR(model='base.en', ...)`, `server.py:337-342` `asr.run(pred_audio_path)`) and behind the WER it publishes.

`Whisper` keeps openai-whisper's module names and state-dict layout (`encoder.conv1.weight`, `decoder.token_embedding.weight`,
`decoder.blocks.N.cross_attn.query.weight`, ...), so the `.pt` file `base.en` names loads as it is (`load_whisper`); a HuggingFace
state dict loads through `HF_RENAMES`.  nn layers only hold parameters; the arithmetic is liblip2speech_hip.so:

  front end   l2s_whisper_logmel (csrc/whisper_logmel.hip)
  encoder     two 3-tap convolutions as tap-GEMMs with GELU epilogues (conv2 adds the sinusoidal position table as its residual
              operand), N pre-LN layers on l2s_tapgemm / l2s_attention / l2s_layernorm exactly as hubert.TransformerEncoder runs
              them (q, k, v in one GEMM, q pre-scaled by 64^-0.5, k_proj without bias), ln_post; every clip has 1 500 rows, no mask
  cross K/V   once per clip and decoder layer: one grouped GEMM into the 16-bit caches [B, 1500, d]
  step        l2s_layernorm / l2s_tapgemm at M = B rows, l2s_kv_attention against the self and cross caches, l2s_vocab_argmax (the
              tied output layer with the greedy choice), l2s_whisper_advance (csrc/whisper_decode.hip).  The position is a device
              int32: one step is a fixed launch sequence, captured once into a graph and replayed (`graph=True`).

Scope: one 30-s window, greedy decoding at temperature 0; no timestamps, temperature fallback,
compression-ratio or no-speech rules, language detection or conditioning on previous text; 16-bit operands (F16 / BF16) with
fp32 accumulation and an fp32 residual stream."""
from dataclasses import asdict, dataclass

import numpy as np
import torch
import torch.nn as nn

from . import audio, ops
from .asr_text import Detokenizer, WhisperDecodeConfig
from .ops import ACT_GELU, F_RES_POST, MODE_CONV1D
from .packing import PackedState, pack_conv1d, state_epoch

N_SAMPLES, N_FRAMES, N_CTX_AUDIO = ops.WHISPER_SAMPLES, ops.WHISPER_FRAMES, 1500
MEL_LD = 128                                     # conv1's operand: 80 bands padded to the tap-GEMM's 64-wide K tile


@dataclass
class WhisperDims:
    """openai-whisper's ModelDimensions."""
    n_mels: int = 80
    n_audio_ctx: int = 1500
    n_audio_state: int = 512
    n_audio_head: int = 8
    n_audio_layer: int = 6
    n_vocab: int = 51864
    n_text_ctx: int = 448
    n_text_state: int = 512
    n_text_head: int = 8
    n_text_layer: int = 6

    @classmethod
    def base_en(cls):
        return cls()


# openai-whisper name fragment -> HuggingFace (transformers WhisperForConditionalGeneration) fragment, applied in this order to
# "model." + key; read backwards for the other direction
HF_RENAMES = (
    ("blocks.", "layers."), (".cross_attn_ln.", ".encoder_attn_layer_norm."), (".cross_attn.", ".encoder_attn."),
    (".attn_ln.", ".self_attn_layer_norm."), (".attn.", ".self_attn."), (".query.", ".q_proj."), (".key.", ".k_proj."),
    (".value.", ".v_proj."), (".out.", ".out_proj."), (".mlp_ln.", ".final_layer_norm."), (".mlp.0.", ".fc1."), (".mlp.2.", ".fc2."),
    ("encoder.ln_post.", "encoder.layer_norm."), ("decoder.ln.", "decoder.layer_norm."), ("token_embedding.", "embed_tokens."),
    ("positional_embedding", "embed_positions.weight"),
)


def openai_to_hf(sd):
    """An openai-whisper state dict under HuggingFace's names (plus the tied `proj_out.weight`)."""
    out = {}
    for k, v in sd.items():
        for a, b in HF_RENAMES:
            k = k.replace(a, b)
        out["model." + k] = v
    out["proj_out.weight"] = out["model.decoder.embed_tokens.weight"]
    return out


def hf_to_openai(sd):
    """A HuggingFace Whisper state dict under openai-whisper's names (`proj_out.weight` is the tied embedding and is dropped)."""
    out = {}
    for k, v in sd.items():
        if k == "proj_out.weight":
            continue
        k = k[len("model."):] if k.startswith("model.") else k
        for a, b in HF_RENAMES:
            k = k.replace(b, a)
        out[k] = v
    return out


def sinusoids(length, channels):
    """openai-whisper's sinusoids(): the encoder's position table, float32 [length, channels]."""
    inc = np.log(10000.0) / (channels // 2 - 1)
    t = np.arange(length)[:, None] * np.exp(-inc * np.arange(channels // 2))[None, :]
    return torch.from_numpy(np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32))


class MultiHeadAttention(nn.Module):
    def __init__(self, n_state, n_head):
        super().__init__()
        self.n_head = n_head
        self.query = nn.Linear(n_state, n_state)
        self.key = nn.Linear(n_state, n_state, bias=False)
        self.value = nn.Linear(n_state, n_state)
        self.out = nn.Linear(n_state, n_state)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, n_state, n_head, cross_attention=False):
        super().__init__()
        self.attn = MultiHeadAttention(n_state, n_head)
        self.attn_ln = nn.LayerNorm(n_state)
        self.cross_attn = MultiHeadAttention(n_state, n_head) if cross_attention else None
        self.cross_attn_ln = nn.LayerNorm(n_state) if cross_attention else None
        self.mlp = nn.Sequential(nn.Linear(n_state, 4 * n_state), nn.GELU(), nn.Linear(4 * n_state, n_state))
        self.mlp_ln = nn.LayerNorm(n_state)


class AudioEncoder(nn.Module):
    def __init__(self, dims):
        super().__init__()
        d = dims.n_audio_state
        self.conv1 = nn.Conv1d(dims.n_mels, d, kernel_size=3, padding=1)
        self.conv2 = nn.Conv1d(d, d, kernel_size=3, stride=2, padding=1)
        self.register_buffer("positional_embedding", sinusoids(dims.n_audio_ctx, d))
        self.blocks = nn.ModuleList([ResidualAttentionBlock(d, dims.n_audio_head) for _ in range(dims.n_audio_layer)])
        self.ln_post = nn.LayerNorm(d)


class TextDecoder(nn.Module):
    def __init__(self, dims):
        super().__init__()
        d = dims.n_text_state
        self.token_embedding = nn.Embedding(dims.n_vocab, d)
        self.positional_embedding = nn.Parameter(torch.zeros(dims.n_text_ctx, d))
        self.blocks = nn.ModuleList([ResidualAttentionBlock(d, dims.n_text_head, cross_attention=True) for _ in range(dims.n_text_layer)])
        self.ln = nn.LayerNorm(d)


def _f32(t, dev):
    return t.detach().float().to(dev).contiguous()


def _ln(m, dev):
    return (_f32(m.weight, dev), _f32(m.bias, dev))


class LogMel(audio._DeviceTables):
    """The tables of l2s_whisper_logmel: the windowed DFT of 400-sample frames (periodic Hann; speaker_encoder.power_basis) and the
    80-band Slaney filterbank of WhisperFeatureExtractor, float64 rounded once."""

    def __init__(self):
        from .speaker_encoder import power_basis
        self.basis = power_basis().astype(np.float32)
        self.fb = audio.mel_filterbank(16000, 400, 80, 0.0, 8000.0).astype(np.float32)
        self.fb_range = audio.band_ranges(self.fb)
        self._dev = {}

    def features(self, wav, n_samples=None, dtype=ops.F16, want_f32=False):
        """wav: device tensor [B, S <= 480 000] fp32 or int16, n_samples: int32 device tensor [B] or None -> 16-bit rows
        [B * 3000, 128] (80 bands, zero columns after them) and, with want_f32, the fp32 values [B * 3000, 80] before the rounding."""
        if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
            raise ops.L2SError("LogMel.features: expected a device tensor (there is no CPU path)")
        if wav.dim() != 2:
            raise ValueError("wav: [B, S]")
        B, S = wav.shape
        if S > N_SAMPLES:
            raise ValueError(f"a clip has at most {N_SAMPLES} samples (one 30-s window), got {S}")
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        if S == 0:                                      # nothing to read: a one-sample buffer of which no sample is real
            wav, S = wav.new_zeros(B, 1), 1
            n_samples = torch.zeros(B, device=wav.device, dtype=torch.int32)
        basis, fb, fb_range = self.tables(wav.device)
        work = torch.empty(ops.whisper_logmel_workspace(B), device=wav.device, dtype=torch.uint8)
        out = torch.empty(B * N_FRAMES, MEL_LD, device=wav.device, dtype=ops.torch_dtype(dtype))
        f32 = torch.empty(B * N_FRAMES, 80, device=wav.device, dtype=torch.float32) if want_f32 else None
        ops.whisper_logmel(wav, work, out, basis, fb, fb_range, B=B, S=S, n_samples=n_samples, ldw=wav.stride(0) if B > 1 else S,
                           out_f32=f32, dtype=dtype)
        return (out, f32) if want_f32 else out


class Whisper(nn.Module, PackedState):
    def __init__(self, dims: WhisperDims = None, dtype=ops.F16):
        super().__init__()
        dims = dims or WhisperDims()
        if dims.n_mels != 80:
            raise NotImplementedError(f"n_mels = {dims.n_mels}: the log-mel front end is built for 80 bands (large-v3's 128 are not)")
        for n, (w, h) in (("audio", (dims.n_audio_state, dims.n_audio_head)), ("text", (dims.n_text_state, dims.n_text_head))):
            if w != 64 * h or w > 1280:
                raise NotImplementedError(f"n_{n}_state = {w} with {h} heads: heads must be 64 wide and the width at most 1280")
        if dims.n_audio_ctx != N_CTX_AUDIO or dims.n_audio_state != dims.n_text_state:
            raise NotImplementedError("n_audio_ctx must be 1500 and the encoder and decoder widths equal")
        if dtype not in (ops.F16, ops.BF16):
            raise NotImplementedError("Whisper runs with F16 or BF16 operands; there is no fp32 mode")
        self.dims, self.dtype = dims, dtype
        self.encoder = AudioEncoder(dims)
        self.decoder = TextDecoder(dims)
        self.logmel = LogMel()
        self._init_packed()

    # ---- weights ---------------------------------------------------------------------------------------------------------------
    def _pack_block(self, blk, dev, t16, cross):
        scale = 64 ** -0.5

        def qkv(a):
            wq, bq = a.query.weight.detach().float() * scale, a.query.bias.detach().float() * scale
            return wq, bq

        a = blk.attn
        wq, bq = qkv(a)
        e = {
            "wqkv": torch.cat([wq, a.key.weight.detach().float(), a.value.weight.detach().float()], 0).to(dev, t16).contiguous(),
            "bqkv": torch.cat([bq, torch.zeros_like(bq), a.value.bias.detach().float()], 0).to(dev).contiguous(),
            "wo": a.out.weight.detach().to(dev, t16).contiguous(), "bo": _f32(a.out.bias, dev),
            "w1": blk.mlp[0].weight.detach().to(dev, t16).contiguous(), "b1": _f32(blk.mlp[0].bias, dev),
            "w2": blk.mlp[2].weight.detach().to(dev, t16).contiguous(), "b2": _f32(blk.mlp[2].bias, dev),
            "ln1": _ln(blk.attn_ln, dev), "ln3": _ln(blk.mlp_ln, dev),
        }
        if cross:
            c = blk.cross_attn
            wq, bq = qkv(c)
            e.update({
                "cwq": wq.to(dev, t16).contiguous(), "cbq": bq.to(dev).contiguous(),
                # K and V of the encoder output as the two groups of one launch: weights [2, d, d], biases [2 d] (key has none)
                "cwkv": torch.stack([c.key.weight.detach().float(), c.value.weight.detach().float()], 0).to(dev, t16).contiguous(),
                "cbkv": torch.cat([torch.zeros_like(bq), c.value.bias.detach().float()], 0).to(dev).contiguous(),
                "cwo": c.out.weight.detach().to(dev, t16).contiguous(), "cbo": _f32(c.out.bias, dev),
                "ln2": _ln(blk.cross_attn_ln, dev),
            })
        return e

    def pack(self, dev):
        t16 = ops.torch_dtype(self.dtype)
        enc, dec, d = self.encoder, self.decoder, self.dims.n_audio_state
        w1 = torch.zeros(d, MEL_LD, 3)
        w1[:, :80] = enc.conv1.weight.detach().float().cpu()
        self._set_packed(dev, {
            "c1w": pack_conv1d(w1).to(dev, t16).contiguous(), "c1b": _f32(enc.conv1.bias, dev),
            "c2w": pack_conv1d(enc.conv2.weight.detach().float()).to(dev, t16).contiguous(), "c2b": _f32(enc.conv2.bias, dev),
            "pos": _f32(enc.positional_embedding, dev),
            "enc": [self._pack_block(b, dev, t16, False) for b in enc.blocks],
            "ln_post": _ln(enc.ln_post, dev),
            "dec": [self._pack_block(b, dev, t16, True) for b in dec.blocks],
            "ln": _ln(dec.ln, dev),
            "emb": dec.token_embedding.weight.detach().to(dev, t16).contiguous(),
            "dpos": _f32(dec.positional_embedding, dev),
        })

    # ---- encoder ---------------------------------------------------------------------------------------------------------------
    def encode_features(self, feats, B):
        """feats: 16-bit rows [B * 3000, 128] (LogMel.features) -> (fp32 [B * 1500, d], its 16-bit copy): ln_post's output."""
        dev = feats.device
        P, dt, dm = self.packed(dev), self.dtype, self.dims
        t16 = ops.torch_dtype(dt)
        d, H, F, T = dm.n_audio_state, dm.n_audio_head, 4 * dm.n_audio_state, N_CTX_AUDIO
        M = B * T
        h1 = torch.empty(B * N_FRAMES, d, device=dev, dtype=t16)
        ops.tapgemm(feats, P["c1w"], h1, M=B * N_FRAMES, N=d, Cin=MEL_LD, ntaps=3, lda=MEL_LD, ldc=d, mode=MODE_CONV1D, T_out=N_FRAMES,
                    T_in=N_FRAMES, stride=1, dil=1, off=-1, bias=P["c1b"], act=ACT_GELU, dtype=dt)
        # x = GELU(conv2(h1)) + positions: the table, repeated per clip, is the residual operand added behind the activation
        pos = self.derived(("pos", B), lambda: P["pos"].repeat(B, 1).contiguous())
        x = torch.empty(M, d, device=dev, dtype=torch.float32)
        ops.tapgemm(h1, P["c2w"], x, M=M, N=d, Cin=d, ntaps=3, lda=d, ldc=d, mode=MODE_CONV1D, T_out=T, T_in=N_FRAMES, stride=2,
                    dil=1, off=-1, bias=P["c2b"], act=ACT_GELU, R=pos, ldr=d, flags=F_RES_POST, dtype=dt)
        h = torch.empty(M, d, device=dev, dtype=t16)
        qkv = torch.empty(M, 3 * d, device=dev, dtype=t16)
        att = torch.empty(M, d, device=dev, dtype=t16)
        f = torch.empty(M, F, device=dev, dtype=t16)
        layers = P["enc"]
        first = layers[0]["ln1"] if layers else P["ln_post"]
        out32 = torch.empty(M, d, device=dev, dtype=torch.float32)
        out16 = torch.empty(M, d, device=dev, dtype=t16)
        if not layers:
            ops.layernorm(x, first[0], first[1], 1e-5, out32, M=M, C=d, y2=out16, ldy2=d, dtype=dt)
            return out32, out16
        ops.layernorm(x, first[0], first[1], 1e-5, h, M=M, C=d, dtype=dt)
        for li, e in enumerate(layers):
            ops.tapgemm(h, e["wqkv"], qkv, M=M, N=3 * d, Cin=d, bias=e["bqkv"], dtype=dt)
            ops.attention(qkv, att, B=B, T=T, H=H, dtype=dt)
            ops.residual_linear(att, e["wo"], e["bo"], x, M=M, N=d, K=d, dtype=dt, cache=e, key="wo", ln=(e["ln3"][0], e["ln3"][1], 1e-5, h))
            ops.tapgemm(h, e["w1"], f, M=M, N=F, Cin=d, bias=e["b1"], act=ACT_GELU, dtype=dt)
            if li + 1 < len(layers):
                nxt = layers[li + 1]["ln1"]
                ops.residual_linear(f, e["w2"], e["b2"], x, M=M, N=d, K=F, dtype=dt, cache=e, key="w2", ln=(nxt[0], nxt[1], 1e-5, h))
            else:
                ops.residual_linear(f, e["w2"], e["b2"], x, M=M, N=d, K=F, dtype=dt, cache=e, key="w2")
                ops.layernorm(x, P["ln_post"][0], P["ln_post"][1], 1e-5, out32, M=M, C=d, y2=out16, ldy2=d, dtype=dt)
        return out32, out16

    def encode(self, wav, n_samples=None):
        """wav: device tensor [B, S] fp32 or int16 -> (fp32 [B, 1500, d], 16-bit copy)."""
        B = wav.shape[0]
        o32, o16 = self.encode_features(self.logmel.features(wav, n_samples, dtype=self.dtype), B)
        return o32.view(B, N_CTX_AUDIO, -1), o16.view(B, N_CTX_AUDIO, -1)

    # ---- decoder ---------------------------------------------------------------------------------------------------------------
    def cross_caches(self, enc16, B):
        """Per decoder layer the cross-attention K and V of the encoder output, 16-bit [2, B, 1500, d] (one grouped GEMM each)."""
        dev = enc16.device
        P, dt, d = self.packed(dev), self.dtype, self.dims.n_text_state
        M = B * N_CTX_AUDIO
        out = []
        for e in P["dec"]:
            kv = torch.empty(2, B, N_CTX_AUDIO, d, device=dev, dtype=ops.torch_dtype(dt))
            ops.tapgemm(enc16, e["cwkv"], kv, M=M, N=d, Cin=d, lda=d, ldc=d, bias=e["cbkv"], groups=2, a_gstride=0, c_gstride=M * d,
                        w_gstride=d * d, dtype=dt)
            out.append(kv)
        return out

    def new_state(self, B, dev, n_cols=None):
        """The buffers of a decode of B clips: fp32 residual row per clip, self caches, bookkeeping and the device scalars."""
        dm, t16 = self.dims, ops.torch_dtype(self.dtype)
        d, n_ctx, L = dm.n_text_state, dm.n_text_ctx, dm.n_text_layer
        z = dict(device=dev)
        return {
            "B": B, "x": torch.zeros(B, d, dtype=torch.float32, **z), "h": torch.empty(B, d, dtype=t16, **z),
            "qkv": torch.empty(B, 3 * d, dtype=t16, **z), "att": torch.empty(B, d, dtype=t16, **z), "qc": torch.empty(B, d, dtype=t16, **z),
            "f": torch.empty(B, 4 * d, dtype=t16, **z),
            "self": [torch.zeros(2, B, n_ctx, d, dtype=t16, **z) for _ in range(L)], "cross": None,
            "pos": torch.zeros(1, dtype=torch.int32, **z), "n_active": torch.zeros(1, dtype=torch.int32, **z),
            "token": torch.zeros(B, dtype=torch.int32, **z), "logprob": torch.zeros(B, dtype=torch.float32, **z),
            "tokens": torch.zeros(B, n_cols or n_ctx, dtype=torch.int32, **z), "sum_logprob": torch.zeros(B, dtype=torch.float32, **z),
            "lengths": torch.zeros(B, dtype=torch.int32, **z), "done": torch.zeros(B, dtype=torch.uint8, **z),
            "work": torch.empty(ops.vocab_argmax_workspace(dm.n_vocab, B), dtype=torch.uint8, **z),
        }

    def step_layers(self, S):
        """The decoder blocks at the device position for the rows S["x"] (appends to the self caches); leaves decoder.ln's output,
        the operand of the output layer, in S["h"]."""
        dev = S["x"].device
        P, dt, dm = self.packed(dev), self.dtype, self.dims
        B, d, H, F = S["B"], dm.n_text_state, dm.n_text_head, 4 * dm.n_text_state
        x, h, qkv, att, qc, f = S["x"], S["h"], S["qkv"], S["att"], S["qc"], S["f"]
        layers = P["dec"]
        first = layers[0]["ln1"] if layers else P["ln"]
        ops.layernorm(x, first[0], first[1], 1e-5, h, M=B, C=d, dtype=dt)
        for li, e in enumerate(layers):
            ops.tapgemm(h, e["wqkv"], qkv, M=B, N=3 * d, Cin=d, bias=e["bqkv"], dtype=dt)
            kc, vc = S["self"][li][0], S["self"][li][1]
            ops.kv_attention(qkv, kc, vc, att, B=B, H=H, pos=S["pos"], k_new=qkv[:, d:2 * d], v_new=qkv[:, 2 * d:], ldq=3 * d,
                             ld_new=3 * d, dtype=dt)
            ops.residual_linear(att, e["wo"], e["bo"], x, M=B, N=d, K=d, dtype=dt, cache=e, key="wo", ln=(e["ln2"][0], e["ln2"][1], 1e-5, h))
            ops.tapgemm(h, e["cwq"], qc, M=B, N=d, Cin=d, bias=e["cbq"], dtype=dt)
            ck, cv = S["cross"][li][0], S["cross"][li][1]
            ops.kv_attention(qc, ck, cv, att, B=B, H=H, n_valid=N_CTX_AUDIO, dtype=dt)
            ops.residual_linear(att, e["cwo"], e["cbo"], x, M=B, N=d, K=d, dtype=dt, cache=e, key="cwo", ln=(e["ln3"][0], e["ln3"][1], 1e-5, h))
            ops.tapgemm(h, e["w1"], f, M=B, N=F, Cin=d, bias=e["b1"], act=ACT_GELU, dtype=dt)
            nxt = layers[li + 1]["ln1"] if li + 1 < len(layers) else P["ln"]
            ops.residual_linear(f, e["w2"], e["b2"], x, M=B, N=d, K=F, dtype=dt, cache=e, key="w2", ln=(nxt[0], nxt[1], 1e-5, h))

    def step_choose(self, S, suppress, begin_suppress, first_step, logits=None):
        P, dm = self.packed(S["x"].device), self.dims
        ops.vocab_argmax(S["h"], P["emb"], S["work"], S["token"], S["logprob"], B=S["B"], V=dm.n_vocab, d=dm.n_text_state,
                         suppress=suppress, begin_suppress=begin_suppress, step=S["pos"], first_step=first_step, logits=logits,
                         dtype=self.dtype)

    def step_advance(self, S, eot, book=None):
        """Books S["token"] and writes the next input row; `book` replaces (tokens, sum_logprob, lengths, done) while the forced
        prefix is fed, whose tokens are not results."""
        P, dm = self.packed(S["x"].device), self.dims
        tokens, sums, lengths, done = book if book is not None else (S["tokens"], S["sum_logprob"], S["lengths"], S["done"])
        ops.whisper_advance(S["token"], S["logprob"], tokens, sums, lengths, done, P["emb"], P["dpos"], S["x"], S["pos"], S["n_active"],
                            B=S["B"], V=dm.n_vocab, d=dm.n_text_state, eot=eot, dtype=self.dtype)

    def start(self, S, first_token):
        """Position 0: the first forced token's row in the residual stream, cleared bookkeeping."""
        P = self.packed(S["x"].device)
        S["x"].copy_((P["emb"][first_token].float() + P["dpos"][0]).expand_as(S["x"]))
        for k in ("pos", "n_active", "tokens", "sum_logprob", "lengths", "done", "token", "logprob"):
            S[k].zero_()

    def teacher_forced_logits(self, enc16, tokens):
        """Raw fp32 logits [B, n, V] of the decoder fed with tokens int [B, n] (row i: the distribution of token i + 1); the test
        and scoring path: every step is launched plainly and its logits are dumped."""
        B, n = tokens.shape
        dev = enc16.device
        S = self.new_state(B, dev)
        S["cross"] = self.cross_caches(enc16.reshape(B * N_CTX_AUDIO, -1), B)
        P = self.packed(dev)
        V = self.dims.n_vocab
        out = torch.empty(B, n, V, device=dev, dtype=torch.float32)
        step_logits = torch.empty(B, V, device=dev, dtype=torch.float32)
        book = (torch.zeros_like(S["tokens"]), torch.zeros_like(S["sum_logprob"]), torch.zeros_like(S["lengths"]), torch.zeros_like(S["done"]))
        tok = tokens.to(dev, torch.int32)
        S["x"].copy_(P["emb"][tok[:, 0].long()].float() + P["dpos"][0])
        for i in range(n):
            self.step_layers(S)
            self.step_choose(S, None, None, 0, logits=step_logits)
            out[:, i] = step_logits
            S["token"].copy_(tok[:, min(i + 1, n - 1)])
            book[3].zero_()
            self.step_advance(S, eot=0, book=book)
        return out


def load_whisper(path, dtype=ops.F16):
    """openai-whisper's checkpoint file (`dims` + `model_state_dict`), or a HuggingFace state dict saved with torch.save (its `dims`
    are read off the tensors' shapes)."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(ck, dict) and "model_state_dict" in ck:
        dims, sd = WhisperDims(**ck["dims"]), ck["model_state_dict"]
    else:
        sd = hf_to_openai(ck.get("state_dict", ck) if isinstance(ck, dict) else ck)
        dims = dims_of(sd)
    model = Whisper(dims, dtype=dtype)
    model.load_state_dict({k: v for k, v in sd.items()}, strict=True)
    return model.eval()


def dims_of(sd):
    """WhisperDims read off an openai-layout state dict (heads are 64 wide at every size)."""
    d = sd["encoder.conv1.weight"].shape[0]
    dt = sd["decoder.token_embedding.weight"].shape[1]
    n = lambda p: 1 + max(int(k.split(".")[2]) for k in sd if k.startswith(p + ".blocks."))
    return WhisperDims(n_mels=sd["encoder.conv1.weight"].shape[1], n_audio_ctx=sd["encoder.positional_embedding"].shape[0],
                       n_audio_state=d, n_audio_head=d // 64, n_audio_layer=n("encoder"),
                       n_vocab=sd["decoder.token_embedding.weight"].shape[0], n_text_ctx=sd["decoder.positional_embedding"].shape[0],
                       n_text_state=dt, n_text_head=dt // 64, n_text_layer=n("decoder"))


def save_openai_checkpoint(model, path):
    """Writes `model` as an openai-whisper checkpoint file."""
    torch.save({"dims": asdict(model.dims), "model_state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, path)


class WhisperASR:
    """Greedy transcription, mirroring the reference's `asr.run` (`server.py:341`).  `tokens(wavs, n_samples)` returns the sampled
    ids, per-clip lengths and mean log-probabilities; `run(wavs)` returns the texts.  One decoder step is a fixed launch sequence;
    with graph=True it is captured once per batch size (a single stream, no parallel branches) and replayed, and re-captured when
    the model's packed weights change (packing.state_epoch).  The host reads the count of unfinished clips every `poll` steps."""

    def __init__(self, model, config: WhisperDecodeConfig, vocab=None, dtype=None, graph=True, poll=8):
        if dtype is not None and dtype != model.dtype:
            raise ValueError("dtype differs from the model's: build the model with it (Whisper(dims, dtype=...))")
        self.model, self.config, self.graph, self.poll = model, config, graph, max(1, int(poll))
        self.detok = vocab if isinstance(vocab, Detokenizer) or vocab is None else Detokenizer.load(vocab)
        V = model.dims.n_vocab
        for name, ids in (("sot_sequence", config.sot_sequence), ("eot", (config.eot,)), ("suppress", config.suppress),
                          ("begin_suppress", config.begin_suppress)):
            if any(not 0 <= int(i) < V for i in ids):
                raise ValueError(f"{name}: an id is outside the vocabulary of {V}")
        if not config.sot_sequence:
            raise ValueError("sot_sequence is empty")
        self._states = {}

    def _masks(self, dev):
        V = self.model.dims.n_vocab
        s, b = torch.zeros(V, dtype=torch.uint8), torch.zeros(V, dtype=torch.uint8)
        s[list(self.config.suppress)] = 1
        b[list(self.config.begin_suppress)] = 1
        return s.to(dev), b.to(dev)

    def _state(self, B, dev):
        epoch = None
        key = (B, str(dev))
        st = self._states.get(key)
        if st is None:
            S = self.model.new_state(B, dev)
            S["cross"] = [torch.empty(2, B, N_CTX_AUDIO, self.model.dims.n_text_state, device=dev, dtype=ops.torch_dtype(self.model.dtype))
                          for _ in range(self.model.dims.n_text_layer)]
            st = {"S": S, "masks": self._masks(dev), "graph": None, "epoch": epoch,
                  "book": (torch.zeros_like(S["tokens"]), torch.zeros_like(S["sum_logprob"]), torch.zeros_like(S["lengths"]),
                           torch.zeros_like(S["done"]))}
            self._states[key] = st
        return st

    def _step(self, st):
        m, S, P = self.model, st["S"], len(self.config.sot_sequence)
        m.step_layers(S)
        m.step_choose(S, st["masks"][0], st["masks"][1], P - 1)
        m.step_advance(S, self.config.eot)

    def _replay(self, st):
        if not self.graph:
            self._step(st)
            return
        m = self.model
        m.packed(st["S"]["x"].device)
        epoch = state_epoch(m)
        if st["graph"] is None or st["epoch"] != epoch:
            S = st["S"]
            keep = {k: S[k].clone() for k in ("x", "pos", "n_active", "token", "logprob", "tokens", "sum_logprob", "lengths", "done")}
            keep_self = [c.clone() for c in S["self"]]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step(st)                           # warm-up: split-K repacks and allocator growth happen outside the capture
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._step(st)
            for k, v in keep.items():                    # the warm-up and the capture's dry run moved the state: put it back
                S[k].copy_(v)
            for c, v in zip(S["self"], keep_self):
                c.copy_(v)
            st["graph"], st["epoch"] = g, state_epoch(m)
        st["graph"].replay()

    @torch.no_grad()
    def tokens(self, wavs, n_samples=None):
        """wavs: device tensor [B, S <= 480 000] fp32 or int16 (n_samples: int32 device tensor [B], host sequence or None).
        Returns (ids: list of B lists of sampled ids without eot, lengths: int32 tensor [B], mean log-probability fp32 tensor [B] =
        sum over the sampled ids (eot's included) / (length + 1), openai-whisper's avg_logprob)."""
        m, cfg = self.model, self.config
        dev, B = wavs.device, wavs.shape[0]
        if n_samples is not None and not isinstance(n_samples, torch.Tensor):
            if any(int(n) > wavs.shape[1] or int(n) < 0 for n in n_samples):
                raise ValueError("n_samples: a length is outside the buffer")
            n_samples = torch.tensor([int(n) for n in n_samples], dtype=torch.int32, device=dev)
        _, enc16 = m.encode(wavs, n_samples)
        st = self._state(B, dev)
        S = st["S"]
        for dst, src in zip(S["cross"], m.cross_caches(enc16.reshape(B * N_CTX_AUDIO, -1), B)):
            dst.copy_(src)
        m.start(S, int(cfg.sot_sequence[0]))
        P = len(cfg.sot_sequence)
        for i in range(1, P):                            # the forced prefix: fill the caches, feed the next forced token
            m.step_layers(S)
            S["token"].fill_(int(cfg.sot_sequence[i]))
            st["book"][3].zero_()
            m.step_advance(S, cfg.eot, book=st["book"])
        n_max = max(0, min(int(cfg.max_new_tokens), m.dims.n_text_ctx - P))
        steps = 0
        while steps < n_max:
            self._replay(st)
            steps += 1
            if steps % self.poll == 0 and int(S["n_active"].item()) == 0:
                break
        self.steps_run = steps
        toks, lengths = S["tokens"][:, P - 1:P - 1 + steps].cpu(), S["lengths"].clone()
        ln = lengths.cpu().tolist()
        mean_lp = S["sum_logprob"] / (lengths.float() + 1.0)
        return [toks[b, :ln[b]].tolist() for b in range(B)], lengths, mean_lp

    def run(self, wavs, n_samples=None):
        """Texts of the clips (list[str]); needs the vocabulary (`vocab=`)."""
        if self.detok is None:
            raise ValueError("WhisperASR.run needs a vocabulary (vocab=...); tokens() does not")
        ids, _, _ = self.tokens(wavs, n_samples)
        return [self.detok.decode(i).strip() for i in ids]
