"""The AV-HuBERT lip reader on gfx950: the fine-tuned seq2seq model of the reference tree (`avhubert/hubert_asr.py:411-507`
AVHubertSeq2Seq, `avhubert/decoder.py:38-243` TransformerDecoder) decoded with fairseq's beam search as `avhubert/infer_s2s.py`
drives it (`conf/s2s_decode.yaml`: beam 50, max_len_a 1.0, lenpen 1.0).  Video only.

`AVHubertSeq2Seq` keeps a fairseq checkpoint's state-dict names (`encoder.w2v_model.*`, `decoder.embed_tokens.weight`,
`decoder.layers.N.self_attn.q_proj.weight`, ..., `decoder.layer_norm.*`, `decoder.embed_out`), so `load_lip_reader` loads the
file as it is.  nn layers only hold parameters; the arithmetic is liblip2speech_hip.so:

  encoder     hubert.AVHubertModel.extract_rows (the stage-1 encoder)
  cross K/V   once per clip and decoder layer: one grouped GEMM into the 16-bit caches [B, T, d], shared by the clip's beams
  step        l2s_layernorm / l2s_tapgemm at M = B * beam rows, l2s_beam_attention against the self caches (addressed through
              the ancestor table: the caches are never reordered) and the cross caches, the output layer as a tap-GEMM with
              fp32 logits, l2s_beam_select, l2s_beam_advance (csrc/s2s_decode.hip).  The position, the live slots and the
              finished clips are device state: a step is a fixed launch sequence, captured once per shape and replayed.

Scope: the pre-LN decoder the fine-tuning configs build (`decoder_normalize_before: true`), sinusoidal or
learned positions, shared or separate output embedding; no audio input, LM fusion, prefix tokens, constraints, n-gram blocking or
sampling; 16-bit operands (F16 / BF16) with fp32 accumulation, an fp32 residual stream and fp32 scores."""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .hubert import AVHubertConfig, AVHubertModel, HubertEncoderWrapper
from .ops import ACT_RELU
from .packing import PackedState, state_epoch
from .plugin import cfg_get

PAD, EOS, UNK = 1, 2, 3
MAX_ROWS = ops.SPLITK_MAX_M          # B * beam of a sub-batch: one form of the residual GEMMs whatever the batch (ops.splitk_slices)


@dataclass
class DecoderConfig:
    """The decoder fields of AVHubertSeq2SeqConfig (hubert_asr.py:213-286); defaults = conf/finetune/large_vox_433h.yaml."""
    decoder_embed_dim: int = 1024
    decoder_ffn_embed_dim: int = 4096
    decoder_layers: int = 9
    decoder_attention_heads: int = 8
    decoder_normalize_before: bool = True
    decoder_learned_pos: bool = False
    no_scale_embedding: bool = True
    share_decoder_input_output_embed: bool = True
    max_target_positions: int = 2048
    encoder_embed_dim: int = 1024            # width of the rows the cross-attention K/V projections take

    @classmethod
    def base(cls, **kw):
        return cls(decoder_embed_dim=768, decoder_ffn_embed_dim=3072, decoder_layers=6, decoder_attention_heads=4,
                   encoder_embed_dim=768, **kw)

    @classmethod
    def from_model_cfg(cls, m, encoder_embed_dim):
        c = cls(encoder_embed_dim=encoder_embed_dim)
        for k, v in list(vars(c).items()):
            if k == "encoder_embed_dim":
                continue
            got = cfg_get(m, k, v)
            if isinstance(v, bool) and isinstance(got, str):
                got = got.strip().lower() in ("true", "1")
            setattr(c, k, type(v)(got))
        return c


@dataclass
class BeamSearchConfig:
    """conf/s2s_decode.yaml's `generation` group (fairseq's defaults for what it leaves out)."""
    beam: int = 50
    max_len_a: float = 1.0
    max_len_b: int = 0
    min_len: int = 1
    lenpen: float = 1.0
    unk_penalty: float = 0.0
    temperature: float = 1.0
    normalize_scores: bool = True
    nbest: int = 1


def sinusoidal_table(n_rows, d, padding_idx=1):
    """fairseq's SinusoidalPositionalEmbedding.get_embedding, float64 rounded once to fp32: row[pos] = [sin(pos inv_k) | cos(pos
    inv_k)], k < d / 2, inv_k = exp(-k ln(10000) / (d / 2 - 1)), the padding row zero.  Token index t of a history reads row
    t + padding_idx + 1 (make_positions; index 0 is the initial eos)."""
    half = d // 2
    inv = np.exp(-np.arange(half, dtype=np.float64) * (math.log(10000.0) / (half - 1)))
    ang = np.arange(n_rows, dtype=np.float64)[:, None] * inv[None, :]
    tab = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    if d % 2:
        tab = np.concatenate([tab, np.zeros((n_rows, 1))], axis=1)
    tab[padding_idx] = 0.0
    return torch.from_numpy(tab.astype(np.float32))


class _Attention(nn.Module):
    def __init__(self, d, kdim):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = nn.Linear(d, d), nn.Linear(kdim, d), nn.Linear(kdim, d), nn.Linear(d, d)


class TransformerDecoderLayer(nn.Module):
    def __init__(self, cfg: DecoderConfig):
        super().__init__()
        d = cfg.decoder_embed_dim
        self.self_attn = _Attention(d, d)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.encoder_attn = _Attention(d, cfg.encoder_embed_dim)
        self.encoder_attn_layer_norm = nn.LayerNorm(d)
        self.fc1, self.fc2 = nn.Linear(d, cfg.decoder_ffn_embed_dim), nn.Linear(cfg.decoder_ffn_embed_dim, d)
        self.final_layer_norm = nn.LayerNorm(d)


class _LearnedPositions(nn.Module):
    def __init__(self, n, d):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n, d))


def _f32(t, dev):
    return t.detach().float().to(dev).contiguous()


def _ln(m, dev):
    return (_f32(m.weight, dev), _f32(m.bias, dev))


class TransformerDecoder(nn.Module, PackedState):
    def __init__(self, cfg: DecoderConfig, n_vocab, dtype=ops.F16):
        super().__init__()
        d, H = cfg.decoder_embed_dim, cfg.decoder_attention_heads
        if d % H or d // H not in (64, 128, 192) or d > 1536:
            raise NotImplementedError(f"decoder width {d} with {H} heads: heads must be 64, 128 or 192 wide and the width at most 1536")
        if not cfg.decoder_normalize_before:
            raise NotImplementedError("decoder_normalize_before = false: the post-LN order is not built (both fine-tuning configs are pre-LN)")
        if (cfg.encoder_embed_dim & 7) or (cfg.decoder_ffn_embed_dim & 7):
            raise NotImplementedError("encoder width and FFN width must be multiples of 8")
        if dtype not in (ops.F16, ops.BF16):
            raise NotImplementedError("the lip reader runs with F16 or BF16 operands")
        self.cfg, self.n_vocab, self.dtype = cfg, n_vocab, dtype
        self.hd = d // H
        self.embed_scale = 1.0 if cfg.no_scale_embedding else math.sqrt(d)
        self.embed_tokens = nn.Embedding(n_vocab, d, padding_idx=PAD)
        self.embed_positions = _LearnedPositions(cfg.max_target_positions + PAD + 1, d) if cfg.decoder_learned_pos else None
        self.layers = nn.ModuleList([TransformerDecoderLayer(cfg) for _ in range(cfg.decoder_layers)])
        self.layer_norm = nn.LayerNorm(d)
        if not cfg.share_decoder_input_output_embed:
            self.embed_out = nn.Parameter(torch.zeros(n_vocab, d))
        self._init_packed()

    def max_positions(self):
        return self.cfg.max_target_positions

    def pack(self, dev):
        t16 = ops.torch_dtype(self.dtype)
        scale = self.hd ** -0.5
        w16 = lambda w: w.detach().float().to(dev, t16).contiguous()
        layers = []
        for L in self.layers:
            a, c = L.self_attn, L.encoder_attn
            layers.append({
                "wqkv": w16(torch.cat([a.q_proj.weight.detach().float() * scale, a.k_proj.weight.detach().float(),
                                       a.v_proj.weight.detach().float()], 0)),
                "bqkv": _f32(torch.cat([a.q_proj.bias.detach().float() * scale, a.k_proj.bias.detach().float(),
                                        a.v_proj.bias.detach().float()], 0), dev),
                "wo": w16(a.out_proj.weight), "bo": _f32(a.out_proj.bias, dev),
                "cwq": w16(c.q_proj.weight.detach().float() * scale), "cbq": _f32(c.q_proj.bias.detach().float() * scale, dev),
                # K and V of the encoder rows as the two groups of one launch: weights [2, d, d_enc], biases [2 d]
                "cwkv": w16(torch.stack([c.k_proj.weight.detach().float(), c.v_proj.weight.detach().float()], 0)),
                "cbkv": _f32(torch.cat([c.k_proj.bias.detach().float(), c.v_proj.bias.detach().float()], 0), dev),
                "cwo": w16(c.out_proj.weight), "cbo": _f32(c.out_proj.bias, dev),
                "w1": w16(L.fc1.weight), "b1": _f32(L.fc1.bias, dev), "w2": w16(L.fc2.weight), "b2": _f32(L.fc2.bias, dev),
                "ln1": _ln(L.self_attn_layer_norm, dev), "ln2": _ln(L.encoder_attn_layer_norm, dev), "ln3": _ln(L.final_layer_norm, dev),
            })
        V, d = self.n_vocab, self.cfg.decoder_embed_dim
        Vp = (V + 7) // 8 * 8                     # the output layer's N: whole 8-row groups, the rows past V are zero
        out = self.embed_tokens.weight if self.cfg.share_decoder_input_output_embed else self.embed_out
        wout = torch.zeros(Vp, d)
        wout[:V] = out.detach().float().cpu()
        self._set_packed(dev, {"dec": layers, "ln": _ln(self.layer_norm, dev), "emb": w16(self.embed_tokens.weight), "wout": w16(wout), "Vp": Vp})

    def position_rows(self, n, dev):
        """fp32 [n, d]: row t = the position embedding of token index t (table row t + 2)."""
        def build():
            if self.embed_positions is not None:
                tab = self.embed_positions.weight.detach().float()
            else:
                tab = sinusoidal_table(n + PAD + 1, self.cfg.decoder_embed_dim, PAD)
            if tab.shape[0] < n + PAD + 1:
                raise ValueError(f"{n} positions asked of a table of {tab.shape[0] - PAD - 1}")
            return tab[PAD + 1:PAD + 1 + n].to(dev).contiguous()
        self.packed(dev)
        return self.derived(("pos", n), build)

    # ---- per-batch device work ---------------------------------------------------------------------------------------------------
    def cross_caches(self, enc16, B, T, out):
        """enc16: 16-bit rows [B * T, d_enc] -> out[layer] = 16-bit [2, B, T, d], K and V of the encoder rows (one grouped GEMM)."""
        P, dt, c = self.packed(enc16.device), self.dtype, self.cfg
        d, de, M = c.decoder_embed_dim, c.encoder_embed_dim, B * T
        for e, kv in zip(P["dec"], out):
            ops.tapgemm(enc16, e["cwkv"], kv, M=M, N=d, Cin=de, lda=de, ldc=d, bias=e["cbkv"], groups=2, a_gstride=0, c_gstride=M * d,
                        w_gstride=d * de, dtype=dt)

    def new_state(self, B, beam, T, L, dev):
        """The buffers of a search over B clips: residual rows, caches, the double-buffered tables and the device scalars."""
        c, t16 = self.cfg, ops.torch_dtype(self.dtype)
        d, F, n, M, K = c.decoder_embed_dim, c.decoder_ffn_embed_dim, c.decoder_layers, B * beam, 2 * beam
        P = self.packed(dev)
        z = dict(device=dev)
        i32, f32 = torch.int32, torch.float32
        return {
            "B": B, "beam": beam, "T": T, "L": L,
            "x": torch.zeros(M, d, dtype=f32, **z), "h": torch.zeros(M, d, dtype=t16, **z), "qkv": torch.zeros(M, 3 * d, dtype=t16, **z),
            "att": torch.zeros(M, d, dtype=t16, **z), "qc": torch.zeros(M, d, dtype=t16, **z), "f": torch.zeros(M, F, dtype=t16, **z),
            "self": [torch.zeros(2, B, beam, L, d, dtype=t16, **z) for _ in range(n)],
            "cross": [torch.zeros(2, B, T, d, dtype=t16, **z) for _ in range(n)],
            "enc16": torch.zeros(B * T, c.encoder_embed_dim, dtype=t16, **z), "enc_lens": torch.zeros(B, dtype=i32, **z),
            "logits": torch.zeros(M, P["Vp"], dtype=f32, **z),
            "cand_score": torch.zeros(B, K, dtype=f32, **z), "cand_slot": torch.zeros(B, K, dtype=i32, **z),
            "cand_token": torch.zeros(B, K, dtype=i32, **z),
            "tokens": torch.zeros(2, B, beam, L, dtype=i32, **z), "anc": torch.zeros(2, B, beam, L, dtype=torch.int16, **z),
            "scores": torch.zeros(2, B, beam, dtype=f32, **z), "n_live": torch.zeros(B, dtype=i32, **z),
            "finished": torch.zeros(B, dtype=torch.uint8, **z), "parents": torch.zeros(B, beam, dtype=i32, **z),
            "hyp_tokens": torch.zeros(B, beam, L, dtype=i32, **z), "hyp_len": torch.zeros(B, beam, dtype=i32, **z),
            "hyp_score": torch.zeros(B, beam, dtype=f32, **z), "nhyp": torch.zeros(B, dtype=i32, **z),
            "out_tokens": torch.zeros(B, beam, L, dtype=i32, **z), "out_len": torch.zeros(B, beam, dtype=i32, **z),
            "out_score": torch.zeros(B, beam, dtype=f32, **z), "max_len": torch.zeros(B, dtype=i32, **z),
            "step": torch.zeros(1, dtype=i32, **z), "n_active": torch.zeros(1, dtype=i32, **z),
            "pos": self.position_rows(L, dev),
        }

    def start(self, S, max_len):
        """Step 0: every slot holds the initial eos; cleared bookkeeping; max_len: host sequence of B per-clip limits."""
        P = self.packed(S["x"].device)
        B, beam = S["B"], S["beam"]
        S["x"].copy_((self.embed_scale * P["emb"][EOS].float() + S["pos"][0]).expand_as(S["x"]))
        for k in ("step", "scores", "finished", "nhyp", "hyp_len", "hyp_score", "out_len", "parents", "anc"):
            S[k].zero_()
        for k in ("tokens", "hyp_tokens", "out_tokens"):
            S[k].fill_(PAD)
        S["tokens"][:, :, :, 0] = EOS
        S["anc"][:, :, :, 0] = torch.arange(beam, device=S["x"].device, dtype=torch.int16).view(1, 1, beam)
        S["out_score"].fill_(float("-inf"))
        S["n_live"].fill_(beam)
        S["n_active"].fill_(B)
        S["max_len"].copy_(torch.tensor([int(m) for m in max_len], dtype=torch.int32))

    def step_layers(self, S):
        """The decoder layers at the device position for the rows S["x"] (appends to the self caches); leaves decoder.layer_norm's
        output, the operand of the output layer, in S["h"]."""
        dev = S["x"].device
        P, dt, c = self.packed(dev), self.dtype, self.cfg
        B, beam, d, H, F = S["B"], S["beam"], c.decoder_embed_dim, c.decoder_attention_heads, c.decoder_ffn_embed_dim
        M = B * beam
        x, h, qkv, att, qc, f = S["x"], S["h"], S["qkv"], S["att"], S["qc"], S["f"]
        live = dict(n_live=S["n_live"], finished=S["finished"])
        layers = P["dec"]
        first = layers[0]["ln1"] if layers else P["ln"]
        ops.layernorm(x, first[0], first[1], 1e-5, h, M=M, C=d, dtype=dt)
        for li, e in enumerate(layers):
            ops.tapgemm(h, e["wqkv"], qkv, M=M, N=3 * d, Cin=d, bias=e["bqkv"], dtype=dt)
            ops.beam_attention(qkv, S["self"][li][0], S["self"][li][1], att, B=B, beam=beam, H=H, hd=self.hd, k_new=qkv[:, d:2 * d],
                               v_new=qkv[:, 2 * d:], anc=S["anc"], step=S["step"], ldq=3 * d, ld_new=3 * d, dtype=dt, **live)
            ops.residual_linear(att, e["wo"], e["bo"], x, M=M, N=d, K=d, dtype=dt, cache=e, key="wo", ln=(e["ln2"][0], e["ln2"][1], 1e-5, h))
            ops.tapgemm(h, e["cwq"], qc, M=M, N=d, Cin=d, bias=e["cbq"], dtype=dt)
            ops.beam_attention(qc, S["cross"][li][0], S["cross"][li][1], att, B=B, beam=beam, H=H, hd=self.hd, enc_lens=S["enc_lens"],
                               dtype=dt, **live)
            ops.residual_linear(att, e["cwo"], e["cbo"], x, M=M, N=d, K=d, dtype=dt, cache=e, key="cwo", ln=(e["ln3"][0], e["ln3"][1], 1e-5, h))
            ops.tapgemm(h, e["w1"], f, M=M, N=F, Cin=d, bias=e["b1"], act=ACT_RELU, dtype=dt)
            nxt = layers[li + 1]["ln1"] if li + 1 < len(layers) else P["ln"]
            ops.residual_linear(f, e["w2"], e["b2"], x, M=M, N=d, K=F, dtype=dt, cache=e, key="w2", ln=(nxt[0], nxt[1], 1e-5, h))

    def step_logits(self, S):
        P, d = self.packed(S["x"].device), self.cfg.decoder_embed_dim
        ops.tapgemm(S["h"], P["wout"], S["logits"], M=S["B"] * S["beam"], N=P["Vp"], Cin=d, dtype=self.dtype)

    def step_search(self, S, cfg: BeamSearchConfig):
        P = self.packed(S["x"].device)
        B, beam, V = S["B"], S["beam"], self.n_vocab
        ops.beam_select(S["logits"], S["scores"], S["step"], S["max_len"], S["cand_score"], S["cand_slot"], S["cand_token"], B=B, beam=beam,
                        V=V, pad=PAD, unk=UNK, eos=EOS, min_len=cfg.min_len, temperature=cfg.temperature, unk_penalty=cfg.unk_penalty,
                        n_live=S["n_live"], finished=S["finished"], ldl=P["Vp"])
        ops.beam_advance(S["cand_score"], S["cand_slot"], S["cand_token"], S["tokens"], S["anc"], S["scores"], S["n_live"], S["finished"],
                         S["parents"], S["hyp_tokens"], S["hyp_len"], S["hyp_score"], S["nhyp"], S["out_tokens"], S["out_len"],
                         S["out_score"], S["max_len"], P["emb"], S["pos"], S["x"], S["step"], S["n_active"], B=B, beam=beam, V=V,
                         d=self.cfg.decoder_embed_dim, eos=EOS, pad=PAD, embed_scale=self.embed_scale, lenpen=cfg.lenpen,
                         normalize_scores=cfg.normalize_scores, dtype=self.dtype)

    def step(self, S, cfg):
        self.step_layers(S)
        self.step_logits(S)
        self.step_search(S, cfg)


class AVHubertSeq2Seq(nn.Module, PackedState):
    """hubert_asr.py:411-507: the encoder wrapper and the decoder under a fairseq checkpoint's names.  Its packed state is that of
    its two halves: `pack(dev)` packs both, and loading a state dict into it invalidates both (packing.PackedState)."""

    def __init__(self, w2v_cfg: AVHubertConfig = None, cfg: DecoderConfig = None, n_vocab=1004, dtype=ops.F16):
        super().__init__()
        w2v_cfg = w2v_cfg or AVHubertConfig()
        cfg = cfg or DecoderConfig(encoder_embed_dim=w2v_cfg.encoder_embed_dim)
        if cfg.encoder_embed_dim != w2v_cfg.encoder_embed_dim:
            raise ValueError("the decoder's cross-attention takes the encoder's width")
        self.cfg, self.dtype = cfg, dtype
        self.encoder = HubertEncoderWrapper(AVHubertModel(w2v_cfg, dtype=dtype))
        self.decoder = TransformerDecoder(cfg, n_vocab, dtype=dtype)
        self._init_packed()

    def pack(self, dev):
        self.encoder.w2v_model.pack(dev)
        self.decoder.pack(dev)
        self._set_packed(dev, {})

    def encode_rows(self, video, padding_mask=None):
        """video [B, 1, T, 88, 88] -> (fp32 rows [B * T, d_enc], lens int32 [B], B, T)."""
        if isinstance(video, dict):
            if video.get("audio") is not None:
                raise NotImplementedError("audio input is outside the lip reader (video only)")
            video = video["video"]
        return self.encoder.w2v_model.extract_rows(video, padding_mask)


def read_seq2seq_checkpoint(path, dtype, accept):
    """The body of the checkpoint loaders: a fairseq-layout file -> (AVHubertSeq2Seq in eval mode, cfg.task or None, the model's
    state-dict keys the file lacks).  `accept(modalities)` sees cfg.task.modalities (a list of names, or None when the file has
    none) before anything is built and raises to refuse the file; a file may lack only `mask_emb` and the audio sub-model."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    m = cfg_get(ck.get("cfg"), "model", None) if ck.get("cfg") is not None else ck.get("args")
    if m is None:
        raise ValueError(f"{path}: neither cfg.model nor args")
    task = cfg_get(ck.get("cfg"), "task", None)
    mods = cfg_get(task, "modalities", None)
    accept(None if mods is None else [str(x) for x in mods])
    w2v = AVHubertConfig.from_w2v_args(cfg_get(m, "w2v_args", None))
    sd = ck["model"]
    cfg = DecoderConfig.from_model_cfg(m, w2v.encoder_embed_dim)
    model = AVHubertSeq2Seq(w2v, cfg, n_vocab=sd["decoder.embed_tokens.weight"].shape[0], dtype=dtype)
    skip = ("decoder.embed_positions._float_tensor", "decoder.version")
    own = model.state_dict()
    sd = {k: v for k, v in sd.items() if k not in skip and not (k.startswith("decoder.embed_positions") and not cfg.decoder_learned_pos)}
    missing = [k for k in own if k not in sd and "mask_emb" not in k and "feature_extractor_audio" not in k]
    unexpected = [k for k in sd if k not in own]
    if missing or unexpected:
        raise ValueError(f"{path}: missing {missing[:5]}, unexpected {unexpected[:5]}")
    model.load_state_dict(sd, strict=False)
    return model.eval(), task, [k for k in own if k not in sd]


def load_lip_reader(path, dtype=ops.F16):
    """A fine-tuned AV-HuBERT seq2seq checkpoint (fairseq layout: `cfg.model` or old-style `args`, `model`) -> AVHubertSeq2Seq in
    eval mode.  The encoder is sized from the pre-training config the checkpoint embeds (`w2v_args`), the decoder from the
    fine-tuning fields, the vocabulary from `decoder.embed_tokens.weight`.  Sinusoidal position buffers are ignored."""
    def accept(mods):
        if mods is not None and mods != ["video"]:
            raise NotImplementedError(f"modalities = {mods}: the lip reader takes video only")
    return read_seq2seq_checkpoint(path, dtype, accept)[0]


def save_checkpoint(model, path, w2v_cfg, modalities=("video",), task=None):
    """Writes `model` in the fairseq layout load_lip_reader reads (cfg.model as plain dicts).  modalities: cfg.task.modalities;
    task: further cfg.task fields (stack_order_audio, normalize) for av_recogniser.load_speech_recogniser."""
    from dataclasses import asdict
    m = {k: v for k, v in asdict(model.cfg).items() if k != "encoder_embed_dim"}
    m["w2v_args"] = {"model": asdict(w2v_cfg)}
    torch.save({"cfg": {"model": m, "task": {"modalities": list(modalities), **(task or {})}},
                "model": {k: v.detach().cpu() for k, v in model.state_dict().items()}}, path)


class LipReader:
    """Beam search over mouth crops, mirroring `avhubert/infer_s2s.py` (`task.inference_step` -> SequenceGenerator.generate).
    `generate(video, padding_mask)` returns per clip a list of {"tokens", "score"}, best first (`nbest` of them);
    `transcribe` the best texts.  One step is a fixed launch sequence; with graph=True it is captured once per (sub-batch size,
    beam, padded lengths) and replayed, and re-captured when the model's packed weights change.  The host reads the count of
    unfinished clips every `poll` steps.

    Length limit: max_len[b] = min(int(max_len_a * frames_b + max_len_b), max_target_positions - 1) from the clip's OWN frame
    count - fairseq's value for the clip decoded alone (it uses the padded batch length, so its result depends on the batch).

    Memory: a sub-batch of n clips holds n * layers * 4 * d * (beam * L + T) bytes of self and cross caches (L = the largest
    max_len + 2 rounded up to a multiple of 32, T = the padded frame count rounded up to a multiple of 64: coarse buckets, so
    batches of similar lengths share a shape) and n * beam * 4 * V bytes of logits; clips are taken in order into sub-batches of
    at most max(1, min(cache_bytes // that, 512 // beam)) clips (default cache_bytes 8 GiB).  The reader holds ONE state - the
    buffers and the captured step of the most recent shape (n, T, L); a sub-batch of another shape frees it first - so what it
    holds never exceeds one sub-batch: `held_bytes()` <= `state_bytes(n, T, L)` = n * clip_bytes + the 16-bit copy of the encoder
    rows (2 n T d_enc) + the step's activations and tables (n * beam * (16 d + 2 ffn + 20 L + 128)) + the position rows (4 L d)."""

    def __init__(self, model: AVHubertSeq2Seq, dictionary=None, config: BeamSearchConfig = None, graph=True, poll=8, cache_bytes=8 << 30):
        self.model, self.dictionary, self.config = model, dictionary, config or BeamSearchConfig()
        self.graph, self.poll, self.cache_bytes = graph, max(1, int(poll)), int(cache_bytes)
        c, V = self.config, model.decoder.n_vocab
        if not 1 <= c.beam <= 64:
            raise ValueError(f"beam = {c.beam}: 1 .. 64")
        if V < 2 * c.beam + 2:
            raise ValueError(f"a vocabulary of {V} cannot fill 2 * beam = {2 * c.beam} candidates (V >= 2 beam + 2)")
        if ops.beam_select_workspace(V, c.beam) == 0:
            raise ValueError(f"vocabulary of {V} with beam {c.beam}: outside l2s_beam_select (V <= 8192)")
        if not c.temperature > 0:
            raise ValueError("temperature must be positive")
        if dictionary is not None and len(dictionary) != V:
            raise ValueError(f"the dictionary has {len(dictionary)} symbols, the model {V}")
        self._states = {}
        self.steps_run = 0

    # ---- sizes -------------------------------------------------------------------------------------------------------------------
    def max_len(self, frames):
        c = self.config
        return min(int(c.max_len_a * int(frames) + c.max_len_b), self.model.decoder.max_positions() - 1)

    def clip_bytes(self, T, L):
        d, c = self.model.decoder, self.model.decoder.cfg
        return c.decoder_layers * 4 * c.decoder_embed_dim * (self.config.beam * L + T) + self.config.beam * 4 * d.n_vocab

    def state_bytes(self, n, T, L):
        """Upper bound of the bytes a state of n clips holds (see the class docstring)."""
        c = self.model.decoder.cfg
        M, d = n * self.config.beam, c.decoder_embed_dim
        return (n * self.clip_bytes(T, L) + 2 * n * T * c.encoder_embed_dim + M * (16 * d + 2 * c.decoder_ffn_embed_dim + 20 * L + 128)
                + 4 * L * d + 64 * n + 256)

    def sub_batch(self, T, L):
        return max(1, min(self.cache_bytes // self.clip_bytes(T, L), MAX_ROWS // self.config.beam))

    # ---- the step ----------------------------------------------------------------------------------------------------------------
    def _state(self, B, T, L, dev):
        key = (B, self.config.beam, T, L, str(dev))
        st = self._states.get(key)
        if st is None:
            self._states.clear()                     # one state at a time: the previous shape's buffers and graph go first
            st = {"S": self.model.decoder.new_state(B, self.config.beam, T, L, dev), "graph": None, "epoch": None}
            self._states[key] = st
        return st

    @staticmethod
    def padded(T, max_len):
        """(T, L) of the state that serves T encoder rows and a largest length limit max_len: multiples of 64 and of 32."""
        return (int(T) + 63) // 64 * 64, (int(max_len) + 2 + 31) // 32 * 32

    def held_bytes(self):
        """Bytes of device memory in the tensors of the states this reader holds (at most one)."""
        n = 0
        for st in self._states.values():
            for v in st["S"].values():
                for t in (v if isinstance(v, list) else [v]):
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        n += t.numel() * t.element_size()
        return n

    def _replay(self, st):
        dec = self.model.decoder
        if not self.graph:
            dec.step(st["S"], self.config)
            return
        st["graph"].replay()

    def _prepare(self, st):
        """Captures the step when there is no live capture (before the search starts: the warm-up and the capture's dry run move
        the state, which `start` sets afterwards)."""
        dec, S = self.model.decoder, st["S"]
        dec.packed(S["x"].device)
        if not self.graph or (st["graph"] is not None and st["epoch"] == state_epoch(dec)):
            return
        dec.start(S, [1] * S["B"])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            dec.step(S, self.config)                 # warm-up: split-K repacks and allocator growth happen outside the capture
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dec.step(S, self.config)
        st["graph"], st["epoch"] = g, state_epoch(dec)

    @torch.no_grad()
    def generate_from_encoder(self, enc, lens):
        """enc: device tensor [B, T, d_enc] (fp32 or the model's 16-bit type), lens: host sequence of B valid row counts.
        Returns per clip a list of {"tokens": list[int] ending in eos, "score": float}, best first, at most `nbest`."""
        dec, c = self.model.decoder, self.config
        dev, (B, T, de) = enc.device, enc.shape
        lens = [int(n) for n in lens]
        if len(lens) != B or any(n < 0 or n > T for n in lens):
            raise ValueError("lens: one valid row count per clip, within the padded length")
        if de != dec.cfg.encoder_embed_dim:
            raise ValueError(f"encoder rows are {de} wide, the decoder expects {dec.cfg.encoder_embed_dim}")
        max_len = [self.max_len(n) for n in lens]
        Tp, L = self.padded(T, max(max_len))
        nb = self.sub_batch(Tp, L)
        out, self.steps_run, self.sub_batches = [], 0, 0
        t16 = ops.torch_dtype(dec.dtype)
        for b0 in range(0, B, nb):
            n = min(nb, B - b0)
            st = self._state(n, Tp, L, dev)
            S = st["S"]
            self._prepare(st)
            dec.start(S, max_len[b0:b0 + n])
            e16 = S["enc16"].view(n, Tp, de)
            e16.zero_()
            part = enc[b0:b0 + n]
            if part.dtype == torch.float32:
                for j in range(n):
                    ops.cast_f32_to_16(part[j].contiguous(), e16[j], T, de, dec.dtype)
            elif part.dtype == t16:
                e16[:, :T].copy_(part)
            else:
                raise ValueError(f"encoder rows must be fp32 or {t16}")
            S["enc_lens"].copy_(torch.tensor(lens[b0:b0 + n], dtype=torch.int32))
            dec.cross_caches(S["enc16"], n, Tp, S["cross"])
            steps, n_max = 0, max(max_len[b0:b0 + n]) + 1
            while steps < n_max:
                self._replay(st)
                steps += 1
                if steps % self.poll == 0 and int(S["n_active"].item()) == 0:
                    break
            self.steps_run = max(self.steps_run, steps)
            self.sub_batches += 1
            toks, ln, sc, nh = S["out_tokens"].cpu(), S["out_len"].cpu(), S["out_score"].cpu(), S["nhyp"].cpu()
            for j in range(n):
                out.append([{"tokens": toks[j, i, :int(ln[j, i])].tolist(), "score": float(sc[j, i])}
                            for i in range(min(int(nh[j]), c.nbest))])
        return out

    @torch.no_grad()
    def generate(self, video, padding_mask=None):
        """video: device tensor [B, 1, T, 88, 88] (or the reference's `source` dict), padding_mask: bool [B, T] or None."""
        rows, lens, B, T = self.model.encode_rows(video, padding_mask)
        return self.generate_from_encoder(rows.view(B, T, -1), lens.cpu().tolist())

    def transcribe(self, video, padding_mask=None):
        if self.dictionary is None:
            raise ValueError("LipReader.transcribe needs a dictionary; generate() does not")
        return [self.dictionary.string(h[0]["tokens"]) if h else "" for h in self.generate(video, padding_mask)]
