"""Speech units from audio on the device: what extract_speech_units.sh:6-11 writes as label/<split>.unt.

The reference runs HuBERT-base (hubert_base_ls960.pt) through fairseq, takes the output of transformer layer 6 and quantises it
with a k-means model (km.bin; avhubert/clustering/dump_km_label.py:26-52, ApplyKmeans).  fairseq is not part of the reference tree;
its HubertModel is restated here as parameter holders with fairseq's state_dict names, and the arithmetic is
liblip2speech_hip.so: l2s_wave_stem (conv layer 0 + GroupNorm + GELU), the CONV1D tap-GEMM (conv layers 1-6), l2s_layernorm,
the post-LN form of hubert.TransformerEncoder and l2s_kmeans_assign.  There is no CPU path.

Labels are a dataset artefact and the reference computes them in fp32, so the default dtype is ops.F32; f16 / bf16 run the
same code on 16-bit operands.  Clips are processed alone whatever their batch mates: the GroupNorm
statistics, the attention keys and the positional convolution of a clip never see another clip's samples or its padding.
"""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import L2SError
from .hubert import TransformerEncoder
from .ops import ACT_GELU, F_DUAL, F_MASK, MODE_CONV1D
from .packing import PackedState

CONV_LAYERS = ((512, 10, 5), (512, 3, 2), (512, 3, 2), (512, 3, 2), (512, 3, 2), (512, 2, 2), (512, 2, 2))   # (dim, k, stride)
MIN_SAMPLES = 400          # the receptive field of one feature frame
IGNORED_KEYS = ("mask_emb", "final_proj.", "label_embs_concat")   # pre-training heads: accepted and ignored


def num_frames(n_samples):
    """Feature frames of a clip: L <- (L - k) // s + 1 through the seven conv layers (68608 -> 214, 39936 -> 124)."""
    n = int(n_samples)
    for _, k, s in CONV_LAYERS:
        n = (n - k) // s + 1 if n >= k else 0
    return n


@dataclass
class HubertConfig:
    """The fields of fairseq's HubertConfig that shape inference; defaults = HuBERT-base (hubert_base_librispeech.yaml)."""
    encoder_layers: int = 12
    encoder_embed_dim: int = 768
    encoder_ffn_embed_dim: int = 3072
    encoder_attention_heads: int = 12
    conv_pos: int = 128
    conv_pos_groups: int = 16
    extractor_mode: str = "default"
    layer_norm_first: bool = False
    normalize: bool = False        # task.normalize: layer-norm of the waveform (the large models)

    @classmethod
    def from_checkpoint_cfg(cls, model_cfg, task_cfg=None):
        """From a checkpoint's embedded `cfg.model` / `cfg.task` groups or its flat old-style `args` (plugin.cfg_get reads
        dataclasses, DictConfigs, Namespaces and dicts alike); absent fields keep the base defaults."""
        from .plugin import cfg_get
        c = cls()
        for k, v in list(vars(c).items()):
            src = task_cfg if k == "normalize" and task_cfg is not None else model_cfg
            got = cfg_get(src, k, v)
            if isinstance(v, bool):
                if isinstance(got, str):
                    if got.strip().lower() not in ("true", "false", "1", "0"):
                        raise ValueError(f"hubert config {k}: cannot read {got!r} as a bool")
                    got = got.strip().lower() in ("true", "1")
                setattr(c, k, bool(got))
            else:
                setattr(c, k, type(v)(got))
        return c


class ConvFeatureExtractionModel(nn.Module, PackedState):
    """fairseq ConvFeatureExtractionModel(mode="default"): parameters conv_layers.{i}.0.weight and conv_layers.0.2.{weight,bias}."""

    def __init__(self, mode="default", dtype=ops.F32):
        super().__init__()
        if mode != "default":
            raise NotImplementedError(f"extractor_mode={mode!r} is not built (HuBERT-base uses 'default': one GroupNorm behind layer 0)")
        self.conv_layers = nn.ModuleList()
        cin = 1
        for i, (dim, k, s) in enumerate(CONV_LAYERS):
            conv = nn.Conv1d(cin, dim, k, stride=s, bias=False)
            if i == 0:
                self.conv_layers.append(nn.Sequential(conv, nn.Dropout(0.0), nn.GroupNorm(dim, dim, eps=1e-5, affine=True), nn.GELU()))
            else:
                self.conv_layers.append(nn.Sequential(conv, nn.Dropout(0.0), nn.GELU()))
            cin = dim
        self.dtype = dtype
        self._init_packed()

    def pack(self, dev):
        t16 = ops.torch_dtype(self.dtype)
        l0 = self.conv_layers[0]
        P = {"w0": l0[0].weight.detach().float().reshape(CONV_LAYERS[0][0], CONV_LAYERS[0][1]).to(dev).contiguous(),
             "g0": l0[2].weight.detach().float().to(dev).contiguous(), "b0": l0[2].bias.detach().float().to(dev).contiguous(),
             # Conv1d weight [Cout, Cin, k] -> the tap-GEMM's [Cout, k * Cin] (tap-major)
             "w": [L[0].weight.detach().float().permute(0, 2, 1).reshape(L[0].weight.shape[0], -1).to(dev, t16).contiguous()
                   for L in list(self.conv_layers)[1:]]}
        self._set_packed(dev, P)

    def forward_rows(self, wav, n_samples):
        """wav: device [B, S] fp32 in (-1, 1) or int16 PCM; n_samples: host list of clip lengths.  Returns (rows [B*T, 512] of the
        operand type - clip b's rows past num_frames(n_b) are padding, not zeros -, T)."""
        dev = wav.device
        P, dt = self.packed(dev), self.dtype
        t16 = ops.torch_dtype(dt)
        B, S = wav.shape
        C = CONV_LAYERS[0][0]
        ns = torch.tensor(n_samples, dtype=torch.int32).to(dev)
        T = ops.wave_stem_frames(S)
        work = torch.empty(ops.wave_stem_workspace_bytes(B, C), device=dev, dtype=torch.uint8)
        x = torch.empty(B * T, C, device=dev, dtype=t16)
        ops.wave_stem(wav, P["w0"], P["g0"], P["b0"], work, x, B=B, S=S, T_rows=T, C=C, n_samples=ns,
                      ldw=wav.stride(0) if B > 1 else S, eps=1e-5, dtype=dt)
        for (dim, k, s), w in zip(CONV_LAYERS[1:], P["w"]):
            To = (T - k) // s + 1
            y = torch.empty(B * To, dim, device=dev, dtype=t16)
            # a valid output frame reads input frames 2 t .. 2 t + k - 1 of its own clip, all valid: padding never enters
            ops.tapgemm(x, w, y, M=B * To, N=dim, Cin=C, ntaps=k, mode=MODE_CONV1D, T_out=To, T_in=T, stride=s, dil=1, off=0,
                        act=ACT_GELU, dtype=dt)
            x, T = y, To
        return x, T


class HubertModel(nn.Module, PackedState):
    """Inference subset of fairseq's HubertModel: extract_features(source, output_layer) with padding handled per clip."""

    def __init__(self, cfg: HubertConfig = None, dtype=ops.F32):
        super().__init__()
        cfg = cfg or HubertConfig()
        if cfg.normalize:
            raise NotImplementedError("task.normalize=True (layer-norm of the waveform, the large models) is not built")
        if cfg.extractor_mode != "default":
            raise NotImplementedError(f"extractor_mode={cfg.extractor_mode!r} is not built (HuBERT-base uses 'default')")
        if cfg.layer_norm_first:
            raise NotImplementedError("layer_norm_first=True is the large models' layout; the audio path builds HuBERT-base")
        if cfg.encoder_embed_dim != 64 * cfg.encoder_attention_heads:
            raise NotImplementedError("the attention kernel serves 64-wide heads")
        self.cfg = cfg
        self.embed = CONV_LAYERS[-1][0]
        self.feature_extractor = ConvFeatureExtractionModel(cfg.extractor_mode, dtype=dtype)
        self.layer_norm = nn.LayerNorm(self.embed, eps=1e-5)
        self.post_extract_proj = nn.Linear(self.embed, cfg.encoder_embed_dim)
        self.encoder = TransformerEncoder(cfg, dtype=dtype)
        self.dtype = dtype
        self._init_packed()

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.startswith(IGNORED_KEYS)}
        return super().load_state_dict(sd, strict=strict, **kw)

    def pack(self, dev):
        t16 = ops.torch_dtype(self.dtype)
        self._set_packed(dev, {
            "ln": (self.layer_norm.weight.detach().float().to(dev).contiguous(),
                   self.layer_norm.bias.detach().float().to(dev).contiguous()),
            "wpe": self.post_extract_proj.weight.detach().to(dev, t16).contiguous(),
            "bpe": self.post_extract_proj.bias.detach().float().to(dev).contiguous(),
        })

    def extract_rows(self, source, n_samples=None, output_layer=None):
        """source: device [B, S] fp32 or int16.  Returns (fp32 [B*T, d] rows (b, t), lens int32 [B] on the device, host lens, B, T)."""
        if not isinstance(source, torch.Tensor) or not source.is_cuda:
            raise L2SError("extract_features: expected a device tensor (there is no CPU path)")
        if source.dim() != 2:
            raise ValueError("source: [B, S]")
        if source.stride(1) != 1:
            source = source.contiguous()
        B, S = source.shape
        ns = [S] * B if n_samples is None else [int(v) for v in (n_samples.tolist() if hasattr(n_samples, "tolist") else n_samples)]
        if len(ns) != B or any(v < MIN_SAMPLES or v > S for v in ns):
            raise ValueError(f"n_samples: every clip needs {MIN_SAMPLES} <= n <= {S} samples, got {ns}")
        dev = source.device
        P, dt = self.packed(dev), self.dtype
        t16 = ops.torch_dtype(dt)
        d = self.cfg.encoder_embed_dim
        feat, T = self.feature_extractor.forward_rows(source, ns)
        M = B * T
        host_lens = [num_frames(v) for v in ns]
        lens = torch.tensor(host_lens, dtype=torch.int32).to(dev)
        normed = torch.empty(M, self.embed, device=dev, dtype=t16)
        ops.layernorm(feat, P["ln"][0], P["ln"][1], 1e-5, normed, M=M, C=self.embed, dtype=dt)
        x32 = torch.empty(M, d, device=dev, dtype=torch.float32)
        x16 = torch.empty(M, d, device=dev, dtype=t16)
        # post_extract_proj; rows of padded frames are zeroed here (TransformerEncoder: x[padding_mask] = 0)
        ops.tapgemm(normed, P["wpe"], x32, M=M, N=d, Cin=self.embed, bias=P["bpe"], C2=x16, ldc2=d, lens=lens, mask_T=T, mask_mul=1,
                    flags=F_MASK | F_DUAL, slope2=1.0, dtype=dt)
        out = self.encoder.forward_rows(x32, x16, lens, B, T, output_layer=len(self.encoder.layers) if output_layer is None else output_layer)
        return out, lens, host_lens, B, T

    def extract_features(self, source, n_samples=None, output_layer=None):
        """fairseq HubertModel.extract_features(source, padding_mask, mask=False, output_layer): fp32 [B, T, d] after
        `output_layer` transformer layers (None = all) and the clips' frame counts (a list); rows past a clip's count are padding."""
        out, _, host_lens, B, T = self.extract_rows(source, n_samples, output_layer)
        return out.view(B, T, -1), host_lens


def load_hubert(path, dtype=ops.F32):
    """A fairseq HuBERT checkpoint (`model` + `cfg` or old-style `args`) -> HubertModel.  No fairseq import."""
    from .plugin import cfg_get
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or "model" not in ck:
        raise ValueError(f"{path}: not a fairseq checkpoint (no `model` entry)")
    cfg = ck.get("cfg")
    if cfg is not None:
        hc = HubertConfig.from_checkpoint_cfg(cfg_get(cfg, "model"), cfg_get(cfg, "task"))
    elif ck.get("args") is not None:
        hc = HubertConfig.from_checkpoint_cfg(ck["args"], ck["args"])
    else:
        raise ValueError(f"{path}: the checkpoint embeds neither `cfg` nor `args`")
    model = HubertModel(hc, dtype=dtype)
    model.load_state_dict(ck["model"])
    return model.eval()


def load_kmeans(path):
    """Cluster centres float32 [K, D]: a joblib-dumped model with `cluster_centers_` (km.bin, as ApplyKmeans.__init__) or a .npy."""
    if str(path).endswith(".npy"):
        c = np.load(path)
    else:
        import joblib
        c = joblib.load(path).cluster_centers_
    c = np.ascontiguousarray(np.asarray(c), dtype=np.float32)
    if c.ndim != 2 or c.shape[0] < 2:
        raise ValueError(f"{path}: expected cluster centres [K >= 2, D], got {c.shape}")
    return c


class SpeechUnitExtractor:
    """wav -> unit ids: HuBERT features of `layer`, nearest centre (ApplyKmeans.__call__)."""

    def __init__(self, hubert, centers, layer=6, dtype=ops.F32):
        if hubert.dtype != dtype:
            raise ValueError("the HuBERT model was built for another dtype")
        if not 0 < layer <= len(hubert.encoder.layers):
            raise ValueError(f"layer={layer}: the model has {len(hubert.encoder.layers)} transformer layers")
        c = torch.as_tensor(np.asarray(centers), dtype=torch.float32).contiguous()
        if c.dim() != 2 or c.shape[1] != hubert.cfg.encoder_embed_dim:
            raise ValueError(f"centers: [K, {hubert.cfg.encoder_embed_dim}], got {tuple(c.shape)}")
        self.hubert, self.layer, self.dtype = hubert, layer, dtype
        self.centers = c
        self.cnorm = c.double().pow(2).sum(1).float()       # |c|^2, rounded once
        self._dev = {}

    def tables(self, dev):
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        if key not in self._dev:
            self._dev[key] = (self.centers.to(dev), self.cnorm.to(dev))
        return self._dev[key]

    def assign(self, rows, lens, B, T, want_best2=False):
        """rows fp32 [B*T, D] -> ids int32 [B*T] on the device (-1 past lens) and, on request, the two smallest distances."""
        cen, cn = self.tables(rows.device)
        ids = torch.empty(B * T, device=rows.device, dtype=torch.int32)
        best2 = torch.empty(B * T, 2, device=rows.device, dtype=torch.float32) if want_best2 else None
        ops.kmeans_assign(rows, cen, cn, ids, B=B, T=T, D=cen.shape[1], K=cen.shape[0], lens=lens, len_mul=1, best2=best2)
        return (ids, best2) if want_best2 else ids

    def units(self, wav, n_samples=None, return_features=False):
        """wav: device [B, S] fp32 or int16 -> a list of int64 arrays, clip b's num_frames(n_b) unit ids."""
        rows, lens, host_lens, B, T = self.hubert.extract_rows(wav, n_samples, self.layer)
        ids = self.assign(rows, lens, B, T).view(B, T).cpu().numpy()
        out = [ids[b, :host_lens[b]].astype(np.int64) for b in range(B)]
        if return_features:
            return out, [rows.view(B, T, -1)[b, :host_lens[b]] for b in range(B)]
        return out
