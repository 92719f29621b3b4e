"""Plain-torch float64 restatement of the speech-unit path (extract_speech_units.sh:6-11): HuBERT-base features of a transformer
layer, quantised by ApplyKmeans (avhubert/clustering/dump_km_label.py:26-52).  Runs on the CPU at test time.

fairseq's HubertModel is not in the reference tree; what is restated here is its published structure, checked in
tests/test_units_cpu.py against HuggingFace's independent port (`transformers.HubertModel`) on the same weights:
  ConvFeatureExtractionModel(mode="default"): Conv1d k (10,3,3,3,3,2,2) stride (5,2,2,2,2,2,2) no bias, GroupNorm(512, 512) behind
  layer 0, erf GELU; LayerNorm(512); post_extract_proj 512 -> 768; x + GELU(SamePad(weight-normed grouped pos_conv(x)));
  LayerNorm; post-LN layers x = LN1(x + attn(x)), x = LN2(x + fc2(GELU(fc1(x)))); no norm behind the last layer taken.
State dicts carry fairseq's names.  Every clip is computed alone.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

CONV_K = (10, 3, 3, 3, 3, 2, 2)
CONV_S = (5, 2, 2, 2, 2, 2, 2)


def frame_count(n):
    """Feature frames of n samples: L <- (L - k) // s + 1 through the seven layers."""
    for k, s in zip(CONV_K, CONV_S):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def init_weights(seed=0, layers=6, dim=768, ffn=3072, conv_dim=512, conv_pos=128, groups=16, perturb=True):
    """Seeded float32 state dict under HuggingFace HubertModel's initialisation rules (modeling_hubert.py _init_weights): Linear
    weights N(0, 0.02) with zero bias, Conv1d weights kaiming-normal (std sqrt(2 / fan_in)) with zero bias - through the weight
    norm of pos_conv that is weight_v = the draw, weight_g = its norm over dims (0, 1) - and norm layers at (1, 0).
    perturb=True then moves what those rules leave at a constant - every bias by N(0, 0.02), every norm weight by N(0, 0.1),
    weight_g by a factor 1 + N(0, 0.1) - so that a kernel that dropped a bias or an affine term cannot pass."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def normal(shape, std):
        return torch.randn(shape, generator=g, dtype=torch.float32) * std

    def bias(n):
        return normal((n,), 0.02) if perturb else torch.zeros(n)

    def norm(prefix, n):
        sd[prefix + ".weight"] = 1.0 + (normal((n,), 0.1) if perturb else torch.zeros(n))
        sd[prefix + ".bias"] = bias(n)

    def linear(prefix, nout, nin):
        sd[prefix + ".weight"] = normal((nout, nin), 0.02)
        sd[prefix + ".bias"] = bias(nout)

    cin = 1
    for i, k in enumerate(CONV_K):
        sd[f"feature_extractor.conv_layers.{i}.0.weight"] = normal((conv_dim, cin, k), math.sqrt(2.0 / (cin * k)))
        cin = conv_dim
    norm("feature_extractor.conv_layers.0.2", conv_dim)
    norm("layer_norm", conv_dim)
    linear("post_extract_proj", dim, conv_dim)
    v = normal((dim, dim // groups, conv_pos), math.sqrt(2.0 / (dim // groups * conv_pos)))
    sd["encoder.pos_conv.0.weight_v"] = v
    wg = v.double().pow(2).sum(dim=(0, 1), keepdim=True).sqrt().float()
    sd["encoder.pos_conv.0.weight_g"] = wg * (1.0 + normal((1, 1, conv_pos), 0.1)) if perturb else wg
    sd["encoder.pos_conv.0.bias"] = bias(dim)
    norm("encoder.layer_norm", dim)
    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            linear(p + "self_attn." + n, dim, dim)
        norm(p + "self_attn_layer_norm", dim)
        linear(p + "fc1", ffn, dim)
        linear(p + "fc2", dim, ffn)
        norm(p + "final_layer_norm", dim)
    return sd


def _d(sd, name):
    return sd[name].detach().double()


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def wave_stem(sd, wav, eps=1e-5):
    """Layer 0 on one clip: wav float64 [n] -> [L0, C]."""
    y = F.conv1d(wav.double().view(1, 1, -1), _d(sd, "feature_extractor.conv_layers.0.0.weight"), stride=CONV_S[0])[0]   # [C, L0]
    mean = y.mean(dim=1, keepdim=True)
    var = y.var(dim=1, unbiased=False, keepdim=True)
    n = (y - mean) / torch.sqrt(var + eps)
    n = n * _d(sd, "feature_extractor.conv_layers.0.2.weight")[:, None] + _d(sd, "feature_extractor.conv_layers.0.2.bias")[:, None]
    return gelu(n).t().contiguous()


def conv_features(sd, wav):
    """The whole conv stack on one clip: [n] -> [T, 512]."""
    x = wave_stem(sd, wav).t().unsqueeze(0)
    for i in range(1, len(CONV_K)):
        x = gelu(F.conv1d(x, _d(sd, f"feature_extractor.conv_layers.{i}.0.weight"), stride=CONV_S[i]))
    return x[0].t().contiguous()


def layer_norm(x, sd, prefix, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), _d(sd, prefix + ".weight"), _d(sd, prefix + ".bias"), eps)


def linear(x, sd, prefix):
    return x @ _d(sd, prefix + ".weight").t() + _d(sd, prefix + ".bias")


def pos_conv(x, sd, groups=16):
    """x [T, d] -> GELU(SamePad(conv(x))) [T, d]; weight_norm(dim=2): w = v * g / |v| over dims (0, 1)."""
    v, g = _d(sd, "encoder.pos_conv.0.weight_v"), _d(sd, "encoder.pos_conv.0.weight_g")
    w = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    k = w.shape[-1]
    y = F.conv1d(x.t().unsqueeze(0), w, _d(sd, "encoder.pos_conv.0.bias"), padding=k // 2, groups=groups)
    if k % 2 == 0:
        y = y[:, :, :-1]
    return gelu(y[0].t())


def attention(x, sd, prefix, heads):
    T, d = x.shape
    hd = d // heads
    q = linear(x, sd, prefix + ".q_proj") * hd ** -0.5
    k = linear(x, sd, prefix + ".k_proj")
    v = linear(x, sd, prefix + ".v_proj")
    q, k, v = (t.view(T, heads, hd).transpose(0, 1) for t in (q, k, v))
    p = torch.softmax(q @ k.transpose(1, 2), dim=-1)
    return linear((p @ v).transpose(0, 1).reshape(T, d), sd, prefix + ".out_proj")


def features(sd, wav, output_layer=6, heads=12, groups=16):
    """HubertModel.extract_features(source, padding_mask=None, output_layer) on one clip: float64 [T, 768]."""
    x = layer_norm(conv_features(sd, wav), sd, "layer_norm")
    x = linear(x, sd, "post_extract_proj")
    x = layer_norm(x + pos_conv(x, sd, groups), sd, "encoder.layer_norm")
    for i in range(output_layer):
        p = f"encoder.layers.{i}"
        x = layer_norm(x + attention(x, sd, p + ".self_attn", heads), sd, p + ".self_attn_layer_norm")
        x = layer_norm(x + linear(gelu(linear(x, sd, p + ".fc1")), sd, p + ".fc2"), sd, p + ".final_layer_norm")
    return x


def kmeans_dist(x, centers):
    """ApplyKmeans.__call__'s distance matrix (dump_km_label.py:40-44), float64 [M, K]."""
    x, c = torch.as_tensor(x).double(), torch.as_tensor(centers).double()
    C = c.t()
    return x.pow(2).sum(1, keepdim=True) - 2 * torch.matmul(x, C) + C.pow(2).sum(0, keepdim=True)


def kmeans_ids(x, centers):
    return kmeans_dist(x, centers).argmin(dim=1)


def flip_margin(x, centers):
    """r_t = min_{j != id} (d_j - d_id) / (2 |c_j - c_id| |x_t|): the largest relative feature error frame t tolerates (a
    perturbation of norm e moves d_j - d_id by at most 2 e |c_j - c_id|).  Returns (ids, r) float64."""
    x, c = torch.as_tensor(x).double(), torch.as_tensor(centers).double()
    d = kmeans_dist(x, c)
    ids = d.argmin(dim=1)
    gap = d - d.gather(1, ids[:, None])
    sep = torch.cdist(c[ids], c)                                  # |c_j - c_id| per frame
    r = gap / (2.0 * sep * x.norm(dim=1, keepdim=True))
    r = torch.where(sep == 0, torch.full_like(r, float("inf")), r)   # an exact duplicate of the winner decides nothing
    r.scatter_(1, ids[:, None], float("inf"))                        # j = id itself
    return ids, r.min(dim=1).values


def pcm_to_wave(pcm):
    """int16 PCM -> float64 in (-1, 1), value / 32768 as soundfile reads it."""
    return torch.from_numpy(np.asarray(pcm).astype(np.float64) / 32768.0)


CENTER_SEED = 3   # the first draw under which test_units_cpu's decidability assertions hold with init_weights(0) (seed 1: one frame at 1.6e-5)


def draw_centers(feats, n=100, seed=CENTER_SEED):
    """n frames of `feats` drawn without replacement under `seed`, as float32 centres [n, D]."""
    idx = torch.randperm(feats.shape[0], generator=torch.Generator().manual_seed(seed))[:n]
    return feats[idx.sort().values].float().contiguous()


def to_huggingface(sd):
    """The same tensors under transformers.HubertModel's parameter names."""
    out = {}
    for k, v in sd.items():
        k = k.replace("encoder.pos_conv.0.weight_g", "encoder.pos_conv_embed.conv.parametrizations.weight.original0")
        k = k.replace("encoder.pos_conv.0.weight_v", "encoder.pos_conv_embed.conv.parametrizations.weight.original1")
        k = k.replace("encoder.pos_conv.0.bias", "encoder.pos_conv_embed.conv.bias")
        if k.startswith("feature_extractor.conv_layers."):
            k = k.replace(".0.weight", ".conv.weight") if k.endswith(".0.weight") else k.replace(".2.", ".layer_norm.")
        elif k.startswith("layer_norm."):
            k = "feature_projection." + k
        elif k.startswith("post_extract_proj."):
            k = k.replace("post_extract_proj", "feature_projection.projection")
        k = k.replace(".self_attn_layer_norm.", ".layer_norm.").replace(".self_attn.", ".attention.")
        k = k.replace(".fc1.", ".feed_forward.intermediate_dense.").replace(".fc2.", ".feed_forward.output_dense.")
        out[k] = v
    return out


_CASE = {}


def shared_case(golden_dir, layers=6):
    """The seeded case the CPU and GPU tests share, computed once per process: weights under seed 0, the float64 features of
    c1_pcm / c2_pcm / c4_pcm (clips alone), and 100 centres drawn from c1's frames."""
    import os
    if layers not in _CASE:
        z = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
        sd = init_weights(0, layers=layers)
        pcm = {c: np.asarray(z[c + "_pcm"]) for c in ("c0", "c1", "c2", "c3", "c4")}
        with torch.no_grad():
            feats = {c: features(sd, pcm_to_wave(pcm[c]), layers) for c in ("c1", "c2", "c4")}
        _CASE[layers] = {"sd": sd, "pcm": pcm, "feats": feats, "centers": draw_centers(feats["c1"])}
    return _CASE[layers]


def kmeans_case(D, K, M=130, seed=0, noise=0.25):
    """Seeded quantiser inputs for the kernel tests: float32 rows [M, D] and centres [K, D] = data rows plus noise (rows reused
    cyclically when K > M), so that every row has a clear nearest centre."""
    rng = np.random.default_rng(1000 * D + K + seed)
    x = rng.standard_normal((M, D)).astype(np.float32)
    rows = np.resize(rng.permutation(M), K)
    c = (x[rows] + noise * rng.standard_normal((K, D))).astype(np.float32)
    return x, c


def decisive_rows(x, centers, rel=1e-5):
    """(ids, best2 [M, 2] of |c|^2 - 2 x.c, mask) in float64: mask = rows whose gap between best and second best exceeds
    rel * (|x|^2 + |c_id|^2) - fp32 product rounding with a decade of headroom."""
    x, c = torch.as_tensor(x).double(), torch.as_tensor(centers).double()
    d = c.pow(2).sum(1)[None, :] - 2 * x @ c.t()
    two = d.topk(2, dim=1, largest=False)
    ids = two.indices[:, 0]
    gap = two.values[:, 1] - two.values[:, 0]
    mask = gap > rel * (x.pow(2).sum(1) + c.pow(2).sum(1)[ids])
    return ids, two.values, mask
