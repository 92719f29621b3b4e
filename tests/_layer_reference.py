"""Per-layer references for the AV-HuBERT encoder (24 layers) and the conformer (12 blocks): the residual stream after every
layer of ONE clip, from the input the HIP stack itself was given (tests/test_layer_taps_gpu.py captures it).

* `encoder_fp64` / `conformer_fp64`: the oracle (oracle/avhubert.py transformer_encoder, oracle/conformer.py
  espnet_encoder_after_frontend) run in float64 on the float64 state dict - the "true" stream.
* `encoder_emulated` / `conformer_emulated`: the same stack with every operand the product stores in 16 bits rounded to the
  run's 16-bit type, at exactly the points listed in ROUNDING_POINTS; accumulation, the residual stream, LayerNorm statistics,
  softmax and the GLU / depthwise conv stay fp32.  `splits` > 1 cuts the reduction dimension of every product into that many
  slices summed in order (split-K's order): a second correct 16-bit implementation, used to size the gates.
* `gate`: the per-layer check  e_i <= C_FROB * eps_i  and  w_i <= C_ROW * omega_i  (tests/test_layer_taps_gpu.py header).

Mutations (`mut=(kind, stack, layer)`) inject one known defect into the emulation at one layer; tests/test_layer_taps_cpu.py
checks that the gate sees each of them at that layer and not before.
"""
import math

import torch
import torch.nn.functional as F

from oracle import avhubert as oa
from oracle import conformer as oc

ENC = "encoder.w2v_model.encoder"
CONF = "conformer.encoder"

# Where the product rounds to 16 bits (everything else of these stacks is fp32 in registers or in HBM):
ROUNDING_POINTS = (
    # weights: every GEMM operand packed 16-bit (hubert.py TransformerEncoder.pack, conformer.py Encoder.pack w16); q's
    # 1/sqrt(d_h) = 1/8 is folded into W_q / b_q before the rounding (exact: a power of two); biases, LayerNorm gains, the
    # BatchNorm-folded depthwise taps (conformer.py "dw"/"db") stay fp32
    "weights",
    # encoder input: the pos_conv tap-GEMM reads the 16-bit copy x16 (hubert.py:160, model's F_DUAL output :275), its
    # residual is the fp32 x32
    "enc_input_16",
    # every LayerNorm that feeds a GEMM writes 16-bit h (norm.hip:66-73 / :171 / :238 store through ET::from_f32 / pack2;
    # hubert.py:175, the ln= of residual_linear :179/:184; conformer.py:255/262/277 and half_ffn's `after`)
    "layernorm_out",
    # the fused QKV projection's output is a 16-bit buffer (hubert.py:177, conformer.py:273)
    "qkv",
    # q+u and q+v rounded before the MFMA (attention.hip:75-76 tiled, :366-367 resident)
    "q_plus_u_v",
    # the projected relative-position table: the fp32 table rounded, times 16-bit W_pos, stored 16-bit (conformer.py:222-225)
    "pos_proj",
    # unnormalised P = exp(s - m) rounded before P.V (attention.hip:188 tiled, :474-475 resident); the row sum is fp32
    "p_before_pv",
    # attention output O / l rounded (attention.hip:222-223, :517-518)
    "attn_out",
    # FFN hidden activations: GELU(fc1) of the encoder (hubert.py:181), ReLU(w_1) of the conformer (conformer.py:256)
    "ffn_hidden",
    # the GLU input: pointwise_cov1's 16-bit output (conformer.py:278); GLU itself stays fp32 in LDS (conformer_conv.hip:34-36)
    "glu_in",
    # the depthwise conv + BatchNorm + Swish output (conformer_conv.hip:57)
    "dwconv_out",
)
# Not rounded: the fp32 residual stream x (tapgemm epilogue F_OUT_F32 | F_RES_F32), the conformer's norm_final output (written
# in place into x, conformer.py:280), the conformer embed (fp32 x, conformer.py:242).

MUTATIONS = {
    "ln_eps": "LayerNorm eps 1e-5 instead of 1e-12 in every LayerNorm of one conformer block",
    "drop_bias": "the out_proj bias of one encoder layer dropped",
    "rel_shift": "rel-shift off by one position (relative position i-j+1 for i-j) in one conformer block",
    "pad_key": "one padded key attended (a zero key / value row with score 0) in one layer's attention",
    "gelu_tanh": "tanh-approximation GELU in place of erf in one encoder layer's FC1",
    "res16": "the residual stream stored as 16 bits after one layer (reported, not asserted)",
}


def sd64(sd, prefix):
    """The float64 copy of the state dict entries under `prefix` (ENC or CONF) that the fp64 references read."""
    return {k: v.double() for k, v in sd.items() if k.startswith(prefix + ".") and v.is_floating_point()}


def encoder_fp64(sd_64, x, layers=24):
    """x: fp32 [n, 1024] - the encoder stack's input rows of ONE clip (valid rows only); sd_64 = sd64(sd, ENC).
    -> [fp64 [n, 1024]] per layer."""
    taps = {}
    with torch.no_grad():
        oa.transformer_encoder(sd_64, ENC, x.double()[None], None, layers, taps=taps)
    return [taps[f"layer{i}"][0] for i in range(layers)]


def conformer_fp64(sd_64, xin, layers=12):
    """xin: [n, 512] (the 16-bit embed input of ONE clip, as fp32); sd_64 = sd64(sd, CONF).  -> [fp64 [n, 512]] per block."""
    taps = {}
    n = xin.shape[0]
    with torch.no_grad():
        oc.espnet_encoder_after_frontend(sd_64, CONF, xin.double()[None], torch.ones(1, 1, n, dtype=torch.bool),
                                         layers, taps=taps)
    return [taps[f"block{i}"][0] for i in range(layers)]


# ---- 16-bit emulation ------------------------------------------------------------------------------------------------


class _Emu:
    def __init__(self, t16, splits):
        self.t16, self.splits = t16, splits

    def r(self, t):
        return t.to(self.t16).float()

    def mm(self, a, b):
        """a [..., K] @ b [..., K, N] in fp32; `splits` > 1: K in that many slices, partial products summed in order."""
        if self.splits <= 1:
            return a @ b
        K = a.shape[-1]
        out = None
        for idx in torch.arange(K).tensor_split(self.splits):
            if idx.numel() == 0:
                continue
            lo, hi = int(idx[0]), int(idx[-1]) + 1
            p = a[..., lo:hi] @ b[..., lo:hi, :]
            out = p if out is None else out + p
        return out

    def lin(self, h16, w16, bias=None, alpha=1.0):
        """tap-GEMM epilogue order: (acc + bias) * alpha (tapgemm_common.h:272-278)."""
        y = self.mm(h16, w16.t())
        if bias is not None:
            y = y + bias
        return y * alpha if alpha != 1.0 else y

    def attention(self, q, k, v, extra_key=False):
        """q, k, v [H, n, 64] fp32 (16-bit values); scores fp32 -> [n, H*64] rounded.  P rounded before P.V, row sum fp32."""
        return self.softmax_pv(self.mm(q, k.transpose(-1, -2)), v, extra_key)

    def softmax_pv(self, s, v, extra_key=False):
        if extra_key:                                                      # mutation: one padded (zero) key attended
            s = torch.cat([s, s.new_zeros(s.shape[:-1] + (1,))], -1)
            v = torch.cat([v, v.new_zeros(v.shape[0], 1, v.shape[-1])], -2)
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o = self.mm(self.r(p), v) / l
        H, n, d = o.shape
        return self.r(o.transpose(0, 1).reshape(n, H * d))


def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _mut_at(mut, kind, stack, i):
    return mut is not None and mut[0] == kind and mut[1] == stack and mut[2] == i


def encoder_emulated(sd, x, t16, layers=24, splits=1, mut=None, heads=16, x16=None):
    """The HIP encoder stack (hubert.py TransformerEncoder.forward_rows) on ONE clip's fp32 input rows x [n, d] (x16: the
    product's 16-bit copy of them, default x rounded) -> the fp32 residual stream after every layer."""
    E = _Emu(t16, splits)
    r = E.r
    p = ENC
    n, d = x.shape
    dh = d // heads
    x = x.float().clone()
    # pos_conv: grouped conv (16 groups, k = 128) over the 16-bit input, taps t-64 .. t+63, + bias, GELU, + x32 (hubert.py:160)
    w = oa.pos_conv_weight(sd, p + ".pos_conv.0").float()
    k = w.shape[-1]
    w16 = r(w)
    xp = F.pad((r(x) if x16 is None else x16.float()).t()[None], (k // 2, k // 2 - 1))
    acc = None
    for idx in torch.arange(k).tensor_split(max(splits, 1)):
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        part = F.conv1d(xp[:, :, lo:lo + n + hi - lo - 1], w16[:, :, lo:hi], groups=16)
        acc = part if acc is None else acc + part
    x = x + F.gelu(acc[0].t() + sd[p + ".pos_conv.0.bias"].float())
    scale = dh ** -0.5
    out = []
    for i in range(layers):
        lp = f"{p}.layers.{i}"
        a = lp + ".self_attn"
        wqkv = r(torch.cat([sd[a + ".q_proj.weight"] * scale, sd[a + ".k_proj.weight"], sd[a + ".v_proj.weight"]], 0))
        bqkv = torch.cat([sd[a + ".q_proj.bias"] * scale, sd[a + ".k_proj.bias"], sd[a + ".v_proj.bias"]], 0)
        h = r(_ln(x, sd, lp + ".self_attn_layer_norm", 1e-5))
        qkv = r(E.lin(h, wqkv, bqkv)).view(n, 3, heads, dh).permute(1, 2, 0, 3)
        att = E.attention(qkv[0], qkv[1], qkv[2], extra_key=_mut_at(mut, "pad_key", "enc", i))
        bo = None if _mut_at(mut, "drop_bias", "enc", i) else sd[a + ".out_proj.bias"]
        x = x + E.lin(att, r(sd[a + ".out_proj.weight"]), bo)
        h = r(_ln(x, sd, lp + ".final_layer_norm", 1e-5))
        gelu = (lambda t: F.gelu(t, approximate="tanh")) if _mut_at(mut, "gelu_tanh", "enc", i) else F.gelu
        f = r(gelu(E.lin(h, r(sd[lp + ".fc1.weight"]), sd[lp + ".fc1.bias"])))
        x = x + E.lin(f, r(sd[lp + ".fc2.weight"]), sd[lp + ".fc2.bias"])
        if _mut_at(mut, "res16", "enc", i):
            x = r(x)
        out.append(x.clone())
    return out


def _rel_attention(E, qkv, pp, u, vb, heads, dh, mut_shift=False, extra_key=False):
    """conformer rel-pos attention on 16-bit qkv [n, 3d] (q pre-scaled) and the 16-bit projected table pp [2n-1, d]."""
    n = qkv.shape[0]
    q, k, v = qkv.view(n, 3, heads, dh).permute(1, 2, 0, 3)
    qu = E.r(q + u[:, None, :])
    qv = E.r(q + vb[:, None, :])
    ppt = pp.view(-1, heads, dh).permute(1, 2, 0)                        # [H, 64, 2n-1]
    if mut_shift:                                                        # row k+1 where row k belongs
        ppt = torch.cat([ppt[..., 1:], ppt.new_zeros(heads, dh, 1)], -1)
    ac = E.mm(qu, k.transpose(-1, -2))
    bd = oc.rel_shift(E.mm(qv, ppt)[None])[0]
    return E.softmax_pv(ac + bd, v, extra_key)


def conformer_emulated(sd, xin, t16, layers=12, splits=1, mut=None, heads=8):
    """The HIP conformer block stack (conformer.py Encoder.forward_rows) on ONE clip's 16-bit embed input xin [n, 512] ->
    the fp32 residual stream after every block (after norm_final, which the product applies to x in place)."""
    E = _Emu(t16, splits)
    r = E.r
    p = CONF
    xin = r(xin.float())
    n = xin.shape[0]
    x = E.lin(xin, r(sd[p + ".embed.0.weight"]), sd[p + ".embed.0.bias"])
    d = x.shape[-1]
    dh = d // heads
    inv = 1.0 / math.sqrt(dh)
    x = x * math.sqrt(d)
    pe = r(oc.rel_pos_table(n, d)[0])
    out = []
    for i in range(layers):
        lp = f"{p}.encoders.{i}"
        eps = 1e-5 if _mut_at(mut, "ln_eps", "conf", i) else 1e-12

        def half_ffn(x, name, norm):
            h = r(_ln(x, sd, f"{lp}.{norm}", eps))
            f = r(torch.relu(E.lin(h, r(sd[f"{lp}.{name}.w_1.weight"]), sd[f"{lp}.{name}.w_1.bias"])))
            return x + E.lin(f, r(sd[f"{lp}.{name}.w_2.weight"]), sd[f"{lp}.{name}.w_2.bias"], alpha=0.5)

        x = half_ffn(x, "feed_forward_macaron", "norm_ff_macaron")
        a = lp + ".self_attn"
        wqkv = r(torch.cat([sd[a + ".linear_q.weight"] * inv, sd[a + ".linear_k.weight"], sd[a + ".linear_v.weight"]], 0))
        bqkv = torch.cat([sd[a + ".linear_q.bias"] * inv, sd[a + ".linear_k.bias"], sd[a + ".linear_v.bias"]], 0)
        h = r(_ln(x, sd, lp + ".norm_mha", eps))
        qkv = r(E.lin(h, wqkv, bqkv))
        pp = r(E.lin(pe, r(sd[a + ".linear_pos.weight"])))
        att = _rel_attention(E, qkv, pp, sd[a + ".pos_bias_u"] * inv, sd[a + ".pos_bias_v"] * inv, heads, dh,
                             mut_shift=_mut_at(mut, "rel_shift", "conf", i), extra_key=_mut_at(mut, "pad_key", "conf", i))
        x = x + E.lin(att, r(sd[a + ".linear_out.weight"]), sd[a + ".linear_out.bias"])
        c = lp + ".conv_module"
        h = r(_ln(x, sd, lp + ".norm_conv", eps))
        g = r(E.lin(h, r(sd[c + ".pointwise_cov1.weight"][:, :, 0]), sd[c + ".pointwise_cov1.bias"]))
        glu = g[:, :d] * torch.sigmoid(g[:, d:])
        sc = sd[c + ".norm.weight"] / torch.sqrt(sd[c + ".norm.running_var"] + 1e-5)
        sh = sd[c + ".norm.bias"] - sd[c + ".norm.running_mean"] * sc
        dw = sd[c + ".depthwise_conv.weight"][:, 0, :] * sc[:, None]
        db = sd[c + ".depthwise_conv.bias"] * sc + sh
        kk = dw.shape[-1]
        y = F.conv1d(glu.t()[None], dw[:, None, :], db, padding=(kk - 1) // 2, groups=d)[0].t()
        cv = r(y * torch.sigmoid(y))
        x = x + E.lin(cv, r(sd[c + ".pointwise_cov2.weight"][:, :, 0]), sd[c + ".pointwise_cov2.bias"])
        x = half_ffn(x, "feed_forward", "norm_ff")
        x = _ln(x, sd, lp + ".norm_final", eps)
        if _mut_at(mut, "res16", "conf", i):
            x = r(x)
        out.append(x.clone())
    return out


# ---- metrics and the gate --------------------------------------------------------------------------------------------


def errors(got, ref):
    """-> (relative Frobenius error, worst per-row relative error, that row) of got vs the fp64 ref, both [n, C]."""
    diff = got.double() - ref
    e = float(diff.norm() / ref.norm())
    rows = diff.norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)
    bad = (~torch.isfinite(rows)).nonzero()
    t = int(bad[0]) if len(bad) else int(rows.argmax())           # a non-finite row is the worst row
    return e, float(rows[t]), t


def layer_errors(stream, ref):
    return [errors(g, r_) for g, r_ in zip(stream, ref)]


def emulation_spread(sd, x, xin, t16, enc_layers=24, conf_layers=12):
    """The spread between two correct 16-bit implementations on one clip: per stack, the largest ratio either way between the
    per-layer errors of the emulation with splits = 1 and with splits = 8 -> {"enc" / "conf": (rho Frobenius, rho worst
    row, max eps, max omega)}.  x: encoder input rows [n, 1024] fp32, xin: conformer input rows [2n, 512] (16-bit values)."""
    out = {}
    for stack, ref, run in (
            ("enc", encoder_fp64(sd64(sd, ENC), x, enc_layers),
             lambda k: encoder_emulated(sd, x, t16, enc_layers, splits=k)),
            ("conf", conformer_fp64(sd64(sd, CONF), xin, conf_layers),
             lambda k: conformer_emulated(sd, xin, t16, conf_layers, splits=k))):
        a, b = layer_errors(run(1), ref), layer_errors(run(8), ref)
        out[stack] = (max(max(p[0] / q[0], q[0] / p[0]) for p, q in zip(a, b)),
                      max(max(p[1] / q[1], q[1] / p[1]) for p, q in zip(a, b)),
                      max(p[0] for p in a), max(p[1] for p in a))
    return out


# Gate constants, set from CPU runs only, before the first GPU run (tools/layer_gate_rho.py recomputes them).  rho = the
# largest ratio, either way, between the per-layer errors of the two emulations (emulation_spread: splits = 1 vs 8) over all
# 24 + 12 layers, both dtypes and every checked clip length of points A / B / C (encoder n = 100, 73, 40, 37, 25, 600;
# conformer 2n), full-strength seed-0 weights, encoder input = the fp32 oracle's post_extract_proj rows of random-pixel clips,
# conformer input = the fp32 oracle's encoder output through proj_in:
#   Frobenius  rho = 1.037 (fp16, conformer n = 25) / 1.030 (bf16, encoder n = 25)  ->  C_FROB = max(2, 1.5 * 1.037) = 2
#   worst row  rho = 1.045 (fp16, conformer n = 40) / 1.044 (bf16, encoder n = 25)  ->  C_ROW  = max(2, 1.5 * 1.045) = 2
# (the first derivation, with the conformer input taken through the fp64 encoder, gave 1.045 / 1.053: the same constants).
# The emulation's own error stayed <= 9.0e-4 (fp16) / 7.5e-3 (bf16) at every layer: no layer above MEANINGLESS.
# What a factor 2 can see: errors add in quadrature, so a defect trips it once its own size reaches sqrt(3) = 1.7 x the
# 16-bit error of that layer (tests/test_layer_taps_cpu.py measures each mutation's size against that).
# First MI355X run of tests/test_layer_taps_gpu.py with these constants: every layer within 1.04 x the emulation's error -
# largest e/eps (w/omega): A fp16 1.01 (1.02), A bf16 1.01 (1.03), B fp16 1.04 (1.03), B bf16 1.03 (1.04), C fp16 1.02 (1.03),
# C bf16 1.01 (1.01); no layer reported instead of gated; the 6 cases took 30 s.
C_FROB = 2.0
C_ROW = 2.0
MEANINGLESS = 0.1          # an emulation error above this (relative) carries no information: the layer is reported, not gated


def gate(got_errs, emu_errs, c=C_FROB, c_row=C_ROW, floor=MEANINGLESS):
    """got_errs / emu_errs: per-layer (e, w, t) of the checked stream and of the emulation.  Returns (first failing layer or
    None, its message, [layers reported instead of gated]).  Non-finite errors fail: a NaN / inf in any valid row of the
    checked stream (every comparison is written so that NaN cannot pass), or in the emulation itself (a broken reference
    must not turn into a skipped layer)."""
    reported = []
    for i, ((e, w, t), (eps, om, _)) in enumerate(zip(got_errs, emu_errs)):
        if not (math.isfinite(eps) and math.isfinite(om)):
            return i, f"layer {i}: the emulation's own error is not finite (eps {eps}, omega {om})", reported
        if not (math.isfinite(e) and math.isfinite(w)):
            return i, f"layer {i}: non-finite values in the checked stream (e {e}, worst row t={t}: w {w})", reported
        if eps > floor or om > floor:
            reported.append(i)
            continue
        if not (e <= c * eps and w <= c_row * om):
            return i, (f"layer {i}: e {e:.3e} vs {c:g} x eps {eps:.3e} (ratio {e / eps:.2f}); worst row t={t}: w {w:.3e} vs "
                       f"{c_row:g} x omega {om:.3e} (ratio {w / om:.2f})"), reported
    return None, "", reported


def table(got_errs, emu_errs):
    lines = ["  layer      e_i    eps_i   e/eps      w_i  omega_i   w/om  row"]
    for i, ((e, w, t), (eps, om, _)) in enumerate(zip(got_errs, emu_errs)):
        lines.append(f"  {i:5d} {e:8.2e} {eps:8.2e} {e / max(eps, 1e-30):7.2f} {w:8.2e} {om:8.2e} {w / max(om, 1e-30):6.2f} {t:4d}")
    return "\n".join(lines)
