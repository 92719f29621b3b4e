"""The fp32 (ops.F32) kernels against fp64 references computed on the CPU.
rows_f32_kernel (l2s_f32_rows) has its matrix, on guarded buffers, in tests/test_glue_matrix_gpu.py.

Tap-GEMM (csrc/tapgemm_f32.hip).  Every output is a k-ordered fp32 fma chain (one rounding per product) followed by the
epilogue's few operations, so the bound is the chain's worst case, not a tolerance:
    |err| <= 1.25 * (K_tot + 8) * 2^-24 * S + 2^-23 * |ref|,     S = |alpha| * (sum|a||w| + |bias|) + |R| + |C_prev|
(1.25 covers the largest activation slopes: GELU 1.13, Swish 1.10; PReLU slopes are kept in [0, 0.5]).

Attention, LayerNorm, GLU-dwconv, stem + pool, avgpool.  Yardstick = the same formula evaluated by torch in float32 on the
CPU; bound: max-abs error <= 4 x that evaluation's max-abs error against fp64, floor 2^-22 * max|ref|.  The two fp32
evaluations share the unit roundoff and differ in summation order and the last ulp of exp / erf only; a 16-bit operand
anywhere would sit about a hundred times outside."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops  # noqa: E402

DT = ops.F32
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22


def _act64(v, act, slope=None, act_slope=0.0):
    if act == ops.ACT_RELU:
        return v.clamp_min(0)
    if act == ops.ACT_GELU:
        return F.gelu(v)
    if act == ops.ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == ops.ACT_PRELU:
        return torch.where(v >= 0, v, v * slope.double())
    if act == ops.ACT_LRELU:
        return torch.where(v >= 0, v, v * act_slope)
    if act == ops.ACT_TANH:
        return torch.tanh(v)
    return v


def _reference(prod, aprod, K, *, bias=None, alpha=1.0, R=None, prev=None, act=ops.ACT_NONE, slope=None, act_slope=0.0,
               res_pre=False, keep=None):
    """prod / aprod: fp64 [M, N] contraction of (a, w) and of (|a|, |w|).  -> (ref, bound) of the tap-GEMM epilogue."""
    b = bias.double() if bias is not None else torch.zeros(prod.shape[1], dtype=torch.float64)
    v = alpha * (prod + b)
    S = abs(alpha) * (aprod + b.abs())
    if R is not None and res_pre:
        v = v + R.double()
    v = _act64(v, act, slope, act_slope)
    if R is not None and not res_pre:
        v = v + R.double()
    if R is not None:
        S = S + R.double().abs()
    if prev is not None:
        v = v + prev.double()
        S = S + prev.double().abs()
    if keep is not None:
        v = v * keep
        S = S * keep
    return v, 1.25 * (K + 8) * U24 * S + U23 * v.abs()


def _assert_within(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = (err - bound).max().item()
    ratio = (err / bound.clamp_min(1e-300)).max().item() if bool((bound > 0).any()) else 0.0
    print(f"\n[f32 tapgemm] {what}: max |err| {err.max().item():.3e}, max |ref| {ref.abs().max().item():.3e}, "
          f"largest err / bound {ratio:.3f}")
    assert torch.isfinite(got).all(), what
    assert worst <= 0.0, f"{what}: |err| exceeds the fma-chain bound by {worst:.3e} (err / bound {ratio:.2f})"


ACTS = [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU, ops.ACT_SWISH, ops.ACT_PRELU, ops.ACT_LRELU, ops.ACT_TANH]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,N,K", [(301, 204, 512), (77, 64, 96)])
def test_linear_every_activation(act, M, N, K):
    g = torch.Generator().manual_seed(M + 31 * act)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    sl = torch.rand(N, generator=g) * 0.5
    ref, bound = _reference(a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t(), K, bias=b, act=act, slope=sl,
                            act_slope=0.1)
    C = torch.empty(M, N, device="cuda")
    ops.tapgemm(a.cuda(), w.cuda(), C, M=M, N=N, Cin=K, bias=b.cuda(), slope=sl.cuda() if act == ops.ACT_PRELU else None,
                act=act, act_slope=0.1, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(C, ref, bound, f"linear act {act} M{M} N{N} K{K}")


@pytest.mark.parametrize("M,N,K", [(1001, 1024, 1024), (333, 204, 512), (129, 160, 4096)])
def test_linear_residual_alpha_in_place(M, N, K):
    g = torch.Generator().manual_seed(M)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    prod, aprod = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    ref, bound = _reference(prod, aprod, K, bias=b, alpha=0.5, R=r)
    x = r.clone().cuda()                        # the residual stream updated in place (R = C), as ops.residual_linear does
    ops.tapgemm(a.cuda(), w.cuda(), x, M=M, N=N, Cin=K, bias=b.cuda(), alpha=0.5, R=x, ldr=N, flags=ops.F_RES_POST, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(x, ref, bound, f"linear RES_POST in place M{M} N{N} K{K}")
    # RES_PRE + PReLU
    sl = torch.rand(N, generator=g) * 0.5
    ref, bound = _reference(prod, aprod, K, bias=b, R=r, res_pre=True, act=ops.ACT_PRELU, slope=sl)
    C = torch.empty(M, N, device="cuda")
    ops.tapgemm(a.cuda(), w.cuda(), C, M=M, N=N, Cin=K, bias=b.cuda(), slope=sl.cuda(), act=ops.ACT_PRELU, R=r.cuda(),
                flags=ops.F_RES_PRE, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(C, ref, bound, f"linear RES_PRE + PReLU M{M} N{N} K{K}")


def test_linear_accum_dual_mask():
    B, T, N, K = 3, 37, 204, 128
    M = B * T
    g = torch.Generator().manual_seed(11)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    prev = torch.randn(M, N, generator=g)
    lens = torch.tensor([37, 17, 0], dtype=torch.int32)
    keep = (torch.arange(T)[None, :] < lens[:, None]).reshape(M, 1).double()
    ref, bound = _reference(a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t(), K, prev=prev, keep=keep)
    Cp = prev.clone().cuda()
    C2 = torch.full((M, N), float("nan"), device="cuda")
    ops.tapgemm(a.cuda(), w.cuda(), Cp, M=M, N=N, Cin=K, C2=C2, lens=lens.cuda(), mask_T=T, mask_mul=1,
                flags=ops.F_ACCUM | ops.F_DUAL | ops.F_MASK, slope2=0.1, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(Cp, ref, bound, "linear ACCUM | MASK")
    _assert_within(C2, torch.where(ref >= 0, ref, ref * 0.1), bound, "linear DUAL copy")
    assert Cp.view(B, T, N)[1, 17:].abs().max().item() == 0.0 and Cp.view(B, T, N)[2].abs().max().item() == 0.0


@pytest.mark.parametrize("B,T,Cin,Cout,k,dil", [(2, 33, 768, 512, 3, 1), (3, 37, 32, 36, 7, 3), (1, 101, 16, 16, 11, 5)])
def test_conv1d_masked_gelu(B, T, Cin, Cout, k, dil):
    """the mel-head convolutions (model_avhubert.py:231-241): Conv1d + GELU with the lens row mask."""
    g = torch.Generator().manual_seed(B * 100 + T + k)
    x = torch.randn(B, Cin, T, generator=g)
    w = torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    lens = torch.tensor([T] + [T // 2] * (B - 1), dtype=torch.int32)
    keepT = (torch.arange(T)[None, :] < lens[:, None])
    x = x * keepT[:, None, :]
    pad = (k * dil - dil) // 2
    prod = F.conv1d(x.double(), w.double(), None, 1, pad, dil).transpose(1, 2).reshape(B * T, Cout)
    aprod = F.conv1d(x.double().abs(), w.double().abs(), None, 1, pad, dil).transpose(1, 2).reshape(B * T, Cout)
    ref, bound = _reference(prod, aprod, Cin * k, bias=b, act=ops.ACT_GELU, keep=keepT.reshape(B * T, 1).double())
    A = x.transpose(1, 2).contiguous().reshape(B * T, Cin).cuda()
    W = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous().cuda()
    C = torch.empty(B * T, Cout, device="cuda")
    ops.tapgemm(A, W, C, M=B * T, N=Cout, Cin=Cin, ntaps=k, mode=ops.MODE_CONV1D, T_out=T, T_in=T, stride=1, dil=dil, off=-pad,
                bias=b.cuda(), act=ops.ACT_GELU, lens=lens.cuda(), mask_T=T, mask_mul=1, flags=ops.F_MASK, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(C, ref, bound, f"conv1d k{k} dil{dil} Cin{Cin}")


def test_conv_transpose1d_phases_row_remap():
    from lip2speech_unit_amd.packing import convtranspose_phases
    B, L, Cin, Cout, k, s = 2, 23, 64, 32, 11, 5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, L, generator=g)
    w = torch.randn(Cin, Cout, k, generator=g) / (Cin * k / s) ** 0.5
    b = torch.randn(Cout, generator=g)
    p = (k - s) // 2
    prod = F.conv_transpose1d(x.double(), w.double(), None, s, p).transpose(1, 2).reshape(B * L * s, Cout)
    aprod = F.conv_transpose1d(x.double().abs(), w.double().abs(), None, s, p).transpose(1, 2).reshape(B * L * s, Cout)
    ref, bound = _reference(prod, aprod, Cin * ((k + s - 1) // s), bias=b)
    A = x.transpose(1, 2).contiguous().reshape(B * L, Cin).cuda()
    C = torch.full((B * L * s, Cout), float("nan"), device="cuda")
    for ph in convtranspose_phases(w, s, p):
        ops.tapgemm(A, ph["w"].float().contiguous().cuda(), C, M=B * L, N=Cout, Cin=Cin, ntaps=ph["ntaps"], mode=ops.MODE_CONV1D,
                    T_out=L, T_in=L, stride=1, dil=-1, off=ph["off"], out_row_mul=s, out_row_add=ph["r"], bias=b.cuda(), dtype=DT)
    torch.cuda.synchronize()
    _assert_within(C, ref, bound, "conv-transpose phases (output-row remap)")


def test_pos_conv_shape_with_mask():
    """fairseq pos_conv (hubert.py:399): k = 128, 16 groups of 64 channels, GELU, + the fp32 input as residual; T = 37 with
    one padded clip (rows past lens zero on the way in and masked on the way out)."""
    B, T, C, G, k = 2, 37, 1024, 16, 128
    cg = C // G
    g = torch.Generator().manual_seed(5)
    lens = torch.tensor([37, 20], dtype=torch.int32)
    keepT = (torch.arange(T)[None, :] < lens[:, None])
    x = torch.randn(B, C, T, generator=g) * keepT[:, None, :]
    w = torch.randn(C, cg, k, generator=g) / (cg * k) ** 0.5
    b = torch.randn(C, generator=g)
    prod = F.conv1d(x.double(), w.double(), None, 1, k // 2, 1, G)[:, :, :-1].transpose(1, 2).reshape(B * T, C)
    aprod = F.conv1d(x.double().abs(), w.double().abs(), None, 1, k // 2, 1, G)[:, :, :-1].transpose(1, 2).reshape(B * T, C)
    A = x.transpose(1, 2).contiguous().reshape(B * T, C)
    ref, bound = _reference(prod, aprod, cg * k, bias=b, act=ops.ACT_GELU, R=A, keep=keepT.reshape(B * T, 1).double())
    W = w.view(G, cg, cg, k).permute(0, 1, 3, 2).reshape(G, cg, k * cg).contiguous().cuda()
    Cc = torch.empty(B * T, C, device="cuda")
    Ad = A.cuda()
    ops.tapgemm(Ad, W, Cc, M=B * T, N=cg, Cin=cg, ntaps=k, lda=C, ldc=C, mode=ops.MODE_CONV1D, T_out=T, T_in=T, stride=1, dil=1,
                off=-(k // 2), bias=b.cuda(), act=ops.ACT_GELU, R=Ad, ldr=C, lens=lens.cuda(), mask_T=T, mask_mul=1,
                flags=ops.F_RES_POST | ops.F_MASK, dtype=DT, groups=G, a_gstride=cg, c_gstride=cg, w_gstride=cg * k * cg)
    torch.cuda.synchronize()
    _assert_within(Cc, ref, bound, "pos_conv k128 G16 T37 masked")


@pytest.mark.parametrize("N,H,Cin,Cout,k,s", [(5, 22, 64, 64, 3, 1), (5, 22, 64, 128, 3, 2), (7, 11, 128, 256, 1, 2),
                                               (9, 6, 256, 256, 3, 1), (11, 3, 512, 512, 3, 1), (3, 11, 128, 256, 3, 2)])
def test_conv2d_prelu_residual(N, H, Cin, Cout, k, s):
    g = torch.Generator().manual_seed(N * 13 + H)
    x = torch.randn(N, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    sl = torch.rand(Cout, generator=g) * 0.5
    pad = k // 2
    Ho = (H + 2 * pad - k) // s + 1
    r = torch.randn(N, Cout, Ho, Ho, generator=g)

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(N * Ho * Ho, Cout)
    ref, bound = _reference(rows(F.conv2d(x.double(), w.double(), None, s, pad)),
                            rows(F.conv2d(x.double().abs(), w.double().abs(), None, s, pad)), Cin * k * k, bias=b,
                            R=rows(r), res_pre=True, act=ops.ACT_PRELU, slope=sl)
    A = x.permute(0, 2, 3, 1).contiguous().reshape(N * H * H, Cin).cuda()
    W = w.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin).contiguous().cuda()
    C = torch.empty(N * Ho * Ho, Cout, device="cuda")
    ops.tapgemm(A, W, C, M=N * Ho * Ho, N=Cout, Cin=Cin, ntaps=k * k, mode=ops.MODE_CONV2D, Ho=Ho, Wo=Ho, Hi=H, Wi=H, KW=k,
                pad=pad, stride=s, bias=b.cuda(), slope=sl.cuda(), act=ops.ACT_PRELU, R=rows(r).contiguous().cuda(),
                flags=ops.F_RES_PRE, dtype=DT)
    torch.cuda.synchronize()
    _assert_within(C, ref, bound, f"conv2d {k}x{k} s{s} {Cin}->{Cout} H{H}")


def test_ktab_is_refused_in_fp32():
    from lip2speech_unit_amd import _lib
    a = torch.zeros(8, 64, device="cuda")
    tab = torch.zeros(1, 20, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.L2SError, match="L2S_EUNSUPPORTED"):
        ops.tapgemm(a, a, torch.empty(8, 8, device="cuda"), M=8, N=8, Cin=64, ktab=tab, dtype=DT)


# ---- the non-GEMM kernels: 4 x the error of torch's own float32 evaluation ---------------------------------------------------


def _assert_4x(got, ref64, y32, what):
    scale = ref64.abs().max().item()
    yard = (y32.double() - ref64).abs().max().item()
    bound = max(4.0 * yard, U22 * scale)
    err = (got.double().cpu() - ref64).abs().max().item()
    print(f"\n[f32 kernels] {what}: max |err| {err:.3e}; torch float32 yardstick {yard:.3e}; bound {bound:.3e}; max |ref| {scale:.3e}")
    assert torch.isfinite(got).all(), what
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"


def _attention_ref(qkv, pos, u, v, lens, B, T, H, dtype):
    """qkv [B*T, 3*H*64], pos [2T-1, H*64] or None -> out [B*T, H*64], evaluated in `dtype`."""
    D = 64
    x = qkv.to(dtype).view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)          # [3, B, H, T, D]
    q, k, val = x[0], x[1], x[2]
    if pos is None:
        s = q @ k.transpose(-1, -2)
    else:
        p = pos.to(dtype).view(2 * T - 1, H, D).permute(1, 2, 0)           # [H, D, 2T-1]
        ac = (q + u.to(dtype)[None, :, None, :]) @ k.transpose(-1, -2)
        full = (q + v.to(dtype)[None, :, None, :]) @ p[None]                # [B, H, T, 2T-1]
        idx = (T - 1) - torch.arange(T)[:, None] + torch.arange(T)[None, :]
        s = ac + full.gather(-1, idx[None, None].expand(B, H, T, T))
    key_ok = torch.arange(T)[None, :] < lens[:, None]
    s = s.masked_fill(~key_ok[:, None, None, :], float("-inf"))
    o = torch.softmax(s, -1) @ val
    return o.permute(0, 2, 1, 3).reshape(B * T, H * D)


@pytest.mark.parametrize("rel", [False, True], ids=["plain", "relpos"])
@pytest.mark.parametrize("T", [37, 200, 600])
def test_attention(T, rel):
    B, H, D = 2, 4, 64
    g = torch.Generator().manual_seed(T + rel)
    qkv = torch.randn(B * T, 3 * H * D, generator=g)
    qkv[:, : H * D] *= D ** -0.5                                            # q arrives pre-scaled
    lens = torch.tensor([T, max(T // 3, 1)], dtype=torch.int32)
    pos = u = v = None
    if rel:
        pos = torch.randn(2 * T - 1, H * D, generator=g) * 0.5
        u, v = torch.randn(H, D, generator=g) * 0.1, torch.randn(H, D, generator=g) * 0.1
    ref = _attention_ref(qkv, pos, u, v, lens, B, T, H, torch.float64)
    y32 = _attention_ref(qkv, pos, u, v, lens, B, T, H, torch.float32)
    out = torch.full((B * T, H * D), float("nan"), device="cuda")
    ops.attention(qkv.cuda(), out, B=B, T=T, H=H, pos=None if pos is None else pos.cuda(), ldp=H * D if rel else 0,
                  bias_u=None if u is None else u.cuda(), bias_v=None if v is None else v.cuda(), lens=lens.cuda(), dtype=DT)
    torch.cuda.synchronize()
    _assert_4x(out, ref, y32, f"attention T{T} {'rel-pos (2T-1 positions)' if rel else 'plain'}, clip 1 padded to {int(lens[1])}")


@pytest.mark.parametrize("C,zp,eps", [(1024, 1024, 1e-5), (1024, 0, 1e-5), (512, 0, 1e-12), (768, 0, 1e-12)])
def test_layernorm(C, zp, eps):
    B, T = 3, 37
    M = B * T
    g = torch.Generator().manual_seed(C + zp)
    x = torch.randn(M, C, generator=g) * 3 + 0.7
    gm, bt = torch.randn(C + zp, generator=g), torch.randn(C + zp, generator=g)
    lens = torch.tensor([37, 11, 0], dtype=torch.int32)
    keep = (torch.arange(T)[None, :] < lens[:, None]).reshape(M, 1)

    def run(dtype):
        xx = torch.cat([torch.zeros(M, zp, dtype=dtype), x.to(dtype)], 1)
        return F.layer_norm(xx, (C + zp,), gm.to(dtype), bt.to(dtype), eps) * keep.to(dtype)
    y = torch.full((M, C + zp), float("nan"), device="cuda")
    wide = torch.full((M, C + zp + 256), float("nan"), device="cuda")     # y2: the mel-head concat buffer's column window
    ops.layernorm(x.cuda(), gm.cuda(), bt.cuda(), eps, y, M=M, C=C, zero_prefix=zp, y2=wide[:, 256:], ldy2=C + zp + 256,
                  lens=lens.cuda(), len_mul=1, mask_T=T, dtype=DT)
    torch.cuda.synchronize()
    _assert_4x(y, run(torch.float64), run(torch.float32), f"layernorm C{C} zero_prefix{zp} eps{eps:g}")
    assert torch.equal(wide[:, 256:], y) and torch.isnan(wide[:, :256]).all()


def test_glu_dwconv_swish():
    B, T, C, k = 2, 200, 512, 31
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B * T, 2 * C, generator=g)
    w = torch.randn(k, C, generator=g) / k ** 0.5
    b = torch.randn(C, generator=g)
    lens = torch.tensor([100, 37], dtype=torch.int32)                      # x len_mul 2 = 200, 74 rows
    keep = (torch.arange(T)[None, :] < 2 * lens[:, None])

    def run(dtype):
        xx = x.to(dtype).view(B, T, 2 * C)
        glu = xx[..., :C] * torch.sigmoid(xx[..., C:]) * keep[..., None].to(dtype)
        y = F.conv1d(glu.transpose(1, 2), w.to(dtype).t()[:, None, :], b.to(dtype), padding=(k - 1) // 2, groups=C).transpose(1, 2)
        return (y * torch.sigmoid(y) * keep[..., None].to(dtype)).reshape(B * T, C)
    y = torch.full((B * T, C), float("nan"), device="cuda")
    ops.glu_dwconv_swish(x.cuda(), w.cuda(), b.cuda(), y, B=B, T=T, C=C, k=k, lens=lens.cuda(), len_mul=2, dtype=DT)
    torch.cuda.synchronize()
    _assert_4x(y, run(torch.float64), run(torch.float32), "glu_dwconv_swish T200 k31")


@pytest.mark.parametrize("relu_type", ["prelu", "swish"])
def test_stem_pool_avgpool(relu_type):
    from lip2speech_unit_amd import weights
    from lip2speech_unit_amd.resnet import ResEncoder
    from oracle import frontend as ofe
    enc = ResEncoder(relu_type, None, dtype=DT)
    sd = weights.synth_state_dict(weights.spec_of(enc), seed=1)
    if relu_type == "prelu":
        sd["frontend3D.2.weight"] = sd["frontend3D.2.weight"].abs().clamp(max=0.5)
    enc.load_state_dict(sd)
    enc.pack("cuda")
    P = enc._packed
    assert P["stem_w"].dtype == torch.float32
    B, T = 2, 5
    g = torch.Generator().manual_seed(7)
    x = ((torch.randint(0, 256, (B, T, 88, 88), generator=g).float() / 255.0 - 0.421) / 0.165).unsqueeze(1)
    rt = "swish" if relu_type == "swish" else None

    def run(dtype):
        s = {k_: (v_.to(dtype) if v_.is_floating_point() else v_) for k_, v_ in sd.items()}
        with torch.no_grad():
            st = ofe.stem(s, x.to(dtype), relu_type=rt)
            return st, ofe.stem_pool(st)
    (ref, refp), (y32, y32p) = run(torch.float64), run(torch.float32)
    y = torch.full((B * T, 44, 44, 64), float("nan"), device="cuda")
    ops.stem_conv3d(x[:, 0].contiguous().cuda(), P["stem_w"], P["stem_b"], P["stem_s"], y, B, T, DT)
    yp = torch.full((B * T, 22, 22, 64), float("nan"), device="cuda")
    ops.maxpool2d_3x3s2(y, yp, B * T, 44, 44, 64, DT)
    feat = torch.full((B * T, 64), float("nan"), device="cuda")
    ops.avgpool_hw(yp.view(B * T, 22 * 22, 64), feat, B * T, 22 * 22, 64, DT)
    torch.cuda.synchronize()

    def cl(t):      # [B, 64, T, h, w] -> [B*T, h, w, 64]
        return t.permute(0, 2, 3, 4, 1).reshape(B * T, t.shape[3], t.shape[4], 64)
    _assert_4x(y, cl(ref), cl(y32), f"stem conv3d ({relu_type})")
    _assert_4x(yp, cl(refp), cl(y32p), f"stem + maxpool ({relu_type})")
    _assert_4x(feat, cl(refp).mean(dim=(1, 2)), cl(y32p).mean(dim=(1, 2)), f"avgpool over 22 x 22 ({relu_type})")
    # the fused forms refuse fp32 instead of running 16-bit code on fp32 buffers
    from lip2speech_unit_amd import _lib
    with pytest.raises(_lib.L2SError, match="L2S_EUNSUPPORTED"):
        ops.stem_pool_fused(x[:, 0].contiguous().cuda(), P["stem_w"], P["stem_b"], P["stem_s"], yp, B, T, DT)


def test_preprocess_repeat_broadcast_rows():
    B, T, Hin, crop = 2, 3, 96, 88
    g = torch.Generator().manual_seed(1)
    u8 = torch.randint(0, 256, (B, T, Hin, Hin), generator=g, dtype=torch.uint8)
    y = torch.empty(B, T, crop, crop, device="cuda")
    ops.preprocess_frames(u8.cuda(), y, B=B, T=T, Hin=Hin, Win=Hin, crop=crop, dtype=DT)
    d = (Hin - crop) // 2
    c = u8[:, :, d:d + crop, d:d + crop]
    _assert_4x(y, (c.double() / 255.0 - 0.421) / 0.165, (c.float() / 255.0 - 0.421) / 0.165, "preprocess_frames")
    x = torch.randn(B * T, 64, generator=g)
    r2 = torch.empty(B * 2 * T, 64, device="cuda")
    ops.repeat2_cast(x.cuda(), r2, B, T, 64, DT)
    assert torch.equal(r2.cpu(), x.repeat_interleave(2, dim=0))
    spk = torch.randn(B, 16, generator=g)
    lens = torch.tensor([3, 1], dtype=torch.int32)
    cat = torch.full((B * T, 24), float("nan"), device="cuda")
    ops.broadcast_rows(spk.cuda(), cat, B=B, T=T, C=16, ldy=24, col0=4, lens=lens.cuda(), len_mul=1, dtype=DT)
    want = spk[:, None, :].expand(B, T, 16).clone()
    want[1, 1:] = 0
    assert torch.equal(cat[:, 4:20].cpu(), want.reshape(B * T, 16)) and torch.isnan(cat[:, :4]).all() and torch.isnan(cat[:, 20:]).all()
    m = torch.full((B * T, 24), float("nan"), device="cuda")
    ops.rows_f32_to_16_masked(x[:, :16].contiguous().cuda(), m, B=B, T=T, C=16, ldx=16, ldy=24, col0=8, lens=lens.cuda(), dtype=DT)
    wantm = x[:, :16].clone().view(B, T, 16)
    wantm[1, 1:] = 0
    assert torch.equal(m[:, 8:].cpu(), wantm.reshape(B * T, 16))
