#!/usr/bin/env python3
"""Runs one part of the sequence-kernel matrix (tests/_seq_cases.py) under the switches of its environment,

    [L2S_ATTN_RESIDENT=0] [L2S_ATTN_RESIDENT_PLAIN=1] [L2S_ATTN_QB=64|128] [L2S_LN_ROWS=0] check_seq_kernels.py <environment>

<environment> is a key of sc.ENVS and the process must carry exactly its switches: the launchers read them once per process, hence
one child process per environment (tests/test_seq_matrix_gpu.py).  Two modes need no device:

    check_seq_kernels.py --route <environment>   the restated selection rules of sc against the library's host-only queries
                                                 (T = 1..1300, with and without pos, ...) and every case against its `inst`
    check_seq_kernels.py --cpu-f32               each operation in torch fp32 on the CPU against fp64: the figures behind sc.F_of

Every case runs on operands that are views into NaN-filled device buffers (guard rows around every buffer, NaN in the padding
columns of the leading dimensions, `out` / `y` prefilled with NaN) and is checked for: the queried instantiation is the one the
case claims, no NaN inside the written window (so every row is written), every byte outside it unchanged, the inputs unchanged,
masked rows exactly zero, and two error criteria against the operation in fp64 on the CPU -
  (a) max error <= tol * max|ref|, the criterion and tolerances of tests/test_kernels_gpu.py for that kernel and type;
  (b) |got - ref| <= 1.5 u |ref| [16-bit output] + 1.5 u A [attention: P is rounded to 16 bits] + F 2^-24 A per element,
      u = 2^-11 f16 / 2^-8 bf16 (|ref| floored at the type's smallest normal number: below it half an ulp is constant),
      A = the operation on absolute values in fp64, F = sc.F_of(op);
  (c) LayerNorm only: (b) with A2 = |gamma| (|x| + mean|x|) rstd + |beta| in the place of A = |gamma| |x - mean| rstd + |beta|
      and its own, small F (profiles/seq_kernels_matrix.md says why (b) alone is loose there).
Prints the worst err / bound per instantiation for both criteria and exits non-zero on any failure."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lip2speech_unit_amd import _lib  # noqa: E402
from tests import _seq_cases as sc  # noqa: E402

U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
MIN_NORMAL = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}
# (a): the tolerances of tests/test_kernels_gpu.py (test_attention, test_layernorm, test_glu_dwconv_swish)
TOL_ATTN = {"f16": 4e-3, "bf16": 2.5e-2}
TOL_LN16 = {"f16": 2e-3, "bf16": 1.2e-2}
TOL_GLU = {"f16": 2e-3, "bf16": 1.2e-2}
LN32_REL, LN32_ABS = 2e-5, 1e-5
EPS24 = 2.0 ** -24
NAN = float("nan")
f64, f32 = torch.float64, torch.float32
FAKE = 0x10000                               # a 16-byte aligned non-null "pointer" for the host-only queries


def t16(dt):
    return torch.float16 if dt == "f16" else torch.bfloat16


def rnd(x, dt):
    return x.to(t16(dt)).to(f64)


def bits(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def seed_of(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c["name"] + c["dt"])) % (2 ** 31)


# ---- the operations, in fp64 (reference) or fp32 (the figures behind F) -------------------------------------------------------------
def attn_inputs(c):
    """q, k, v [B, H, T, 64], pos [H, 2T-1, 64] (values of the 16-bit type), u, vb [H, 64] (fp32 values); all fp64."""
    B, T, H, dt = c["B"], c["T"], c["H"], c["dt"]
    g = torch.Generator().manual_seed(seed_of(c))
    qkv = torch.randn(B, T, 3, H, sc.D, generator=g, dtype=f64)
    qkv[:, :, 0] *= 0.35
    if c["data"] == "rescale":
        a = 0.35 * torch.randn(H, sc.D, generator=g, dtype=f64)
        gain = 60.0 / (a * a).sum(-1, keepdim=True)
        sign = torch.where(torch.arange(T) < T // 2, 1.0, -1.0).to(f64).view(1, T, 1, 1)
        qkv[:, :, 0] = sign * a + 0.05 * torch.randn(B, T, H, sc.D, generator=g, dtype=f64)
        qkv[:, T - 1, 1] = gain * a            # the dominant key of rows < T / 2: last key tile
        qkv[:, 0, 1] = -gain * a               # ... of the other rows: first key tile
    for b, n in enumerate(sc.klens(c)):
        qkv[b, n:] = 1000.0                    # rows past the clip's length: finite on purpose (0 x NaN in V would be NaN)
    qkv = rnd(qkv, dt)
    pos = rnd(0.5 * torch.randn(2 * T - 1, H, sc.D, generator=g, dtype=f64), dt)
    u = (0.1 * torch.randn(H, sc.D, generator=g)).to(f64)
    vb = (0.1 * torch.randn(H, sc.D, generator=g)).to(f64)
    return qkv, pos, u, vb


def attn_eval(c, qkv, pos, u, vb, ft, mirror=True):
    """(out, A) [B, T, H*64] in float type ft.  mirror: q+u and q+v are formed in fp32 and rounded to 16 bits, as the kernels
    document; A = softmax(s) |v|."""
    B, T, H, dt = c["B"], c["T"], c["H"], c["dt"]
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).to(ft) for i in range(3))
    outs, As = [], []
    for b, n in enumerate(sc.klens(c)):
        if c["pos"]:
            if mirror:
                qu = rnd(q[b].float() + u.float()[:, None], dt).to(ft)
                qv = rnd(q[b].float() + vb.float()[:, None], dt).to(ft)
            else:
                qu, qv = q[b] + u.to(ft)[:, None], q[b] + vb.to(ft)[:, None]
            full = (qv @ pos.permute(1, 2, 0).to(ft)).contiguous()              # [H, T, 2T-1]; score (i, j) uses row T-1-i+j
            bd = torch.as_strided(full, (H, T, T), (T * (2 * T - 1), 2 * T - 2, 1), T - 1)
            s = qu @ k[b].transpose(-1, -2) + bd
        else:
            s = q[b] @ k[b].transpose(-1, -2)
        if n == 0:
            p = torch.zeros_like(s)
        else:
            s = s.masked_fill((torch.arange(T) >= n)[None, None, :], float("-inf"))
            p = torch.softmax(s, -1)
        outs.append((p @ v[b]).transpose(0, 1).reshape(T, H * sc.D))
        As.append((p @ v[b].abs()).transpose(0, 1).reshape(T, H * sc.D))
    return torch.stack(outs), torch.stack(As)


def ln_inputs(c, C=None):
    M, C, dt = c["M"], c["C"], c["dt"]
    W = C + c.get("zp", 0)
    g = torch.Generator().manual_seed(seed_of(c))
    if c.get("data") == "offset":
        x = 100.0 + 0.01 * torch.randn(M, C, generator=g)
    else:
        x = 0.3 + 2.0 * torch.randn(M, C, generator=g)
    if c.get("zero_row"):
        x[0] = 0.0
    x = x.to(f64) if c.get("xf", True) else rnd(x, dt)
    gamma = (torch.rand(W, generator=g) + 0.5).to(f64)
    beta = (0.1 * torch.randn(W, generator=g)).to(f64)
    P = torch.randn(M, c["S"], C, generator=g).to(f64) if c["op"] == "skln" else None
    return x, gamma, beta, P


def ln_eval(c, x, gamma, beta, ft, xabs=None):
    """(y, A, A2) [M, zp + C]: LayerNorm of [zeros(zp) || x] in float type ft; A = |gamma| |x - mean| rstd + |beta|,
    A2 = |gamma| (|x| + mean|x|) rstd + |beta| (absolute values BEFORE the mean is taken off, `xabs` for a row that is itself a sum)."""
    xin = torch.cat([torch.zeros(x.shape[0], c.get("zp", 0), dtype=ft), x.to(ft)], 1)
    gamma, beta = gamma.to(ft), beta.to(ft)
    if ft == f32:
        y = F.layer_norm(xin, (xin.shape[1],), gamma, beta, c["eps"])
        return y, None, None
    mean = xin.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xin - mean) ** 2).mean(1, keepdim=True) + c["eps"])
    xa = xin.abs() if xabs is None else xabs
    return ((xin - mean) * rstd * gamma + beta, gamma.abs() * (xin - mean).abs() * rstd + beta.abs(),
            gamma.abs() * (xa + xa.mean(1, keepdim=True)) * rstd + beta.abs())


def skln_sum(x, P, ft):
    v = x.to(ft)
    for s in range(P.shape[1]):
        v = v + P[:, s].to(ft)
    return v


def glu_inputs(c):
    B, T, C, k, dt = c["B"], c["T"], c["C"], c["k"], c["dt"]
    g = torch.Generator().manual_seed(seed_of(c))
    x = rnd(torch.randn(B, T, 2 * C, generator=g), dt)
    w = (torch.randn(C, k, generator=g) / k ** 0.5).to(f64)
    bias = (0.1 * torch.randn(C, generator=g)).to(f64)
    return x, w, bias


def glu_eval(c, x, w, bias, ft):
    """(y, A) [B, T, C]: GLU -> depthwise conv (zero padding at the clip's length) -> swish; A = sum |w| |glu| + |bias|."""
    T, C, k = c["T"], c["C"], c["k"]
    ys, As = [], []
    for b, n in enumerate(sc.glu_lims(c)):
        y, A = torch.zeros(T, C, dtype=ft), torch.zeros(T, C, dtype=ft)
        if n > 0:
            gl = F.glu(x[b:b + 1, :n].to(ft).transpose(1, 2), dim=1)
            acc = F.conv1d(gl, w.to(ft)[:, None, :], bias.to(ft), padding=(k - 1) // 2, groups=C)
            y[:n] = (acc * torch.sigmoid(acc)).transpose(1, 2)[0]
            A[:n] = F.conv1d(gl.abs(), w.to(ft).abs()[:, None, :], bias.to(ft).abs(), padding=(k - 1) // 2, groups=C).transpose(1, 2)[0]
        ys.append(y)
        As.append(A)
    return torch.stack(ys), torch.stack(As)


# ---- criteria --------------------------------------------------------------------------------------------------------------------------
def bound_b(ref, A, dt, out16, kind, attn=False):
    # half an ulp of the output type is u |ref| down to the type's smallest normal number and constant below it (f16: 2^-25
    # under 2^-14; a swish or LayerNorm output that crosses zero gets there)
    ulp = U16[dt] * ref.abs().clamp(min=MIN_NORMAL[dt])
    return (sc.FU * ulp if out16 else 0.0) + (sc.FU * U16[dt] * A if attn else 0.0) + sc.F_of(kind) * EPS24 * A


def ratio_b(err, bound):
    """max err / bound; an element whose bound is zero must be exact."""
    q = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return q.max().item() if q.numel() else 0.0


class Report:
    def __init__(self, env):
        self.env, self.fail, self.worst, self.count = env, [], {}, {}

    def ratio(self, case, crit, r):
        k = (case["inst"], crit)
        self.worst[k] = max(self.worst.get(k, 0.0), r)

    def bad(self, case, why):
        self.fail.append(f"FAIL env={self.env} {case['dt']} {case['name']} inst={case['inst'][2]}: {why}")

    def judge(self, case, what, got, ref, A, tol_abs, out16, kind, attn=False):
        """Both criteria on one window (got, ref, A: fp64, same shape).  A case with `skip_a` reports (a) as (s) and is not held to it."""
        if got.numel() == 0:
            return
        err = (got - ref).abs()
        ra = err.max().item() / tol_abs
        self.ratio(case, "s" if case.get("skip_a") else "a", ra)
        if ra > 1.0 and not case.get("skip_a"):
            self.bad(case, f"(a) {what}: max err / tolerance = {ra:.3f}")
        bound = bound_b(ref, A, case["dt"], out16, kind, attn)
        rb = ratio_b(err, bound)
        self.ratio(case, "b", rb)
        if rb > 1.0:
            i = (err / bound.clamp(min=1e-300)).reshape(-1).argmax().item()
            self.bad(case, f"(b) {what}: err / bound = {rb:.3f} at flat index {i} (got {got.reshape(-1)[i].item():.9g}, "
                           f"ref {ref.reshape(-1)[i].item():.9g})")


def guarded(rows, ld, dtype, guard):
    return torch.full((rows + 2 * guard, ld), NAN, dtype=dtype)


def unchanged(rep, case, name, dev, host):
    if not torch.equal(bits(dev.cpu()), bits(host)):
        rep.bad(case, f"operand {name} changed")


def outside_unchanged(rep, case, name, after, before, win):
    stray = (bits(after) != bits(before)) & ~win
    if stray.any():
        rep.bad(case, f"{stray.sum().item()} elements of {name} outside the window changed")


# ---- queries ---------------------------------------------------------------------------------------------------------------------------
def dtc(dt):
    return _lib.F16 if dt == "f16" else _lib.BF16


def query_attn(lib, c, qkv=FAKE, out=FAKE, pos=FAKE, aux=FAKE):
    has = c["pos"]
    return lib.l2s_attention_variant(qkv, c["ldq"], out, c["ldo"], pos if has else None, c["ldp"] if has else 0, aux if has else None,
                                     aux if has else None, aux if c["lens"] is not None else None, c["len_mul"], c["B"], c["T"], c["H"],
                                     dtc(c["dt"]))


def query_ln(lib, c, x=FAKE, y=None, y2=FAKE, aux=FAKE):
    y = y if y is not None else FAKE + 2 * c["y_off"]
    m = c["mask"]
    return lib.l2s_layernorm_variant(x, int(c["xf"]), c["ldx"], aux, aux, y, int(c["yf"]), c["ldy"], y2 if c["y2"] else None, c["ldy2"],
                                     c["M"], c["C"], c["zp"], aux if m else None, m[1] if m else 1, m[0] if m else 0, dtc(c["dt"]))


def query_glu(lib, c):
    return lib.l2s_glu_dwconv_tile(c["B"], c["T"], c["C"], c["k"], dtc(c["dt"]))


# ---- one case on the device ------------------------------------------------------------------------------------------------------------
def run_attn(c, lib, ops, rep):
    B, T, H, dt, G = c["B"], c["T"], c["H"], c["dt"], sc.ATTN_GUARD
    HD, el = H * sc.D, t16(dt)
    qkv, pos, u, vb = attn_inputs(c)
    hq = guarded(B * T, c["ldq"], el, G)
    hq[G: G + B * T, : 3 * HD] = qkv.reshape(B * T, 3 * HD).to(el)
    ho = guarded(B * T, c["ldo"], el, G)
    dq, do = hq.cuda(), ho.cuda()
    kw = {}
    dp = hp = None
    if c["pos"]:
        hp = guarded(2 * T - 1, c["ldp"], el, G)
        hp[G: G + 2 * T - 1, sc.POS_LI * HD: (sc.POS_LI + 1) * HD] = pos.reshape(2 * T - 1, HD).to(el)
        dp = hp.cuda()
        kw = dict(pos=dp[G:, sc.POS_LI * HD:], ldp=c["ldp"], bias_u=u.float().cuda(), bias_v=vb.float().cuda())
    dlens = torch.tensor(c["lens"], dtype=torch.int32).cuda() if c["lens"] is not None else None
    var = query_attn(lib, c, dq[G:].data_ptr(), do[G:].data_ptr(), kw["pos"].data_ptr() if c["pos"] else None)
    if var != c["inst"][2]:
        rep.bad(c, f"instantiation: the query answers {var}")
        return
    ops.attention(dq[G:], do[G:], B=B, T=T, H=H, ldq=c["ldq"], ldo=c["ldo"], lens=dlens, len_mul=c["len_mul"], dtype=dtc(dt), **kw)
    torch.cuda.synchronize()
    after = do.cpu()
    win = torch.zeros(ho.shape, dtype=torch.bool)
    win[G: G + B * T, :HD] = True
    outside_unchanged(rep, c, "out", after, ho, win)
    unchanged(rep, c, "qkv", dq, hq)
    if dp is not None:
        unchanged(rep, c, "pos", dp, hp)
    got = after[G: G + B * T, :HD].to(f64).view(B, T, HD)
    if not torch.isfinite(got).all():
        rep.bad(c, f"{(~torch.isfinite(got)).sum().item()} NaN / Inf in the window of out")
        return
    ref, A = attn_eval(c, qkv, pos, u, vb, f64)
    ref_plain = attn_eval(c, qkv, pos, u, vb, f64, mirror=False)[0] if c["pos"] else ref
    lens = sc.klens(c)
    valid = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(lens):
        valid[b, :n] = True
        if n == 0 and bool((got[b] != 0).any()):
            rep.bad(c, f"clip {b} has no keys: its rows are not exactly zero")
    if not valid.any():
        return
    tol = TOL_ATTN[dt]
    rep.judge(c, "out", got[valid], ref[valid], A[valid], tol * ref[valid].abs().max().item(), True, "attn", attn=True)
    ru = (got[valid] - ref_plain[valid]).abs().max().item() / (2 * tol * ref_plain[valid].abs().max().item())
    rep.ratio(c, "u", ru)
    if ru > 1.0:
        rep.bad(c, f"(a) un-mirrored: max err / tolerance = {ru:.3f}")


def flat_window(rows, ld, W, off, guard):
    """A flat NaN buffer holding [rows, ld] behind `guard` rows and `off` elements; (buffer length, base, window mask)."""
    n = (rows + 2 * guard) * ld + 8
    base = guard * ld + off
    win = torch.zeros(n, dtype=torch.bool)
    for r in range(rows):
        win[base + r * ld: base + r * ld + W] = True
    return n, base, win


def read_window(flat, base, rows, ld, W):
    return torch.stack([flat[base + r * ld: base + r * ld + W] for r in range(rows)]) if rows else flat[:0].view(0, W)


def check_ln_output(rep, c, what, got, ref, A, A2, keep, out16, kind, beta):
    dt = c["dt"]
    if torch.isnan(got).any():
        rep.bad(c, f"{torch.isnan(got).sum().item()} NaN in the window of {what}")
        return
    got = got.to(f64)
    if keep is not None:
        k = torch.tensor(keep)
        if bool((got[~k] != 0).any()):
            rep.bad(c, f"masked rows of {what} are not exactly zero")
        got, ref, A, A2 = got[k], ref[k], A[k], A2[k]
    if c.get("zero_row"):
        want = rnd(beta, dt) if out16 else beta.float().to(f64)
        if not torch.equal(got[0], want):
            rep.bad(c, f"the all-zero row of {what} is not exactly beta")
    mx = ref.abs().max().item() if ref.numel() else 0.0
    tol_abs = TOL_LN16[dt] * mx if out16 else LN32_REL * mx + LN32_ABS
    rep.judge(c, what, got, ref, A, tol_abs, out16, kind)
    # (c): the same bound on the scale that carries the rounding of the mean (A vanishes where x = mean and beta = 0, that error
    # does not): the tight one of the two, F = sc.F_of("ln2")
    if got.numel():
        rc = ratio_b((got - ref).abs(), bound_b(ref, A2, dt, out16, "ln2" if kind != "skln" else "skln2"))
        rep.ratio(c, "c", rc)
        if rc > 1.0:
            rep.bad(c, f"(c) {what}: err / bound = {rc:.3f}")


def run_ln(c, lib, ops, rep):
    M, C, dt, G = c["M"], c["C"], c["dt"], sc.LN_GUARD
    W, el = C + c["zp"], t16(dt)
    x, gamma, beta, _ = ln_inputs(c)
    keep = sc.ln_keep(c)
    hx = guarded(M, c["ldx"], f32 if c["xf"] else el, G)
    hx[G: G + M, :C] = x.to(hx.dtype)
    if keep is not None:
        for r in range(M):
            if not keep[r]:
                hx[G + r, :C] = NAN           # a masked row is never used
    dx = hx.cuda()
    ydt = f32 if c["yf"] else el
    if c["inplace"]:
        dy_view, hy, dy, ybase = dx[G:], None, None, None
    else:
        n, ybase, ywin = flat_window(M, c["ldy"], W, c["y_off"], G)
        hy = torch.full((n,), NAN, dtype=ydt)
        dy = hy.cuda()
        dy_view = dy[ybase:]
    dy2 = hy2 = None
    if c["y2"]:
        n2, y2base, y2win = flat_window(M, c["ldy2"], W, 0, G)
        hy2 = torch.full((n2,), NAN, dtype=el)
        dy2 = hy2.cuda()
    m = c["mask"]
    dlens = torch.tensor(m[2], dtype=torch.int32).cuda() if m else None
    var = query_ln(lib, c, dx[G:].data_ptr(), dy_view.data_ptr(), dy2[y2base:].data_ptr() if c["y2"] else None)
    if var != c["inst"][2]:
        rep.bad(c, f"instantiation: the query answers {var}")
        return
    ops.layernorm(dx[G:], gamma.float().cuda(), beta.float().cuda(), c["eps"], dy_view, M=M, C=C, ldx=c["ldx"], ldy=c["ldy"],
                  y2=dy2[y2base:] if c["y2"] else None, ldy2=c["ldy2"], zero_prefix=c["zp"], lens=dlens, len_mul=m[1] if m else 1,
                  mask_T=m[0] if m else 0, dtype=dtc(dt))
    torch.cuda.synchronize()
    ref, A, A2 = ln_eval(c, x, gamma, beta, f64)
    if c["inplace"]:
        after = dx.cpu()
        win = torch.zeros(hx.shape, dtype=torch.bool)
        win[G: G + M, :W] = True
        outside_unchanged(rep, c, "y (in place)", after, hx, win)
        got = after[G: G + M, :W]
    else:
        after = dy.cpu()
        outside_unchanged(rep, c, "y", after, hy, ywin)
        unchanged(rep, c, "x", dx, hx)
        got = read_window(after, ybase, M, c["ldy"], W)
    check_ln_output(rep, c, "y", got, ref, A, A2, keep, not c["yf"], "ln-offset" if c["data"] == "offset" else "ln", beta)
    if c["y2"]:
        after2 = dy2.cpu()
        outside_unchanged(rep, c, "y2", after2, hy2, y2win)
        check_ln_output(rep, c, "y2", read_window(after2, y2base, M, c["ldy2"], W), ref, A, A2, keep, True,
                        "ln-offset" if c["data"] == "offset" else "ln", beta)


def run_skln(c, lib, ops, rep):
    M, C, S, dt, G = c["M"], c["C"], c["S"], c["dt"], sc.LN_GUARD
    el = t16(dt)
    x, gamma, beta, P = ln_inputs(c)
    keep = sc.ln_keep(c)
    hx = guarded(M, c["ldx"], f32, G)
    hx[G: G + M, :C] = x.float()
    hP = guarded(M, c["ldp"], f32, G)
    hP[G: G + M, : S * C] = P.reshape(M, S * C).float()
    dx, dP = hx.cuda(), hP.cuda()
    if c["inplace"]:
        dy_view = dx[G:]
    else:
        n, ybase, ywin = flat_window(M, c["ldy"], C, 0, G)
        hy = torch.full((n,), NAN, dtype=el)
        dy = hy.cuda()
        dy_view = dy[ybase:]
    m = c["mask"]
    dlens = torch.tensor(m[2], dtype=torch.int32).cuda() if m else None
    ops.splitk_reduce_layernorm(dP[G:], dx[G:], gamma.float().cuda(), beta.float().cuda(), c["eps"], dy_view, M=M, C=C, S=S,
                                ldp=c["ldp"], ldx=c["ldx"], ldy=c["ldy"], lens=dlens, len_mul=m[1] if m else 1,
                                mask_T=m[0] if m else 0, dtype=dtc(dt))
    torch.cuda.synchronize()
    v = skln_sum(x, P, f64)
    Sabs = x.abs() + P.abs().sum(1)
    ref, A, A2 = ln_eval(c, v, gamma, beta, f64, xabs=Sabs)
    unchanged(rep, c, "P", dP, hP)
    afterx = dx.cpu()
    win = torch.zeros(hx.shape, dtype=torch.bool)
    win[G: G + M, :C] = True
    outside_unchanged(rep, c, "x", afterx, hx, win)
    gotx = afterx[G: G + M, :C]
    if c["inplace"]:
        check_ln_output(rep, c, "y (over x)", gotx, ref, A, A2, keep, False, "skln", beta)
        return
    # the updated stream: S fp32 additions in ascending order, each within half an ulp of its partial sum <= |x| + sum |P|
    rx = ratio_b((gotx.to(f64) - v).abs(), (S + 1) * EPS24 * Sabs)
    rep.ratio(c, "x", rx)
    if not rx <= 1.0:
        rep.bad(c, f"updated x: err / ((S + 1) 2^-24 (|x| + sum |P|)) = {rx:.3f}")
    after = dy.cpu()
    outside_unchanged(rep, c, "y", after, hy, ywin)
    check_ln_output(rep, c, "y", read_window(after, ybase, M, c["ldy"], C), ref, A, A2, keep, True, "skln", beta)


def run_glu(c, lib, ops, rep):
    B, T, C, k, dt, G = c["B"], c["T"], c["C"], c["k"], c["dt"], sc.GLU_GUARD
    el = t16(dt)
    x, w, bias = glu_inputs(c)
    lims = sc.glu_lims(c)
    hx = guarded(B * T, 2 * C, el, G)
    hx[G: G + B * T] = x.reshape(B * T, 2 * C).to(el)
    for b, n in enumerate(lims):
        hx[G + b * T + n: G + (b + 1) * T] = NAN          # rows past the clip's length are never read
    hy = guarded(B * T, C, el, G)
    hw = torch.cat([w.t().contiguous().reshape(-1).float(), torch.full((256,), NAN)])
    hb = torch.cat([bias.float(), torch.full((64,), NAN)])
    dx, dy, dw, db = hx.cuda(), hy.cuda(), hw.cuda(), hb.cuda()
    dlens = torch.tensor(c["lens"], dtype=torch.int32).cuda() if c["lens"] is not None else None
    var = query_glu(lib, c)
    if var != c["inst"][2]:
        rep.bad(c, f"instantiation: the query answers {var}")
        return
    ops.glu_dwconv_swish(dx[G:], dw, db, dy[G:], B=B, T=T, C=C, k=k, lens=dlens, len_mul=c["len_mul"], dtype=dtc(dt))
    torch.cuda.synchronize()
    after = dy.cpu()
    win = torch.zeros(hy.shape, dtype=torch.bool)
    win[G: G + B * T] = True
    outside_unchanged(rep, c, "y", after, hy, win)
    unchanged(rep, c, "x", dx, hx)
    got = after[G: G + B * T]
    if torch.isnan(got).any():
        rep.bad(c, f"{torch.isnan(got).sum().item()} NaN in the window of y")
        return
    got = got.to(f64).view(B, T, C)
    for b, n in enumerate(lims):
        if bool((got[b, n:] != 0).any()):
            rep.bad(c, f"rows past the length of clip {b} are not exactly zero")
    ref, A = glu_eval(c, x, w, bias, f64)
    rep.judge(c, "y", got, ref, A, TOL_GLU[dt] * ref.abs().max().item() + 1e-300, True, "glu")


RUN = {"attn": run_attn, "ln": run_ln, "skln": run_skln, "glu": run_glu}


# ---- host-only modes -------------------------------------------------------------------------------------------------------------------
def route(env_name, lib):
    """The restated rules against the queries under this process's switches; every case of the environment against its `inst`."""
    env = {k: os.environ[k] for k in sc.SWITCHES if k in os.environ}
    bad = n = 0

    def expect(what, got, want):
        nonlocal bad, n
        n += 1
        if got != want:
            bad += 1
            if bad < 20:
                print(f"ROUTE {what}: the query answers {got}, the restated rule {want}")

    for dt in sc.DTYPES:
        for T in range(1, 1301):
            for pos in (False, True):
                for H in (1, 8, 256, 257):
                    c = dict(dt=dt, B=2, T=T, H=H, pos=pos, lens=[T, 1], len_mul=1, ldq=3 * H * 64 + 8, ldo=H * 64 + 4, ldp=3 * H * 64)
                    expect(f"attention {dt} T={T} H={H} pos={pos}", query_attn(lib, c), sc.attention_variant(T, H, pos, env))
            expect(f"glu {dt} T={T}", lib.l2s_glu_dwconv_tile(2, T, 64, 31, dtc(dt)), sc.glu_tile(T))
        for C in (4, 252, 256, 260, 512, 768, 1024, 2048):
            for xf in (0, 1):
                for yf in (0, 1):
                    for y2 in (0, 1):
                        for zp in (0, 4):
                            for ldy in (C + zp, C + zp + 4, C + zp + 8):
                                for yoff in (0, 4, 8):
                                    c = dict(dt=dt, M=5, C=C, xf=xf, yf=yf, y2=y2, zp=zp, ldx=C, ldy=ldy, ldy2=C + zp, y_off=yoff, mask=None)
                                    want = sc.layernorm_variant(C, xf, yf, y2, zp, ldy, (2 * yoff) % 16 == 0, env)
                                    expect(f"layernorm {dt} C={C} xf={xf} yf={yf} y2={y2} zp={zp} ldy={ldy} yoff={yoff}", query_ln(lib, c), want)
    # what a launch refuses, the query refuses with the same code; fp32 names no 16-bit kernel
    expect("attention ldq % 8", lib.l2s_attention_variant(FAKE, 3 * 64 + 4, FAKE, 64, None, 0, None, None, None, 1, 1, 5, 1, 0), sc.EALIGN)
    expect("attention fp32", lib.l2s_attention_variant(FAKE, 192, FAKE, 64, None, 0, None, None, None, 1, 1, 5, 1, _lib.F32), sc.SEQ_VARIANT_F32)
    expect("layernorm C % 4", lib.l2s_layernorm_variant(FAKE, 1, 8, FAKE, FAKE, FAKE, 1, 8, None, 0, 1, 6, 0, None, 1, 0, 0), sc.EALIGN)
    expect("layernorm fp32", lib.l2s_layernorm_variant(FAKE, 1, 8, FAKE, FAKE, FAKE, 1, 8, None, 0, 1, 8, 0, None, 1, 0, _lib.F32), sc.SEQ_VARIANT_F32)
    expect("glu C % 64", lib.l2s_glu_dwconv_tile(1, 5, 32, 31, 0), sc.EALIGN)
    expect("glu fp32", lib.l2s_glu_dwconv_tile(1, 5, 64, 31, _lib.F32), sc.SEQ_VARIANT_F32)
    if env_name in sc.ENVS and env == sc.ENVS[env_name]:
        for c in sc.cases_of(env_name):
            if c["op"] != "skln":
                expect(f"case {c['dt']} {c['name']}", {"attn": query_attn, "ln": query_ln, "glu": query_glu}[c["op"]](lib, c), c["inst"][2])
    print(f"routed {n - bad} of {n} queries under {env}")
    return bad


def cpu_f32():
    """Each operation in torch fp32 on the CPU against fp64, in units of 2^-24 A: the figures of sc.CPU_F32_WORST."""
    worst = {}
    seen = set()
    for env_name in sc.ENVS:
        for c in sc.cases_of(env_name):
            key = (c["op"], c["dt"], c["name"])
            if key in seen:
                continue
            seen.add(key)
            if c["op"] == "attn":
                ins = attn_inputs(c)
                ref, A = attn_eval(c, *ins, f64)
                got = attn_eval(c, *ins, f32)[0].to(f64)
                valid = torch.zeros(c["B"], c["T"], dtype=torch.bool)
                for b, n in enumerate(sc.klens(c)):
                    valid[b, :n] = True
                got, ref, A, kind = got[valid], ref[valid], A[valid], "attn"
            elif c["op"] in ("ln", "skln"):
                x, gamma, beta, P = ln_inputs(c)
                xabs = None
                if c["op"] == "skln":
                    got = ln_eval(c, skln_sum(x, P, f32), gamma, beta, f32)[0].to(f64)
                    xabs = x.abs() + P.abs().sum(1)
                    x = skln_sum(x, P, f64)
                else:
                    got = ln_eval(c, x, gamma, beta, f32)[0].to(f64)
                ref, A, A2 = ln_eval(c, x, gamma, beta, f64, xabs=xabs)
                kind = "skln" if c["op"] == "skln" else ("ln-offset" if c["data"] == "offset" else "ln")
                k2 = ("skln2" if c["op"] == "skln" else "ln2", c["dt"])
                r2 = ratio_b((got - ref).abs(), EPS24 * A2)
                if r2 > worst.get(k2, (0.0, ""))[0]:
                    worst[k2] = (r2, c["name"])
            else:
                ins = glu_inputs(c)
                ref, A = glu_eval(c, *ins, f64)
                got, kind = glu_eval(c, *ins, f32)[0].to(f64), "glu"
            r = ratio_b((got - ref).abs(), EPS24 * A)
            k = (kind, c["dt"])
            if r > worst.get(k, (0.0, ""))[0]:
                worst[k] = (r, c["name"])
    for (kind, dt), (r, name) in sorted(worst.items()):
        print(f"CPUF32 {kind:10s} {dt:4s} worst |fp32 - fp64| / (2^-24 A) = {r:8.3f}  ({name})")
    for kind in sorted({k for k, _ in worst}):
        print(f"CPUF32 {kind:10s} worst over both types = {max(worst[(kind, dt)][0] for dt in sc.DTYPES if (kind, dt) in worst):.3f}")


def main():
    args = sys.argv[1:]
    usage = f"usage: check_seq_kernels.py [--route] <{' | '.join(sc.ENVS)}>  or  check_seq_kernels.py --cpu-f32"
    if not args or args[0] in ("-h", "--help"):
        sys.exit(usage)
    if args[0] == "--cpu-f32":
        cpu_f32()
        return
    route_only = args[0] == "--route"
    env_name = args[-1]
    if len(args) != (2 if route_only else 1) or (not route_only and env_name not in sc.ENVS):
        sys.exit(usage)
    lib = _lib.load()
    if route_only:
        sys.exit(1 if route(env_name, lib) else 0)
    for name in sc.SWITCHES:                 # exactly the environment's switches
        assert os.environ.get(name) == sc.ENVS[env_name].get(name), (name, os.environ.get(name))
    from lip2speech_unit_amd import ops
    rep = Report(env_name)
    t0 = time.time()
    cases = sc.cases_of(env_name)
    count = {}
    for case in cases:
        RUN[case["op"]](case, lib, ops, rep)
        count[case["inst"]] = count.get(case["inst"], 0) + 1
    dt_s = time.time() - t0
    print(f"env {env_name}: {len(cases)} cases, {len(rep.fail)} failures, {dt_s:.1f} s")
    for inst in sorted(count):
        cells = " ".join(f"({crit}) {rep.worst[(inst, crit)]:6.3f}" for crit in "abcuxs" if (inst, crit) in rep.worst)
        print(f"RATIO {env_name} {inst[0]} {inst[1]} {inst[2]} cases {count[inst]} {cells}")
    for line in rep.fail:
        print(line)
    sys.exit(1 if rep.fail else 0)


if __name__ == "__main__":
    main()
