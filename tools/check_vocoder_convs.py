#!/usr/bin/env python3
"""Runs one part of the vocoder-convolution matrix (tests/_vocconv_cases.py) under the switches of its environment,

    [L2S_RESPAIR_PHASE=0] [L2S_RESPAIR_XCD=0] [L2S_RESPAIR_SLOTS=8] check_vocoder_convs.py <environment>

<environment> is a key of vc.ENVS and the process must carry exactly its switches: the launchers read them once per process, hence
one child process per environment (tests/test_vocconv_matrix_gpu.py).  Two modes need no device:

    check_vocoder_convs.py --route <environment>   the restated selection rule of vc against l2s_respair_variant (every C, k, dil)
                                                   and every `pair` case of the environment against its `inst`
    check_vocoder_convs.py --cpu-f32               each operation in torch fp32 on the CPU, with the kernels' 16-bit intermediate
                                                   roundings, against the mirrored fp64 reference: the figures behind vc.F_of

References are fp64 on the CPU, each clip alone over its valid rows, convolutions as unfold + matmul.  The MIRRORED reference
applies the 16-bit roundings the kernels document: the input is the leaky_relu copy, the residual is recovered from it by the
inverse, t1 is rounded after bias + LeakyReLU + length mask, and in csrc/resblock.hip the hand-over between the pairs goes through
the 16-bit XL buffer (so the next pair's residual is the inverse of that ROUNDED copy; tests/test_kernels_gpu.py carries it
unrounded).  The UN-MIRRORED reference is speech-resynthesis/models.py in fp64 with no intermediate rounding.

Every output is a view into a device buffer with vc.GUARD rows in front and behind, prefilled with NaN (pcm: a pattern).  Checks:
the queried instantiation of a `pair` case is the one it claims; every byte outside the written windows is unchanged (guard rows,
XS under last = 2); the inputs are unchanged; no NaN in a row < T; rows at or past a clip's length are exactly zero in Y, XS,
xl_out, wav and pcm (an accumulating l2s_resblock_fused: exactly the previous xs and its leaky_relu, as the header says);
`tapcode` results are bit-exact; a refused launch answers its code and writes nothing; and
  (a) max error <= the tolerance of tests/test_kernels_gpu.py for that kernel and type, against the mirrored fp64 reference;
  (b) |got - ref| <= 1.5 u max(|ref|, smallest normal) [16-bit output] + F 2^-24 A per element, u = 2^-11 f16 / 2^-8 bf16,
      A = the operation on absolute values (pair: |b2| + sum |w2| |t1| + |x| (+ |XS before|); ResBlock: that of its last pair; post:
      (|b| + sum |w| |leaky_relu x|) (1 - ref^2) + |ref|), F = vc.F_of(vc.fkind(case), type);
  (u) max error against the un-mirrored reference <= twice the tolerance of (a).
Prints the worst ratio per instantiation and criterion (RATIO lines) and exits non-zero on any failure."""
import ctypes
import functools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lip2speech_unit_amd import _lib  # noqa: E402
from tests import _vocconv_cases as vc  # noqa: E402

U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
MIN_NORMAL = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}
# (a): the tolerances of tests/test_kernels_gpu.py, as fractions of max|ref| (test_respair_fused_conv_pair, _respair_final_case,
# test_resblock_fused_kernel) and absolute (test_conv_post_tanh_and_pcm).  test_resblock_fused_kernel runs fp16 only; bf16 takes
# that tolerance times the ratio the pair tests use between the two types (2e-2 / 3e-3)
TOL_PAIR = {"f16": 3e-3, "bf16": 2e-2}
TOL_PAIR_Y2 = {"f16": 2e-3, "bf16": 1.6e-2}           # the extra term on Y = leaky_relu(XS) of a last pair
TOL_RB = {"f16": 6e-3, "bf16": 6e-3 * (2e-2 / 3e-3)}
TOL_POST = 2e-5
EPS24 = 2.0 ** -24
NAN = float("nan")
f64, f32 = torch.float64, torch.float32
FAKE = 0x10000                               # a 16-byte aligned non-null "pointer" for the host-only query
POST_SLOPE = 0.01


def t16(dt):
    return torch.float16 if dt == "f16" else torch.bfloat16


def dtc(dt):
    return _lib.F16 if dt == "f16" else _lib.BF16


def rnd(x, dt):
    return x.to(t16(dt)).to(x.dtype)


def chop16(x, dt):
    """The 16-bit value below x in magnitude: the fp32 bits cut, not rounded."""
    shift = 13 if dt == "f16" else 16
    v = x.float().contiguous()
    cut = ((v.view(torch.int32) >> shift) << shift).view(f32)
    if dt == "f16":                          # below f16's normal range the cut bits are not the f16 mantissa: round there (no such case decides)
        cut = torch.where(v.abs() < 2.0 ** -14, v.half().float(), cut)
    return cut.to(x.dtype)


def bits(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def seed_of(*key):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(repr(key))) % (2 ** 31)


def lrelu(x, slope):
    return torch.where(x >= 0, x, x * slope)


def inv_lrelu(xl, slope):
    return torch.where(xl >= 0, xl, xl / slope)


def slope_of(c):
    return float(np.float32(c["slope"]))     # the launch takes a float


# ---- convolutions as unfold + matmul ----------------------------------------------------------------------------------------------------
def unfold(xp, n, k, dil):
    """xp [n + (k - 1) dil, C] -> [n, k C], K index = tap * C + c (the packed weight layout)."""
    return torch.cat([xp[t * dil: t * dil + n] for t in range(k)], 1)


def conv_same(x, W, k, dil):
    """x [n, C], W [Co, k C] -> [n, Co], zero padding (k - 1) / 2 * dil on both sides."""
    n, C = x.shape
    h = (k - 1) // 2 * dil
    xp = torch.zeros(n + 2 * h, C, dtype=x.dtype)
    xp[h: h + n] = x
    return unfold(xp, n, k, dil) @ W.t()


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def tap_weights(C, k, conv, mod):
    """tapcode: diagonal in the channels, channel c carries ONE tap of each convolution - tap c % k of a first, tap (c / k + c) % k
    of a second convolution - with the weight 2^(tap % mod): the row a response lands on names the taps that were read."""
    W = torch.zeros(C, k * C, dtype=f64)
    for ch in range(C):
        tap = ch % k if conv == 0 else (ch // k + ch) % k
        W[ch, tap * C + ch] = 2.0 ** (tap % mod)
    return W


def tap_rows(n, marks):
    return sorted({r for r in marks if 0 <= r < n})


def pair_operands(dt, C, k, slope, data, g):
    if data == "tapcode":
        return tap_weights(C, k, 0, 3), tap_weights(C, k, 1, 2), torch.zeros(C, dtype=f64), torch.zeros(C, dtype=f64)
    w1 = rnd(torch.randn(C, k * C, generator=g, dtype=f64) * (C * k) ** -0.5, dt)
    w2 = rnd(torch.randn(C, k * C, generator=g, dtype=f64) * (C * k) ** -0.5, dt)
    b1 = (torch.randn(C, generator=g) * 0.1).to(f64)
    b2 = (torch.randn(C, generator=g) * 0.1).to(f64)
    return w1, w2, b1, b2


def activations(dt, B, T, C, lim, slope, data, g, marks=()):
    """xl = leaky_relu(x) as 16-bit values [B, T, C], zero at and past each clip's length."""
    if data == "tapcode":
        xl = torch.zeros(B, T, C, dtype=f64)
        for b, n in enumerate(lim):
            for r in tap_rows(n, (0, n - 1) + tuple(marks)):
                xl[b, r] = 1.0
        return xl
    x = torch.randn(B, T, C, generator=g, dtype=f64) - (1.0 if data == "negative" else 0.0)
    xl = rnd(lrelu(x, slope), dt)
    for b, n in enumerate(lim):
        xl[b, n:] = 0.0
    return xl


def sum_before(B, T, C, data, g):
    """XS before an accumulating launch: non-zero in EVERY row, those past the clips' lengths included (the launch writes zero there)."""
    if data == "tapcode":
        return torch.randint(1, 4, (B, T, C), generator=g).to(f64)
    return torch.randn(B, T, C, generator=g).to(f64) + 0.25


@functools.lru_cache(maxsize=4)
def _pair_inputs(dt, C, k, dil, B, T, lens, len_mul, slope, data, S):
    g = torch.Generator().manual_seed(seed_of("pair", dt, C, k, dil, B, T, lens, len_mul, slope, data))
    lim = [T] * B if lens is None else [min(n * len_mul, T) for n in lens]
    w1, w2, b1, b2 = pair_operands(dt, C, k, slope, data, g)
    xl = activations(dt, B, T, C, lim, slope, data, g, marks=(S - 1, S, (k - 1) // 2 * dil))
    return dict(xl=xl, w1=w1, w2=w2, b1=b1, b2=b2, xs0=sum_before(B, T, C, data, g), lim=lim)


def pair_inputs(c):
    return _pair_inputs(c["dt"], c["C"], c["k"], c["dil"], c["B"], c["T"], None if c["lens"] is None else tuple(c["lens"]), c["len_mul"],
                        c["slope"], c["data"], c["S"])


def final_inputs(c):
    g = torch.Generator().manual_seed(seed_of("final", c["dt"], c["C"], c["ks"], c["dils"], c["B"], c["T"], c["lens"], c["len_mul"], c["data"]))
    lim, out = vc.lims(c), []
    for k, dil in zip(c["ks"], c["dils"]):
        w1, w2, b1, b2 = pair_operands(c["dt"], c["C"], k, c["slope"], c["data"], g)
        out.append(dict(xl=activations(c["dt"], c["B"], c["T"], c["C"], lim, slope_of(c), c["data"], g), w1=w1, w2=w2, b1=b1, b2=b2, lim=lim))
    return out


def rb_operands(dt, C, k, data, g):
    if data == "tapcode":
        return [tap_weights(C, k, i & 1, 2) for i in range(6)], [torch.zeros(C, dtype=f64) for _ in range(6)]
    return ([rnd(torch.randn(C, k * C, generator=g, dtype=f64) * (C * k) ** -0.5, dt) for _ in range(6)],
            [(torch.randn(C, generator=g) * 0.1).to(f64) for _ in range(6)])


def resblock_inputs(c):
    g = torch.Generator().manual_seed(seed_of("rb", c["dt"], c["C"], c["k"], c["dils"], c["T"], c["lens"], c["len_mul"], c["data"], c["slope"]))
    lim = vc.lims(c)
    ws, bs = rb_operands(c["dt"], c["C"], c["k"], c["data"], g)
    TT, H = vc.rb_tt(c["C"], c["k"]), vc.rb_halo(c["k"], c["dils"])
    xl = activations(c["dt"], c["B"], c["T"], c["C"], lim, slope_of(c), c["data"], g, marks=(TT - 1, TT, H))
    return dict(xl=xl, ws=ws, bs=bs, xs0=sum_before(c["B"], c["T"], c["C"], c["data"], g), lim=lim)


def resstage_inputs(c):
    g = torch.Generator().manual_seed(seed_of("rs", c["dt"], c["C"], c["table"], c["T"], c["lens"], c["len_mul"], c["data"]))
    lim = vc.lims(c)
    ops = [rb_operands(c["dt"], c["C"], k, c["data"], g) for k in (3, 7, 11)]
    xl = activations(c["dt"], c["B"], c["T"], c["C"], lim, slope_of(c), c["data"], g)
    return dict(xl=xl, ws=[o[0] for o in ops], bs=[o[1] for o in ops], lim=lim)


def post_inputs(c):
    g = torch.Generator().manual_seed(seed_of("post", c["C"], c["k"], c["T"], c["lens"], c["len_mul"], c["data"]))
    C, k = c["C"], c["k"]
    gain = 1.5 * 12.0 / (0.2 * (C * k / 2.0) ** 0.5) if c["data"] == "saturate" else 1.0     # pre-activations of spread 18: past +-12
    x = (torch.randn(c["B"], c["T"], C, generator=g) * gain).to(f64)
    w = (torch.randn(k, C, generator=g) * 0.2).to(f64)
    return dict(x=x, w=w, b=0.05, lim=vc.lims(c))


# ---- the operations, in fp64 (references) or fp32 (the figures behind F, the mutation test) ---------------------------------------------
def pair_clip(xl, w1, w2, b1, b2, k, dil, slope, dt, ft, mirror=True, mut=None, S=0):
    """One clip alone over its n valid rows: (x' [n, C], A [n, C]).  mut: a subtle error planted for the mutation test."""
    n, C = xl.shape
    h2 = (k - 1) // 2
    h1 = h2 * dil
    xl, w1, w2, b1, b2 = xl.to(ft), w1.to(ft), w2.to(ft), b1.to(ft), b2.to(ft)
    # conv1 on rows -h2 .. n + h2 (input zero outside the clip), so that the length mask is a step of its own
    xp = torch.zeros(n + 2 * h2 + 2 * h1, C, dtype=ft)
    xp[h2 + h1: h2 + h1 + n] = xl
    t1 = lrelu(unfold(xp, n + 2 * h2, k, dil) @ w1.t() + b1, slope)
    if mirror:
        t1 = rnd(t1, dt)
    t1[:h2] = 0.0                                         # rows t < 0
    if mut != "t1-unmasked":
        t1[h2 + n:] = 0.0                                 # rows t >= len: the reference's zero padding
    res = xl if mut == "residual-no-inverse" else inv_lrelu(xl, slope)
    U = unfold(t1, n, k, 1)
    xo = U @ w2.t() + b2 + res
    if mut == "tap-dropped" and n > S:                    # conv2's tap 0 at the first row of the clip's second tile
        xo[S] -= t1[S] @ w2[:, :C].t()
    A = (U.abs().float() @ w2.abs().float().t()).to(f64) + b2.abs().to(f64) + res.abs().to(f64)
    return xo, A


_PAIR_MEMO = {}


def pair_eval(c, ins, ft, mirror=True, mut=None):
    """(x' [B, T, C] in ft, A [B, T, C] fp64), zero at and past each clip's length.  The four kinds of a geometry share their inputs
    and hence x': the last few results are kept."""
    key = (id(ins), c["k"], c["dil"], c["slope"], ft, mirror, mut)
    if key not in _PAIR_MEMO:
        if len(_PAIR_MEMO) >= 8:
            _PAIR_MEMO.pop(next(iter(_PAIR_MEMO)))
        _PAIR_MEMO[key] = (ins, _pair_eval(c, ins, ft, mirror, mut))      # (ins is held: its id stays its own)
    xo, A = _PAIR_MEMO[key][1]
    return xo.clone(), A.clone()


def _pair_eval(c, ins, ft, mirror, mut):
    B, T, C = c["B"], c["T"], c["C"]
    xo, A = torch.zeros(B, T, C, dtype=ft), torch.zeros(B, T, C, dtype=f64)
    for b, n in enumerate(ins["lim"]):
        if n > 0:
            xo[b, :n], A[b, :n] = pair_clip(ins["xl"][b, :n], ins["w1"], ins["w2"], ins["b1"], ins["b2"], c["k"], c["dil"], slope_of(c),
                                            c["dt"], ft, mirror, mut, c.get("S", 0))
    return xo, A


def valid_mask(c, lim):
    m = torch.zeros(c["B"], c["T"], 1, dtype=torch.bool)
    for b, n in enumerate(lim):
        m[b, :n] = True
    return m


def to16(x, dt, chop=False):
    """The output conversion of an EVALUATION (fp32: rounded, or chopped for the mutation test).  A REFERENCE (fp64) keeps the exact
    value: the output's own rounding is the 1.5 u |ref| term of (b)."""
    if x.dtype == f64:
        return x
    return chop16(x, dt) if chop else rnd(x, dt)


def pair_outputs(c, ins, xo, A, ft, chop=False):
    """name -> (value in ft, A, is 16-bit) for the outputs the case's kind writes."""
    kind, s, dt = c["kind"], slope_of(c), c["dt"]
    if kind == "mid":
        return {"Y": (to16(lrelu(xo, s), dt, chop), A, True)}
    if kind == "last":
        return {"XS": (xo.float().to(ft) if ft == f32 else xo, A, False)}
    keep = valid_mask(c, ins["lim"])
    tot = (xo + ins["xs0"].to(ft)) * keep
    At = (A + ins["xs0"].abs()) * keep
    out = {"Y": (to16(lrelu(tot, s), dt, chop), At, True)}
    if kind == "acc":
        out["XS"] = (tot, At, False)
    return out


def final_eval(c, ins, ft, mirror=True):
    xo, A = None, None
    for j, (k, dil) in enumerate(zip(c["ks"], c["dils"])):
        cj = dict(c, k=k, dil=dil)
        x1, A1 = pair_eval(cj, ins[j], ft, mirror)
        xo, A = (x1, A1) if xo is None else (xo + x1, A + A1)
    return xo, A


def resblock_clip(xl, ws, bs, k, dils, slope, dt, ft, mirror=True, mut=None):
    """One clip alone: (ResBlock output [n, C], A [n, C]).  A is the pair's |b2| + sum |w2| |t1| + |x| at the LAST pair, on the
    intermediates that came through the first four convolutions: the scale of the result's own terms.  (All six convolutions on
    absolute values were tried first: that A is 10^4 .. 10^6 times |ref| - |w| loses the cancellation of six random-sign sums - and
    a bound in its units holds nothing.)"""
    XL = xl.to(ft)
    res = inv_lrelu(XL, slope)
    v = A = None
    for m in range(3):
        d = dils[m] + (1 if (mut == "dilation-off-by-one" and m == 1) else 0)
        w1, w2, b1, b2 = ws[2 * m].to(ft), ws[2 * m + 1].to(ft), bs[2 * m].to(ft), bs[2 * m + 1].to(ft)
        t1 = lrelu(conv_same(XL, w1, k, d) + b1, slope)
        if mirror:
            t1 = rnd(t1, dt)
        v = conv_same(t1, w2, k, 1) + b2 + res
        if m == 2:
            A = (conv_same(t1.abs().float(), w2.abs().float(), k, 1) + b2.abs().float() + res.abs().float()).to(f64)
        if m < 2:
            if mirror:                                    # the hand-over: the 16-bit XL buffer, the residual recovered from it
                XL = rnd(lrelu(v, slope), dt)
                res = XL if mut == "residual-no-inverse" else inv_lrelu(XL, slope)
            else:
                XL, res = lrelu(v, slope), v
    return v, A


def resblock_eval(c, ins, ft, mirror=True, mut=None, ws=None, bs=None, k=None, dils=None):
    B, T, C = c["B"], c["T"], c["C"]
    xo, A = torch.zeros(B, T, C, dtype=ft), torch.zeros(B, T, C, dtype=f64)
    for b, n in enumerate(ins["lim"]):
        if n > 0:
            xo[b, :n], A[b, :n] = resblock_clip(ins["xl"][b, :n], ws or ins["ws"], bs or ins["bs"], k or c["k"], dils or c["dils"],
                                                slope_of(c), c["dt"], ft, mirror, mut)
    return xo, A


def resblock_outputs(c, ins, xo, A, ft, chop=False):
    if c["accumulate"]:                                   # rows past the length: 0 + the previous sum (include/lip2speech_hip.h)
        xo, A = xo + ins["xs0"].to(ft), A + ins["xs0"].abs()
    out = {"xs": (xo, A, False)}
    if c["xl_out"]:
        out["xl_out"] = (to16(lrelu(xo, slope_of(c)), c["dt"], chop), A, True)
    return out


RS_ORDER = {32: (2, 1, 0), 16: (0, 1, 2)}                 # the stage kernel's order of the ResBlocks k = 3, 7, 11


def resstage_eval(c, ins, ft, mirror=True):
    xo, A = None, None
    for j in RS_ORDER[c["C"]]:
        x1, A1 = resblock_eval(c, ins, ft, mirror, ws=ins["ws"][j], bs=ins["bs"][j], k=(3, 7, 11)[j], dils=c["table"][j])
        xo, A = (x1, A1) if xo is None else (xo + x1, A + A1)
    return xo, A


def post_eval(c, ins, ft):
    """(wav [B, T], A [B, T]): A = (|b| + sum |w| |leaky_relu x|) (1 - ref^2) + |ref|."""
    B, T, C, k = c["B"], c["T"], c["C"], c["k"]
    wav, A = torch.zeros(B, T, dtype=ft), torch.zeros(B, T, dtype=f64)
    w = ins["w"].to(ft).reshape(k * C)
    for b, n in enumerate(ins["lim"]):
        if n > 0:
            xr = lrelu(ins["x"][b, :n].to(ft), POST_SLOPE)
            h = (k - 1) // 2
            xp = torch.zeros(n + 2 * h, C, dtype=ft)
            xp[h: h + n] = xr
            U = unfold(xp, n, k, 1)
            y = torch.tanh(U @ w + ins["b"])
            wav[b, :n] = y
            y64 = y.to(f64)
            A[b, :n] = (abs(ins["b"]) + U.abs().to(f64) @ w.abs().to(f64)) * (1.0 - y64 * y64) + y64.abs()
    return wav, A


# ---- criteria -----------------------------------------------------------------------------------------------------------------------------
def bound_b(ref, A, dt, out16, kind):
    ulp = U16[dt] * ref.abs().clamp(min=MIN_NORMAL[dt]) if out16 else 0.0
    return (vc.FU * ulp if out16 else 0.0) + vc.F_of(kind, dt) * EPS24 * A


def ratio_b(err, bound):
    """max err / bound; an element whose bound is zero must be exact."""
    q = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return q.max().item() if q.numel() else 0.0


class Report:
    def __init__(self, env):
        self.env, self.fail, self.worst = env, [], {}

    def ratio(self, case, crit, r):
        k = (case["inst"], crit)
        self.worst[k] = max(self.worst.get(k, 0.0), r)

    def bad(self, case, why):
        self.fail.append(f"FAIL env={self.env} {case['dt']} {case['op']} {case['name']} inst={case['inst'][2]}: {why}")

    def judge(self, case, what, got, ref, A, tol_abs, out16, ref_u=None):
        """(a), (b) and (u) on one output (fp64, same shape)."""
        if got.numel() == 0:
            return
        err = (got - ref).abs()
        ra = err.max().item() / tol_abs if tol_abs > 0 else (0.0 if err.max().item() == 0 else float("inf"))
        self.ratio(case, "a", ra)
        if ra > 1.0:
            self.bad(case, f"(a) {what}: max err / tolerance = {ra:.3f}")
        bound = bound_b(ref, A, case["dt"], out16, vc.fkind(case))
        rb = ratio_b(err, bound)
        self.ratio(case, "b", rb)
        if rb > 1.0:
            i = (err / bound.clamp(min=1e-300)).reshape(-1).argmax().item()
            self.bad(case, f"(b) {what}: err / bound = {rb:.3f} at flat index {i} (got {got.reshape(-1)[i].item():.9g}, "
                           f"ref {ref.reshape(-1)[i].item():.9g})")
        if ref_u is not None:
            ru = (got - ref_u).abs().max().item() / (2 * tol_abs) if tol_abs > 0 else 0.0
            self.ratio(case, "u", ru)
            if ru > 1.0:
                self.bad(case, f"(u) {what}: max err against the un-mirrored reference / (2 x tolerance) = {ru:.3f}")


# ---- guarded device buffers -----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A [rows, C] window behind vc.GUARD guard rows (and `off` elements) of a flat buffer; the host copy keeps what was uploaded."""

    def __init__(self, rows, C, dtype, fill=NAN, off=0, content=None):
        self.rows, self.C, self.base = rows, C, vc.GUARD * C + off
        n = (rows + 2 * vc.GUARD) * C + off + 8
        self.host = torch.full((n,), fill, dtype=dtype)
        if content is not None:
            self.host[self.base: self.base + rows * C] = content.reshape(-1).to(dtype)
        self.dev = self.host.cuda()

    def ptr(self):
        return self.dev.data_ptr() + self.base * self.dev.element_size()

    def view(self):
        return self.dev[self.base: self.base + self.rows * self.C].view(self.rows, self.C)

    def after(self):
        return self.dev.cpu()

    def check(self, rep, case, name, win_rows=None, written=True):
        """Everything outside the window (rows of win_rows, a [rows] bool tensor; None: all rows) is bit-identical; returns the window."""
        after = self.after()
        win = torch.zeros(after.shape, dtype=torch.bool)
        if written:
            w = torch.ones(self.rows, dtype=torch.bool) if win_rows is None else win_rows
            win[self.base: self.base + self.rows * self.C] = w[:, None].expand(self.rows, self.C).reshape(-1)
        stray = (bits(after) != bits(self.host)) & ~win
        if stray.any():
            rep.bad(case, f"{stray.sum().item()} elements of {name} outside the written window changed")
        return after[self.base: self.base + self.rows * self.C].view(self.rows, self.C)


def dev_in(x, dtype):
    """An input on the device and its host copy (for the unchanged check)."""
    h = x.to(dtype).contiguous()
    return h.cuda(), h


def unchanged(rep, case, name, dev, host):
    if not torch.equal(bits(dev.cpu()), bits(host)):
        rep.bad(case, f"operand {name} changed")


def check_window(rep, c, name, got, lim, T, past=None):
    """No NaN in a row < T, rows at or past the clip's length exactly zero (or exactly `past` [B, T, C], where the header says they
    keep a previous content); returns the window as fp64 [B, T, C] or None."""
    if torch.isnan(got.float()).any():
        rep.bad(c, f"{torch.isnan(got.float()).sum().item()} NaN in the window of {name}")
        return None
    got = got.to(f64).view(c["B"], T, -1)
    for b, n in enumerate(lim):
        want = 0.0 if past is None else past[b, n:].to(f64)
        if bool((got[b, n:] != want).any()):
            rep.bad(c, f"rows at or past the length of clip {b} are not exactly {'zero' if past is None else 'the previous sum'} in {name}")
    return got


def dlens(c):
    return torch.tensor(c["lens"], dtype=torch.int32).cuda() if c["lens"] is not None else None


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- one case on the device -----------------------------------------------------------------------------------------------------------------
def pair_desc(c, X=FAKE, W1=FAKE, W2=FAKE, b1=FAKE, b2=FAKE, Y=FAKE, XS=FAKE, lens=FAKE):
    d = _lib.RespairDesc()
    kind = c["kind"]
    d.X, d.W1, d.W2, d.b1, d.b2 = X, W1, W2, b1, b2
    d.Y = Y if kind != "last" else None
    d.XS = XS if kind != "mid" else None
    d.lens = lens if c["lens"] is not None else None
    d.len_mul, d.B, d.T, d.C, d.k, d.dil = c["len_mul"], c["B"], c["T"], c["C"], c["k"], c["dil"]
    d.last = {"mid": 0, "last": 1, "acc": 1, "last2": 2}[kind]
    d.accumulate = int(kind in ("acc", "last2"))
    d.dtype, d.slope = dtc(c["dt"]), c["slope"]
    return d


def judge_outputs(rep, c, lim, wins, refs, refs_u, tol16, tolf, past=None):
    """wins: name -> window tensor; refs / refs_u: name -> (value, A, is16); past: name -> what rows past the length hold (default 0)."""
    for name, (ref, A, is16) in refs.items():
        got = check_window(rep, c, name, wins[name], lim, c["T"], past.get(name) if past else None)
        if got is None:
            continue
        ref = ref.to(f64)
        if c["data"] == "tapcode":
            if not torch.equal(got, ref):
                rep.bad(c, f"tapcode: {(got != ref).sum().item()} elements of {name} differ from the exact result, first at flat index "
                           f"{(got != ref).reshape(-1).nonzero()[0].item()}")
            rep.ratio(c, "b", 0.0)
            continue
        rep.judge(c, name, got, ref, A, tol16 if is16 else tolf, is16, refs_u[name][0].to(f64) if refs_u else None)


def run_pair(c, lib, rep):
    B, T, C, dt, el = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    ins = pair_inputs(c)
    kind = c["kind"]
    dx, hx = dev_in(ins["xl"].reshape(B * T, C), el)
    dw1, hw1 = dev_in(ins["w1"], el)
    dw2, hw2 = dev_in(ins["w2"], el)
    db1, db2 = ins["b1"].float().cuda(), ins["b2"].float().cuda()
    gy = Guarded(B * T, C, el) if kind != "last" else None
    gxs = None
    if kind == "last":
        gxs = Guarded(B * T, C, f32)
    elif kind != "mid":
        gxs = Guarded(B * T, C, f32, content=ins["xs0"])
    dl = dlens(c)
    d = pair_desc(c, dx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), db1.data_ptr(), db2.data_ptr(), gy.ptr() if gy else None,
                  gxs.ptr() if gxs else None, ptr(dl))
    var = lib.l2s_respair_variant(ctypes.byref(d))
    if var != c["inst"][2][0]:
        rep.bad(c, f"instantiation: the query answers {var}")
        return
    rc = lib.l2s_respair(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    wins = {}
    if gy:
        wins["Y"] = gy.check(rep, c, "Y", written=rc == 0)
    if gxs:
        wins["XS"] = gxs.check(rep, c, "XS", written=rc == 0 and kind != "last2")
    unchanged(rep, c, "X", dx, hx)
    unchanged(rep, c, "W1", dw1, hw1)
    unchanged(rep, c, "W2", dw2, hw2)
    if rc != 0:
        return
    xo, A = pair_eval(c, ins, f64)
    refs = pair_outputs(c, ins, xo, A, f64)
    refs_u = pair_outputs(c, ins, pair_eval(c, ins, f64, mirror=False)[0], A, f64) if c["data"] != "tapcode" else None
    mx = xo.abs().max().item()
    tol = TOL_PAIR[dt] * mx
    tol_y = tol
    if kind in ("acc", "last2"):
        tol_y = tol + TOL_PAIR_Y2[dt] * (xo + ins["xs0"] * valid_mask(c, ins["lim"])).abs().max().item()
    judge_outputs(rep, c, ins["lim"], wins, refs, refs_u, tol_y, tol)


def run_final(c, lib, rep):
    B, T, C, dt, el = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    ins = final_inputs(c)
    d = _lib.RespairFinalDesc()
    keep = []
    for j, (k, dil) in enumerate(zip(c["ks"], c["dils"])):
        t = [dev_in(ins[j]["xl"].reshape(B * T, C), el), dev_in(ins[j]["w1"], el), dev_in(ins[j]["w2"], el),
             ins[j]["b1"].float().cuda(), ins[j]["b2"].float().cuda()]
        keep.append(t)
        d.X[j], d.W1[j], d.W2[j], d.b1[j], d.b2[j] = t[0][0].data_ptr(), t[1][0].data_ptr(), t[2][0].data_ptr(), t[3].data_ptr(), t[4].data_ptr()
        d.k[j], d.dil[j] = k, dil
    gy = Guarded(B * T, C, el)
    dl = dlens(c)
    d.Y, d.lens = gy.ptr(), ptr(dl)
    d.n, d.len_mul, d.B, d.T, d.C, d.dtype, d.slope = len(c["ks"]), c["len_mul"], B, T, C, dtc(dt), c["slope"]
    rc = lib.l2s_respair_final(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "Y", written=rc == 0)
    for j, t in enumerate(keep):
        for i, name in enumerate(("X", "W1", "W2")):
            unchanged(rep, c, f"{name}[{j}]", *t[i])
    xo, A = final_eval(c, ins, f64)
    s = slope_of(c)
    refs = {"Y": (lrelu(xo, s), A, True)}
    refs_u = {"Y": (lrelu(final_eval(c, ins, f64, mirror=False)[0], s), A, True)}
    judge_outputs(rep, c, ins[0]["lim"], {"Y": win}, refs, refs_u, TOL_PAIR[dt] * xo.abs().max().item(), 0.0)


def rb_pack(ws, bs, C, k, el):
    """[6][C][Kpad] 16-bit, K zero-padded to a multiple of 32; [6][C] fp32."""
    kpad = vc.cdiv(k * C, 32) * 32
    w = torch.zeros(6, C, kpad, dtype=f64)
    for i in range(6):
        w[i, :, : k * C] = ws[i]
    return w.to(el).contiguous(), torch.stack(bs).float().contiguous()


def nan_past(xl, lim, el):
    """The ResBlock kernels never read a row at or past the clip's length: NaN there."""
    x = xl.clone().to(el)
    for b, n in enumerate(lim):
        x[b, n:] = NAN
    return x


def rb_launch(lib, c, dx, dw, db, xs_ptr, out_ptr, dl, k, dils, accumulate):
    return lib.l2s_resblock_fused(dx.data_ptr(), dw.data_ptr(), db.data_ptr(), xs_ptr, out_ptr, ptr(dl), c["len_mul"], c["B"], c["T"], c["C"],
                                  k, dils[0], dils[1], dils[2], int(accumulate), c["slope"], dtc(c["dt"]),
                                  torch.cuda.current_stream().cuda_stream)


def run_resblock(c, lib, rep):
    B, T, C, k, dt, el = c["B"], c["T"], c["C"], c["k"], c["dt"], t16(c["dt"])
    ins = resblock_inputs(c)
    hx = nan_past(ins["xl"], ins["lim"], el).reshape(B * T, C)
    dx = hx.cuda()
    hw, hb = rb_pack(ins["ws"], ins["bs"], C, k, el)
    dw, db = hw.cuda(), hb.cuda()
    gxs = Guarded(B * T, C, f32, content=ins["xs0"]) if c["accumulate"] else Guarded(B * T, C, f32)
    gout = Guarded(B * T, C, el, off=c["xl_off"]) if c["xl_out"] else None
    dl = dlens(c)
    rc = rb_launch(lib, c, dx, dw, db, gxs.ptr(), gout.ptr() if gout else None, dl, k, c["dils"], c["accumulate"])
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    wins = {"xs": gxs.check(rep, c, "xs", written=rc == 0)}
    if gout:
        wins["xl_out"] = gout.check(rep, c, "xl_out", written=rc == 0)
    unchanged(rep, c, "xl", dx, hx)
    unchanged(rep, c, "w", dw, hw)
    if rc != 0:
        return
    xo, A = resblock_eval(c, ins, f64)
    refs = resblock_outputs(c, ins, xo, A, f64)
    refs_u = resblock_outputs(c, ins, resblock_eval(c, ins, f64, mirror=False)[0], A, f64) if c["data"] != "tapcode" else None
    tol = TOL_RB[dt] * refs["xs"][0].abs().max().item()
    past = None
    if c["accumulate"]:                                   # bit for bit: 0 + xs in fp32, and leaky_relu of it rounded to 16 bits
        x0 = ins["xs0"].float()
        past = {"xs": x0 + 0.0, "xl_out": rnd(torch.where(x0 >= 0, x0, x0 * np.float32(c["slope"])), dt)}
    judge_outputs(rep, c, ins["lim"], wins, refs, refs_u, tol, tol, past)


def run_resstage(c, lib, rep):
    B, T, C, dt, el = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    ins = resstage_inputs(c)
    hx = nan_past(ins["xl"], ins["lim"], el).reshape(B * T, C)
    dx = hx.cuda()
    packs = [rb_pack(ins["ws"][j], ins["bs"][j], C, (3, 7, 11)[j], el) for j in range(3)]
    dws, dbs = [p[0].cuda() for p in packs], [p[1].cuda() for p in packs]
    gxs = Guarded(B * T, C, f32)
    gout = Guarded(B * T, C, el, off=c["xl_off"]) if c["xl_out"] else None
    dl = dlens(c)
    wp = (ctypes.c_void_p * 3)(*[w.data_ptr() for w in dws])
    bp = (ctypes.c_void_p * 3)(*[b.data_ptr() for b in dbs])
    kk = (ctypes.c_int * 3)(3, 7, 11)
    dd = (ctypes.c_int * 9)(*[d for row in c["table"] for d in row])
    rc = lib.l2s_resstage_fused(dx.data_ptr(), wp, bp, kk, dd, 3, gxs.ptr(), gout.ptr() if gout else None, ptr(dl), c["len_mul"], B, T, C,
                                c["slope"], int(c["xs_final"]), dtc(dt), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    # xs under xs_final = 0 is scratch: it may change inside its window, and must stay finite where it was written
    xs_win = gxs.check(rep, c, "xs", written=rc == 0)
    wins = {}
    if c["xs_final"]:
        wins["xs"] = xs_win
    elif rc == 0 and torch.isinf(xs_win).any():
        rep.bad(c, "xs (scratch under xs_final = 0) holds Inf")
    if gout:
        wins["xl_out"] = gout.check(rep, c, "xl_out", written=rc == 0)
    unchanged(rep, c, "xl", dx, hx)
    for j in range(3):
        unchanged(rep, c, f"w[{j}]", dws[j], packs[j][0])
    if rc != 0:
        return
    xo, A = resstage_eval(c, ins, f64)
    xu = resstage_eval(c, ins, f64, mirror=False)[0]
    s = slope_of(c)
    refs, refs_u = {}, {}
    if c["xs_final"]:
        refs["xs"], refs_u["xs"] = (xo, A, False), (xu, A, False)
    if c["xl_out"]:
        refs["xl_out"], refs_u["xl_out"] = (lrelu(xo, s), A, True), (lrelu(xu, s), A, True)
    tol = TOL_RB[dt] * xo.abs().max().item()
    judge_outputs(rep, c, ins["lim"], wins, refs, refs_u, tol, tol)
    # bit-equality with the three l2s_resblock_fused launches in the stage kernel's order (accumulate 0, 1, 1; xl_out on the last)
    hxs = Guarded(B * T, C, f32)
    hout = Guarded(B * T, C, el, off=c["xl_off"]) if c["xl_out"] else None
    for n, j in enumerate(RS_ORDER[C]):
        r = rb_launch(lib, c, dx, dws[j], dbs[j], hxs.ptr(), hout.ptr() if (hout and n == 2) else None, dl, (3, 7, 11)[j], c["table"][j], n > 0)
        if r != 0:
            rep.bad(c, f"l2s_resblock_fused k = {(3, 7, 11)[j]} answers {r}")
            return
    torch.cuda.synchronize()
    if c["xs_final"] and not torch.equal(bits(hxs.view().cpu()), bits(xs_win)):
        rep.bad(c, "xs differs from the three l2s_resblock_fused launches")
    if hout and not torch.equal(bits(hout.view().cpu()), bits(wins["xl_out"])):
        rep.bad(c, "xl_out differs from the three l2s_resblock_fused launches")


def run_post(c, lib, rep):
    B, T, C, k = c["B"], c["T"], c["C"], c["k"]
    ins = post_inputs(c)
    hx = torch.full((B * T * C + 8,), NAN, dtype=f32)
    x = ins["x"].float().clone()
    for b, n in enumerate(ins["lim"]):
        x[b, n:] = NAN                                    # rows at or past the clip's length are never read
    off = c["x_off"]
    hx[off: off + B * T * C] = x.reshape(-1)
    dx = hx.cuda()
    dw = ins["w"].float().contiguous().cuda()
    gw = Guarded(B * T, 1, f32)
    gp = Guarded(B * T, 1, torch.int16, fill=0x5A5A) if c["pcm"] else None
    dl = dlens(c)
    rc = lib.l2s_conv_post_tanh(dx.data_ptr() + 4 * off, dw.data_ptr(), ins["b"], gw.ptr(), gp.ptr() if gp else None, ptr(dl), c["len_mul"],
                                B, T, C, k, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    wav = gw.check(rep, c, "wav", written=rc == 0)
    pcm = gp.check(rep, c, "pcm", written=rc == 0) if gp else None
    unchanged(rep, c, "x", dx, hx)
    if rc != 0:
        return
    got = check_window(rep, c, "wav", wav, ins["lim"], T)
    if got is None:
        return
    got = got.view(B, T)
    ref, A = post_eval(c, ins, f64)
    rep.judge(c, "wav", got, ref, A, TOL_POST, False)
    if c["data"] == "saturate" and not (bool((got == 1.0).any()) and bool((got == -1.0).any())):
        rep.bad(c, "saturate: no sample of wav is exactly +1 and -1")
    if pcm is not None:
        pcm = pcm.view(B, T)
        # numpy's astype('int16') of the kernel's own fp32 samples times 32768, the saturated samples included
        want = torch.from_numpy((wav.view(B, T).numpy() * np.float32(32768.0)).astype("int16"))
        if not torch.equal(pcm, want):
            rep.bad(c, f"pcm: {(pcm != want).sum().item()} samples differ from astype('int16') of wav * 32768")
        for b, n in enumerate(ins["lim"]):
            if bool((pcm[b, n:] != 0).any()):
                rep.bad(c, f"pcm past the length of clip {b} is not zero")
        # within one count of the truncated fp64 reference wherever ref * 32768 is further from an integer than the error bound
        s = ref * 32768.0
        far = (s - s.round()).abs() > vc.F_of("post", "f32") * EPS24 * A * 32768.0
        d = (pcm.to(f64) - s.trunc()).abs()
        if bool((d[far] > 1).any()):
            rep.bad(c, f"pcm: {(d[far] > 1).sum().item()} samples are more than one count from the truncated fp64 reference")


RUN = {"pair": run_pair, "final": run_final, "resblock": run_resblock, "resstage": run_resstage, "post": run_post}


# ---- host-only modes ------------------------------------------------------------------------------------------------------------------------
def route(env_name, lib):
    """The restated rule against l2s_respair_variant under this process's switches; every pair case of the environment against `inst`."""
    env = {k: os.environ[k] for k in vc.SWITCHES if k in os.environ}
    bad = n = 0

    def expect(what, got, want):
        nonlocal bad, n
        n += 1
        if got != want:
            bad += 1
            if bad < 20:
                print(f"ROUTE {what}: the query answers {got}, the restated rule {want}")

    for dt in vc.DTYPES:
        for C in (32, 64, 128, 256, 512):
            for k in range(1, 23, 2):
                for dil in range(1, 36):
                    for kind in vc.KINDS:
                        c = dict(dt=dt, C=C, k=k, dil=dil, B=2, T=300, lens=[300, 1], len_mul=1, kind=kind, slope=0.1)
                        expect(f"respair {dt} C={C} k={k} dil={dil} {kind}", lib.l2s_respair_variant(ctypes.byref(pair_desc(c))),
                               vc.respair_variant(C, k, dil, env))
    c = dict(dt="f16", C=64, k=3, dil=1, B=2, T=300, lens=None, len_mul=1, kind="mid", slope=0.1)
    expect("respair no lens", lib.l2s_respair_variant(ctypes.byref(pair_desc(c))), vc.respair_variant(64, 3, 1, env))
    expect("respair Y % 16", lib.l2s_respair_variant(ctypes.byref(pair_desc(c, Y=FAKE + 8))), -3)
    expect("respair last = 2 without Y", lib.l2s_respair_variant(ctypes.byref(pair_desc(dict(c, kind="last2"), Y=None))), -1)
    expect("respair slope", lib.l2s_respair_variant(ctypes.byref(pair_desc(dict(c, slope=1.5)))), -1)
    expect("respair even k", lib.l2s_respair_variant(ctypes.byref(pair_desc(dict(c, k=4)))), -2)
    expect("respair null", lib.l2s_respair_variant(None), -1)
    if env_name in vc.ENVS and env == vc.ENVS[env_name]:
        for c in vc.pair_cases(env_name):
            expect(f"case {c['dt']} {c['name']}", lib.l2s_respair_variant(ctypes.byref(pair_desc(c))), c["inst"][2][0])
    print(f"routed {n - bad} of {n} queries under {env}")
    return bad


def eval_case(c, ft, mut=None, chop=False, mirror=True):
    """name -> (value, A, is16) of the case's outputs with the operation evaluated in float type ft (the device-free twin of RUN)."""
    op = c["op"]
    if op == "pair":
        ins = pair_inputs(c)
        xo, A = pair_eval(c, ins, ft, mirror, mut)
        return pair_outputs(c, ins, xo, A, ft, chop)
    if op == "final":
        xo, A = final_eval(c, final_inputs(c), ft, mirror)
        return {"Y": (to16(lrelu(xo, slope_of(c)), c["dt"], chop), A, True)}
    if op == "resblock":
        ins = resblock_inputs(c)
        xo, A = resblock_eval(c, ins, ft, mirror, mut)
        return resblock_outputs(c, ins, xo, A, ft, chop)
    if op == "resstage":
        xo, A = resstage_eval(c, resstage_inputs(c), ft, mirror)
        out = {"xs": (xo, A, False)} if c["xs_final"] else {}
        if c["xl_out"]:
            out["xl_out"] = (to16(lrelu(xo, slope_of(c)), c["dt"], chop), A, True)
        return out
    wav, A = post_eval(c, post_inputs(c), ft)
    return {"wav": (wav, A, False)}


def ratio_b_of_case(c, got, ref):
    """Worst err / bound (b) over the outputs of a case; got, ref: eval_case results."""
    worst = 0.0
    for name, (r, A, is16) in ref.items():
        g = got[name][0].to(f64)
        worst = max(worst, ratio_b((g - r.to(f64)).abs(), bound_b(r.to(f64), A, c["dt"], is16, vc.fkind(c))))
    return worst


def cpu_f32(ops_filter=None):
    """Each operation in torch fp32 on the CPU (16-bit intermediates as in the kernels) against the mirrored fp64 reference, in units of
    2^-24 A: the figures of vc.CPU_F32_WORST."""
    worst, seen = {}, set()
    for env_name in vc.ENVS:
        for c in vc.cases_of(env_name):
            key = (c["op"], c["dt"], c["name"])
            if key in seen or c["expect"] != 0 or c["data"] == "tapcode" or (ops_filter and c["op"] not in ops_filter):
                continue
            seen.add(key)
            ref, got = eval_case(c, f64), eval_case(c, f32)
            for name, (r, A, is16) in ref.items():
                err = (got[name][0].to(f64) - r.to(f64)).abs()
                if is16:                                   # the output's own rounding is the other term of (b)
                    err = (err - vc.FU * U16[c["dt"]] * r.to(f64).abs().clamp(min=MIN_NORMAL[c["dt"]])).clamp(min=0.0)
                q = ratio_b(err, EPS24 * A)
                k = (vc.fkind(c), c["dt"])
                if q > worst.get(k, (0.0, ""))[0]:
                    worst[k] = (q, f"{c['name']} {name}")
    for (kind, dt), (r, name) in sorted(worst.items()):
        print(f"CPUF32 {kind:12s} {dt:4s} worst |fp32 - fp64| / (2^-24 A) = {r:10.3f}  ({name})")
    print("CPU_F32_WORST = {" + ", ".join(f"({k!r}, {dt!r}): {r:.3f}" for (k, dt), (r, _) in sorted(worst.items())) + "}")


def main():
    args = sys.argv[1:]
    usage = f"usage: check_vocoder_convs.py [--route] <{' | '.join(vc.ENVS)}>  or  check_vocoder_convs.py --cpu-f32 [op ...]"
    if not args or args[0] in ("-h", "--help"):
        sys.exit(usage)
    if args[0] == "--cpu-f32":
        cpu_f32(set(args[1:]))
        return
    route_only = args[0] == "--route"
    env_name = args[-1]
    if len(args) != (2 if route_only else 1) or (not route_only and env_name not in vc.ENVS):
        sys.exit(usage)
    lib = _lib.load()
    if route_only:
        sys.exit(1 if route(env_name, lib) else 0)
    for name in vc.SWITCHES:                 # exactly the environment's switches
        assert os.environ.get(name) == vc.ENVS[env_name].get(name), (name, os.environ.get(name))
    rep = Report(env_name)
    t0 = time.time()
    cases = vc.cases_of(env_name)
    count, spent = {}, {}
    for case in cases:
        t1 = time.time()
        RUN[case["op"]](case, lib, rep)
        count[case["inst"]] = count.get(case["inst"], 0) + 1
        spent[case["op"]] = spent.get(case["op"], 0.0) + time.time() - t1
    dt_s = time.time() - t0
    print(f"env {env_name}: {len(cases)} cases, {len(rep.fail)} failures, {dt_s:.1f} s  (" +
          ", ".join(f"{op} {s:.1f} s" for op, s in spent.items()) + ")")
    for inst in sorted(count, key=repr):
        cells = " ".join(f"({crit}) {rep.worst[(inst, crit)]:6.3f}" for crit in "abu" if (inst, crit) in rep.worst)
        print(f"RATIO {env_name} {inst[0]} {inst[1]} {'/'.join(map(str, inst[2]))} cases {count[inst]} {cells}")
    for line in rep.fail:
        print(line)
    sys.exit(1 if rep.fail else 0)


if __name__ == "__main__":
    main()
