#!/usr/bin/env python3
"""Runs one part of the lip front end's kernel matrix (tests/_frontend_cases.py) under the switches of its environment,

    [L2S_BASICBLOCK_PHASE=0] [L2S_STEM_FT=n] check_frontend_kernels.py <environment>

<environment> is a key of fc.ENVS and the process must carry exactly its switches: the launchers read them once per process, hence
one child process per environment (tests/test_frontend_matrix_gpu.py).  Two modes need no device:

    check_frontend_kernels.py --route <part | child>   the restated rules of fc against l2s_basicblock_variant and l2s_stem_pool_frames
                                                      under this process's switches, and every case of the environment against `inst`
    check_frontend_kernels.py --cpu-f32 [op ...]      each operation in torch fp32 on the CPU, with the kernels' 16-bit intermediate
                                                      roundings, against the mirrored fp64 reference: the figures behind fc.F_of

References are fp64 on the CPU, convolutions as unfold + matmul.  The MIRRORED reference applies the 16-bit roundings the kernels
document: t1 after bias + PReLU, the hand-over between the blocks of an l2s_basiclayer_fused launch, out0 of the TAIL kernel, the
stem's input frames (fp32 and uint8 frames are rounded to 16 bits when they are staged; uint8 in l2s_preprocess_frames' fp32
arithmetic) and the order of the monotone stem path (round the conv value, pool, activate, round).  The UN-MIRRORED reference is
avhubert/resnet.py in fp64 with no intermediate rounding.

Every output is a window behind fc.GUARD guard rows (and in front of as many) of a NaN-filled device buffer.  Checks: the queried
instantiation (and the stem's frames per block) is the one the case claims; every byte outside the window is unchanged; the inputs
are unchanged; no NaN inside the window; a refused launch answers its code and writes nothing; `coded` results are bit-exact;
l2s_basiclayer_fused equals n_blocks single launches bit for bit; maxpool equals the maximum of the same stored values bit for bit; and
  (a) max error <= the tolerance of tests/test_kernels_gpu.py (BasicBlocks 2e-3 / 1.5e-2, stem 3e-3 / 2e-2 of max|ref|), mirrored;
  (b) |got - ref| <= 1.5 u max(|ref|, smallest normal) [16-bit output] + F 2^-24 A per element, u = 2^-11 f16 / 2^-8 bf16, A = the
      operation on absolute values (BasicBlock: |b2| + sum |w2| |t1| + |x| at the last convolution, TAIL with out0 as the residual;
      stem: (|b| + sum |w| |x|) max(1, |slope|), Swish 1.1, the maximum over the pooling window; avgpool: mean |x|; preprocess:
      (x / 255 + |mean|) / |std|), F = fc.F_of(fc.fkind(case), type);
  (u) max error against the un-mirrored reference <= twice the tolerance of (a).
Every stem case prints a digest of its output bytes (DIGEST lines: equal in all four stem children).  Prints the worst ratio per
instantiation and criterion (RATIO lines) and exits non-zero on any failure."""
import ctypes
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lip2speech_unit_amd import _lib  # noqa: E402
from tests import _frontend_cases as fc  # noqa: E402

U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
MIN_NORMAL = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126, "f32": 2.0 ** -126}
TOL_BB = {"f16": 2e-3, "bf16": 1.5e-2}       # tests/test_kernels_gpu.py: test_basicblock_fused_vs_torch and its C = 128 / TAIL twins
TOL_STEM = {"f16": 3e-3, "bf16": 2e-2}       # test_stem_pool_fused_vs_torch
EPS24 = 2.0 ** -24
NAN = float("nan")
f64, f32 = torch.float64, torch.float32
U8_MEAN, U8_STD = 0.421, 0.165


def t16(dt):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dt]


def dtc(dt):
    return {"f16": _lib.F16, "bf16": _lib.BF16, "f32": _lib.F32}[dt]


def rnd(x, dt):
    return x.to(t16(dt)).to(x.dtype)


def bits(x):
    return x.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[x.element_size()])


def seed_of(*key):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(repr(key))) % (2 ** 31)


def prelu(x, s):
    return torch.where(x >= 0, x, x * s)


# ---- convolutions as unfold + matmul ----------------------------------------------------------------------------------------------------
def unfold3x3(x):
    """x [n, H, W, C] -> [n H W, 9 C], K index = (ky * 3 + kx) * C + c (the packed weight layout), zero padding 1."""
    n, H, W, C = x.shape
    xp = torch.zeros(n, H + 2, W + 2, C, dtype=x.dtype)
    xp[:, 1: H + 1, 1: W + 1] = x
    return torch.cat([xp[:, ky: ky + H, kx: kx + W] for ky in range(3) for kx in range(3)], 3).reshape(n * H * W, 9 * C)


def conv3x3(x, w):
    n, H, W, _ = x.shape
    return (unfold3x3(x) @ w.t()).view(n, H, W, -1)


# ---- BasicBlock operands ----------------------------------------------------------------------------------------------------------------
def marks_of(H, W):
    """The marked positions of a coded map: corners, mid-edges, centre, kept at least 3 apart."""
    out = []
    for y in (0, H // 2, H - 1):
        for x in (0, W // 2, W - 1):
            if all(max(abs(y - a), abs(x - b)) >= 3 for a, b in out):
                out.append((y, x))
    return out


def coded_map(n, H, W, C, shift=0, levels=3):
    """x is non-zero only at the marks (image i drops mark i % len and rotates the channel code): value 1 + (c + i) % levels."""
    x = torch.zeros(n, H, W, C, dtype=f64)
    mk = marks_of(H, W)
    ch = torch.arange(C)
    for i in range(n):
        for j, (y, xx) in enumerate(mk):
            if len(mk) > 1 and j == (i + shift) % len(mk):
                continue
            x[i, y, xx] = (1 + (ch + i + shift) % levels).to(f64)
    return x


def coded_conv(C, j, rich, Cin=None, amp=2.0):
    """Weights [C, 9 Cin] of convolution j of a coded launch.  rich: output channel co reads ONE input channel per tap, a different one
    for each tap - (5 co + 3 tap + 1 + j) % Cin, not diagonal - with the weight amp^((tap + j) % 2)
    (amp = 2, or 1 in a launch of four blocks, whose values would pass 256 otherwise); thin: co reads the single tap
    (co + j) % 9 of channel (5 co + 1 + j) % Cin with the weight 1 (a shifted, permuted copy: the values do not grow)."""
    Cin = Cin or C
    w = torch.zeros(C, 9 * Cin, dtype=f64)
    for co in range(C):
        if rich:
            for tap in range(9):
                w[co, tap * Cin + (5 * co + 3 * tap + 1 + j) % Cin] = amp ** ((tap + j) % 2)
        else:
            w[co, ((co + j) % 9) * Cin + (5 * co + 1 + j) % Cin] = 1.0
    return w


def bb_operands(c, g):
    """2 nb convolutions: (ws, bs, ss), distinct per convolution."""
    C, nb, data, dt = c["C"], c["nb"], c["data"], c["dt"]
    ws, bs, ss = [], [], []
    ch = torch.arange(C)
    for j in range(2 * nb):
        if data == "coded":
            ws.append(coded_conv(C, j, rich=j < 2, amp=1.0 if nb >= 4 else 2.0))
            bs.append(((ch + j) % 2).to(f64))
            ss.append((2.0 ** -((ch + j) % 3).to(f64)))
            continue
        ws.append(rnd(torch.randn(C, 9 * C, generator=g, dtype=f64) / (9 * C) ** 0.5, dt))
        b = torch.randn(C, generator=g) * 0.1 - (0.5 if data == "negative" else 0.0)
        s = torch.rand(C, generator=g) * 0.4
        if data == "mixed-slope":
            s = torch.randn(C, generator=g) * 0.3
            s[(3 + j) % 5::5] = 0.0
            s[(1 + j) % 7::7] = 1.0
        bs.append(b.to(f64))
        ss.append(s.to(f64))
    return ws, bs, ss


def n_distinct(c):
    return min(c["N"], fc.POOL) if c["walk"] else c["N"]


_INPUTS = {}


def memo(key, make):
    if key not in _INPUTS:
        if len(_INPUTS) >= 6:
            _INPUTS.pop(next(iter(_INPUTS)))
        _INPUTS[key] = make()
    return _INPUTS[key]


def bb_inputs(c):
    def make():
        g = torch.Generator().manual_seed(seed_of("bb", c["dt"], c["N"], c["H"], c["W"], c["C"], c["nb"], c["data"]))
        n, H, W, C = n_distinct(c), c["H"], c["W"], c["C"]
        ws, bs, ss = bb_operands(c, g)
        if c["data"] == "coded":
            x = coded_map(n, H, W, C, levels=2 if c["nb"] >= 4 else 3)
        else:
            x = rnd(torch.randn(n, H, W, C, generator=g, dtype=f64) - (1.0 if c["data"] == "negative" else 0.0), c["dt"])
        return dict(x=x, ws=ws, bs=bs, ss=ss)
    return memo(("bb", c["dt"], c["name"]), make)


def tail_inputs(c):
    def make():
        g = torch.Generator().manual_seed(seed_of("tail", c["dt"], c["N"], c["data"]))
        n, H, W, dt = n_distinct(c), c["H"], c["W"], c["dt"]
        ch = torch.arange(128)
        if c["data"] == "coded":
            t0 = coded_map(n, H, W, 128)
            x0 = torch.zeros(n, 2 * H, 2 * W, 64, dtype=f64)
            c64 = torch.arange(64)
            for i in range(n):                            # even positions are seen by the stride-2 downsample, odd ones must not be
                for j, (y, xx) in enumerate(((0, 0), (2 * H - 2, 2 * W - 2), (10, 4), (1, 1), (3, 8), (2 * H - 1, 0), (6, 2 * W - 1))):
                    if j != i % 7:
                        x0[i, y, xx] = (1 + (c64 + i + j) % 3).to(f64)
            wa, wd = coded_conv(128, 0, True), torch.zeros(128, 64, dtype=f64)
            for co in range(128):
                wd[co, (5 * co + 1) % 64] = 4.0
            ws = [coded_conv(128, 1, False), coded_conv(128, 2, False)]
            bs = [((ch + j) % 2).to(f64) for j in range(3)]
            ss = [2.0 ** -((ch + j) % 3).to(f64) for j in range(3)]
            return dict(x0=x0, t0=t0, wa=wa, wd=wd, ba=bs[0], sa=ss[0], ws=ws, bs=bs[1:], ss=ss[1:])
        shift = 1.0 if c["data"] == "negative" else 0.0
        x0 = rnd(torch.randn(n, 2 * H, 2 * W, 64, generator=g, dtype=f64) - shift, dt)
        t0 = rnd(torch.randn(n, H, W, 128, generator=g, dtype=f64) - shift, dt)
        wa, w1, w2 = (rnd(torch.randn(128, 9 * 128, generator=g, dtype=f64) / (9 * 128) ** 0.5, dt) for _ in range(3))
        wd = rnd(torch.randn(128, 64, generator=g, dtype=f64) / 8, dt)      # the downsample's own scale: as large as the 3x3 term
        bs = [(torch.randn(128, generator=g) * 0.1 - (0.5 if c["data"] == "negative" else 0.0)).to(f64) for _ in range(3)]
        ss = []
        for j in range(3):
            s = torch.rand(128, generator=g) * 0.4
            if c["data"] == "mixed-slope":
                s = torch.randn(128, generator=g) * 0.3
                s[(3 + j) % 5::5] = 0.0
                s[(1 + j) % 7::7] = 1.0
            ss.append(s.to(f64))
        return dict(x0=x0, t0=t0, wa=wa, wd=wd, ba=bs[0], sa=ss[0], ws=[w1, w2], bs=bs[1:], ss=ss[1:])
    return memo(("tail", c["dt"], c["name"]), make)


def blocks_eval(x, ws, bs, ss, dt, ft, mirror=True, mut=None):
    """len(ws) / 2 BasicBlocks back to back on x [n, H, W, C]: (out [n, H, W, C] in ft, unrounded; A [n, H, W, C] fp64 of the last
    convolution).  mut: a subtle error planted for the mutation test."""
    cur = x.to(ft)
    nb = len(ws) // 2
    out = A = None
    for b in range(nb):
        w1, w2, b1, b2, s1, s2 = (t.to(ft) for t in (ws[2 * b], ws[2 * b + 1], bs[2 * b], bs[2 * b + 1], ss[2 * b], ss[2 * b + 1]))
        t1 = prelu(conv3x3(cur, w1) + b1, s1)
        if mirror:
            t1 = rnd(t1, dt)
        v = conv3x3(t1, w2) + b2 + cur
        if mut is not None and b == nb - 1:               # ONE term of conv2 dropped at one output element of a border position
            (i, y, xx, co), (tap, cin) = mut
            ky, kx = tap // 3, tap % 3
            v[i, y, xx, co] -= w2[co, tap * t1.shape[3] + cin] * t1[i, y + ky - 1, xx + kx - 1, cin]
        out = prelu(v, s2)
        if b == nb - 1:
            A = (conv3x3(t1.abs().to(f64), w2.abs().to(f64)) + b2.abs().to(f64) + cur.abs().to(f64)) * s2.abs().clamp(min=1.0).to(f64)
        elif mirror:
            cur = rnd(out, dt)
        else:
            cur = out
    return out, A


def planted_term(c, ins, i, y, x, cap, bound, ref):
    """The mutation that drops ONE term w2 t1 of the last convolution at output position (y, x) of image i (nb = 1): among the terms no
    larger than cap, the one largest against its element's bound (bound: [C], criterion (b) at that position) - an element that is
    quiet against the loudest sample - whose output (ref: [C]) stays positive, so that no PReLU slope scales the error.  Returns ((i, y, x, co), (tap, cin)) and the term's size."""
    C, H, W = c["C"], c["H"], c["W"]
    t1 = rnd(prelu(conv3x3(ins["x"], ins["ws"][0]) + ins["bs"][0], ins["ss"][0]), c["dt"])
    best = (0.0, None, 0.0)
    for tap in range(9):
        yy, xx = y + tap // 3 - 1, x + tap % 3 - 1
        if 0 <= yy < H and 0 <= xx < W:
            p = (ins["ws"][1][:, tap * C: (tap + 1) * C] * t1[i, yy, xx]).abs()
            q = torch.where((p <= cap) & (ref.view(C, 1) > cap), p, torch.zeros_like(p)) / bound.view(C, 1)
            co, cin = divmod(int(q.argmax()), C)
            if float(q[co, cin]) > best[0]:
                best = (float(q[co, cin]), ((i, y, x, co), (tap, cin)), float(p[co, cin]))
    return best[1], best[2]


def bb_eval(c, ins, ft, mirror=True, mut=None):
    return blocks_eval(ins["x"], ins["ws"], ins["bs"], ins["ss"], c["dt"], ft, mirror, mut)


def tail_eval(c, ins, ft, mirror=True, mut=None):
    t0, x0 = ins["t0"].to(ft), ins["x0"].to(ft)
    ds = x0[:, ::2, ::2] @ ins["wd"].to(ft).t()
    out0 = prelu(conv3x3(t0, ins["wa"].to(ft)) + ds + ins["ba"].to(ft), ins["sa"].to(ft))
    if mirror:
        out0 = rnd(out0, c["dt"])
    return blocks_eval(out0, ins["ws"], ins["bs"], ins["ss"], c["dt"], ft, mirror, mut)


# ---- stem operands -----------------------------------------------------------------------------------------------------------------------
CODED_PIX = ((0, 0), (0, 87), (87, 0), (87, 87), (0, 44), (44, 0), (87, 43), (43, 87), (44, 44))


def stem_slopes(kind, g, coded=False):
    if kind == "swish":
        return None
    ch = torch.arange(64)
    if coded:
        s = 2.0 ** -(ch % 3).to(f64)
        if kind == "mixed":
            s[5::7] = -s[5::7]
        elif kind == "zero-and-one":
            s = (ch % 2).to(f64)
        return s
    s = torch.rand(64, generator=g) * 0.5
    if kind == "mixed":
        s[5::7] = -s[5::7] - 0.1
    elif kind == "zero-and-one":
        s = ((ch * 7 // 3) % 2).float()
    return s.to(f64)


def stem_inputs(c):
    """frames: what is uploaded ([nclip, T, Hin, Win] uint8, or [nclip, T, 88, 88] fp64 values exact in the input type); x: the frames
    as the kernel sees them (fp64 [nclip, T, 88, 88], mirrored: rounded to 16 bits); xu: un-mirrored."""
    def make():
        dt, T, xk, data = c["dt"], c["T"], c["xk"], c["data"]
        g = torch.Generator().manual_seed(seed_of("stem", dt, c["B"], T, xk, c["Hin"], c["Win"], c["slopes"], data, c["wset"]))
        n = c["pool"] or c["B"]
        coded = data == "coded"
        mean, std = (0.0, 1.0) if coded else (U8_MEAN, U8_STD)
        if coded:
            base = torch.zeros(n, T, 88, 88, dtype=f64)
            for b in range(n):
                for t in range(T):
                    for k in range(3):
                        y, x = CODED_PIX[(t + 3 * k + b) % 9]
                        base[b, t, y, x] = 1.0
            w = torch.zeros(64, 245, dtype=f64)
            for co in range(64):
                if co + 64 * c["wset"] < 245:
                    w[co, co + 64 * c["wset"]] = 1.0
            bias = (torch.arange(64) % 3).to(f64)
        else:
            base = None
            w = rnd(torch.randn(64, 245, generator=g, dtype=f64) * 0.06, dt)
            bias = (torch.randn(64, generator=g) * 0.2 - {"negbias": 2.5, "lowbias": 0.3}.get(data, 0.0)).to(f64)
        if xk == "u8":
            dy, dx = (c["Hin"] - 88) // 2, (c["Win"] - 88) // 2
            frames = torch.randint(0, 256, (n, T, c["Hin"], c["Win"]), generator=g, dtype=torch.uint8)
            if coded:
                frames[:, :, dy: dy + 88, dx: dx + 88] = (base * 255).to(torch.uint8)
            crop = frames[:, :, dy: dy + 88, dx: dx + 88]
            v = crop.to(f32)
            x = rnd(((v / 255.0 - np.float32(mean)) * (np.float32(1.0) / np.float32(std))).to(f64), dt)   # l2s_preprocess_frames' fp32 arithmetic
            xu = (crop.to(f64) / 255.0 - float(np.float32(mean))) / float(np.float32(std))
        else:
            raw = base if coded else torch.randn(n, T, 88, 88, generator=g, dtype=f64)
            frames = raw.float().to(f64) if xk == "f32" else rnd(raw, dt)
            x, xu = rnd(frames, dt), frames
        return dict(frames=frames, x=x, xu=xu, w=w, bias=bias, slope=stem_slopes(c["slopes"], g, coded), mean=mean, std=std)
    return memo(("stem", c["dt"], c["name"]), make)


def stem_conv(x, w, bias, ft):
    """x [n, T, 88, 88], w [64, 245] (tap = (dt * 7 + dy) * 7 + dx): (conv [n, T, 64, 44, 44] in ft, A fp64 the same on absolute values)."""
    n, T = x.shape[:2]
    U = F.unfold(x.to(ft).reshape(n * T, 1, 88, 88), 7, padding=3, stride=2).view(n, T, 49, 1936)
    Ua = U.abs().to(f64)
    wt, wa = w.to(ft).view(64, 5, 49), w.abs().to(f64).view(64, 5, 49)
    out = torch.zeros(n, T, 64, 1936, dtype=ft)
    A = torch.zeros(n, T, 64, 1936, dtype=f64)
    for d in range(5):
        lo, hi = max(0, 2 - d), min(T, T + 2 - d)         # output frames t with 0 <= t + d - 2 < T
        if lo < hi:
            out[:, lo:hi] += wt[:, d] @ U[:, lo + d - 2: hi + d - 2]
            A[:, lo:hi] += wa[:, d] @ Ua[:, lo + d - 2: hi + d - 2]
    return (out + bias.to(ft).view(64, 1)).view(n, T, 64, 44, 44), (A + bias.abs().to(f64).view(64, 1)).view(n, T, 64, 44, 44)


def stem_act(v, slope):
    if slope is None:
        return v * torch.sigmoid(v)
    return prelu(v, slope.to(v.dtype).view(64, 1, 1))


def pool3x3(v):
    n, T = v.shape[:2]
    return F.max_pool2d(v.reshape(n * T, 64, 44, 44), 3, 2, 1).view(n, T, 64, 22, 22)


def stem_eval(c, ins, ft, mirror=True, pooled=True):
    """(y [n, T, 22, 22, 64] (pooled) or [n, T, 44, 44, 64] in ft, unrounded; A the same shape, fp64)."""
    slope, dt = ins["slope"], c["dt"]
    conv, A = stem_conv(ins["x"] if mirror else ins["xu"], ins["w"], ins["bias"], ft)
    A = A * (1.1 if slope is None else slope.abs().clamp(min=1.0).view(64, 1, 1))
    mono = slope is not None and bool((slope >= 0).all())
    if not pooled:
        y = stem_act(conv, slope)
    elif mirror and mono:                                 # the monotone path: round the conv value, pool, activate (, round)
        y, A = stem_act(pool3x3(rnd(conv, dt)), slope), pool3x3(A)
    else:
        y, A = pool3x3(stem_act(conv, slope)), pool3x3(A)
    return y.permute(0, 1, 3, 4, 2).contiguous(), A.permute(0, 1, 3, 4, 2).contiguous()


# ---- pools and preprocess -----------------------------------------------------------------------------------------------------------------
def pool_inputs(c):
    def make():
        g = torch.Generator().manual_seed(seed_of(c["op"], c["dt"], c["name"]))
        if c["op"] == "maxpool":
            n = min(c["N"], fc.POOL)
            return rnd(torch.randn(n, c["H"], c["W"], c["C"], generator=g).to(f64) - (3.0 if c["data"] == "negative" else 0.0), c["dt"])
        if c["op"] == "avgpool":
            return rnd(torch.randn(min(c["N"], 64), c["HW"], c["C"], generator=g).to(f64) + 0.25, c["dt"])
        n = min(c["B"] * c["T"], fc.POOL)
        fr = torch.randint(0, 256, (n, c["Hin"], c["Win"]), generator=g, dtype=torch.uint8)
        dy, dx = (c["Hin"] - c["crop"]) // 2, (c["Win"] - c["crop"]) // 2
        fr[0, dy: dy + 16, dx: dx + 16] = torch.arange(256, dtype=torch.uint8).view(16, 16)     # all 256 byte values inside the crop
        return fr
    return memo((c["op"], c["dt"], c["name"]), make)


def expand(x, n):
    """image i = pool[i % len(pool)]"""
    return x if x.shape[0] == n else x[torch.arange(n) % x.shape[0]]


def avgpool_eval(x, ft):
    """fp64: the mean; fp32: the kernel's sum in the order of the positions, times the rounded 1 / HW."""
    if ft == f64:
        return x.mean(1)
    s = torch.zeros(x.shape[0], x.shape[2], dtype=f32)
    for p in range(x.shape[1]):
        s += x[:, p].float()
    return s * (np.float32(1.0) / np.float32(x.shape[1]))


def preproc_eval(c, fr, ft):
    dy, dx = (c["Hin"] - c["crop"]) // 2, (c["Win"] - c["crop"]) // 2
    v = fr[:, dy: dy + c["crop"], dx: dx + c["crop"]]
    mean, std = np.float32(U8_MEAN), np.float32(U8_STD)
    A = (v.to(f64) / 255.0 + abs(float(mean))) / abs(float(std))
    if ft == f64:
        return (v.to(f64) / 255.0 - float(mean)) / float(std), A
    if c["dt"] == "f32":
        return (v.float() / 255.0 - mean) / std, A
    return (v.float() / 255.0 - mean) * (np.float32(1.0) / std), A


# ---- criteria -----------------------------------------------------------------------------------------------------------------------------
def bound_b(ref, A, dt, kind):
    ulp = fc.FU * U16[dt] * ref.abs().clamp(min=MIN_NORMAL[dt]) if dt in U16 else 0.0
    return ulp + fc.F_of(kind, dt) * EPS24 * A


def ratio_b(err, bound):
    """max err / bound; an element whose bound is zero must be exact."""
    q = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return q.max().item() if q.numel() else 0.0


class Report:
    def __init__(self, env):
        self.env, self.fail, self.worst, self.digest = env, [], {}, []

    def ratio(self, case, crit, r):
        k = (case["inst"], crit)
        self.worst[k] = max(self.worst.get(k, 0.0), r)

    def bad(self, case, why):
        self.fail.append(f"FAIL env={self.env} {case['dt']} {case['op']} {case['name']} inst={case['inst'][2]}: {why}")

    def judge(self, case, got, ref, A, tol, ref_u=None):
        """(a), (b) and (u) on one output (fp64, same shape); tol: fraction of max|ref| or None."""
        err = (got - ref).abs()
        if tol is not None:
            ta = tol * ref.abs().max().item()
            ra = err.max().item() / ta if ta > 0 else (0.0 if err.max().item() == 0 else float("inf"))
            self.ratio(case, "a", ra)
            if ra > 1.0:
                self.bad(case, f"(a) max err / tolerance = {ra:.3f}")
        bound = bound_b(ref, A, case["dt"], fc.fkind(case))
        rb = ratio_b(err, bound)
        self.ratio(case, "b", rb)
        if rb > 1.0:
            i = (err / bound.clamp(min=1e-300)).reshape(-1).argmax().item()
            self.bad(case, f"(b) err / bound = {rb:.3f} at flat index {i} (got {got.reshape(-1)[i].item():.9g}, ref {ref.reshape(-1)[i].item():.9g})")
        if ref_u is not None and tol is not None:
            tu = 2 * tol * ref_u.abs().max().item()
            ru = (got - ref_u).abs().max().item() / tu if tu > 0 else 0.0
            self.ratio(case, "u", ru)
            if ru > 1.0:
                self.bad(case, f"(u) max err against the un-mirrored reference / (2 x tolerance) = {ru:.3f}")

    def exact(self, case, got, ref):
        if not torch.equal(got, ref):
            i = (got != ref).reshape(-1).nonzero()[0].item()
            self.bad(case, f"coded: {(got != ref).sum().item()} elements differ from the exact result, first at flat index {i} "
                           f"(got {got.reshape(-1)[i].item()}, exact {ref.reshape(-1)[i].item()})")
        self.ratio(case, "b", 0.0)


# ---- guarded device buffers -----------------------------------------------------------------------------------------------------------------
class Guarded:
    """A [rows, C] window behind fc.GUARD guard rows of a NaN-filled flat buffer (and in front of as many)."""

    def __init__(self, rows, C, dtype, off=0):
        self.rows, self.C, self.base = rows, C, fc.GUARD * C + off
        self.host = torch.full(((rows + 2 * fc.GUARD) * C + off,), NAN, dtype=dtype)
        self.dev = self.host.cuda()

    def ptr(self):
        return self.dev.data_ptr() + self.base * self.dev.element_size()

    def check(self, rep, case, name, written=True):
        """Everything outside the window is bit-identical; returns the window [rows, C] on the host."""
        after = self.dev.cpu()
        lo, hi = self.base, self.base + self.rows * self.C
        if not (torch.equal(bits(after[:lo]), bits(self.host[:lo])) and torch.equal(bits(after[hi:]), bits(self.host[hi:]))):
            rep.bad(case, f"elements of {name} outside the window changed")
        if not written and not torch.equal(bits(after[lo:hi]), bits(self.host[lo:hi])):
            rep.bad(case, f"a refused launch wrote into {name}")
        return after[lo:hi].view(self.rows, self.C)


def dev_in(x, dtype):
    h = x.to(dtype).contiguous()
    return h.cuda(), h


def unchanged(rep, case, name, dev, host):
    if not torch.equal(bits(dev.cpu()), bits(host)):
        rep.bad(case, f"operand {name} changed")


def window(rep, c, name, win):
    if torch.isnan(win.float()).any():
        rep.bad(c, f"{torch.isnan(win.float()).sum().item()} NaN in the window of {name}")
        return None
    return win.to(f64)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ---- one case on the device -----------------------------------------------------------------------------------------------------------------
def layer_launch(lib, c, dx, dws, dbs, dss, yptr, nb, first=0):
    N, H, W, C = c["N"], c["H"], c["W"], c["C"]
    if nb == 1:
        j = 2 * first
        return lib.l2s_basicblock_fused(dx, dws[j].data_ptr(), dbs[j].data_ptr(), dss[j].data_ptr(), dws[j + 1].data_ptr(), dbs[j + 1].data_ptr(),
                                        dss[j + 1].data_ptr(), yptr, N, H, W, C, dtc(c["dt"]), stream())
    return lib.l2s_basiclayer_fused(dx, ptr_array(dws), ptr_array(dbs), ptr_array(dss), nb, yptr, N, H, W, C, dtc(c["dt"]), stream())


def judge_images(rep, c, win, out, A, out_u, shape):
    """win: the window [N rows, C]; out / A / out_u: the references of the distinct images."""
    got = window(rep, c, "y", win)
    if got is None:
        return
    N, n = c["N"], out.shape[0]
    if n < N:                                             # image i = pool[i % n]: the same bytes in, the same bytes out; the pool is judged
        flat = bits(win).view(N, -1)
        twin = (flat != flat[torch.arange(N) % n]).any(1)
        if twin.any():
            rep.bad(c, f"{int(twin.sum())} images differ from the image of the same content, first image {int(twin.nonzero()[0])}")
    got = got.view(N, *shape)[:n]
    if c["data"] == "coded":
        rep.exact(c, got, out)
        return
    rep.judge(c, got, out, A, TOL_BB[c["dt"]], out_u)


def run_bb(c, lib, rep):
    N, H, W, C, nb, dt, el = c["N"], c["H"], c["W"], c["C"], c["nb"], c["dt"], t16(c["dt"])
    var = lib.l2s_basicblock_variant(N, H, W, C, nb, dtc(dt))
    if var != c["inst"][2]:
        rep.bad(c, f"instantiation: the query answers {var}")
        return
    ins = bb_inputs(c)
    dx, hx = dev_in(expand(ins["x"], N).reshape(N * H * W, C), el)
    nconv = 2 * min(nb, 4) if c["expect"] == 0 else 2 * nb
    ops = [(dev_in(ins["ws"][j % len(ins["ws"])], el)) for j in range(nconv)]
    dws, dbs, dss = [o[0] for o in ops], [ins["bs"][j % len(ins["bs"])].float().cuda() for j in range(nconv)], \
        [ins["ss"][j % len(ins["ss"])].float().cuda() for j in range(nconv)]
    gy = Guarded(N * H * W, C, el)
    rc = layer_launch(lib, c, dx.data_ptr(), dws, dbs, dss, gy.ptr(), nb)
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y", written=rc == 0)
    unchanged(rep, c, "x", dx, hx)
    for j, o in enumerate(ops):
        unchanged(rep, c, f"w[{j}]", *o)
    if rc != 0:
        return
    out, A = bb_eval(c, ins, f64)
    out_u = bb_eval(c, ins, f64, mirror=False)[0] if c["data"] != "coded" else None
    judge_images(rep, c, win, out, A, out_u, (H, W, C))
    if nb > 1:                                            # bit-equality with nb single launches
        cur = dx
        for b in range(nb):
            gs = Guarded(N * H * W, C, el)
            r = layer_launch(lib, c, cur.data_ptr(), dws, dbs, dss, gs.ptr(), 1, first=b)
            if r != 0:
                rep.bad(c, f"single launch of block {b} answers {r}")
                return
            torch.cuda.synchronize()
            cur = gs.dev[gs.base: gs.base + N * H * W * C]
        if not torch.equal(bits(cur.cpu().view(N * H * W, C)), bits(win)):
            rep.bad(c, f"l2s_basiclayer_fused differs from {nb} l2s_basicblock_fused launches")


def run_tail(c, lib, rep):
    N, H, W, dt, el = c["N"], c["H"], c["W"], c["dt"], t16(c["dt"])
    ins = tail_inputs(c)
    mis = c["misalign"]
    pad = lambda t: torch.cat([t.reshape(-1), t.new_zeros(8)])     # room to shift a pointer by 8 bytes
    dx0, hx0 = dev_in(pad(expand(ins["x0"], N)), el)
    dt0, ht0 = dev_in(pad(expand(ins["t0"], N)), el)
    wa = torch.cat([ins["wa"], ins["wd"], torch.zeros(128, 64, dtype=f64)], 1)
    dwa, hwa = dev_in(pad(wa), el)
    dw1, hw1 = dev_in(ins["ws"][0], el)
    dw2, hw2 = dev_in(ins["ws"][1], el)
    fl = lambda t: pad(t.float()).cuda()
    dba, dsa, db1, ds1, db2, ds2 = fl(ins["ba"]), fl(ins["sa"]), fl(ins["bs"][0]), fl(ins["ss"][0]), fl(ins["bs"][1]), fl(ins["ss"][1])
    gy = Guarded(N * H * W, 128, el, off=4 if mis == "y" else 0)
    sh = lambda name, t: t.data_ptr() + (8 if mis == name else 0)
    rc = lib.l2s_basicstage128_tail_fused(sh("x0", dx0), sh("t0", dt0), sh("wa", dwa), dba.data_ptr(), dsa.data_ptr(), dw1.data_ptr(), db1.data_ptr(),
                                          ds1.data_ptr(), dw2.data_ptr(), sh("b2", db2), ds2.data_ptr(), gy.ptr(), N, H, W, dtc(dt), stream())
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y", written=rc == 0)
    for name, d, h in (("x0", dx0, hx0), ("t0", dt0, ht0), ("wa", dwa, hwa), ("w1", dw1, hw1), ("w2", dw2, hw2)):
        unchanged(rep, c, name, d, h)
    if rc != 0:
        return
    out, A = tail_eval(c, ins, f64)
    out_u = tail_eval(c, ins, f64, mirror=False)[0] if c["data"] != "coded" else None
    judge_images(rep, c, win, out, A, out_u, (H, W, 128))


def pack_stem_w(w, el):
    """[64, 245] -> [64, 288]: k = (dt * 7 + dy) * 8 + dx, dx == 7 zero, K 280 -> 288."""
    wk = torch.zeros(64, 35, 8, dtype=f64)
    wk[:, :, :7] = w.view(64, 35, 7)
    wp = torch.zeros(64, 288, dtype=f64)
    wp[:, :280] = wk.reshape(64, 280)
    return wp.to(el).contiguous()


def stem_device_operands(c, ins):
    el, B = t16(c["dt"]), c["B"]
    fr = expand(ins["frames"], B).contiguous()
    hx = fr if c["xk"] == "u8" else fr.to(f32 if c["xk"] == "f32" else el).contiguous()
    hw = pack_stem_w(ins["w"], el)
    ds = ins["slope"].float().cuda() if ins["slope"] is not None else None
    return hx.cuda(), hx, hw.cuda(), hw, ins["bias"].float().cuda(), ds


def stem_launch(lib, c, ins, dx, dw, db, ds, yptr):
    sp = ds.data_ptr() if ds is not None else None
    if c["xk"] == "u8":
        return lib.l2s_stem_pool_fused_u8(dx.data_ptr(), c["Hin"], c["Win"], 88, ins["mean"], ins["std"], dw.data_ptr(), db.data_ptr(), sp, yptr,
                                          c["B"], c["T"], dtc(c["dt"]), stream())
    return lib.l2s_stem_pool_fused(dx.data_ptr(), int(c["xk"] == "f32"), dw.data_ptr(), db.data_ptr(), sp, yptr, c["B"], c["T"], 88, 88,
                                   dtc(c["dt"]), stream())


def run_stem(c, lib, rep):
    B, T, dt, el = c["B"], c["T"], c["dt"], t16(c["dt"])
    ft = lib.l2s_stem_pool_frames(B, T)
    if ft != c["ft"]:
        rep.bad(c, f"frames per block: the query answers {ft}, the case claims {c['ft']}")
        return
    ins = stem_inputs(c)
    dx, hx, dw, hw, db, ds = stem_device_operands(c, ins)
    gy = Guarded(B * T * 484, 64, el)
    rc = stem_launch(lib, c, ins, dx, dw, db, ds, gy.ptr())
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y")
    unchanged(rep, c, "x", dx, hx)
    unchanged(rep, c, "w", dw, hw)
    rep.digest.append(f"DIGEST {dt} {c['name']} {hashlib.sha1(bits(win).numpy().tobytes()).hexdigest()}")
    got = window(rep, c, "y", win)
    if got is None:
        return
    got = got.view(B, T, 22, 22, 64)
    ref, A = stem_eval(c, ins, f64)
    ref, A = expand(ref, B), expand(A, B)
    if c["data"] == "coded":
        rep.exact(c, got, ref)
        return
    rep.judge(c, got, ref, A, TOL_STEM[dt], expand(stem_eval(c, ins, f64, mirror=False)[0], B))


def run_stem2(c, lib, rep):
    """l2s_stem_conv3d against fp64; l2s_maxpool2d_3x3s2 of it against the fused kernel: <= 2 ulp (TWOSTEP lines: the figures)."""
    B, T, dt, el = c["B"], c["T"], c["dt"], t16(c["dt"])
    ins = stem_inputs(c)
    dx, hx, dw, hw, db, ds = stem_device_operands(c, ins)
    gc = Guarded(B * T * 1936, 64, el)
    rc = lib.l2s_stem_conv3d(dx.data_ptr(), int(c["xk"] == "f32"), dw.data_ptr(), db.data_ptr(), ds.data_ptr() if ds is not None else None, gc.ptr(),
                             B, T, 88, 88, dtc(dt), stream())
    torch.cuda.synchronize()
    if rc != 0:
        rep.bad(c, f"l2s_stem_conv3d answers {rc}")
        return
    win = gc.check(rep, c, "conv")
    unchanged(rep, c, "x", dx, hx)
    got = window(rep, c, "conv", win)
    if got is None:
        return
    ref, A = stem_eval(c, ins, f64, pooled=False)
    rep.judge(c, got.view(B, T, 44, 44, 64), ref, A, TOL_STEM[dt], stem_eval(c, ins, f64, mirror=False, pooled=False)[0])
    g2, gf = Guarded(B * T * 484, 64, el), Guarded(B * T * 484, 64, el)
    r1 = lib.l2s_maxpool2d_3x3s2(gc.ptr(), g2.ptr(), B * T, 44, 44, 64, dtc(dt), stream())
    r2 = stem_launch(lib, c, ins, dx, dw, db, ds, gf.ptr())
    torch.cuda.synchronize()
    if r1 != 0 or r2 != 0:
        rep.bad(c, f"maxpool answers {r1}, the fused stem {r2}")
        return
    y2, yf = g2.check(rep, c, "pooled"), gf.check(rep, c, "fused")
    a, b = bits(yf).int(), bits(y2).int()
    d = (a - b).abs()                                     # same sign: adjacent 16-bit patterns differ by exactly 1
    far = ((a < 0) != (b < 0)) & (y2.float() != 0) & (yf.float() != 0) | ((a < 0) == (b < 0)) & (d > 2)
    # an output that has cancelled to less than the two kernels' accumulation-order allowance (F = 8 each, criterion (b)) has no
    # meaningful ulp: there the two are held to that allowance instead (profiles/frontend_matrix.md, Finding 2)
    allow = 2 * 8.0 * EPS24 * stem_eval(c, ins, f64)[1].reshape(-1, 64)
    far &= (yf.double() - y2.double()).abs() > allow
    frac = float((d > 0).float().mean())
    rep.digest.append(f"TWOSTEP {dt} {c['name']}: max {int(d.max())} ulp, {int((d > 2).sum())} of {d.numel()} past 2 ulp, {int(far.sum())} of them past the "
                      f"allowance, {frac:.4f} differ")
    if bool(far.any()):                                   # (the share that differs follows the share of negative outputs: it is printed, not bounded)
        rep.bad(c, f"fused stem vs conv3d + maxpool: {int(far.sum())} outputs past 2 ulp and the allowance, {frac:.4f} of the outputs differ")


def run_maxpool(c, lib, rep):
    N, H, W, C, dt, el = c["N"], c["H"], c["W"], c["C"], c["dt"], t16(c["dt"])
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pool = pool_inputs(c)
    dx, hx = dev_in(expand(pool.to(el), N).reshape(N * H * W, C), el)
    gy = Guarded(N * Ho * Wo, C, el)
    rc = lib.l2s_maxpool2d_3x3s2(dx.data_ptr(), gy.ptr(), N, H, W, C, dtc(dt), stream())
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y", written=rc == 0)
    unchanged(rep, c, "x", dx, hx)
    if rc != 0:
        return
    ref = F.max_pool2d(pool.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(el)      # the maximum of the same stored values
    if not torch.equal(bits(win.view(N, Ho, Wo, C)), bits(expand(ref, N).contiguous())):
        rep.bad(c, "maxpool is not the maximum of the stored values, bit for bit")
    rep.ratio(c, "b", 0.0)


def run_avgpool(c, lib, rep):
    N, HW, C, dt, el = c["N"], c["HW"], c["C"], c["dt"], t16(c["dt"])
    pool = pool_inputs(c)
    dx, hx = dev_in(expand(pool.to(el), N).reshape(N * HW, C), el)
    gy = Guarded(N, C, el)
    rc = lib.l2s_avgpool_hw(dx.data_ptr(), gy.ptr(), N, HW, C, dtc(dt), stream())
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y")
    unchanged(rep, c, "x", dx, hx)
    got = window(rep, c, "y", win)
    if got is None:
        return
    rep.judge(c, got, expand(avgpool_eval(pool, f64), N), expand(pool.abs().mean(1), N), None)
    if HW == 1 and not torch.equal(bits(win), bits(hx.view(N, C))):
        rep.bad(c, "the average over one position is not that position, bit for bit")


def run_preproc(c, lib, rep):
    B, T, crop, dt, el = c["B"], c["T"], c["crop"], c["dt"], t16(c["dt"])
    pool = pool_inputs(c)
    fr = expand(pool, B * T).contiguous()
    dx = fr.cuda()
    gy = Guarded(B * T * crop, crop, el)
    rc = lib.l2s_preprocess_frames(dx.data_ptr(), gy.ptr(), B, T, c["Hin"], c["Win"], crop, U8_MEAN, U8_STD, dtc(dt), stream())
    torch.cuda.synchronize()
    if rc != c["expect"]:
        rep.bad(c, f"the launch answers {rc}, expected {c['expect']}")
        return
    win = gy.check(rep, c, "y")
    unchanged(rep, c, "frames", dx, fr)
    got = window(rep, c, "y", win)
    if got is None:
        return
    ref, A = preproc_eval(c, pool, f64)
    rep.judge(c, got.view(B * T, crop, crop), expand(ref, B * T), expand(A, B * T), None)


RUN = {"bb": run_bb, "tail": run_tail, "stem": run_stem, "stem2": run_stem2, "maxpool": run_maxpool, "avgpool": run_avgpool,
       "preproc": run_preproc}


# ---- host-only modes ------------------------------------------------------------------------------------------------------------------------
def route(env_name, lib):
    """The restated rules against the two queries under this process's switches; every case of the environment against its claim."""
    env = {k: os.environ[k] for k in fc.SWITCHES if k in os.environ}
    bad = n = 0

    def expect(what, got, want):
        nonlocal bad, n
        n += 1
        if got != want:
            bad += 1
            if bad < 20:
                print(f"ROUTE {what}: the query answers {got}, the restated rule {want}")

    for dtn in (0, 1):
        for C in (32, 64, 128, 256):
            for nb in (0, 1, 2, 4, 5):
                for H in (0, 1, 2, 3, 4, 5, 10, 11, 13, 15, 16, 17, 21, 22, 23, 24, 93, 94, 95, 96, 190, 191, 574, 575):
                    for W in (0, 1, 2, 3, 4, 5, 10, 11, 13, 21, 22, 23, 28, 29, 30, 31):
                        for N in (0, 1, 300):
                            expect(f"basicblock N={N} H={H} W={W} C={C} nb={nb}", lib.l2s_basicblock_variant(N, H, W, C, nb, dtn),
                                   fc.basicblock_variant(N, H, W, C, nb, env))
    for C, H, W in ((64, 22, 22), (64, 5, 7), (128, 11, 11)):
        expect(f"basicblock fp32 C={C}", lib.l2s_basicblock_variant(2, H, W, C, 1, _lib.F32), fc.basicblock_variant(2, H, W, C, 1, env, dtype_ok=False))
    expect("basicblock 2^31 elements at C = 128", lib.l2s_basicblock_variant(138655, 11, 11, 128, 1, 0), fc.basicblock_variant(138655, 11, 11, 128, 1, env))
    for B in list(range(1, 40)) + [340, 341, 342, 343, 682, 683, 2048]:
        for T in list(range(1, 80)) + [500, 2047, 2048]:
            expect(f"stem frames B={B} T={T}", lib.l2s_stem_pool_frames(B, T), fc.stem_ft(B, T, env))
    expect("stem frames B=0", lib.l2s_stem_pool_frames(0, 5), fc.ESHAPE)
    expect("stem frames T=0", lib.l2s_stem_pool_frames(5, 0), fc.ESHAPE)
    part = fc.part_of(env_name)[0]                        # a child, or a part: the cases of all its children
    if part in fc.PARTS and env == fc.PARTS[part]:
        for c in (fc.cases_of(env_name) if env_name in fc.ENVS else [c for e in fc.ENVS if fc.part_of(e)[0] == part for c in fc.cases_of(e)]):
            if c["op"] == "bb":
                expect(f"case {c['dt']} {c['name']}", lib.l2s_basicblock_variant(c["N"], c["H"], c["W"], c["C"], c["nb"], dtc(c["dt"])), c["inst"][2])
            elif c["op"] == "stem":
                expect(f"case {c['dt']} {c['name']}", lib.l2s_stem_pool_frames(c["B"], c["T"]), c["ft"])
    print(f"routed {n - bad} of {n} queries under {env}")
    return bad


def eval_case(c, ft, mirror=True, mut=None):
    """(value of the distinct images / clips, unrounded in fp64 and rounded to the output type in fp32; A): the device-free twin of RUN."""
    op = c["op"]
    if op == "bb":
        y, A = bb_eval(c, bb_inputs(c), ft, mirror, mut)
    elif op == "tail":
        y, A = tail_eval(c, tail_inputs(c), ft, mirror, mut)
    elif op in ("stem", "stem2"):
        y, A = stem_eval(c, stem_inputs(c), ft, mirror, pooled=op == "stem")
    elif op == "avgpool":
        x = pool_inputs(c)
        y, A = avgpool_eval(x, ft), x.abs().mean(1)
    elif op == "preproc":
        y, A = preproc_eval(c, pool_inputs(c), ft)
    else:
        raise ValueError(op)
    return (y if ft == f64 else rnd(y, c["dt"])), A


def ratio_a_of(c, got, ref):
    tol = (TOL_STEM if c["op"] in ("stem", "stem2") else TOL_BB)[c["dt"]]
    return (got.to(f64) - ref).abs().max().item() / (tol * ref.abs().max().item())


def ratio_b_of(c, got, ref, A):
    return ratio_b((got.to(f64) - ref).abs(), bound_b(ref, A, c["dt"], fc.fkind(c)))


def cpu_f32(ops_filter=None):
    """Each operation in torch fp32 on the CPU (16-bit intermediates as in the kernels) against the mirrored fp64 reference, in units of
    2^-24 A: the figures of fc.CPU_F32_WORST."""
    worst, seen = {}, set()
    for env_name in fc.ENVS:
        for c in fc.cases_of(env_name):
            key = (c["op"], c["dt"], c["name"])
            if key in seen or c["expect"] != 0 or c.get("data") == "coded" or c["op"] == "maxpool" or (ops_filter and c["op"] not in ops_filter):
                continue
            seen.add(key)
            (ref, A), got = eval_case(c, f64), eval_case(c, f32)[0]
            err = (got.to(f64) - ref).abs()
            if c["dt"] in U16:                             # the output's own rounding is the other term of (b)
                err = (err - fc.FU * U16[c["dt"]] * ref.abs().clamp(min=MIN_NORMAL[c["dt"]])).clamp(min=0.0)
            q = ratio_b(err, EPS24 * A)
            k = (fc.fkind(c), c["dt"])
            if q > worst.get(k, (-1.0, ""))[0]:
                worst[k] = (q, c["name"])
    for (kind, dt), (r, name) in sorted(worst.items()):
        print(f"CPUF32 {kind:12s} {dt:4s} worst |fp32 - fp64| / (2^-24 A) = {r:10.3f}  ({name})")
    print("CPU_F32_WORST = {" + ", ".join(f"({k!r}, {dt!r}): {r:.3f}" for (k, dt), (r, _) in sorted(worst.items())) + "}")


def main():
    args = sys.argv[1:]
    usage = f"usage: check_frontend_kernels.py [--route] <{' | '.join(fc.ENVS)}>  or  check_frontend_kernels.py --cpu-f32 [op ...]"
    if not args or args[0] in ("-h", "--help"):
        sys.exit(usage)
    if args[0] == "--cpu-f32":
        cpu_f32(set(args[1:]))
        return
    route_only = args[0] == "--route"
    env_name = args[-1]
    if len(args) != (2 if route_only else 1) or (not route_only and env_name not in fc.ENVS):
        sys.exit(usage)
    lib = _lib.load()
    if route_only:
        sys.exit(1 if route(env_name, lib) else 0)
    for name in fc.SWITCHES:                 # exactly the environment's switches
        assert os.environ.get(name) == fc.ENVS[env_name].get(name), (name, os.environ.get(name))
    rep = Report(env_name)
    t0 = time.time()
    cases = fc.cases_of(env_name)
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
        print(f"RATIO {env_name} {inst[0]} {inst[1]} {inst[2]} cases {count[inst]} {cells}")
    for line in rep.digest:
        print(line)
    for line in rep.fail:
        print(line)
    sys.exit(1 if rep.fail else 0)


if __name__ == "__main__":
    main()
