#!/usr/bin/env python3
"""Runs one part of the unit decoders' and layout / cast kernels' matrix (tests/_glue_cases.py) on the device,

    check_glue_kernels.py <part>            part: a member of gc.PARTS; one child process per part (tests/test_glue_matrix_gpu.py)

Two modes need no device:

    check_glue_kernels.py --cpu-ref [part ...]   every reference of every case, with the time each part takes
    check_glue_kernels.py --cpu-f32              each inexact operation in torch fp32 on the CPU (the decoders: oracle/decode.py) against
                                                 its fp64 reference in units of 2^-24 A: the figures behind gc.F_of, and the G of every
                                                 random beam case

Every operand is a window of a larger device buffer: gc.GUARD guard rows in front of and behind it, the padding columns of its leading
dimension around it, all filled with a canary (NaN for fp32, 0x5A5A5A5A for int32, 0x5A5A for int16 and the 16-bit float types, 0x5A
for bytes).  Every launch runs twice into fresh buffers.  Checks, every case: the launch answers the code the case expects; every byte
outside the documented window of an output is unchanged; every input is unchanged; a refused launch writes nothing at all; the two runs
give the same bytes; no NaN canary is left where the reference holds a number.  Then per kernel:
  * casts, repeat2_cast, rows_f32_to_16_masked, broadcast_rows, transpose, both embeddings, lens_from_mask, splitk_reduce,
    ctc_repeat_labels, split_hi_lo with act 0 / 1 and every f32 route: bit-exact against torch on the CPU (NaN-ness only for NaN);
    masked rows are exactly +0.
  * split_hi_lo: |hi + lo - y| <= u^2 |y| + the type's smallest subnormal (y exact for act 0 / 1); act 2: the same against GELU in fp64
    plus F 2^-24 A, A = |x| (0.5 (1 + |erf(x / sqrt 2)|) + |x| phi(x)).
  * conv_post_tanh: (a) 2e-5 absolute; (b) F 2^-24 A, A = (|bias| + sum |leaky(x)| |w|) (1 - tanh^2(acc)) + |tanh(acc)|; pcm ==
    trunc(wav 32768) through int32, wrapped, from the kernel's own wav; the saturated samples are exactly +-1.0 and -32768.
  * greedy / beam decode: tokens exact (beam: every rank of a coded clip, the separated ranks of a random one), pad and zeros behind EOS,
    (a) 1e-4 and (b) F 2^-24 A on positional scores and scores, A = |x_tok / temp| + |max x / temp| + |log sum exp| + 1 (beam: plus the
    cumulative score's magnitude), the score's A = sum A / (L + 1)^lenpen.
  * ctc_frames: labels and top-K classes exact, log(p + FLT_MIN) within F 2^-24 (|x - max| + |log sum exp| + 1).
Prints the worst ratio per instantiation and criterion (RATIO lines) and exits non-zero on any failure."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lip2speech_unit_amd import _lib  # noqa: E402
from tests import _decode_reference as dr  # noqa: E402
from tests import _glue_cases as gc  # noqa: E402

f64, f32, i32, i16, u8 = torch.float64, torch.float32, torch.int32, torch.int16, torch.uint8
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
MIN_SUB = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}
MAX16 = {"f16": 6e4, "bf16": 1e30}
EPS24 = 2.0 ** -24
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
NAN = float("nan")
G = gc.GUARD


def t16(dt):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": f32}[dt]


def dtc(dt):
    return {"f16": _lib.F16, "bf16": _lib.BF16, "f32": _lib.F32}[dt]


def bits(x):
    return x.view({1: u8, 2: i16, 4: i32}[x.element_size()])


def seed_of(*key):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(repr(key))) % (2 ** 31)


def gen(c):
    return torch.Generator().manual_seed(seed_of(c["op"], c["name"].replace("-offset", ""), c["dt"]))      # conv_post: both twins get the same data


def stream():
    return torch.cuda.current_stream().cuda_stream


def canary(n, td):
    if td == f32:
        return torch.full((n,), NAN, dtype=f32)
    size = torch.empty(0, dtype=td).element_size()
    return torch.full((n,), {1: 0x5A, 2: gc.CANARY16, 4: gc.CANARY32}[size], dtype={1: u8, 2: i16, 4: i32}[size]).view(td)


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------------------
class Spec:
    """A [rows, cols] window at column col0 of rows of `ld` elements, gc.GUARD guard rows on either side, `off` elements in front."""

    def __init__(self, td, rows, cols, ld=None, col0=0, data=None, out=False, off=0):
        self.td, self.rows, self.cols, self.ld, self.col0, self.out, self.off = td, rows, cols, ld or (col0 + cols), col0, out, off
        self.data = None if data is None else data.reshape(rows, cols).to(td)

    def build(self):
        h = canary(self.off + (self.rows + 2 * G) * self.ld, self.td)
        if self.data is not None:
            self.window(h).copy_(self.data)
        return h

    def elem0(self):
        return self.off + G * self.ld

    def window(self, flat):
        return flat[self.off:].view(self.rows + 2 * G, self.ld)[G: G + self.rows, self.col0: self.col0 + self.cols]

    def mask(self):
        m = torch.zeros(self.off + (self.rows + 2 * G) * self.ld, dtype=torch.bool)
        self.window(m).fill_(True)
        return m


class Kase:
    """specs: name -> Spec; call(lib, p) -> code with p: name -> device address (None for an absent operand); ref() -> whatever judge needs;
    judge(rep, c, got, ref) with got: name -> the window of every output on the host; cpuf32() -> {kind: ratio at F = 1} or None."""

    def __init__(self, specs, call, ref, judge, cpuf32=None):
        self.specs, self.call, self.ref, self.judge, self.cpuf32 = specs, call, ref, judge, cpuf32


def ratio_b(err, bound):
    """max err / bound; an element whose bound is zero must be exact."""
    q = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return q.max().item() if q.numel() else 0.0


class Report:
    def __init__(self, part):
        self.part, self.fail, self.worst = part, [], {}

    def ratio(self, case, crit, r):
        k = (case["inst"], crit)
        self.worst[k] = max(self.worst.get(k, 0.0), r)

    def bad(self, case, why):
        self.fail.append(f"FAIL part={self.part} {case['dt']} {case['name']} inst={case['inst']}: {why}")

    def exact(self, case, name, got, ref):
        """bit for bit; two NaN are equal whatever their payload"""
        if got.shape != ref.shape or got.dtype != ref.dtype:
            self.bad(case, f"{name}: shape / type {tuple(got.shape)} {got.dtype}, reference {tuple(ref.shape)} {ref.dtype}")
            return
        ne = bits(got.contiguous()) != bits(ref.contiguous())
        if got.is_floating_point():
            ne &= ~(torch.isnan(got) & torch.isnan(ref))
        if ne.any():
            i = ne.reshape(-1).nonzero()[0].item()
            self.bad(case, f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the exact result, first at flat index {i} "
                           f"(got {got.reshape(-1)[i].item()!r}, exact {ref.reshape(-1)[i].item()!r})")
        self.ratio(case, "exact", 0.0)

    def bounded(self, case, crit, got, ref, bound):
        got = got.to(f64)
        if torch.isnan(got).any():
            self.bad(case, f"({crit}) {int(torch.isnan(got).sum())} NaN left in the window")
            return
        err = (got - ref).abs()
        bound = bound if torch.is_tensor(bound) else torch.full_like(err, bound)
        r = ratio_b(err, bound)
        self.ratio(case, crit, r)
        if r > 1.0:
            i = (err / bound.clamp(min=1e-300)).reshape(-1).argmax().item()
            self.bad(case, f"({crit}) err / bound = {r:.3f} at flat index {i} (got {got.reshape(-1)[i].item():.9g}, ref {ref.reshape(-1)[i].item():.9g})")


def run_case(c, lib, rep):
    k = BUILD[c["op"]](c)
    runs = []
    for _ in range(2):
        host = {n: s.build() for n, s in k.specs.items()}
        dev = {n: h.cuda() for n, h in host.items()}
        p = {n: dev[n].data_ptr() + k.specs[n].elem0() * dev[n].element_size() for n in dev}
        rc = k.call(lib, p)
        torch.cuda.synchronize()
        runs.append((rc, host, {n: d.cpu() for n, d in dev.items()}))
    (rc, host, after), (rc2, _, again) = runs
    if rc != c["expect"] or rc2 != rc:
        rep.bad(c, f"the launch answers {rc} (then {rc2}), expected {c['expect']}")
        return
    got = {}
    for n, s in k.specs.items():
        b0, b1 = bits(host[n]), bits(after[n])
        if not s.out or rc != 0:
            if not torch.equal(b0, b1):
                rep.bad(c, f"a refused launch wrote into {n}" if rc != 0 else f"operand {n} changed")
            continue
        m = s.mask()
        if not torch.equal(b0[~m], b1[~m]):
            rep.bad(c, f"{int((b0[~m] != b1[~m]).sum())} elements of {n} outside its window changed")
        if not torch.equal(b1, bits(again[n])):
            rep.bad(c, f"{n}: two runs of the same launch give different bytes")
        got[n] = s.window(after[n]).clone()
    if rc == 0:
        k.judge(rep, c, got, k.ref())


# ---- data --------------------------------------------------------------------------------------------------------------------------------------
_CODED = {}


def cast_coded(dt):
    """The fp32 data that tell round-to-nearest-even from truncation and from round-half-away: every 16-bit value widened, the midpoints
    between neighbours (the one between the largest finite value and the next power of two included: the overflow threshold) with their
    fp32 neighbours either side, both signs, +-0, fp32 subnormals, +-inf, NaN."""
    if dt not in _CODED:
        t = t16(dt)
        every = torch.arange(-32768, 32768, dtype=i16).view(t).float()
        top = {"f16": 0x7BFF, "bf16": 0x7F7F}[dt]
        lo = torch.arange(0, top + 1, dtype=i32).to(i16).view(t).to(f64)
        hi = torch.cat([lo[1:], (2 * lo[-1] - lo[-2]).reshape(1)])
        mid = ((lo + hi) / 2).float()
        assert torch.equal(mid.to(f64), (lo + hi) / 2)
        near = torch.cat([mid, torch.nextafter(mid, torch.tensor(math.inf)), torch.nextafter(mid, torch.tensor(-math.inf))])
        sub = torch.tensor([2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 3 * 2.0 ** -149, 0.75 * 2.0 ** -126], dtype=f64).float()
        special = torch.tensor([0.0, -0.0, math.inf, -math.inf, NAN, 65504.0, 65519.996, 65520.0, -65520.0], dtype=f32)
        _CODED[dt] = torch.cat([every, near, -near, sub, -sub, special])
    return _CODED[dt]


def coded_fill(dt, n):
    """n elements of cast_coded: all of it (repeated) where it fits, a stride through it otherwise"""
    cd = cast_coded("f16" if dt == "f32" else dt)
    i = torch.arange(n)
    return cd[i % cd.numel()] if n >= cd.numel() else cd[(i * 7919 + 65536) % cd.numel()]


def mixed_f32(c, n, scale=3.0):
    """random values with every third element from the coded rounding set"""
    x = torch.randn(n, generator=gen(c)) * scale
    cd = coded_fill(c["dt"], n)
    pick = (torch.arange(n) % 3 == 1) & torch.isfinite(cd)
    return torch.where(pick, cd, x)


def lens_setup(c, T):
    """(lens or None, the rows kept per clip)"""
    B, m = c["B"], c.get("len_mul", 1)
    if c["lens"] == "none":
        return None, [T] * B
    ln = gc.lens_of(B, T, max(m, 1))
    return ln, [max(0, min(n * m, T)) for n in ln]


def lens_spec(ln):
    return Spec(i32, 1, len(ln), data=torch.tensor(ln, dtype=i32))


def keep_rows(lim, T):
    return (torch.arange(T)[None, :] < torch.tensor(lim)[:, None]).reshape(-1)


def exact_judge(names):
    def judge(rep, c, got, ref):
        for n in names:
            rep.exact(c, n, got[n], ref[n])
    return judge


def with_lens(specs, ln):
    if ln is not None:
        specs["lens"] = lens_spec(ln)
    return specs


# ---- casts and row kernels -----------------------------------------------------------------------------------------------------------------------
def b_cast32(c):
    M, C, dt, t = c["M"], c["C"], c["dt"], t16(c["dt"])
    x = coded_fill("f32", M * C) if dt == "f32" else ((torch.arange(M * C) % 65536) - 32768).to(i16).view(t)
    x = x.view(M, C)
    specs = {"x": Spec(t, M, C, c["ldx"], data=x), "y": Spec(f32, M, C, c["ldy"], out=True)}
    return Kase(specs, lambda lib, p: lib.l2s_cast_16_to_f32(p["x"], c["ldx"], p["y"], c["ldy"], M, C, dtc(dt), stream()),
                lambda: {"y": x.to(f32)}, exact_judge(["y"]))


def b_cast16(c):
    M, C, dt, t = c["M"], c["C"], c["dt"], t16(c["dt"])
    x = coded_fill(dt, M * C).view(M, C)
    specs = {"x": Spec(f32, M, C, c["ldx"], data=x), "y": Spec(t, M, C, c["ldy"], out=True)}
    return Kase(specs, lambda lib, p: lib.l2s_cast_f32_to_16(p["x"], c["ldx"], p["y"], c["ldy"], M, C, dtc(dt), stream()),
                lambda: {"y": x.to(t)}, exact_judge(["y"]))


def b_repeat2(c):
    B, T, C, dt, t = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    x = mixed_f32(c, B * T * C).view(B * T, C)
    specs = {"x": Spec(f32, B * T, C, data=x), "y": Spec(t, 2 * B * T, C, out=True)}
    return Kase(specs, lambda lib, p: lib.l2s_repeat2_cast(p["x"], p["y"], B, T, C, dtc(dt), stream()),
                lambda: {"y": x.repeat_interleave(2, 0).to(t)}, exact_judge(["y"]))


def b_rows16(c):
    B, T, C, dt, t = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    ln, lim = lens_setup(c, T)
    x = mixed_f32(c, B * T * C).view(B * T, C)
    specs = with_lens({"x": Spec(f32, B * T, C, c["ldx"], data=x), "y": Spec(t, B * T, C, c["ldy"], c["col0"], out=True)}, ln)
    return Kase(specs, lambda lib, p: lib.l2s_rows_f32_to_16_masked(p["x"], c["ldx"], p["y"], c["ldy"], c["col0"], p.get("lens"), c["len_mul"], B, T, C,
                                                                    dtc(dt), stream()),
                lambda: {"y": torch.where(keep_rows(lim, T)[:, None], x, torch.zeros_like(x)).to(t)}, exact_judge(["y"]))


def b_bcast(c):
    B, T, C, dt, t = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    tv = f32 if c["v32"] else (t if dt != "f32" else torch.float16)
    ln, lim = lens_setup(c, T)
    v = mixed_f32(c, B * C).view(B, C).to(tv)
    specs = with_lens({"v": Spec(tv, B, C, c["ldv"], data=v), "y": Spec(t, B * T, C, c["ldy"], c["col0"], out=True)}, ln)

    def ref():
        rows = v.float()[:, None, :].expand(B, T, C).reshape(B * T, C)
        return {"y": torch.where(keep_rows(lim, T)[:, None], rows, torch.zeros_like(rows)).to(t)}
    return Kase(specs, lambda lib, p: lib.l2s_broadcast_rows(p["v"], c["ldv"], p["y"], c["ldy"], c["col0"], p.get("lens"), c["len_mul"], B, T, C,
                                                             int(c["v32"]), dtc(dt), stream()), ref, exact_judge(["y"]))


def b_transpose(c):
    B, T, C, dt, t = c["B"], c["T"], c["C"], c["dt"], t16(c["dt"])
    ln, lim = lens_setup(c, T)
    x = mixed_f32(c, B * C * T).view(B * C, T)
    specs = with_lens({"x": Spec(f32, B * C, T, data=x), "y": Spec(t, B * T, C, c["ldy"], c["col0"], out=True)}, ln)

    def ref():
        rows = x.view(B, C, T).transpose(1, 2).reshape(B * T, C)
        return {"y": torch.where(keep_rows(lim, T)[:, None], rows, torch.zeros_like(rows)).to(t)}
    return Kase(specs, lambda lib, p: lib.l2s_transpose_ct_to_tc(p["x"], p["y"], c["ldy"], c["col0"], p.get("lens"), c["len_mul"], B, C, T, dtc(dt),
                                                                 stream()), ref, exact_judge(["y"]))


# ---- look-ups and lens_from_mask -----------------------------------------------------------------------------------------------------------------
def table_of(c, n, C):
    return (torch.randn(n, C, generator=gen(c)) * 3).to(t16(c["dt"]))


def b_embedding(c):
    B, L, C, n, dt, t = c["B"], c["L"], c["C"], c["n"], c["dt"], t16(c["dt"])
    ln, lim = lens_setup(c, L)
    code = torch.randint(0, n, (B, L), generator=gen(c), dtype=i32)
    code.view(-1)[0], code.view(-1)[-1], code[B // 2, L // 2] = 0, n - 1, n - 1          # the table's first and last row; never out of range
    if B > 1:
        code[1, 0], code[1, 1] = n - 1, 0                 # clip 1 is never masked
    tab = table_of(c, n, C)
    specs = with_lens({"code": Spec(i32, B, L, data=code), "table": Spec(t, n, C, data=tab), "y": Spec(t, B * L, C, c["ldy"], out=True)}, ln)

    def ref():
        rows = tab[code.view(-1).long()]
        return {"y": torch.where(keep_rows(lim, L)[:, None], rows, torch.zeros_like(rows))}
    return Kase(specs, lambda lib, p: lib.l2s_embedding(p["code"], p["table"], p["y"], c["ldy"], p.get("lens"), B, L, C, dtc(dt), stream()),
                ref, exact_judge(["y"]))


def b_embtok(c):
    B, L, C, n, off, dt, t = c["B"], c["L"], c["C"], c["n"], c["off"], c["dt"], t16(c["dt"])
    ln, lim = lens_setup(c, L)
    ldt = c["ldt"]
    tok = torch.randint(off, off + n, (B, L), generator=gen(c), dtype=i32)
    if B > 1 and L > 3:                                   # clip 1 is never masked: both ends of the clamp inside the valid range
        tok[1, 0], tok[1, 1], tok[1, 2], tok[1, 3] = off - 1, off + n, off - 3, off + n + 1000
    tab = table_of(c, n, C)
    specs = with_lens({"tok": Spec(i32, B, min(L, ldt), ldt, data=tok[:, :min(L, ldt)]), "table": Spec(t, n, C, data=tab),
                       "y": Spec(t, B * L, C, c["ldy"], out=True)}, ln)

    def ref():
        rows = tab[(tok.view(-1).long() - off).clamp(0, n - 1)]
        return {"y": torch.where(keep_rows(lim, L)[:, None], rows, torch.zeros_like(rows))}
    return Kase(specs, lambda lib, p: lib.l2s_embedding_tokens(p["tok"], ldt, off, p["table"], n, p["y"], c["ldy"], p.get("lens"), c["len_mul"], B, L, C,
                                                               dtc(dt), stream()), ref, exact_judge(["y"]))


def lensmask_rows(B, T, g):
    """all padded, none padded, one pad at the last position, random, random with byte values other than 1"""
    m = torch.zeros(B, T, dtype=u8)
    m[0] = 1
    m[2, T - 1] = 1
    m[3] = (torch.rand(T, generator=g) < 0.4).to(u8)
    m[4] = (torch.rand(T, generator=g) < 0.5).to(u8) * torch.randint(1, 256, (T,), generator=g).to(u8)
    return m


def b_lensmask(c):
    B, T = c["B"], c["T"]
    m = lensmask_rows(B, T, gen(c))
    specs = {"lens": Spec(i32, 1, B, out=True)}
    if c["mask"]:
        specs["mask"] = Spec(u8, B, T, data=m)
    return Kase(specs, lambda lib, p: lib.l2s_lens_from_mask(p.get("mask"), p["lens"], B, T, stream()),
                lambda: {"lens": ((T - (m != 0).sum(1)) if c["mask"] else torch.full((B,), T)).to(i32).view(1, B)}, exact_judge(["lens"]))


# ---- split_hi_lo ---------------------------------------------------------------------------------------------------------------------------------
def split_data(c):
    """signed magnitudes log-uniform from 2^-20 to the type's range (f16: residues that are subnormal or underflow to zero come with it),
    with zeros and some values near one"""
    n = c["B"] * c["T"] * c["C"]
    g = gen(c)
    e = torch.rand(n, generator=g, dtype=f64) * (math.log2(MAX16[c["dt"] if c["dt"] in MAX16 else "f16"]) + 20.0) - 20.0
    x = (2.0 ** e) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    x = torch.where(torch.arange(n) % 4 == 3, torch.randn(n, generator=g, dtype=f64) * 2, x)       # where GELU bends
    x[::97] = 0.0
    return x.float().view(c["B"] * c["T"], c["C"])


def gelu64(x):
    x = x.to(f64)
    erf = torch.erf(x / math.sqrt(2.0))
    phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return 0.5 * x * (1.0 + erf), x.abs() * (0.5 * (1.0 + erf.abs()) + x.abs() * phi)


def split_y32(x, act):
    """the activation in fp32 as the kernel computes it (act 0 / 1: exact operations)"""
    if act == 1:
        return torch.where(x >= 0, x, x * torch.tensor(gc.SLOPE, dtype=f32))
    if act == 2:
        return 0.5 * x * (1.0 + torch.erf(x * torch.tensor(0.70710678118654752, dtype=f32)))
    return x


def b_split(c):
    B, T, C, act, dt = c["B"], c["T"], c["C"], c["act"], c["dt"]
    t = t16(dt) if dt != "f32" else torch.float16
    ln, lim = lens_setup(c, T)
    x = split_data(c)
    specs = with_lens({"x": Spec(f32, B * T, C, c["ldx"], data=x), "hi": Spec(t, B * T, C, c["ld16"], out=True),
                       "lo": Spec(t, B * T, C, c["ld16"], out=True)}, ln)
    keep = keep_rows(lim, T)[:, None]

    def ref():
        xm = torch.where(keep, x, torch.zeros_like(x))
        y = split_y32(xm, act)
        hi = y.to(t)
        r = {"y32": y, "hi": hi, "lo": (y - hi.float()).to(t), "keep": keep}
        if act == 2:
            r["gelu"], r["A"] = gelu64(xm)
        return r

    def judge(rep, c, got, ref):
        s = got["hi"].to(f64) + got["lo"].to(f64)
        z = ~ref["keep"].expand_as(got["hi"])
        if bits(got["hi"])[z].any() or bits(got["lo"])[z].any():
            rep.bad(c, "masked rows are not exactly +0")
        if act < 2:
            rep.exact(c, "hi", got["hi"], ref["hi"])
            rep.exact(c, "lo", got["lo"], ref["lo"])
            y = ref["y32"].to(f64)
            rep.bounded(c, "sum", s, y, U16[dt] ** 2 * y.abs() + MIN_SUB[dt])
        else:
            y = ref["gelu"]
            rep.bounded(c, "b", s, y, U16[dt] ** 2 * y.abs() + MIN_SUB[dt] + gc.F_of("split-gelu") * EPS24 * ref["A"])

    def cpuf32():
        if act != 2:
            return None
        r = ref()
        return {"split-gelu": ratio_b((r["y32"].to(f64) - r["gelu"]).abs(), EPS24 * r["A"])}
    return Kase(specs, lambda lib, p: lib.l2s_split_hi_lo(p["x"], c["ldx"], p["hi"], p["lo"], c["ld16"], act, gc.SLOPE, p.get("lens"), c["len_mul"], B, T, C,
                                                          dtc(dt), stream()), ref, judge, cpuf32)


# ---- splitk_reduce -------------------------------------------------------------------------------------------------------------------------------
def splitk_sum(x, P, S, N, descending=False):
    v = x.clone()
    for s in (range(S - 1, -1, -1) if descending else range(S)):
        v = v + P[:, s * N: (s + 1) * N]
    return v


def splitk_data(c):
    S, N, M, g = c["S"], c["N"], c["M"], gen(c)
    x, P = torch.randn(M, N, generator=g), torch.randn(M, S * N, generator=g)
    if c["data"] == "order":                              # every other slice 2^20 times larger: any other order of the additions changes bits
        for s in range(0, S, 2):
            P[:, s * N: (s + 1) * N] *= 2.0 ** 20
    return x, P


def b_splitk(c):
    S, N, M = c["S"], c["N"], c["M"]
    x, P = splitk_data(c)
    specs = {"P": Spec(f32, M, S * N, c["ldp"], data=P), "x": Spec(f32, M, N, c["ldx"], data=x, out=True)}      # in place on x
    return Kase(specs, lambda lib, p: lib.l2s_splitk_reduce(p["P"], c["ldp"], S, p["x"], c["ldx"], M, N, stream()),
                lambda: {"x": splitk_sum(x, P, S, N)}, exact_judge(["x"]))


# ---- conv_post_tanh ------------------------------------------------------------------------------------------------------------------------------
SAT_POS, SAT_NEG = (range(23, 57), range(243, 267)), (range(103, 137),)     # the saturated samples of a "saturated" case: acc = +-56


def convpost_data(c):
    B, T, C, k, g = c["B"], c["T"], c["C"], c["k"], gen(c)
    if c["data"] == "saturated":                          # runs of +1 and of -100 (leaky: -1) under weights of 0.5: acc = +-7 * 16 * 0.5
        x = torch.randn(B, T, C, generator=g) * 0.01
        x[:, 20:60], x[:, 240:270], x[:, 100:140] = 1.0, 1.0, -100.0
        return x, torch.full((k, C), 0.5), 0.0
    x = torch.randn(B, T, C, generator=g)
    w = torch.randn(k, C, generator=g) / math.sqrt(k * C) * 1.5
    return x, w, 0.125


def convpost_eval(c, x, w, bias, lim, ft):
    """(wav, A, acc) in ft: the inputs of frames at or past the clip's length are zero, as are its outputs"""
    B, T, C, k = c["B"], c["T"], c["C"], c["k"]
    half = (k - 1) // 2
    keep = keep_rows(lim, T).view(B, T, 1)
    xl = torch.where(x >= 0, x, x * torch.tensor(0.01, dtype=f32)).to(ft) * keep            # the slope product is one fp32 multiplication
    xp = torch.zeros(B, T + k - 1, C, dtype=ft)
    xp[:, half: half + T] = xl
    acc = torch.full((B, T), float(np.float32(bias)), dtype=ft)
    mag = torch.full((B, T), abs(float(np.float32(bias))), dtype=ft)
    wf = w.to(ft)
    for tap in range(k):
        acc = acc + (xp[:, tap: tap + T] * wf[tap]).sum(2)
        mag = mag + (xp[:, tap: tap + T].abs() * wf[tap].abs()).sum(2)
    o = torch.tanh(acc)
    A = mag * (1.0 - o * o) + o.abs()
    o = o * keep.view(B, T)
    return o, A, acc


def b_convpost(c):
    B, T, C, k = c["B"], c["T"], c["C"], c["k"]
    ln, lim = lens_setup(c, T)
    x, w, bias = convpost_data(c)
    specs = with_lens({"x": Spec(f32, B * T, C, data=x, off=c["xoff"]), "w": Spec(f32, k, C, data=w), "wav": Spec(f32, B, T, out=True)}, ln)
    if c["pcm"]:
        specs["pcm"] = Spec(i16, B, T, out=True)

    def call(lib, p):
        if c["expect"] == 0 and (C, k) == (16, 7):
            assert bool(p["x"] & 15) == bool(c["xoff"]), "the aligned case is aligned, the offset case is not"
        return lib.l2s_conv_post_tanh(p["x"], p["w"], bias, p["wav"], p.get("pcm"), p.get("lens"), c["len_mul"], B, T, C, k, stream())

    def ref():
        o, A, acc = convpost_eval(c, x, w, bias, lim, f64)
        return {"wav": o, "A": A, "acc": acc}

    def judge(rep, c, got, ref):
        wav = got["wav"]
        rep.bounded(c, "a", wav, ref["wav"], gc.TOL_ABS["convpost"])
        rep.bounded(c, "b", wav, ref["wav"], gc.F_of("convpost") * EPS24 * ref["A"])
        z = ~keep_rows(lim, T).view(B, T)
        if bits(wav)[z].any() or (c["pcm"] and got["pcm"][z].any()):
            rep.bad(c, "frames past the clip's length are not exactly zero")
        if c["pcm"]:
            rep.exact(c, "pcm", got["pcm"], (wav * 32768.0).to(i32).to(i16))       # truncation toward zero through int32, wrapped
        if c["data"] == "saturated":
            for sign, sets in ((1.0, SAT_POS), (-1.0, SAT_NEG)):
                idx = torch.tensor([t for r in sets for t in r])
                if not (ref["acc"][:, idx] * sign > 20.0).all():
                    rep.bad(c, "the reference is not saturated where the case says")
                if not (wav[:, idx] == sign).all():
                    rep.bad(c, f"saturated samples: wav is not exactly {sign}")
                if not (got["pcm"][:, idx] == -32768).all():
                    rep.bad(c, f"saturated samples of sign {sign}: pcm is not -32768")
        DIGESTS[("convpost", c["name"].replace("-offset", ""))] = DIGESTS.get(("convpost", c["name"].replace("-offset", "")), []) + \
            [(bits(wav).clone(), got["pcm"].clone() if c["pcm"] else None)]

    def cpuf32():
        r = ref()
        o = convpost_eval(c, x, w, bias, lim, f32)[0]
        return {"convpost": ratio_b((o.to(f64) - r["wav"]).abs(), EPS24 * r["A"])}
    return Kase(specs, call, ref, judge, cpuf32)


DIGESTS = {}


def convpost_twins(rep, cases):
    """the aligned (conv_post16_kernel) and the offset (conv_post_kernel) run of every (16, 7) case give identical bytes"""
    by = {c["name"]: c for c in cases if c["op"] == "convpost"}
    for (op, name), runs in DIGESTS.items():
        if op != "convpost" or "C16-k7" not in name:
            continue
        c = by[name]
        if len(runs) != 2:
            rep.bad(c, f"{len(runs)} of the two runs (aligned, offset) were judged")
        elif not torch.equal(runs[0][0], runs[1][0]) or (runs[0][1] is not None and not torch.equal(runs[0][1], runs[1][1])):
            rep.bad(c, "conv_post16_kernel and conv_post_kernel differ on the same data")


# ---- decoders ------------------------------------------------------------------------------------------------------------------------------------
def greedy_data(c):
    B, T2, V, g = c["B"], c["T2"], c["V"], gen(c)
    x = torch.randn(B, T2, V, generator=g) * 2.5
    for b in range(B):
        for t in range(T2):
            u = x[b, t, 4:]
            if V - 4 >= 2 and (t + b) % 5 == 0:           # an exact tie at the top between two unit ids
                i, j = torch.randperm(V - 4, generator=g)[:2].tolist()
                u[i] = u[j] = float(u.max()) + 1.5
            if V - 4 >= 5 and (t + b) % 4 == 2:           # -inf on losing unit ids
                top = int(u.argmax())
                for d in (1, 2, 3):
                    u[(top + d) % (V - 4)] = -math.inf
            if (t + b) % 3 == 1:                          # a special symbol far above every unit
                x[b, t, (t + b) % 4] = 40.0
    return x


def b_greedy(c):
    B, T2, V, ldl, temp, lenpen = c["B"], c["T2"], c["V"], c["ldl"], c["temp"], c["lenpen"]
    ln, len_mul, Ls = gc.greedy_lens(c["lens"], B, T2)
    x = greedy_data(c)
    cols = min(V, ldl)
    specs = with_lens({"logits": Spec(f32, B * T2, cols, ldl, data=x[:, :, :cols]), "tokens": Spec(i32, B, T2 + 1, out=True),
                       "lprobs": Spec(f32, B, T2 + 1, out=True), "score": Spec(f32, 1, B, out=True)}, ln)

    def ref():
        tok, lp, A = torch.full((B, T2 + 1), dr.PAD, dtype=i32), torch.zeros(B, T2 + 1, dtype=f64), torch.zeros(B, T2 + 1, dtype=f64)
        sc, As = torch.zeros(1, B, dtype=f64), torch.zeros(1, B, dtype=f64)
        for b in range(B):
            L = Ls[b]
            t_, l_, a_, sc[0, b], As[0, b] = dr.greedy(x[b], L, temp, lenpen)
            tok[b, : L + 1], lp[b, : L + 1], A[b, : L + 1] = t_.to(i32), l_, a_
        return {"tokens": tok, "lprobs": lp, "A": A, "score": sc, "As": As}

    def judge(rep, c, got, ref):
        rep.exact(c, "tokens", got["tokens"], ref["tokens"])
        behind = torch.arange(T2 + 1)[None, :] >= torch.tensor(Ls)[:, None]
        if bits(got["lprobs"])[behind].any():
            rep.bad(c, "lprobs at and behind EOS are not exactly zero")
        rep.bounded(c, "a", got["lprobs"], ref["lprobs"], gc.TOL_ABS["greedy"])
        rep.bounded(c, "b", got["lprobs"], ref["lprobs"], gc.F_of("greedy-lprob") * EPS24 * ref["A"])
        rep.bounded(c, "a-score", got["score"], ref["score"], gc.TOL_ABS["greedy"])
        rep.bounded(c, "b-score", got["score"], ref["score"], gc.F_of("greedy-score") * EPS24 * ref["As"])

    def cpuf32():
        from oracle import decode as od
        r = ref()
        hyp = od.greedy_decode(x.transpose(0, 1), Ls, temp, lenpen)
        out = {"greedy-lprob": 0.0, "greedy-score": 0.0}
        for b in range(B):
            L = Ls[b]
            for t in (hyp[b]["tokens"].to(i32) != r["tokens"][b, : L + 1]).nonzero().view(-1).tolist():      # two units whose fp32 lprobs coincide
                assert abs(float(x[b, t, hyp[b]["tokens"][t]] - x[b, t, r["tokens"][b, t]])) < 1e-5 * temp, (c["name"], b, t)
            out["greedy-lprob"] = max(out["greedy-lprob"], ratio_b((hyp[b]["positional_scores"].to(f64) - r["lprobs"][b, : L + 1]).abs(),
                                                                   EPS24 * r["A"][b, : L + 1]))
            out["greedy-score"] = max(out["greedy-score"], ratio_b((hyp[b]["score"].to(f64) - r["score"][0, b]).abs().reshape(1),
                                                                   EPS24 * r["As"][0, b].reshape(1)))
        return out
    return Kase(specs, lambda lib, p: lib.l2s_greedy_decode(p["logits"], ldl, p.get("lens"), len_mul, B, T2, V, temp, lenpen, p["tokens"], p["lprobs"],
                                                            p["score"], stream()), ref, judge, cpuf32)


def coded_steps(L):
    n = gc.n_coded(L)
    return [(i * L) // n for i in range(n)]


def beam_data(c):
    """logits [B, T2, V] and, for coded clips, (best [T2], runner-up per coded step) per clip"""
    B, T2, V, g = c["B"], c["T2"], c["V"], gen(c)
    if c["data"] == "random":
        return torch.randn(B, T2, V, generator=g) * 2.5, None
    x = -12.0 + 8.0 * torch.rand(B, T2, V, generator=g)                     # losers, uniform in [-12, -4]
    x[:, :, :4] = -12.0 + 17.0 * torch.rand(B, T2, 4, generator=g)          # specials, some above every unit
    code = []
    for b in range(B):
        best = torch.randint(4, V, (T2,), generator=g)
        x[b, torch.arange(T2), best] = 0.0
        steps = coded_steps(c["Ls"][b]) if V - 4 >= 2 else []
        runner = []
        for i, s in enumerate(steps):
            r = 4 + (int(best[s]) - 4 + 1 + int(torch.randint(0, V - 5, (1,), generator=g))) % (V - 4)
            x[b, s, r] = -gc.DELTA * 2.0 ** i
            runner.append(r)
        code.append((best, steps, runner))
    return x, code


def coded_hypothesis(code_b, L, h):
    """hypothesis h flips the coded steps in the binary expansion of h"""
    best, steps, runner = code_b
    tok = best[:L].clone()
    for i, s in enumerate(steps):
        if (h >> i) & 1:
            tok[s] = runner[i]
    return tok


def coded_ranks(c, b):
    L = c["Ls"][b]
    return 2 ** (gc.n_coded(L) if c["V"] - 4 >= 2 else 0)


def beam_lens(c):
    Ls, T2, m = c["Ls"], c["T2"], c["len_mul"]
    if c["lens"] == "none":
        assert all(L == T2 for L in Ls)
        return None
    assert all(L % m == 0 for L in Ls)
    return [L // m + (5 if c["lens"] == "clamp" and L == T2 else 0) for L in Ls]


def beam_reference(c, x, b):
    """(tokens [n', L + 1], scores [n']) of the beam + 1 best hypotheses of clip b in fp64"""
    return dr.nbest(x[b], c["Ls"][b], c["temp"], c["lenpen"], c["beam"] + 1)


def separated(scores, h, G_):
    lo = h == 0 or float(scores[h - 1] - scores[h]) > G_
    hi = h + 1 >= scores.numel() or float(scores[h] - scores[h + 1]) > G_
    return lo and hi


def b_beam(c):
    B, T2, V, ldl, temp, lenpen, beam, Ls = c["B"], c["T2"], c["V"], c["ldl"], c["temp"], c["lenpen"], c["beam"], c["Ls"]
    x, code = beam_data(c)
    ln = beam_lens(c)
    nws = B * (T2 + 1) * beam * 8
    rows = B * beam
    specs = with_lens({"logits": Spec(f32, B * T2, V, ldl, data=x), "ws": Spec(i32, 1, nws // 4 + 1, out=True),
                       "tokens": Spec(i32, rows, T2 + 1, out=True), "pos": Spec(f32, rows, T2 + 1, out=True), "score": Spec(f32, 1, rows, out=True),
                       "nhyp": Spec(i32, 1, B, out=True), "gtok": Spec(i32, B, T2 + 1, out=True), "glp": Spec(f32, B, T2 + 1, out=True),
                       "gsc": Spec(f32, 1, B, out=True)}, ln)

    def call(lib, p):
        if c["expect"] == 0:
            assert lib.l2s_beam_decode_workspace(B, T2, beam) == nws
        rc = lib.l2s_beam_decode(p["logits"], ldl, p.get("lens"), c["len_mul"], B, T2, V, temp, lenpen, beam, p["ws"] + c.get("ws_off", 0),
                                 nws - c.get("ws_short", 0), p["tokens"], p["pos"], p["score"], p["nhyp"], stream())
        if rc == 0:
            rc = lib.l2s_greedy_decode(p["logits"], ldl, p.get("lens"), c["len_mul"], B, T2, V, temp, lenpen, p["gtok"], p["glp"], p["gsc"], stream())
        return rc

    def ref():
        return [beam_reference(c, x, b) for b in range(B)]

    def judge(rep, c, got, ref):
        tok, pos = got["tokens"].view(B, beam, T2 + 1), got["pos"].view(B, beam, T2 + 1)
        sc, nh = got["score"].view(B, beam), got["nhyp"].view(B)
        G_ = gc.BEAM_G.get(c["name"], 0.0)
        skipped = total = 0
        for b in range(B):
            L = Ls[b]
            n = beam if L > 0 else 1
            if int(nh[b]) != n:
                rep.bad(c, f"clip {b}: nhyp {int(nh[b])}, expected {n}")
                continue
            if (tok[b, n:] != dr.PAD).any() or bits(pos[b, n:]).any() or not (sc[b, n:] == -math.inf).all():
                rep.bad(c, f"clip {b}: the rows past nhyp are not pad / 0 / -inf")
            if (tok[b, :n, L] != dr.EOS).any() or (tok[b, :n, L + 1:] != dr.PAD).any() or bits(pos[b, :n, L:]).any():
                rep.bad(c, f"clip {b}: EOS, the pad behind it or the zero scores from it on")
            units = tok[b, :n, :L]
            if ((units < 4) | (units >= V)).any():
                rep.bad(c, f"clip {b}: a token outside the unit ids")
                continue
            if len({tuple(r.tolist()) for r in units}) != n:
                rep.bad(c, f"clip {b}: the hypotheses are not distinct")
            if (sc[b, 1:n] > sc[b, : n - 1]).any():
                rep.bad(c, f"clip {b}: the scores increase somewhere")
            if not torch.equal(tok[b, 0], got["gtok"][b]):
                rep.bad(c, f"clip {b}: hypothesis 0 differs from l2s_greedy_decode")
            rtok, rsc = ref[b]
            for h in range(n):
                total += 1
                if c["data"] == "coded":
                    want = coded_hypothesis(code[b], L, h) if h < coded_ranks(c, b) else None
                    if want is None or not torch.equal(rtok[h, :L], want):
                        rep.bad(c, f"clip {b} rank {h}: the reference is not the binary-expansion order")
                elif h >= rtok.shape[0] or not separated(rsc, h, G_):
                    skipped += 1
                    continue
                if not torch.equal(units[h].long(), rtok[h, :L]):
                    rep.bad(c, f"clip {b} rank {h}: tokens differ from the exact n-best")
            if L > 0:
                lp, _, A = dr.step_lprobs(x[b, :L], temp)
                P, AP, S, AS = zip(*[dr.score_of(lp, A, lenpen, units[h].long()) for h in range(n)])
                P, AP = torch.stack(P), torch.stack(AP)
                S, AS = torch.tensor(S, dtype=f64), torch.tensor(AS, dtype=f64)
                rep.bounded(c, "a", pos[b, :n, : L + 1], P, gc.TOL_ABS["beam"])
                rep.bounded(c, "b", pos[b, :n, : L + 1], P, gc.F_of("beam-pos") * EPS24 * AP)
                rep.bounded(c, "a-score", sc[b, :n], S, gc.TOL_ABS["beam"])
                rep.bounded(c, "b-score", sc[b, :n], S, gc.F_of("beam-score") * EPS24 * AS)
            elif bits(sc[b, :1]).any():
                rep.bad(c, f"clip {b}: the empty clip's score is not 0")
        if total and skipped / total > gc.SKIP_CAP:
            rep.bad(c, f"{skipped} of {total} ranks skipped")
        rep.ratio(c, "skipped", skipped / max(total, 1))
    return Kase(specs, call, ref, judge, lambda: beam_cpu(c, x, code))


def beam_cpu(c, x, code, want_oracle=True):
    """Host side of a beam case: the fp64 restatement (and oracle/decode.py in fp32) against the coded order; the oracle's deviation from the
    restatement in units of 2^-24 A; the share of ranks the stored G would skip and the G measured now."""
    from oracle import decode as od
    out = {"beam-pos": 0.0, "beam-score": 0.0, "dev": 0.0, "skipped": 0, "total": 0, "min-gap": math.inf, "order-ok": True}
    G_ = gc.BEAM_G.get(c["name"], 0.0)
    for b, L in enumerate(c["Ls"]):
        rtok, rsc = beam_reference(c, x, b)
        n = c["beam"] if L > 0 else 1
        hyps = od.beam_search_decode(x[b, :max(L, 1)].unsqueeze(1), [L], c["beam"], c["temp"], c["lenpen"])[0] if want_oracle else None
        if L > 0:
            lp, _, A = dr.step_lprobs(x[b, :L], c["temp"])
        for h in range(n):
            out["total"] += 1
            if c["data"] == "coded":
                want = coded_hypothesis(code[b], L, h) if h < coded_ranks(c, b) else None
                ok = want is not None and torch.equal(rtok[h, :L], want) and (hyps is None or torch.equal(hyps[h]["tokens"][:L], want))
                out["order-ok"] = out["order-ok"] and ok
                if h:
                    out["min-gap"] = min(out["min-gap"], float(rsc[h - 1] - rsc[h]) * float(L + 1) ** c["lenpen"])
            elif h >= rtok.shape[0] or not separated(rsc, h, G_):
                out["skipped"] += 1
            if hyps is not None and L > 0:
                P, AP, S, AS = dr.score_of(lp, A, c["lenpen"], hyps[h]["tokens"][:L])
                out["beam-pos"] = max(out["beam-pos"], ratio_b((hyps[h]["positional_scores"].to(f64) - P).abs(), EPS24 * AP))
                out["beam-score"] = max(out["beam-score"], abs(float(hyps[h]["score"]) - S) / (EPS24 * AS))
                out["dev"] = max(out["dev"], abs(float(hyps[h]["score"]) - float(rsc[h])) if h < rsc.numel() else 0.0)
    return out


def ctc_data(c):
    """Every frame: min(V, 64) classes on a ladder from 0 down to -60 (p stays normal in fp32 down to the last), the others below it, at
    shuffled class ids; frame 0 of clip 1 has an exact tie at the top."""
    B, L, V, g = c["B"], c["L"], c["V"], gen(c)
    x = -70.0 + 8.0 * torch.rand(B * L, V, generator=g)
    n = min(V, 64)
    for r in range(B * L):
        ids = torch.randperm(V, generator=g)[:n]
        x[r, ids] = -60.0 * torch.arange(n) / max(n - 1, 1) - (0.3 * torch.rand(n, generator=g) if n > 2 else 0.0)
        if r == L and n >= 2:                             # (clip 1 is never masked)
            x[r, ids[1]] = x[r, ids[0]]
    return x


def b_ctcframes(c):
    B, L, V, K_, ldl = c["B"], c["L"], c["V"], c["K"], c["ldl"]
    ln, lim = lens_setup(c, L)
    x = ctc_data(c)
    cols = min(V, ldl)
    specs = with_lens({"logits": Spec(f32, B * L, cols, ldl, data=x[:, :cols]), "labels": Spec(i32, B, L, out=True)}, ln)
    if K_ > 0:
        specs["cls"], specs["lp"] = Spec(i32, B * L, K_, out=True), Spec(f32, B * L, K_, out=True)
    keep = keep_rows(lim, L)

    def soft(ft):
        xx = x.to(ft)
        mx = xx.max(1, keepdim=True).values
        e = (xx - mx).exp()
        se = e.sum(1, keepdim=True)
        p = e / se
        ps, ids = torch.sort(p, dim=1, descending=True, stable=True)          # ties: the smaller class id first
        return ps, ids, (xx - mx).abs().gather(1, ids) + se.log().abs() + 1.0

    def ref():
        ps, ids, A = soft(f64)
        r = {"labels": torch.where(keep, ids[:, 0], torch.zeros_like(ids[:, 0])).to(i32).view(B, L)}
        if K_ > 0:
            r["cls"] = torch.where(keep[:, None], ids[:, :K_], torch.zeros_like(ids[:, :K_])).to(i32)
            r["lp"] = torch.where(keep[:, None], (ps[:, :K_] + FLT_MIN).log(), torch.full_like(ps[:, :K_], -FLT_MAX))
            r["A"] = torch.where(keep[:, None], A[:, :K_], torch.zeros_like(A[:, :K_]))           # a padded frame: -FLT_MAX exactly
        return r

    def judge(rep, c, got, ref):
        rep.exact(c, "labels", got["labels"], ref["labels"])
        if K_ > 0:
            rep.exact(c, "cls", got["cls"], ref["cls"])
            rep.bounded(c, "b", got["lp"], ref["lp"], gc.F_of("ctc-lp") * EPS24 * ref["A"])

    def cpuf32():
        if K_ == 0:
            return None
        r = ref()
        ps, ids, _ = soft(f32)
        assert torch.equal(ids[keep][:, :K_].to(i32), r["cls"][keep])
        lp = (ps[:, :K_] + torch.tensor(FLT_MIN, dtype=f32)).log().to(f64)
        return {"ctc-lp": ratio_b((lp - r["lp"]).abs()[keep], EPS24 * r["A"][keep])}
    return Kase(specs, lambda lib, p: lib.l2s_ctc_frames(p["logits"], ldl, p.get("lens"), c["len_mul"], B, L, V, K_, p["labels"], p.get("cls"), p.get("lp"),
                                                         stream()), ref, judge, cpuf32)


def ctcrepeat_rows(B, L, g):
    """one label at t = 0 carried across every 64-frame round; all zero; zero-free; sparse; sparse; one label at t = 63 only"""
    x = torch.zeros(B, L, dtype=i32)
    x[0, 0] = 7
    x[2] = torch.randint(1, 30, (L,), generator=g, dtype=i32)
    for b in (3, 4):
        x[b] = torch.randint(1, 30, (L,), generator=g, dtype=i32) * (torch.rand(L, generator=g) < 0.05 * b - 0.1).to(i32)
    if L > 63:
        x[5, 63] = 9
    return x


def b_ctcrepeat(c):
    B, L, ldx, ldy = c["B"], c["L"], c["ldx"], c["ldy"]
    ln, lim = lens_setup(c, L)
    x = ctcrepeat_rows(B, L, gen(c))
    if c["inplace"]:
        specs = with_lens({"x": Spec(i32, B, L, ldx, data=x, out=True)}, ln)
    else:
        specs = with_lens({"x": Spec(i32, B, L, ldx, data=x), "y": Spec(i32, B, L, ldy, out=True)}, ln)
    yn = "x" if c["inplace"] else "y"

    def ref():
        y = torch.zeros(B, L, dtype=i32)
        for b in range(B):
            if lim[b]:
                y[b, : lim[b]] = torch.tensor(dr.repeat_labels(x[b, : lim[b]].tolist()), dtype=i32)
        return {yn: y}
    return Kase(specs, lambda lib, p: lib.l2s_ctc_repeat_labels(p["x"], ldx, p.get("lens"), c["len_mul"], B, L, p[yn], ldy, stream()), ref,
                exact_judge([yn]))


BUILD = {"cast32": b_cast32, "cast16": b_cast16, "repeat2": b_repeat2, "rows16": b_rows16, "bcast": b_bcast, "transpose": b_transpose,
         "embedding": b_embedding, "embtok": b_embtok, "lensmask": b_lensmask, "split": b_split, "splitk": b_splitk, "convpost": b_convpost,
         "greedy": b_greedy, "beam": b_beam, "ctcframes": b_ctcframes, "ctcrepeat": b_ctcrepeat}


# ---- host-only modes --------------------------------------------------------------------------------------------------------------------------
def cpu_ref(parts):
    """every reference of every case that launches; the time of each part and its slowest case"""
    for part in parts or gc.PARTS:
        t0, slow = time.time(), (0.0, "")
        for c in gc.cases_of(part):
            if c["expect"] != 0:
                continue
            t1 = time.time()
            BUILD[c["op"]](c).ref()
            slow = max(slow, (time.time() - t1, c["name"]))
        print(f"CPUREF {part}: {time.time() - t0:.1f} s, slowest case {slow[1]} {slow[0]:.2f} s")


def cpu_f32():
    worst, beams = {}, {}
    for part, c in gc.all_cases():
        if c["expect"] != 0:
            continue
        k = BUILD[c["op"]](c)
        r = k.cpuf32() if k.cpuf32 else None
        if not r:
            continue
        if c["op"] == "beam":
            beams[c["name"]] = r
        for kind, q in r.items():
            if kind in gc.CPU_F32_WORST and q > worst.get(kind, (-1.0, ""))[0]:
                worst[kind] = (q, f"{c['dt']} {c['name']}")
    for kind, (q, name) in sorted(worst.items()):
        print(f"CPUF32 {kind:14s} worst |fp32 - fp64| / (2^-24 A) = {q:10.3f}  ({name})")
    print("CPU_F32_WORST = {" + ", ".join(f"{k!r}: {q:.3f}" for k, (q, _) in sorted(worst.items())) + "}")
    for name, r in beams.items():
        extra = f"min gap {r['min-gap']:.3e} order {'ok' if r['order-ok'] else 'WRONG'}" if "coded" in name else \
            f"skipped {r['skipped']} of {r['total']} at the stored G"
        print(f"BEAM {name}: oracle deviation {r['dev']:.3e}  G = 16 x = {16 * r['dev']:.3e}  {extra}")
    print("BEAM_G = {" + ", ".join(f"{n!r}: {16 * r['dev']:.3e}" for n, r in beams.items() if "random" in n) + "}")


def main():
    args = sys.argv[1:]
    usage = f"usage: check_glue_kernels.py <{' | '.join(gc.PARTS)}>  or  check_glue_kernels.py --cpu-ref [part ...] | --cpu-f32"
    if not args or args[0] in ("-h", "--help"):
        sys.exit(usage)
    if args[0] == "--cpu-f32":
        cpu_f32()
        return
    if args[0] == "--cpu-ref":
        if any(p not in gc.PARTS for p in args[1:]):
            sys.exit(usage)
        cpu_ref(args[1:])
        return
    part = args[0]
    if len(args) != 1 or part not in gc.PARTS:
        sys.exit(usage)
    lib = _lib.load()
    rep = Report(part)
    t0 = time.time()
    cases = gc.cases_of(part)
    count, spent = {}, {}
    for case in cases:
        t1 = time.time()
        run_case(case, lib, rep)
        count[case["inst"]] = count.get(case["inst"], 0) + 1
        spent[case["op"]] = spent.get(case["op"], 0.0) + time.time() - t1
    convpost_twins(rep, cases)
    print(f"part {part}: {len(cases)} cases, {len(rep.fail)} failures, {time.time() - t0:.1f} s  (" + ", ".join(f"{op} {s:.1f} s" for op, s in spent.items()) + ")")
    for inst in sorted(count, key=repr):
        cells = " ".join(f"({crit}) {r:6.3f}" for (i, crit), r in sorted(rep.worst.items(), key=repr) if i == inst)
        print(f"RATIO {part} {inst[0]} {inst[1]} {inst[2]} cases {count[inst]} {cells}")
    for line in rep.fail:
        print(line)
    sys.exit(1 if rep.fail else 0)


if __name__ == "__main__":
    main()
