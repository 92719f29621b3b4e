#!/usr/bin/env python3
"""Runs one part of the autoregressive decoding kernels' matrix (tests/_step_cases.py) on the device,

    check_step_kernels.py <part>              part: a key of sc.PARTS; one child process per part (tests/test_step_matrix_gpu.py)
    check_step_kernels.py --cpu-ref [part ..] no device: every reference and every condition on the inputs (decisive gaps, bit-exact
                                              ties, cache rows that are never read), with the time each part takes

Every operand is a window of a larger device buffer: sc.GUARD guard rows (16 elements for the one-dimensional ones) in front of and behind
it and the padding columns of its leading dimension, filled with a canary (NaN for fp32, 0x5A5A5A5A for int32, 0x5A5A for int16 and the
16-bit float types, 0x5A for bytes).  Cache rows that must not be read hold NaN.  Every launch runs twice into fresh buffers.  Checks, every
case: the code the case expects; every byte outside an output's window unchanged (workspaces and guards included); every input unchanged; a
refused launch writes nothing; the two runs give the same bytes; every clip of a multi-clip case, launched alone, gives the bytes of its
rows in the batch.  Then
  exact     caches, tokens, ancestors, counts, flags, hypotheses, x_next of both advance kernels, argmax ids and selected candidates (the
            case first shows on the fp64 reference that every deciding gap exceeds sc.DECISIVE x the value bound or that the tie is
            bit-exact by construction: no case is left out), zero rows of dead slots, every element a launch must leave alone;
  attention |gpu - f64| <= sc.ATTN_F max |round16(ref) - ref| over the case;
  logits    4 x the larger error of two fp32 CPU evaluations (BLAS; products ascending in k, 32 at a time), never below one fp32 ulp at the
            values' scale; the log-probability the same against its fp32 evaluation;
  select    sr.select_tol(V, s), the bound tests/test_lipread_kernels_gpu.py derives;
  ctc       labels and lengths of the n best exactly, scores to sc.CTC_TOL max(1, |score|) (tests/test_text_gpu.py), a beam that does not
            exist with length 0 and score FLT_MAX exactly; the case first shows that in every frame the survivors and the first
            candidate dropped lie more than sc.DECISIVE x that tolerance apart, are both the literal -FLT_MAX, or (kind ties) are the
            same fp32 sum of the same two numbers.  The size queries (l2s_ctc_beam_workspace, l2s_vocab_argmax_workspace,
            l2s_beam_select_workspace) are compared with their restatement at every launch, refused sizes included.
Prints one MEASURE line per kind with the worst err / bound and its case; exits non-zero on the first failing case, after its name and the
offending index."""
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lip2speech_unit_amd import _lib  # noqa: E402
from tests import _step_cases as sc  # noqa: E402
from tests import _step_reference as sr  # noqa: E402

f32, i32, i16, u8 = torch.float32, torch.int32, torch.int16, torch.uint8
T16 = {"f16": torch.float16, "bf16": torch.bfloat16}
G = sc.GUARD
NAN = float("nan")
TEMPERATURE = 1.25
SPACING = 0.2
UNK_PENALTY = 2 * SPACING + SPACING / 130.0          # tests/test_lipread_kernels_gpu.py


class Fail(Exception):
    pass


def dtc(dt):
    return {"f16": _lib.F16, "bf16": _lib.BF16}[dt]


def bits(x):
    return x.contiguous().view({1: u8, 2: i16, 4: i32, 8: torch.int64}[x.element_size()])


def seed_of(*key):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(repr(key))) % (2 ** 31)


def rng_of(c, *key):
    name = c["name"].split("/", 1)[1]
    for dt in sc.DTS:                                   # the two types of a case get the same data
        name = name.replace("-" + dt, "")
    return np.random.default_rng(seed_of(name, c.get("seed", 0), *key))


def stream():
    return torch.cuda.current_stream().cuda_stream


def canary(n, td):
    if td == f32:
        return torch.full((n,), NAN, dtype=td)
    size = torch.empty(0, dtype=td).element_size()
    return torch.full((n,), {1: 0x5A, 2: sc.CANARY16, 4: sc.CANARY32}[size], dtype={1: u8, 2: i16, 4: i32}[size]).view(td)


class Buf:
    """A [rows, cols] window of rows of `ld` elements with `guard` elements (default: sc.GUARD rows) on either side.  data: the window's
    content (None: canary).  out: the launch may write inside the window.  null: the launch gets NULL; off: bytes added to the pointer."""

    def __init__(self, td, rows, cols, ld=None, data=None, out=False, guard=None, null=False, off=0):
        self.td, self.rows, self.cols, self.out, self.null, self.off = td, rows, cols, out, null, off
        self.ld = max(ld if ld is not None else cols, cols)
        self.guard = G * self.ld if guard is None else guard
        if data is not None:
            data = torch.as_tensor(np.ascontiguousarray(data) if isinstance(data, np.ndarray) else data).reshape(rows, cols).to(td)
        self.data = data

    def numel(self):
        return 2 * self.guard + self.rows * self.ld + 8

    def build(self):
        h = canary(self.numel(), self.td)
        if self.data is not None:
            self.window(h).copy_(self.data)
        return h

    def window(self, flat):
        return flat[self.guard: self.guard + self.rows * self.ld].view(self.rows, self.ld)[:, : self.cols]

    def mask(self):
        m = torch.zeros(self.numel(), dtype=torch.bool)
        self.window(m).fill_(True)
        return m

    def ptr(self, dev):
        return None if self.null else dev.data_ptr() + self.guard * dev.element_size() + self.off


def vec(td, data, **kw):
    data = np.asarray(data)
    return Buf(td, 1, data.size, data=data.reshape(1, -1), guard=16, **kw)


class Report:
    def __init__(self, part):
        self.part, self.worst, self.count = part, {}, {}

    def bad(self, case, why):
        raise Fail(f"FAIL part={self.part} case={case['name']}: {why}")

    def measure(self, case, kind, r, where=""):
        self.count[kind] = self.count.get(kind, 0) + 1
        if r >= self.worst.get(kind, (-1.0, ""))[0]:
            self.worst[kind] = (r, case["name"])
        if not r <= 1.0:
            self.bad(case, f"({kind}) err / bound = {r:.3f} {where}")

    def same(self, case, what, a, b):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        if a.shape != b.shape or a.dtype != b.dtype:
            self.bad(case, f"{what}: shape / type {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}")
        ne = bits(a) != bits(b)
        if ne.any():
            i = ne.reshape(-1).nonzero()[0].item()
            self.bad(case, f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at flat index {i} ({a.reshape(-1)[i].item()!r} against "
                           f"{b.reshape(-1)[i].item()!r})")

    def values(self, case, kind, got, ref, bound, what=""):
        """|got - ref| <= bound (an array or a number); where the bound is 0 the value must be the reference's, exactly"""
        got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
        if got.shape != ref.shape:
            self.bad(case, f"({kind}) {what}: shape {got.shape}, reference {ref.shape}")
        if got.size == 0:
            return
        if np.isnan(got).any():
            self.bad(case, f"({kind}) {what}: {int(np.isnan(got).sum())} NaN in the window, first at flat index {int(np.isnan(got).reshape(-1).argmax())}")
        bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
        err = np.abs(got - ref)
        err = np.where(got == ref, 0.0, err)              # -inf against -inf
        tight = bound <= 0
        if (err[tight] != 0).any():
            self.bad(case, f"({kind}) {what}: a value with bound 0 differs, flat index {int(((err != 0) & tight).reshape(-1).argmax())}")
        q = np.where(tight, 0.0, err / np.where(tight, 1.0, bound))
        i = int(q.reshape(-1).argmax())
        self.measure(case, kind, float(q.reshape(-1)[i]), f"{what} at flat index {i} (got {got.reshape(-1)[i]:.9g}, ref {ref.reshape(-1)[i]:.9g}, "
                                                         f"bound {bound.reshape(-1)[i]:.3e})")


def t16(a, dt):
    """float64 values of the type -> the type; every NaN gets one bit pattern (a conversion may pick its own, and rows are compared as bytes)"""
    t = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(T16[dt]).contiguous()
    t.view(i16)[t.isnan()] = {"f16": 0x7E00, "bf16": 0x7FC0}[dt]
    return t


class Kase:
    multi = True                                         # clips are independent: each is also launched alone

    def __init__(self, c):
        self.c = c
        self.B = c["B"]

    def arg(self, key, default):
        return self.c.get(key + "_arg", default)

    def flags(self, name):
        c = self.c
        return dict(null=c.get("null") == name, off=c.get("off", {}).get(name, 0))

    def attn_check(self, rep, got, ref, what):
        c = self.c
        eps = float(np.abs(sr.round16(ref, c["dt"]) - ref).max())
        rep.values(c, f"attention-{c['dt']}", got, ref, np.where(ref == 0, 0.0, sc.ATTN_F * eps), what)


# ---- l2s_kv_attention ---------------------------------------------------------------------------------------------------------------------------
class KvKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        H, B, T, dt = c["H"], c["B"], c["T"], c["dt"]
        W = self.W = 64 * H
        r = rng_of(c)
        R = lambda x: sr.round16(x, dt)
        q = R(r.standard_normal((B, W)) * 0.125)
        k, v = R(r.standard_normal((B, T, W))), R(r.standard_normal((B, T, W)))
        kn, vn = R(r.standard_normal((B, W))), R(r.standard_normal((B, W)))
        val = c["value"]
        if val.startswith("dom:"):
            lead = np.empty((B, W))
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                lead[:, sl] = q[:, sl] * (45.0 / (q[:, sl] ** 2).sum(1, keepdims=True))
            if val == "dom:new":
                kn = R(lead)
            else:
                k[:, int(val[4:])] = R(lead)
        elif val == "equal":
            k[:] = k[:, :1]
            kn = k[:, 0].copy()
        elif val == "pm60":
            q[:] = 1.0
            sign = np.where(r.random((B, T, H)) < 0.5, -1.0, 1.0)
            k[:] = np.repeat(sign, 64, axis=2) * 0.9375
            kn[:] = 0.9375
        self.self_form = c["form"] == "self"
        self.append = self.self_form and c["append"]
        self.pos = None
        if self.self_form:
            self.pos = np.asarray(c["pos"] if c["stride"] == 1 else [c["pos"][0]] * B, np.int64)
        self.q, self.kn, self.vn = q, kn, vn
        a = dict(pos=self.pos, n_valid=c["n_valid"], k_new=kn if self.append else None, v_new=vn if self.append else None)
        _, _, _, read = sr.kv_attention(q, k, v, H, **a)
        k[~read], v[~read] = np.nan, np.nan              # rows that must not be read
        self.k, self.v = k, v
        self.ref, self.k2, self.v2, _ = sr.kv_attention(q, k, v, H, **a) if c["expect"] == 0 else (None, k, v, None)
        if val.startswith("dom:") and c["expect"] == 0:
            self.lead_check()

    def lead_check(self):
        """the planted key leads every other score of its (clip, head) by >= 30"""
        c, H = self.c, self.c["H"]
        for b in range(self.B):
            p = int(self.pos[b])
            keys = np.concatenate([self.k2[b, :p + 1]], 0)
            for h in range(H):
                sl = slice(64 * h, 64 * h + 64)
                s = np.sort(keys[:, sl] @ self.q[b, sl])
                assert s[-1] - s[-2] >= 30.0, (c["name"], b, h, s[-1] - s[-2])

    def specs(self, sel):
        c, W, T, dt = self.c, self.W, self.c["T"], self.c["dt"]
        n = len(sel)
        lda = c.get("ld_arg", {})
        self.ld = dict(q=W + c["pads"][0], out=W + c["pads"][1], new=W + c["pads"][2])
        d = OrderedDict()
        d["q"] = Buf(T16[dt], n, W, self.ld["q"], data=t16(self.q[sel], dt), **self.flags("q"))
        d["kc"] = Buf(T16[dt], n * T, W, data=t16(self.k[sel], dt), out=True, **self.flags("kc"))
        d["vc"] = Buf(T16[dt], n * T, W, data=t16(self.v[sel], dt), out=True, **self.flags("vc"))
        if self.append or c.get("null") in ("k_new", "v_new"):
            d["k_new"] = Buf(T16[dt], n, W, self.ld["new"], data=t16(self.kn[sel], dt), **self.flags("k_new"))
            d["v_new"] = Buf(T16[dt], n, W, self.ld["new"], data=t16(self.vn[sel], dt), **self.flags("v_new"))
        if self.self_form:
            d["pos"] = vec(i32, self.pos[sel] if c["stride"] == 1 else self.pos[:1], **self.flags("pos"))
        d["out"] = Buf(T16[dt], n, W, self.ld["out"], out=True, **self.flags("out"))
        self.ld.update(lda)
        return d

    def call(self, lib, p, sel):
        c = self.c
        return lib.l2s_kv_attention(p["q"], self.ld["q"], p["kc"], p["vc"], self.arg("T", c["T"]), p.get("k_new"), p.get("v_new"), self.ld["new"],
                                    p.get("pos"), c["stride"], c["n_valid"], self.arg("B", len(sel)), self.arg("H", c["H"]), p["out"], self.ld["out"],
                                    self.arg("dtype", dtc(c["dt"])), stream())

    def clip_out(self, outs, i):
        T = self.c["T"]
        return [outs["out"][i:i + 1], outs["kc"][i * T:(i + 1) * T], outs["vc"][i * T:(i + 1) * T]]

    def judge(self, rep, outs):
        c, dt = self.c, self.c["dt"]
        rep.same(c, "k cache", outs["kc"], t16(self.k2, dt).reshape(-1, self.W))
        rep.same(c, "v cache", outs["vc"], t16(self.v2, dt).reshape(-1, self.W))
        self.attn_check(rep, outs["out"].double().numpy(), self.ref, "out")


# ---- l2s_beam_attention -------------------------------------------------------------------------------------------------------------------------
class BaKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        hd, H, beam, B, T, dt = c["hd"], c["H"], c["beam"], c["B"], c["T"], c["dt"]
        W = self.W = H * hd
        r = rng_of(c)
        R = lambda x: sr.round16(x, dt)
        self.self_form = c["form"] == "self"
        self.q = R(r.standard_normal((B, beam, W)) * hd ** -0.5)
        self.kn, self.vn = R(r.standard_normal((B, beam, W))), R(r.standard_normal((B, beam, W)))
        self.n_live = None if c["n_live"] is None else np.asarray(c["n_live"], np.int64)
        self.fin = None if c["finished"] is None else np.asarray(c["finished"], np.int64)
        p = c["p"]
        if self.self_form:
            k, v = R(r.standard_normal((B, beam, T, W))), R(r.standard_normal((B, beam, T, W)))
            kind = c["anc"]
            a = r.integers(0, beam, (B, beam, T))
            if kind == "identity":
                a[:] = np.arange(beam)[None, :, None]
            elif kind == "one":
                a[:] = (beam - 1) // 2
            elif kind == "perm":
                for b in range(B):
                    for t in range(T):
                        a[b, :, t] = r.permutation(beam)
            elif kind == "clamp":
                m = r.random((B, beam, T))
                a = np.where(m < 0.25, -3, np.where(m < 0.5, beam + 2, a))
            other = np.where((a >= 0) & (a < beam), (a + 1) % beam, a[:, ::-1])
            self.anc = np.stack([a, other] if (p & 1) == 0 else [other, a])
            if 0 <= p < T:
                cur = np.clip(a, 0, beam - 1)
                read = np.zeros((B, beam, T), bool)
                for b in range(B):
                    for i in range(beam):
                        if not sr.beam_dead(b, i, self.n_live, self.fin):
                            read[b, cur[b, i, :p], np.arange(p)] = True
                k[~read], v[~read] = np.nan, np.nan
            self.k, self.v = k, v
            if c["expect"] == 0:
                self.ref, self.k2, self.v2 = sr.beam_attention_self(self.q, k, v, self.kn, self.vn, self.anc, p, H, self.n_live, self.fin)
        else:
            k, v = R(r.standard_normal((B, T, W))), R(r.standard_normal((B, T, W)))
            self.lens = np.asarray(c["enc_lens"], np.int64)
            for b in range(B):
                n = min(max(int(self.lens[b]), 0), T)
                k[b, n:], v[b, n:] = np.nan, np.nan
                if sr.beam_dead(b, 0, self.n_live, self.fin):
                    k[b], v[b] = np.nan, np.nan
            self.k, self.v, self.k2, self.v2 = k, v, k, v
            if c["expect"] == 0:
                self.ref = sr.beam_attention_cross(self.q, k, v, self.lens, H, self.n_live, self.fin)
            self.anc = np.zeros((2, B, beam, T), np.int64)

    def specs(self, sel):
        c, W, T, dt, beam = self.c, self.W, self.c["T"], self.c["dt"], self.c["beam"]
        n = len(sel)
        self.ld = dict(q=W + c["pads"][0], out=W + c["pads"][1], new=W + c["pads"][2])
        d = OrderedDict()
        d["q"] = Buf(T16[dt], n * beam, W, self.ld["q"], data=t16(self.q[sel], dt), **self.flags("q"))
        rows = n * beam * T if self.self_form else n * T
        d["kc"] = Buf(T16[dt], rows, W, data=t16(self.k[sel], dt), out=True, **self.flags("kc"))
        d["vc"] = Buf(T16[dt], rows, W, data=t16(self.v[sel], dt), out=True, **self.flags("vc"))
        if self.self_form:
            d["k_new"] = Buf(T16[dt], n * beam, W, self.ld["new"], data=t16(self.kn[sel], dt), **self.flags("k_new"))
            d["v_new"] = Buf(T16[dt], n * beam, W, self.ld["new"], data=t16(self.vn[sel], dt), **self.flags("v_new"))
            d["step"] = vec(i32, [c["p"]], **self.flags("step"))
        if self.self_form or c.get("extra") == "anc":
            d["anc"] = Buf(i16, 2 * n * beam, T, data=self.anc[:, sel].astype(np.int16), **self.flags("anc"))
        if not self.self_form or c.get("extra") == "enc_lens":
            d["enc_lens"] = vec(i32, self.lens[sel] if not self.self_form else np.ones(n), **self.flags("enc_lens"))
        if self.n_live is not None:
            d["n_live"] = vec(i32, self.n_live[sel], **self.flags("n_live"))
        if self.fin is not None:
            d["finished"] = vec(u8, self.fin[sel])
        d["out"] = Buf(T16[dt], n * beam, W, self.ld["out"], out=True, **self.flags("out"))
        self.ld.update(c.get("ld_arg", {}))
        return d

    def call(self, lib, p, sel):
        c = self.c
        return lib.l2s_beam_attention(p["q"], self.ld["q"], p["kc"], p["vc"], self.arg("T", c["T"]), p.get("k_new"), p.get("v_new"), self.ld["new"],
                                      p.get("anc"), p.get("step"), p.get("enc_lens"), p.get("n_live"), p.get("finished"), self.arg("B", len(sel)),
                                      self.arg("beam", c["beam"]), self.arg("H", c["H"]), self.arg("hd", c["hd"]), p["out"], self.ld["out"],
                                      self.arg("dtype", dtc(c["dt"])), stream())

    def clip_out(self, outs, i):
        beam = self.c["beam"]
        n = beam * self.c["T"] if self.self_form else self.c["T"]
        return [outs["out"][i * beam:(i + 1) * beam], outs["kc"][i * n:(i + 1) * n], outs["vc"][i * n:(i + 1) * n]]

    def judge(self, rep, outs):
        c, dt = self.c, self.c["dt"]
        rep.same(c, "k cache", outs["kc"], t16(self.k2, dt).reshape(-1, self.W))
        rep.same(c, "v cache", outs["vc"], t16(self.v2, dt).reshape(-1, self.W))
        self.attn_check(rep, outs["out"].double().numpy().reshape(self.ref.shape), self.ref, "out")


# ---- l2s_vocab_argmax ---------------------------------------------------------------------------------------------------------------------------
class VaKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        V, d, B, dt = c["V"], c["d"], c["B"], c["dt"]
        r = rng_of(c)
        R = lambda x: sr.round16(x, dt)
        plant = c["plant"]
        n = len(plant)
        base = R(r.standard_normal((n, d)))
        self.x = base[np.arange(B) % n]
        emb = R(r.standard_normal((V, d)) * 0.05)
        for i, (top, dup) in enumerate(plant):
            emb[top] = R(base[i] * 0.05)
            if dup is not None:
                emb[dup] = emb[top]
        self.emb = emb
        tops = [t for t, _ in plant]
        dups = [u for _, u in plant if u is not None]
        sup, beg = np.zeros(V, bool), np.zeros(V, bool)
        m = c["mask"]
        if m in ("top", "both"):
            sup[tops] = True
        if m == "all":
            sup[:] = True
        if m == "begin":
            beg[tops] = True
        if m == "both":
            beg[dups] = True
        self.sup = sup if m in ("top", "all", "both") else None
        self.beg = beg if m in ("begin", "both") else None
        self.forbid = sup | (beg if c["step"] == c["first"] else np.zeros(V, bool))
        self.with_logits = True
        if c["expect"] == 0:
            self.reference()

    def reference(self):
        c = self.c
        ref = self.ref = sr.vocab_logits(self.x, self.emb)
        blas, chain = sr.vocab_logits_f32(self.x, self.emb)
        eps = max(float(np.abs(blas - ref).max()), float(np.abs(chain - ref).max()), 2.0 ** -23 * max(1.0, float(np.abs(ref).max())))
        self.b_logit = 4.0 * eps
        ids, lp = sr.masked_argmax(ref, self.forbid)
        # decisive: every allowed id within DECISIVE x the bound of the maximum is a bit-identical embedding row - an exact tie
        allowed = np.flatnonzero(~self.forbid)
        for b in range(self.B):
            if allowed.size == 0:
                continue
            near = allowed[ref[b, allowed] >= ref[b, ids[b]] - sc.DECISIVE * self.b_logit]
            for j in near:
                assert np.array_equal(self.emb[j], self.emb[ids[b]]), f"{c['name']}: clip {b} lost its gap (ids {ids[b]} and {j})"
            assert ids[b] == near.min()
        self.ids, self.lp = ids, lp
        if allowed.size:
            sub = blas[:, allowed]
            top = sub.max(axis=1)
            lp32 = -np.log(np.exp(sub - top[:, None]).sum(axis=1, dtype=np.float32))
            self.b_lp = 4.0 * max(float(np.abs(lp32.astype(np.float64) - lp).max()), float(2.0 ** -23 * max(1.0, np.abs(lp).max())))
        else:
            self.b_lp = 0.0

    def specs(self, sel):
        c, V, d, dt = self.c, self.c["V"], self.c["d"], self.c["dt"]
        n = len(sel)
        self.ld = dict(x=d + c["ldpad"][0], emb=d + c["ldpad"][1])
        o = OrderedDict()
        o["x"] = Buf(T16[dt], n, d, self.ld["x"], data=t16(self.x[sel], dt), **self.flags("x"))
        o["emb"] = Buf(T16[dt], V, d, self.ld["emb"], data=t16(self.emb, dt), **self.flags("emb"))
        if self.sup is not None:
            o["suppress"] = vec(u8, self.sup.astype(np.uint8))
        if self.beg is not None:
            o["begin"] = vec(u8, self.beg.astype(np.uint8))
        if c["step"] is not None:
            o["step"] = vec(i32, [c["step"]], **self.flags("step"))
        o["work"] = Buf(i32, 1, ((V + 63) // 64) * n * 3, out=True, guard=64, **self.flags("work"))
        o["token"] = Buf(i32, 1, n, out=True, guard=16, **self.flags("token"))
        o["logprob"] = Buf(f32, 1, n, out=True, guard=16, **self.flags("logprob"))
        if self.with_logits:
            o["logits"] = Buf(f32, n, V, out=True, guard=64, **self.flags("logits"))
        self.ld.update(c.get("ld_arg", {}))
        return o

    def call(self, lib, p, sel):
        c = self.c
        V, B = self.arg("V", c["V"]), self.arg("B", len(sel))
        want = ((V + 63) // 64) * B * 12 if 0 < V <= 65536 and B > 0 else 0
        if lib.l2s_vocab_argmax_workspace(V, B) != want:
            raise Fail(f"FAIL case={c['name']}: l2s_vocab_argmax_workspace({V}, {B}) = {lib.l2s_vocab_argmax_workspace(V, B)}, the window has {want} bytes")
        return lib.l2s_vocab_argmax(p["x"], self.ld["x"], p["emb"], self.ld["emb"], self.arg("B", len(sel)), self.arg("V", c["V"]), self.arg("d", c["d"]),
                                    p.get("suppress"), p.get("begin"), p.get("step"), c["first"], p["work"], p["token"], p["logprob"], p.get("logits"),
                                    self.arg("dtype", dtc(c["dt"])), stream())

    def clip_out(self, outs, i):
        return [outs["token"][:, i], outs["logprob"][:, i]] + ([outs["logits"][i]] if "logits" in outs else [])

    def judge(self, rep, outs):
        c = self.c
        rep.values(c, f"logits-{c['dt']}", outs["logits"].double().numpy(), self.ref, self.b_logit, "logits")
        rep.same(c, "token", outs["token"][0], torch.from_numpy(self.ids.astype(np.int32)))
        rep.values(c, f"logprob-{c['dt']}", outs["logprob"][0].double().numpy(), self.lp, self.b_lp, "logprob")


# ---- l2s_whisper_advance ------------------------------------------------------------------------------------------------------------------------
class WaKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        B, d, V, dt, eot = c["B"], c["d"], c["V"], c["dt"], c["eot"]
        r = rng_of(c)
        self.emb = sr.round16(r.standard_normal((V, d)), dt)
        self.pe = r.standard_normal((c["n_ctx"], d)).astype(np.float32)
        tok = r.integers(8, V, B)
        tok[0] = -1
        if B > 1:
            tok[1] = V
        if B > 2:
            tok[2] = eot
        tok[4::5] = eot
        done = np.zeros(B, bool)
        if c["live"] == "mixed":
            done[3::3] = True
        elif c["live"] == "only256":
            done[:] = True
            done[256] = False
            tok[256] = 9
        else:
            done[:] = True
        self.st = dict(token=tok.astype(np.int32), logprob=(-r.integers(1, 640, B) / 64.0).astype(np.float32),
                       tokens=r.integers(0, V, (B, c["ld_tok"])).astype(np.int32), sum_logprob=(-r.integers(0, 6400, B) / 64.0).astype(np.float32),
                       lengths=r.integers(0, 9, B).astype(np.int32), done=done)

    def reference(self, sel):
        c, s = self.c, self.st
        return sr.whisper_advance(s["token"][sel], s["logprob"][sel], s["tokens"][sel], s["sum_logprob"][sel], s["lengths"][sel], s["done"][sel], self.emb,
                                  self.pe, c["pos"], c["eot"], np.full((len(sel), c["d"]), np.nan, np.float32))

    def specs(self, sel):
        c, d, dt, s = self.c, self.c["d"], self.c["dt"], self.st
        n = len(sel)
        self.ld = dict(emb=d + c["ldpad"][1], x=d + c["ldpad"][0])
        o = OrderedDict()
        o["token"] = vec(i32, s["token"][sel], out=True, **self.flags("token"))
        o["logprob"] = vec(f32, s["logprob"][sel], **self.flags("logprob"))
        o["tokens"] = Buf(i32, n, c["ld_tok"], data=s["tokens"][sel], out=True, **self.flags("tokens"))
        o["sum_logprob"] = vec(f32, s["sum_logprob"][sel], out=True, **self.flags("sum_logprob"))
        o["lengths"] = vec(i32, s["lengths"][sel], out=True, **self.flags("lengths"))
        o["done"] = vec(u8, s["done"][sel].astype(np.uint8), out=True, **self.flags("done"))
        o["emb"] = Buf(T16[dt], c["V"], d, self.ld["emb"], data=t16(self.emb, dt), **self.flags("emb"))
        o["pos_emb"] = Buf(f32, c["n_ctx"], d, data=self.pe, **self.flags("pos_emb"))
        o["x"] = Buf(f32, n, d, self.ld["x"], out=True, **self.flags("x"))
        o["pos"] = vec(i32, [c["pos"]], out=True, **self.flags("pos"))
        o["n_active"] = Buf(i32, 1, 1, out=True, guard=16, **self.flags("n_active"))
        self.ld.update(c.get("ld_arg", {}))
        return o

    def call(self, lib, p, sel):
        c = self.c
        return lib.l2s_whisper_advance(p["token"], p["logprob"], p["tokens"], self.arg("ld_tok", c["ld_tok"]), p["sum_logprob"], p["lengths"], p["done"], p["emb"],
                                       self.ld["emb"], p["pos_emb"], self.arg("n_ctx", c["n_ctx"]), p["x"], self.ld["x"], p["pos"], p["n_active"],
                                       self.arg("B", len(sel)), self.arg("V", c["V"]), self.arg("d", c["d"]), self.arg("eot", c["eot"]),
                                       self.arg("dtype", dtc(c["dt"])), stream())

    def clip_out(self, outs, i):
        return [outs[n][:, i] for n in ("token", "sum_logprob", "lengths", "done")] + [outs["tokens"][i], outs["x"][i]]

    def judge(self, rep, outs):
        c = self.c
        w = self.reference(list(range(self.B)))
        for n, td in (("token", np.int32), ("sum_logprob", np.float32), ("lengths", np.int32), ("done", np.uint8)):
            rep.same(c, n, outs[n][0], torch.from_numpy(w[n].astype(td)))
        rep.same(c, "tokens", outs["tokens"], torch.from_numpy(w["tokens"].astype(np.int32)))
        rep.same(c, "x_next", outs["x"], torch.from_numpy(w["x_next"]))
        rep.same(c, "pos", outs["pos"][0], torch.tensor([w["pos"]], dtype=i32))
        rep.same(c, "n_active", outs["n_active"][0], torch.tensor([w["n_active"]], dtype=i32))


# ---- l2s_beam_select ----------------------------------------------------------------------------------------------------------------------------
def crafted(B, beam, V, seed, temperature):
    # the issue asks for the existing construction itself, so it is imported from the GPU test's module, which must stay importable
    # without a device (it touches the device only inside its tests); tests/test_step_matrix_cpu.py depends on that too
    from tests.test_lipread_kernels_gpu import _crafted
    return _crafted(B, beam, V, seed, temperature)


class BsKase(Kase):
    EOS = 2

    def __init__(self, c):
        super().__init__(c)
        beam, V, B = c["beam"], c["V"], c["B"]
        r = rng_of(c)
        self.temp, self.pen = TEMPERATURE, UNK_PENALTY
        kind = c["kind"]
        if kind == "crafted":
            lg, cum = crafted(B, beam, V, seed_of(c["name"], c.get("seed", 0)), self.temp)
            lg[0, 0, min(5, V - 1)] = np.nan
            if beam > 1 and B > 1:
                lg[1, beam - 1, :] = np.nan
        elif kind == "topbyte":
            self.temp = 1.0
            lg = r.uniform(-100, -90, (B, beam, V)).astype(np.float32)
            for b in range(B):
                lg[b, 0, [0, 2, 4, 5]] = np.float32(-0.3) * r.permutation(4).astype(np.float32)
            cum = np.zeros((2, B, beam), np.float32)
        else:
            self.temp = 1.0
            row = r.permutation(V).astype(np.float32) * np.float32(0.25)
            row[7] = row[9] = row.max() + 20.0
            lg = np.broadcast_to(row, (B, beam, V)).copy()
            cum = np.full((2, B, beam), -1.5, np.float32)
        self.lg, self.cum = lg, cum
        self.max_len = np.asarray(([9, 5, 9] * B)[:B])
        nl = c["n_live"]
        self.n_live = np.asarray([beam, max(1, beam - 1), beam][:B] if nl == "mixed" else [beam] * B if nl == "beam" else nl)
        self.fin = np.asarray(([0, 0, 1] * B)[:B] if (kind == "crafted" and nl == "mixed") else [0] * B)
        if c["expect"] == 0:
            self.refs = [self.reference(b) for b in range(B)]

    def reference(self, b):
        """(score, slot, token) of the K best; asserts that every deciding gap (the K + 1-th candidate included) is decisive"""
        c, beam, V = self.c, self.c["beam"], self.c["V"]
        st = c["step"]
        s, sl, tk = sr.beam_select(self.lg[b].astype(np.float64), self.cum[st & 1, b], st, self.max_len[b], beam, None if c["null_live"] else self.n_live[b],
                                   c["min_len"], self.temp, self.pen, c["pad"], c["unk"], self.EOS, extra=1)
        for i in range(len(s) - 1):
            if s[i] == NEG_INF and s[i + 1] == NEG_INF:
                continue
            tol = float(sr.select_tol(V, s[i])) if np.isfinite(s[i]) else 0.0
            if s[i] - s[i + 1] > sc.DECISIVE * tol:
                continue
            a, z = (sl[i], tk[i]), (sl[i + 1], tk[i + 1])
            tie = (self.lg[b][a].tobytes() == self.lg[b][z].tobytes() and self.lg[b, a[0]].tobytes() == self.lg[b, z[0]].tobytes()
                   and (st <= 0 or self.cum[st & 1, b, a[0]].tobytes() == self.cum[st & 1, b, z[0]].tobytes()) and (a[1] == c["unk"]) == (z[1] == c["unk"]))
            assert tie, f"{c['name']}: clip {b} lost its gap at rank {i}: {s[i]!r} {s[i + 1]!r}"
        return s[:-1], sl[:-1], tk[:-1]

    def specs(self, sel):
        c, beam, V = self.c, self.c["beam"], self.c["V"]
        n, K = len(sel), 2 * beam
        o = OrderedDict()
        self.ldl = V + c["ldpad"]
        o["logits"] = Buf(f32, n * beam, V, self.ldl, data=self.lg[sel], **self.flags("logits"))
        o["scores"] = Buf(f32, 2 * n, beam, data=self.cum[:, sel], **self.flags("scores"))
        o["step"] = vec(i32, [c["step"]], **self.flags("step"))
        o["max_len"] = vec(i32, self.max_len[sel], **self.flags("max_len"))
        if not c["null_live"]:
            o["n_live"] = vec(i32, self.n_live[sel], **self.flags("n_live"))
        if not c.get("null_fin"):
            o["finished"] = vec(u8, self.fin[sel])
        o["cand_score"] = Buf(f32, n, K, out=True, **self.flags("cand_score"))
        o["cand_slot"] = Buf(i32, n, K, out=True, **self.flags("cand_slot"))
        o["cand_token"] = Buf(i32, n, K, out=True, **self.flags("cand_token"))
        self.ldl = c.get("ldl_arg", self.ldl)
        return o

    def call(self, lib, p, sel):
        c = self.c
        V, beam = self.arg("V", c["V"]), self.arg("beam", c["beam"])
        want = 16 if 0 < beam <= 64 and V <= 8192 and V >= 2 * beam + 2 else 0
        if lib.l2s_beam_select_workspace(V, beam) != want:
            raise Fail(f"FAIL case={c['name']}: l2s_beam_select_workspace({V}, {beam}) = {lib.l2s_beam_select_workspace(V, beam)}, expected {want}")
        return lib.l2s_beam_select(p["logits"], self.ldl, p["scores"], p["step"], p["max_len"], p.get("n_live"), p.get("finished"), self.arg("B", len(sel)),
                                   self.arg("beam", c["beam"]), self.arg("V", c["V"]), c["pad"], c["unk"], self.arg("eos", self.EOS), c["min_len"],
                                   self.arg("temp", self.temp), self.pen, p["cand_score"], p["cand_slot"], p["cand_token"], stream())

    def clip_out(self, outs, i):
        return [outs[n][i] for n in ("cand_score", "cand_slot", "cand_token")]

    def judge(self, rep, outs):
        c, K = self.c, 2 * self.c["beam"]
        for b in range(self.B):
            if self.fin[b] and not c.get("null_fin"):
                for n, td in (("cand_score", f32), ("cand_slot", i32), ("cand_token", i32)):
                    rep.same(c, f"clip {b} is finished: {n} untouched", outs[n][b], canary(K, td))
                continue
            s, sl, tk = self.refs[b]
            rep.same(c, f"clip {b}: cand_slot", outs["cand_slot"][b], torch.from_numpy(sl.astype(np.int32)))
            rep.same(c, f"clip {b}: cand_token", outs["cand_token"][b], torch.from_numpy(tk.astype(np.int32)))
            rep.values(c, "select", outs["cand_score"][b].double().numpy(), s, np.where(np.isfinite(s), sr.select_tol(c["V"], np.where(np.isfinite(s), s, 0.0)), 0.0),
                       f"clip {b}: cand_score")


NEG_INF = -np.inf


# ---- l2s_beam_advance ---------------------------------------------------------------------------------------------------------------------------
ADV_STATE = (("tokens", i32), ("anc", i16), ("scores", f32), ("n_live", i32), ("finished", u8), ("parents", i32), ("hyp_tokens", i32), ("hyp_len", i32),
             ("hyp_score", f32), ("nhyp", i32), ("out_tokens", i32), ("out_len", i32), ("out_score", f32))
EMBED_SCALE = 1.75


def state_of_clip(t, name, nsel, i):
    """the part of a state table (its window on the host, `nsel` clips) that belongs to clip i"""
    if name in ("tokens", "anc", "scores"):
        return t.reshape(2, nsel, -1)[:, i]
    if name in ("n_live", "finished", "nhyp"):
        return t.reshape(-1)[i:i + 1]
    return t.reshape(nsel, -1)[i]


def adv_script(c, r, b):
    """the steps of clip b: [(score [K], slot [K], token [K])], and its max_len"""
    beam, V, script = c["beam"], c["V"], c["script"]
    K = 2 * beam

    def cands(eos=(), all_eos=False):
        tk = r.integers(4, V, K)
        tk[[e for e in eos if e < K]] = 2
        if all_eos:
            tk[:] = 2
        s = -np.sort(r.integers(32, 600, K)) / 64.0
        return s.astype(np.float32), r.integers(0, beam, K), tk
    late = [beam, K - 1]
    if script in ("eos-first", "inert", "noroom"):
        return [cands()] + [cands([0] + late[1:]) for _ in range(4)], 9
    if script == "eos-late":
        return [cands(late) for _ in range(3)] + [cands(all_eos=True) for _ in range(2)], 3
    if script == "eos-neginf":
        steps = []
        for _ in range(3):
            s, sl, tk = cands([0])
            s[0] = -np.inf
            steps.append((s, sl, tk))
        return steps, 9
    if script == "nhyp-mid":
        return [cands(), cands([0]), cands(range(beam + 1)), cands()], 9
    if script == "maxlen":
        s, sl, tk = cands(all_eos=True)
        s[1:] = -np.inf
        return [cands(), cands(), (s, sl, tk)], 2
    if script == "equal":
        return [cands(), cands(), (np.full(K, -2.0, np.float32), r.integers(0, beam, K), np.where(np.arange(K) < beam, 2, 9))], 9
    if script == "outlen":
        s, sl, tk = cands(all_eos=True)
        s[2:] = -np.inf
        return [cands(), cands([0]), cands([0]), cands([1]), (s, sl, tk)], 4
    if script == "clamp":
        steps = []
        for i in range(4):
            s, sl, tk = cands([1] if i == 2 else [])
            sl[::3], sl[1::3] = -3, beam + 2
            tk[0], tk[K - 1] = -1, V + 5
            if beam > 1:
                tk[1] = V + 5 if i != 2 else 2
            steps.append((s, sl, tk))
        return steps, 9
    raise ValueError(script)


class BdKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        beam, L, d, B, V, dt = c["beam"], c["L"], c["d"], c["B"], c["V"], c["dt"]
        r = rng_of(c)
        self.emb = sr.round16(r.standard_normal((V, d)), dt)
        self.pos = (np.round(r.standard_normal((L, d)) * 4096) / 4096).astype(np.float32)
        per = [adv_script(c, rng_of(c, b), b) for b in range(B)]
        self.nsteps = max(len(s) for s, _ in per)
        self.max_len = np.asarray([m for _, m in per], np.int32)
        K = 2 * beam
        self.cs, self.cl, self.ct = np.zeros((self.nsteps, B, K), np.float32), np.zeros((self.nsteps, B, K), np.int32), np.zeros((self.nsteps, B, K), np.int32)
        for b, (steps, _) in enumerate(per):
            for s in range(self.nsteps):
                self.cs[s, b], self.cl[s, b], self.ct[s, b] = steps[min(s, len(steps) - 1)]
        self.pre = np.zeros(B, np.uint8)
        if c["script"] == "inert" and B > 1:
            self.pre[1] = 1

    def reference(self, sel):
        c = self.c
        S = sr.advance_state(len(sel), c["beam"], c["L"], c["d"], self.pre[sel])
        for s in range(self.nsteps):
            sr.beam_advance(S, self.cs[s][sel], self.cl[s][sel], self.ct[s][sel], self.max_len[sel], self.emb, self.pos, EMBED_SCALE, c["V"],
                            lenpen=c["lenpen"], normalize=bool(c["normalize"]))
        return S

    def specs(self, sel):
        c, beam, L, d, dt = self.c, self.c["beam"], self.c["L"], self.c["d"], self.c["dt"]
        n, K = len(sel), 2 * beam
        S = sr.advance_state(n, beam, L, d, self.pre[sel])
        self.ld = dict(emb=d + c["ldpad"][0], x=d + c["ldpad"][1])
        o = OrderedDict()
        o["cand_score"] = Buf(f32, self.nsteps * n, K, data=self.cs[:, sel], **self.flags("cand_score"))
        o["cand_slot"] = Buf(i32, self.nsteps * n, K, data=self.cl[:, sel], **self.flags("cand_slot"))
        o["cand_token"] = Buf(i32, self.nsteps * n, K, data=self.ct[:, sel], **self.flags("cand_token"))
        for name, td in ADV_STATE:
            a = S[name]
            o[name] = Buf(td, int(np.prod(a.shape[:-1])) if a.ndim > 1 else 1, a.shape[-1], data=a, out=True, guard=None if a.ndim > 1 else 16, **self.flags(name))
        o["max_len"] = vec(i32, self.max_len[sel], **self.flags("max_len"))
        o["emb"] = Buf(T16[dt], c["V"], d, self.ld["emb"], data=t16(self.emb, dt), **self.flags("emb"))
        o["pos_table"] = Buf(f32, L, d, data=self.pos, **self.flags("pos_table"))
        o["x"] = Buf(f32, n * beam, d, self.ld["x"], out=True, **self.flags("x"))
        o["step"] = vec(i32, [0], out=True, **self.flags("step"))
        o["n_active"] = Buf(i32, 1, 1, out=True, guard=16, **self.flags("n_active"))
        self.ld.update(c.get("ld_arg", {}))
        return o

    def call(self, lib, p, sel):
        c = self.c
        n, K = len(sel), 2 * c["beam"]
        rc = 0
        for s in range(self.nsteps if c["expect"] == 0 else 1):
            cand = [None if p[k] is None else p[k] + s * n * K * 4 for k in ("cand_score", "cand_slot", "cand_token")]
            rc = lib.l2s_beam_advance(*cand, *[p[name] for name, _ in ADV_STATE], p["max_len"], p["emb"], self.ld["emb"], p["pos_table"], EMBED_SCALE, p["x"],
                                      self.ld["x"], p["step"], p["n_active"], self.arg("B", n), self.arg("beam", c["beam"]), self.arg("L", c["L"]),
                                      self.arg("V", c["V"]), self.arg("d", c["d"]), self.arg("eos", 2), 1, c["lenpen"], c["normalize"],
                                      self.arg("dtype", dtc(c["dt"])), stream())
            if rc != 0:
                break
        return rc

    def clip_out(self, outs, i):
        beam = self.c["beam"]
        out = [outs["x"][i * beam:(i + 1) * beam]]
        nsel = outs["n_live"].shape[1]
        for name, _ in ADV_STATE:
            out.append(state_of_clip(outs[name], name, nsel, i))
        return out

    def judge(self, rep, outs):
        c = self.c
        S = self.reference(list(range(self.B)))
        for name, td in ADV_STATE:
            rep.same(c, name, outs[name].reshape(-1), torch.from_numpy(S[name]).reshape(-1))
        rep.same(c, "x_next", outs["x"], torch.from_numpy(S["x"]))
        rep.same(c, "step", outs["step"][0], torch.from_numpy(S["step"]))
        rep.same(c, "n_active", outs["n_active"][0], torch.from_numpy(S["n_active"]))


# ---- l2s_ctc_beam_search ------------------------------------------------------------------------------------------------------------------------
def ctc_need_bytes(B, L, beam):
    """l2s_ctc_beam_workspace restated: per clip a hash table of the first power of two >= 2 (beam L + 1) (at least 64) and beam L + 1 nodes, 8 bytes each"""
    if B <= 0 or L <= 0 or beam <= 0 or beam > 64 or beam * L + 1 >= 1 << 19:
        return 0
    cap = 64
    while cap < 2 * (beam * L + 1):
        cap <<= 1
    return B * (cap + beam * L + 1) * 8


def ctc_logits(c, b):
    """[L, V] fp32 logits of clip b.  Rank k of a frame gets -(a min(k, 8) + g max(k - 8, 0)) - jitter (g = 0.37; beam > 2: 0.2 + 0.005 per frame): a = 5 in a peaked frame, one
    of six incommensurate slopes in an ambiguous one, so that candidate scores are sums of distinct steps; which class holds which rank is
    the kind: any (geo), blank last and outside the top-K (noblank), blank first (blankfirst), one order for every frame with a non-blank
    class first (repeat), two classes with the same logit in every third frame (ties).  A beam above 2 gets no ambiguous frames and a
    slope of its own per frame (3.0, 3.06, ... in a seeded order; the deepest rank stays above the fp32 underflow of its probability).  revival: N(0, 1.5), as tests/test_text_cpu.py."""
    from tests import _ctc_reference as cr
    L, V, K, kind = c["L"], c["V"], c["K"], c["kind"]
    r = np.random.default_rng(seed_of("ctc", c["kind"], c["seed"], b, L, V))
    if kind == "revival":
        return (r.normal(size=(L, V)).astype(np.float32) * 1.5).astype(np.float32)
    slopes = (0.31, 0.47, 0.73, 1.09, 1.61, 2.33)
    x = np.empty((L, V), np.float32)
    fixed = np.concatenate([[1], [0], 2 + r.permutation(V - 2)]) if V > 2 else np.arange(V)[::-1]
    spread = r.permutation(L)
    for t in range(L):
        amb = (r.random() < 0.15 or L <= 2) and c["beam"] <= 2
        # a wide beam holds the best path and its cheapest single deviations: every frame its own slope, 0.06 apart
        a = slopes[int(r.integers(0, 6))] if amb else (5.0 if c["beam"] <= 2 else 3.0 + 0.06 * spread[t])
        k = np.arange(V)
        val = -(a * np.minimum(k, 8) + (0.37 if c["beam"] <= 2 else 0.2 + 0.005 * spread[t]) * np.maximum(k - 8, 0)) - r.uniform(0.0, 0.05, V)
        if kind == "noblank":
            order = np.concatenate([1 + r.permutation(V - 1), [0]])
        elif kind == "blankfirst":
            order = np.concatenate([[0], 1 + r.permutation(V - 1)])
        elif kind == "repeat":
            order = fixed
        else:
            order = r.permutation(V)
        if kind == "ties" and t % 3 == 1:
            val[2] = val[1]
        x[t, order] = val.astype(np.float32)
    return x


class CtKase(Kase):
    def __init__(self, c):
        super().__init__(c)
        from tests import _ctc_reference as cr
        self.cr = cr
        B, L, V, K = c["B"], c["L"], c["V"], c["K"]
        self.probs = [cr.softmax32(ctc_logits(c, b)) for b in range(B)]
        self.cls, self.lp = np.zeros((B, L, K), np.int32), np.full((B, L, K), -3.0e38, np.float32)
        for b in range(B):
            for t in range(L):
                for k, (cl, lp) in enumerate(cr.pruned_log_probs(self.probs[b][t], K)):
                    self.cls[b, t, k], self.lp[b, t, k] = cl, lp
        self.frames = [L if c["lens"] is None else min(max(c["lens"][b] * c["len_mul"], 0), L) for b in range(B)]
        if c["expect"] == 0:
            self.refs = [self.reference(b) for b in range(B)]

    def reference(self, b):
        """the final beam of clip b, best first; asserts that in every frame the survivors and the first candidate dropped are decided by
        gaps above DECISIVE x the score tolerance, or (kind ties) by scores that are the same fp32 sum of the same two numbers"""
        c, cr = self.c, self.cr
        trace = []
        out = cr.beam_search(self.probs[b][:self.frames[b]], beam=c["beam"], cutoff_top_n=c["K"], trace=trace)
        for t, cands in enumerate(trace):
            for i in range(len(cands) - 1):
                (s0, k0, l0, m0), (s1, k1, l1, m1) = cands[i], cands[i + 1]
                if s0 <= cr.NEG and s1 <= cr.NEG:
                    continue                                 # both are the literal -FLT_MAX (a repeat without a blank between): the same bits everywhere
                tol = sc.CTC_TOL * max(1.0, abs(float(s0)))
                if float(s0) - float(s1) > sc.DECISIVE * tol:
                    continue
                tie = c["kind"] == "ties" and np.float32(s0).tobytes() == np.float32(s1).tobytes() and k0 == k1 == "ext" and \
                    np.float32(self.lp[b, t, l0]).tobytes() == np.float32(self.lp[b, t, l1]).tobytes()
                assert tie, f"{c['name']}: clip {b} frame {t} lost its gap at rank {i}: {float(s0)!r} {float(s1)!r}"
        return out

    def specs(self, sel):
        c = self.c
        n, L, K, nbest = len(sel), c["L"], c["K"], c["nbest"]
        self.need = ctc_need_bytes(n, L, c["beam"])
        o = OrderedDict()
        o["topk_cls"] = Buf(i32, n * L, K, data=self.cls[sel], **self.flags("topk_cls"))
        o["topk_lp"] = Buf(f32, n * L, K, data=self.lp[sel], **self.flags("topk_lp"))
        if c["lens"] is not None:
            o["lens"] = vec(i32, np.asarray(c["lens"])[sel])
        o["work"] = Buf(i32, 1, self.need // 4, out=True, guard=64, **self.flags("work"))
        o["work"].scratch = True                             # its content after a launch is unspecified
        o["labels"] = Buf(i32, n * nbest, L, out=True, **self.flags("labels"))
        o["lengths"] = Buf(i32, 1, n * nbest, out=True, guard=16, **self.flags("lengths"))
        o["scores"] = Buf(f32, 1, n * nbest, out=True, guard=16, **self.flags("scores"))
        return o

    def call(self, lib, p, sel):
        c = self.c
        B, L, beam = self.arg("B", len(sel)), self.arg("L", c["L"]), self.arg("beam", c["beam"])
        got = lib.l2s_ctc_beam_workspace(B, L, beam)
        if got != ctc_need_bytes(B, L, beam):
            raise Fail(f"FAIL case={c['name']}: l2s_ctc_beam_workspace({B}, {L}, {beam}) = {got}, restated {ctc_need_bytes(B, L, beam)}")
        return lib.l2s_ctc_beam_search(p["topk_cls"], p["topk_lp"], p.get("lens"), c["len_mul"], B, L, self.arg("K", c["K"]), beam, self.arg("nbest", c["nbest"]),
                                       p["work"], self.need - c.get("ws_short", 0), p["labels"], p["lengths"], p["scores"], stream())

    def clip_out(self, outs, i):
        nb = self.c["nbest"]
        return [outs["labels"][i * nb:(i + 1) * nb], outs["lengths"][0, i * nb:(i + 1) * nb], outs["scores"][0, i * nb:(i + 1) * nb]]

    def judge(self, rep, outs):
        c, cr = self.c, self.cr
        L, nb = c["L"], c["nbest"]
        for b in range(self.B):
            ref = self.refs[b][:nb]
            lab, ln, scv = np.zeros((nb, L), np.int32), np.zeros(nb, np.int32), np.full(nb, cr.FLT_MAX, np.float32)
            for h, (labels, s) in enumerate(ref):
                lab[h, :len(labels)], ln[h], scv[h] = labels, len(labels), s
            rep.same(c, f"clip {b}: labels", outs["labels"][b * nb:(b + 1) * nb], torch.from_numpy(lab))
            rep.same(c, f"clip {b}: lengths", outs["lengths"][0, b * nb:(b + 1) * nb], torch.from_numpy(ln))
            bound = np.array([sc.CTC_TOL * max(1.0, abs(float(s))) for _, s in ref] + [0.0] * (nb - len(ref)))
            rep.values(c, "ctc-score", outs["scores"][0, b * nb:(b + 1) * nb].double().numpy(), scv.astype(np.float64), bound, f"clip {b}: scores")


# ---- the closed loop ----------------------------------------------------------------------------------------------------------------------------
class LoopKase(Kase):
    """l2s_beam_attention (self) -> a seeded logits table -> l2s_beam_select -> l2s_beam_advance, `steps` times on device state.  The
    reference carries the same tables (sr.advance_state) with fp32 scores; a candidate's device score differs from the reference's by at
    most select_tol per step taken, so step s is held to (s + 1) select_tol and must be decisive by DECISIVE x that."""
    min_len, d = 2, 8

    def __init__(self, c):
        super().__init__(c)
        beam, hd, H, L, B, V, dt, n = c["beam"], c["hd"], c["H"], c["L"], c["B"], c["V"], c["dt"], c["steps"]
        W = self.W = H * hd
        r = rng_of(c)
        R = lambda x: sr.round16(x, dt)
        self.q = R(r.standard_normal((n, B, beam, W)) * hd ** -0.5)
        self.kn, self.vn = R(r.standard_normal((n, B, beam, W))), R(r.standard_normal((n, B, beam, W)))
        lg = r.uniform(-100.0, -90.0, (n, B, beam, V))
        for s in range(n):
            for b in range(B):
                for i in range(beam):
                    hi = r.permutation(V)[:12]
                    lg[s, b, i, hi] = -np.sort(r.uniform(0.0, 6.0, 12))
                lg[s, b, 0, 2] = -0.5 if s % 3 == 2 else lg[s, b, 0, 2]      # eos near the top of slot 0 every third step
        self.lg = lg.astype(np.float32)
        self.emb = R(r.standard_normal((V, self.d)))
        self.pos = (np.round(r.standard_normal((L, self.d)) * 4096) / 4096).astype(np.float32)
        self.max_len = np.asarray(c["max_len"], np.int32)

    def reference(self, sel):
        """per step: (attention rows, candidate scores / slots / tokens, a copy of the tables after the step)"""
        c = self.c
        beam, H, L, V, n = c["beam"], c["H"], c["L"], c["V"], len(sel)
        S = sr.advance_state(n, beam, L, self.d)
        kc, vc = np.full((n, beam, L, self.W), np.nan), np.full((n, beam, L, self.W), np.nan)
        trace = []
        for s in range(c["steps"]):
            fin, live = S["finished"].copy(), S["n_live"].copy()
            att, kc, vc = sr.beam_attention_self(self.q[s][sel], kc, vc, self.kn[s][sel], self.vn[s][sel], S["anc"], s, H, live, fin)
            K = 2 * beam
            cs, cl, ct = np.zeros((n, K), np.float32), np.zeros((n, K), np.int32), np.zeros((n, K), np.int32)
            for j, b in enumerate(sel):
                if fin[j]:
                    continue
                sc_, sl, tk = sr.beam_select(self.lg[s, b].astype(np.float64), S["scores"][s & 1, j].astype(np.float64), s, self.max_len[b], beam, live[j],
                                             self.min_len, TEMPERATURE, UNK_PENALTY, extra=1)
                fi = np.isfinite(sc_)
                tol = (s + 1) * sr.select_tol(V, sc_[fi])
                gaps = sc_[:-1][fi[:-1] & fi[1:]] - sc_[1:][fi[:-1] & fi[1:]]
                assert gaps.size == 0 or (gaps > sc.DECISIVE * tol[:gaps.size]).all(), f"{c['name']}: clip {b} step {s} lost its gap ({gaps.min():.3e})"
                cs[j], cl[j], ct[j] = sc_[:-1].astype(np.float32), sl[:-1], tk[:-1]
            sr.beam_advance(S, cs, cl, ct, self.max_len[sel], self.emb, self.pos, EMBED_SCALE, V)
            trace.append((att, cs.copy(), cl.copy(), ct.copy(), fin, {k: v.copy() for k, v in S.items()}))
        self.kc_ref, self.vc_ref = kc, vc
        if n == self.B:
            first_done = [next((s for s, t in enumerate(trace) if t[5]["finished"][b]), None) for b in range(n)]
            assert first_done[1] is not None and all(f is None or f > first_done[1] for i, f in enumerate(first_done) if i != 1), f"{c['name']}: clip 1 finishes early"
        return trace

    def specs(self, sel):
        c, W, dt = self.c, self.W, self.c["dt"]
        beam, L, V, n, ns, K = c["beam"], c["L"], c["V"], len(sel), c["steps"], 2 * c["beam"]
        S = sr.advance_state(n, beam, L, self.d)
        o = OrderedDict()
        for name, a in (("q", self.q), ("k_new", self.kn), ("v_new", self.vn)):
            o[name] = Buf(T16[dt], ns * n * beam, W, W + 8, data=t16(a[:, sel], dt))
        o["kc"] = Buf(T16[dt], n * beam * L, W, data=t16(torch.full((n * beam * L, W), NAN, dtype=T16[dt]), dt), out=True)
        o["vc"] = Buf(T16[dt], n * beam * L, W, data=t16(torch.full((n * beam * L, W), NAN, dtype=T16[dt]), dt), out=True)
        o["att"] = Buf(T16[dt], ns * n * beam, W, W + 16, out=True)
        o["logits"] = Buf(f32, ns * n * beam, V, V + 4, data=self.lg[:, sel])
        o["cand_score"] = Buf(f32, ns * n, K, out=True)
        o["cand_slot"] = Buf(i32, ns * n, K, out=True)
        o["cand_token"] = Buf(i32, ns * n, K, out=True)
        for name, td in ADV_STATE:
            a = S[name]
            o[name] = Buf(td, int(np.prod(a.shape[:-1])) if a.ndim > 1 else 1, a.shape[-1], data=a, out=True, guard=None if a.ndim > 1 else 16)
        o["max_len"] = vec(i32, self.max_len[sel])
        o["emb"] = Buf(T16[dt], V, self.d, data=t16(self.emb, dt))
        o["pos_table"] = Buf(f32, L, self.d, data=self.pos)
        o["x"] = Buf(f32, n * beam, self.d, out=True)
        o["step"] = vec(i32, [0], out=True)
        o["n_active"] = Buf(i32, 1, 1, out=True, guard=16)
        return o

    def call(self, lib, p, sel):
        c, W = self.c, self.W
        beam, L, V, n, K = c["beam"], c["L"], c["V"], len(sel), 2 * c["beam"]
        self.snaps = []
        for s in range(c["steps"]):
            o16, o4 = s * n * beam * 2, s * n * K * 4
            rc = lib.l2s_beam_attention(p["q"] + o16 * (W + 8), W + 8, p["kc"], p["vc"], L, p["k_new"] + o16 * (W + 8), p["v_new"] + o16 * (W + 8), W + 8,
                                        p["anc"], p["step"], None, p["n_live"], p["finished"], n, beam, c["H"], c["hd"], p["att"] + o16 * (W + 16), W + 16,
                                        dtc(c["dt"]), stream())
            if rc != 0:
                return rc
            rc = lib.l2s_beam_select(p["logits"] + s * n * beam * (V + 4) * 4, V + 4, p["scores"], p["step"], p["max_len"], p["n_live"], p["finished"], n, beam,
                                     V, 1, 3, 2, self.min_len, TEMPERATURE, UNK_PENALTY, p["cand_score"] + o4, p["cand_slot"] + o4, p["cand_token"] + o4, stream())
            if rc != 0:
                return rc
            rc = lib.l2s_beam_advance(p["cand_score"] + o4, p["cand_slot"] + o4, p["cand_token"] + o4, *[p[name] for name, _ in ADV_STATE], p["max_len"],
                                      p["emb"], self.d, p["pos_table"], EMBED_SCALE, p["x"], self.d, p["step"], p["n_active"], n, beam, L, V, self.d, 2, 1,
                                      1.0, 1, dtc(c["dt"]), stream())
            if rc != 0:
                return rc
            if self.snap is not None:
                torch.cuda.synchronize()
                self.snaps.append({name: self.snap[name].cpu() for name, _ in ADV_STATE})
        return 0

    snap = None

    def clip_out(self, outs, i):
        c = self.c
        beam, L, ns, K = c["beam"], c["L"], c["steps"], 2 * c["beam"]
        nsel = outs["n_live"].shape[1]
        out = [outs["att"].reshape(ns, nsel, -1)[:, i], outs["kc"].reshape(nsel, -1)[i], outs["vc"].reshape(nsel, -1)[i], outs["x"].reshape(nsel, -1)[i]]
        out += [outs[k].reshape(ns, nsel, K)[:, i] for k in ("cand_score", "cand_slot", "cand_token")]
        for name, _ in ADV_STATE:
            out.append(state_of_clip(outs[name], name, nsel, i))
        return out

    def judge(self, rep, outs):
        c, dt = self.c, self.c["dt"]
        beam, V, B, ns, K = c["beam"], c["V"], self.B, c["steps"], 2 * c["beam"]
        trace = self.reference(list(range(B)))
        att = outs["att"].double().numpy().reshape(ns, B, beam, self.W)
        exact = ("tokens", "anc", "n_live", "finished", "parents", "hyp_tokens", "hyp_len", "nhyp", "out_tokens", "out_len")
        for s, (ra, cs, cl, ct, fin, S) in enumerate(trace):
            eps = float(np.abs(sr.round16(ra, dt) - ra).max())
            rep.values(c, f"attention-{dt}", att[s], ra, np.where(ra == 0, 0.0, sc.ATTN_F * eps), f"step {s}: attention rows")
            gs = outs["cand_score"].reshape(ns, B, K)[s]
            for b in range(B):
                if fin[b]:
                    rep.same(c, f"step {s} clip {b} (finished): cand_slot untouched", outs["cand_slot"].reshape(ns, B, K)[s, b], canary(K, i32))
                    continue
                rep.same(c, f"step {s} clip {b}: cand_slot", outs["cand_slot"].reshape(ns, B, K)[s, b], torch.from_numpy(cl[b]))
                rep.same(c, f"step {s} clip {b}: cand_token", outs["cand_token"].reshape(ns, B, K)[s, b], torch.from_numpy(ct[b]))
                r64 = cs[b].astype(np.float64)
                fi = np.isfinite(r64)
                rep.values(c, "select-loop", gs[b].double().numpy(), r64, np.where(fi, (s + 1) * sr.select_tol(V, np.where(fi, r64, 0.0)), 0.0),
                           f"step {s} clip {b}: cand_score")
            snap = self.snaps_first[s]
            for name in exact:
                rep.same(c, f"after step {s}: {name}", snap[name].reshape(-1), torch.from_numpy(S[name]).reshape(-1))
            for name in ("scores", "hyp_score", "out_score"):
                g, w = snap[name].double().numpy().reshape(-1), S[name].astype(np.float64).reshape(-1)
                fi = np.isfinite(w)
                rep.values(c, "select-loop", g, w, np.where(fi, (s + 1) * sr.select_tol(V, np.where(fi, w, 0.0)), 0.0), f"after step {s}: {name}")
        rep.same(c, "k cache", outs["kc"], t16(self.kc_ref, dt).reshape(-1, self.W))
        rep.same(c, "v cache", outs["vc"], t16(self.vc_ref, dt).reshape(-1, self.W))


BUILD = {"kv": KvKase, "ba": BaKase, "va": VaKase, "wa": WaKase, "bs": BsKase, "bd": BdKase, "loop": LoopKase, "ct": CtKase}


# ---- one launch, checked ------------------------------------------------------------------------------------------------------------------------
def launch(rep, c, k, lib, sel, twice=True, snap=False):
    """runs the launch (twice into fresh buffers) -> (code, {output name: its window on the host})"""
    runs = []
    for i in range(2 if twice else 1):
        specs = OrderedDict((n, s) for n, s in k.specs(sel).items() if s is not None)
        host = {n: s.build() for n, s in specs.items()}
        dev = {n: h.cuda() for n, h in host.items()}
        if snap and i == 0:
            k.snap = {n: _Win(specs[n], dev[n]) for n, _ in ADV_STATE}
        rc = k.call(lib, {n: specs[n].ptr(dev[n]) for n in dev}, sel)
        torch.cuda.synchronize()
        if snap and i == 0:
            k.snaps_first, k.snap = k.snaps, None
        runs.append((rc, specs, host, {n: d.cpu() for n, d in dev.items()}))
    rc, specs, host, after = runs[0]
    tag = f"clips {sel if len(sel) < 8 else f'{sel[0]} .. {sel[-1]}'}"
    if rc != c["expect"] or runs[-1][0] != rc:
        rep.bad(c, f"{tag}: the launch answers {rc} (then {runs[-1][0]}), expected {c['expect']}")
    outs = {}
    for n, s in specs.items():
        b0, b1 = bits(host[n]), bits(after[n])
        if not s.out or rc != 0:
            if not torch.equal(b0, b1):
                i = (b0 != b1).nonzero()[0].item()
                rep.bad(c, f"{tag}: a refused launch wrote into {n} at element {i}" if rc != 0 else f"{tag}: operand {n} changed at element {i}")
            continue
        m = s.mask()
        if not torch.equal(b0[~m], b1[~m]):
            i = ((b0 != b1) & ~m).nonzero()[0].item()
            rep.bad(c, f"{tag}: {int((b0[~m] != b1[~m]).sum())} elements of {n} outside its window changed, first at element {i} of the buffer "
                       f"(the window starts at {s.guard}, {s.rows} rows of {s.cols} with stride {s.ld})")
        if twice and not getattr(s, "scratch", False) and not torch.equal(b1, bits(runs[1][3][n])):
            i = (b1 != bits(runs[1][3][n])).nonzero()[0].item()
            rep.bad(c, f"{tag}: {n}: two runs of the same launch give different bytes, first at element {i} of the buffer")
        outs[n] = s.window(after[n]).clone()
    return rc, outs


class _Win:
    def __init__(self, spec, dev):
        self.spec, self.dev = spec, dev

    def cpu(self):
        return self.spec.window(self.dev.cpu()).clone()


def run_case(c, lib, rep):
    k = BUILD[c["op"]](c)
    every = list(range(k.B))
    rc, first = launch(rep, c, k, lib, every, snap=c["op"] == "loop")
    if c["expect"] != 0:
        return
    if k.B > 1:
        for b in every:
            _, alone = launch(rep, c, k, lib, [b], twice=False)
            for j, (a, t) in enumerate(zip(k.clip_out(alone, 0), k.clip_out(first, b))):
                rep.same(c, f"clip {b} alone against its rows in the batch (output {j})", a, t)
    k.judge(rep, first)
    if c["op"] == "va":                                  # logits NULL: the same token and log-probability bytes, and the same workspace
        k.with_logits = False
        _, bare = launch(rep, c, k, lib, every, twice=False)
        for n in ("token", "logprob", "work"):
            rep.same(c, f"{n}: logits NULL against logits given", bare[n], first[n])


# ---- host-only mode -----------------------------------------------------------------------------------------------------------------------------
def host_reference(c):
    """builds the case and evaluates its reference and every condition on its inputs (AssertionError when one fails)"""
    k = BUILD[c["op"]](c)
    if c["expect"] == 0:
        sel = list(range(k.B))
        if c["op"] in ("wa", "bd", "loop"):
            k.reference(sel)
    return k


def cpu_ref(parts):
    for part in parts or list(sc.PARTS):
        t0, slow, n = time.time(), (0.0, ""), 0
        for c in sc.cases_of(part):
            t1 = time.time()
            host_reference(c)
            n += 1
            slow = max(slow, (time.time() - t1, c["name"]))
        print(f"CPUREF {part}: {n} cases, {time.time() - t0:.1f} s, slowest case {slow[1]} {slow[0]:.2f} s")


def main():
    args = sys.argv[1:]
    usage = f"usage: check_step_kernels.py <{' | '.join(sc.PARTS)}>  or  check_step_kernels.py --cpu-ref [part ...]"
    if not args or args[0] in ("-h", "--help"):
        sys.exit(usage)
    if args[0] == "--cpu-ref":
        if any(p not in sc.PARTS for p in args[1:]):
            sys.exit(usage)
        cpu_ref(args[1:])
        return
    part = args[0]
    if len(args) != 1 or part not in sc.PARTS:
        sys.exit(usage)
    lib = _lib.load()
    rep = Report(part)
    t0 = time.time()
    cases = sc.cases_of(part)
    spent, done = {}, 0
    try:
        for case in cases:
            t1 = time.time()
            run_case(case, lib, rep)
            done += 1
            spent[case["op"]] = spent.get(case["op"], 0.0) + time.time() - t1
    except Fail as e:
        print(e)
    print(f"part {part}: {done} of {len(cases)} cases passed, {time.time() - t0:.1f} s  (" + ", ".join(f"{op} {s:.1f} s" for op, s in spent.items()) + ")")
    for kind, (r, name) in sorted(rep.worst.items()):
        print(f"MEASURE {part} {kind} checks {rep.count[kind]} worst err / bound {r:.3f} ({name})")
    sys.exit(0 if done == len(cases) else 1)


if __name__ == "__main__":
    main()
