#!/usr/bin/env python3
"""Runs one part of the tap-GEMM instantiation matrix (tests/_tapgemm_cases.py): a generic tile forced by L2S_FORCE_TILE,

    L2S_FORCE_TILE=<tile> L2S_PHASEGEMM=0 L2S_NO_PATCHCONV=1 check_tapgemm_matrix.py families|schedule|band

or the phase-staggered kernel (256256) / the LDS-patch kernel (999064, 999128) under the switches of tc.PART_ENV[part],

    L2S_PHASEGEMM=2 [L2S_PHASE_SLOTS=2] check_tapgemm_matrix.py phase-families|phase-walk|phase-natural 256256
    L2S_PATCH_MIN_M=1 L2S_PHASEGEMM=0 [L2S_PATCH_SLOTS=4] check_tapgemm_matrix.py patch-families|patch-walk|patch-natural 999064

With --route in front of the part only the dispatch is checked (every launch of every case is routed to the kernel and the
epilogue family the case claims): no device needed.
The library reads these switches once per process, hence one child process per (tile, part): tests/test_tapgemm_matrix_gpu.py.
Every case runs on operands that are views into NaN-filled device buffers (guard rows around A / C / C2 / R, NaN in the padding
columns of the leading dimensions, a NaN guard behind W) and is checked for: no NaN inside the written window, every byte outside
it unchanged, masked rows exactly zero, and two error criteria against the oracle op in fp64 on the CPU -
  (a) max error <= TOL * max|ref| (the criterion of tests/test_tapgemm_gpu.py), every case;
  (b) |got - ref| <= FU u |ref| + FK (Ktot + 8) 2^-24 S + 2^-24 per element, the cases whose activation is none / relu / prelu /
      lrelu (fp32 accumulation, one rounding to the output type; u = 2^-11 f16, 2^-8 bf16, 0 for fp32 outputs;
      S = |alpha| (|A| |W|^T + |bias|) + |R| + |prev| in fp64).
Prints the worst err / bound per (type, family) for both criteria and exits non-zero on any failure."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from lip2speech_unit_amd import _lib, ops  # noqa: E402
from lip2speech_unit_amd.packing import convtranspose_phases  # noqa: E402
from tests import _tapgemm_cases as tc  # noqa: E402

TOL = {"f16": 2e-3, "bf16": 1.5e-2}          # (a): TOL of tests/test_tapgemm_gpu.py
U16 = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
FU, FK, ABS = 1.5, 4.0, 2.0 ** -24           # (b): margins over the half-ulp and gamma_K bounds; f16 subnormal step
GENERIC_PARTS = ("families", "schedule", "band")   # on a forced generic tile; every other part names its kernel and switches
GUARD = 4                                    # guard rows (keeps every window 16-byte aligned: leading dimensions are 4 | ld)
NAN = float("nan")
f64 = torch.float64


def t16(dt):
    return torch.float16 if dt == "f16" else torch.bfloat16


def rnd(x, dt):
    return x.to(t16(dt)).to(f64)


# ---- operands and the oracle op in fp64 (shared by every epilogue of one geometry) ------------------------------------------------
_operand_cache = {}


def oracle(g, A, W):
    """fp64 result [rows_out, groups, N] of the op the geometry stands for; A [rows_in, a_cols], W [groups, N, Ktot]."""
    G, N, Cin = g["groups"], g["N"], g["Cin"]
    outs = []
    for grp in range(G):
        a = A[:, grp * g["a_gstride"]: grp * g["a_gstride"] + Cin]
        w = W[grp]
        if g["kind"] == "linear":
            y = F.linear(a, w)
        elif g["kind"] == "conv1d":
            x = a.reshape(g["B"], g["T"], Cin).permute(0, 2, 1)
            wc = w.reshape(N, g["k"], Cin).permute(0, 2, 1)
            right = (g["k"] - 1) * g["dil"] + g["off"]
            if right != -g["off"]:                                   # even k: taps off .. off + (k - 1) dil around frame t
                x, pad = F.pad(x, (-g["off"], right)), 0
            else:
                pad = -g["off"]
            y = F.conv1d(x, wc, None, 1, pad, g["dil"]).permute(0, 2, 1).reshape(-1, N)[: g["M"]]
        elif g["kind"] == "conv2d":
            H = g["H"]
            x = a.reshape(g["nimg"], H, g.get("Wi", H), Cin).permute(0, 3, 1, 2)
            wc = w.reshape(N, 3, 3, Cin).permute(0, 3, 1, 2)
            y = F.conv2d(x, wc, None, g["stride"], 1).permute(0, 2, 3, 1).reshape(-1, N)[: g["M"]]
        else:  # convt: W holds the ConvTranspose1d weight [Cin, N, k]
            x = a.reshape(g["B"], g["T"], Cin).permute(0, 2, 1)
            y = F.conv_transpose1d(x, w, None, g["s"], g["p"]).permute(0, 2, 1).reshape(-1, N)
        outs.append(y)
    return torch.stack(outs, 1).contiguous()


def operands(case):
    g, dt = case["geom"], case["dt"]
    key = (dt, id(g))
    if key in _operand_cache:
        return _operand_cache[key]
    _operand_cache.clear()                   # geometries come in runs: keep one
    gen = torch.Generator().manual_seed(1000 * g["M"] + 10 * g["N"] + g["Cin"] + len(dt))
    G, N, Cin = g["groups"], g["N"], g["Cin"]
    rows_in = {"linear": g["M"], "conv1d": g.get("B", 0) * g.get("T", 0), "convt": g.get("B", 0) * g.get("T", 0),
               "conv2d": g.get("nimg", 0) * g.get("H", 0) * g.get("Wi", g.get("H", 0))}[g["kind"]]
    A = rnd(torch.randn(rows_in, g["a_cols"], generator=gen, dtype=f64), dt)
    if g["kind"] == "convt":
        fan = Cin * g["k"] / g["s"]
        W = rnd(torch.randn(1, Cin, N, g["k"], generator=gen, dtype=f64) / fan ** 0.5, dt)
    else:
        Ktot = Cin * g["ntaps"]
        W = rnd(torch.randn(G, N, Ktot, generator=gen, dtype=f64) / Ktot ** 0.5, dt)
    acc = oracle(g, A, W)
    sabs = oracle(g, A.abs(), W.abs())
    rows_out = acc.shape[0]
    o = dict(A=A, W=W, acc=acc, sabs=sabs, rows_out=rows_out,
             bias=torch.randn(G * N, generator=gen).to(f64),                      # fp32 values
             slope=(torch.rand(G * N, generator=gen) * 0.3).to(f64),
             R=torch.randn(rows_out, G, N, generator=gen).to(f64),                # fp32 values; rounded again for a 16-bit R
             prev=torch.randn(rows_out, G, N, generator=gen).to(f64))
    _operand_cache[key] = o
    return o


def act_ref(v, act, slope):
    if act == tc.ACT_RELU:
        return v.clamp(min=0)
    if act == tc.ACT_GELU:
        return F.gelu(v)
    if act == tc.ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == tc.ACT_PRELU:
        return torch.where(v >= 0, v, v * slope)
    if act == tc.ACT_LRELU:
        return torch.where(v >= 0, v, v * float(torch.tensor(tc.ACT_SLOPE, dtype=torch.float32)))
    if act == tc.ACT_TANH:
        return torch.tanh(v)
    return v


def reference(case, o):
    """(ref, ref2 = the DUAL copy, S, keep [rows_out], R, prev) in fp64, [rows_out, G, N]: the epilogue in the order
    include/lip2speech_hip.h states - alpha (acc + bias), R before the activation, activation, R after it, previous C, row mask."""
    g, e, dt = case["geom"], case["epi"], case["dt"]
    G, N = g["groups"], g["N"]
    bias, slope = o["bias"].view(1, G, N), o["slope"].view(1, G, N)
    R = o["R"] if e["res"] == "32" else rnd(o["R"], dt)
    prev = o["prev"] if e["out32"] else rnd(o["prev"], dt)
    v = e["alpha"] * (o["acc"] + bias)
    S = abs(e["alpha"]) * (o["sabs"] + bias.abs())
    if e["res"] and e["when"] == "pre":
        v = v + R
    v = act_ref(v, e["act"], slope)
    if e["res"] and e["when"] == "post":
        v = v + R
    if e["res"]:
        S = S + R.abs()
    if e["accum"]:
        v = v + prev
        S = S + prev.abs()
    keep = torch.ones(o["rows_out"], dtype=torch.bool)
    if e["mask"]:
        T = g["mask_T"]
        rows = torch.arange(o["rows_out"])
        keep = (rows % T) < torch.tensor(tc.mask_lens(case))[rows // T]
        v = v * keep.view(-1, 1, 1)
    s2 = float(torch.tensor(tc.SLOPE2, dtype=torch.float32))
    return v, torch.where(v >= 0, v, v * s2), S, keep, R, prev


# ---- guarded device buffers -------------------------------------------------------------------------------------------------------
def guarded(rows, ld, dtype, guard=GUARD):
    """NaN-filled host buffer [guard + rows + guard, ld] and the row offset of its window."""
    return torch.full((rows + 2 * guard, ld), NAN, dtype=dtype), guard


def scatter_cols(buf, g0, vals, G, gstride):
    """vals [rows, G, N] -> buf rows g0.., columns grp * gstride + n."""
    rows, _, N = vals.shape
    for grp in range(G):
        buf[g0: g0 + rows, grp * gstride: grp * gstride + N] = vals[:, grp].to(buf.dtype)


def gather_cols(buf, g0, rows, G, gstride, N):
    return torch.stack([buf[g0: g0 + rows, grp * gstride: grp * gstride + N] for grp in range(G)], 1)


def bits(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def bound_b(ref, S, Ktot, dt, is32):
    """Element-wise bound of criterion (b): one rounding to the output type on top of an fp32 accumulation of Ktot products."""
    return (0.0 if is32 else FU * U16[dt]) * ref.abs() + FK * (Ktot + 8) * 2.0 ** -24 * S + ABS


class Report:
    def __init__(self, tile):
        self.tile, self.fail, self.worst = tile, [], {}

    def ratio(self, case, crit, r):
        k = (case["inst"] if "inst" in case else (case["dt"], case["family"]), crit)
        self.worst[k] = max(self.worst.get(k, 0.0), r)

    def bad(self, case, why):
        self.fail.append(f"FAIL tile={self.tile} type={case['dt']} mode={case['mode']}{'u' if case['uni'] else ''} "
                         f"family={case['family']} case={case['name']}: {why}")


def run_case(case, lib, tile, rep):
    g, e, dt = case["geom"], case["epi"], case["dt"]
    descs = tc.descriptors(case)
    o = operands(case)
    G, N, rows_out = g["groups"], g["N"], o["rows_out"]
    ref, ref2, S, keep, R, prev = reference(case, o)
    el = t16(dt)
    out_t = torch.float32 if e["out32"] else el

    hA, a0 = guarded(o["A"].shape[0], g["lda"], el)
    hA[a0: a0 + o["A"].shape[0], : g["a_cols"]] = o["A"].to(el)
    dA = hA.cuda()
    hC, c0 = guarded(rows_out, g["ldc"], out_t)
    if e["accum"]:
        scatter_cols(hC, c0, prev, G, g["c_gstride"])
    if e["inplace"]:
        scatter_cols(hC, c0, R, G, g["c_gstride"])
    dC = hC.cuda()
    dR = hR = None
    if e["res"] and not e["inplace"]:
        hR, r0 = guarded(rows_out, descs[0]["ldr"], torch.float32 if e["res"] == "32" else el)
        scatter_cols(hR, r0, R, G, g["c_gstride"])
        dR = hR.cuda()
    dC2 = hC2 = None
    c20 = GUARD - 1 if g["c2_skew"] else GUARD          # an odd row offset at ldc2 % 8 == 4: C2 is 8- but not 16-byte aligned
    if e["dual"]:
        hC2, _ = guarded(rows_out, g["ldc2"], el)
        dC2 = hC2.cuda()
    dbias = o["bias"].float().cuda()
    dslope = o["slope"].float().cuda() if e["act"] == tc.ACT_PRELU else None
    dlens = torch.tensor(tc.mask_lens(case), dtype=torch.int32).cuda() if e["mask"] else None

    if g["kind"] == "convt":
        phases = convtranspose_phases(o["W"][0], g["s"], g["p"])
        assert [(p["r"], p["off"], p["ntaps"]) for p in phases] == [(p["r"], p["off"], p["ntaps"]) for p in g["phases"]]
        weights = [p["w"] for p in phases]
    else:
        weights = [o["W"]]

    written = torch.zeros(hC.shape, dtype=torch.bool)
    before, before2 = hC, hC2
    for d, w in zip(descs, weights):
        hW = torch.cat([w.reshape(-1).to(el), torch.full((512,), NAN, dtype=el)])
        dW = hW.cuda()
        gd = _lib.GemmDesc(**d)
        var, fam = lib.l2s_tapgemm_variant(ctypes.byref(gd)), lib.l2s_tapgemm_epilogue_family(ctypes.byref(gd))
        if var != tile or fam != case["family"]:
            rep.bad(case, f"instantiation: variant {var} family {fam}")
            return
        kw = {k: v for k, v in d.items() if k not in ("dtype", "flags")}
        ops.tapgemm(dA[a0:], dW, dC[c0:], bias=dbias, slope=dslope, lens=dlens,
                    R=(dC[c0:] if e["inplace"] else (dR[GUARD:] if dR is not None else None)),
                    C2=dC2[c20:] if dC2 is not None else None,
                    flags=d["flags"], dtype=d["dtype"], **kw)
        torch.cuda.synchronize()
        # this launch's window: rows m * out_row_mul + out_row_add, columns grp * c_gstride + [0, N)
        win = torch.zeros(hC.shape, dtype=torch.bool)
        rows = c0 + torch.arange(g["M"]) * d["out_row_mul"] + d["out_row_add"]
        for grp in range(G):
            win[rows, grp * g["c_gstride"]: grp * g["c_gstride"] + N] = True
        written |= win
        after = dC.cpu()
        stray = (bits(after) != bits(before)) & ~win
        if stray.any():
            rep.bad(case, f"{stray.sum().item()} elements of C outside the window changed (out_row_add {d['out_row_add']})")
        before = after
        if dC2 is not None:
            after2 = dC2.cpu()
            win2 = torch.zeros(hC2.shape, dtype=torch.bool)
            for grp in range(G):
                win2[rows - c0 + c20, grp * g["c_gstride"]: grp * g["c_gstride"] + N] = True
            if ((bits(after2) != bits(before2)) & ~win2).any():
                rep.bad(case, "elements of C2 outside the window changed")
            before2 = after2
    for name, dev, host in (("A", dA, hA), ("R", dR, hR)):
        if dev is not None and not torch.equal(bits(dev.cpu()), bits(host)):
            rep.bad(case, f"operand {name} changed")

    full = bool(written[c0: c0 + rows_out].reshape(-1).sum().item() == rows_out * G * N)
    if not full:
        rep.bad(case, "the launches do not cover the output")
        return
    outs = [("C", gather_cols(before, c0, rows_out, G, g["c_gstride"], N), ref, e["out32"])]
    if e["dual"]:
        outs.append(("C2", gather_cols(before2, c20, rows_out, G, g["c_gstride"], N), ref2, False))
    Ktot = g["Cin"] * max(d["ntaps"] for d in descs)
    for name, got, rf, is32 in outs:
        if torch.isnan(got).any():
            rep.bad(case, f"{torch.isnan(got).sum().item()} NaN in the window of {name}")
            continue
        got = got.to(f64)
        if e["mask"] and bool((got[~keep] != 0).any()):
            rep.bad(case, f"masked rows of {name} are not exactly zero")
        err = (got - rf).abs()
        ra = err.max().item() / (TOL[dt] * (rf.abs().max().item() + 1e-6))
        rep.ratio(case, "a", ra)
        if ra > 1.0:
            rep.bad(case, f"(a) {name}: max err / (tol max|ref|) = {ra:.3f}")
        if e["act"] in tc.LIN_ACTS:
            q = err / bound_b(rf, S, Ktot, dt, is32)
            rb = q.max().item()
            rep.ratio(case, "b", rb)
            if rb > 1.0:
                i = q.reshape(-1).argmax().item()
                rep.bad(case, f"(b) {name}: err / bound = {rb:.3f} at flat index {i} (got {got.reshape(-1)[i].item():.9g}, "
                              f"ref {rf.reshape(-1)[i].item():.9g}, {(q > 1).sum().item()} elements over)")


def route(part, kernel, lib):
    """Dispatch only: how many launches of the part's cases are NOT routed to the kernel / epilogue family they claim."""
    bad = n = 0
    for case in tc.cases_of(part, kernel):
        for d in tc.descriptors(case):
            gd = _lib.GemmDesc(**d)
            got = (lib.l2s_tapgemm_variant(ctypes.byref(gd)), lib.l2s_tapgemm_epilogue_family(ctypes.byref(gd)))
            n += 1
            if got != (kernel, case["family"]):
                bad += 1
                print(f"ROUTE {part} {case['dt']} {case['name']}: variant {got[0]} family {got[1]}")
    print(f"routed {n - bad} of {n} launches of {part} to {kernel}")
    if part == "phase-families":            # what the kernel must decline although forced: served by a generic tile
        for case in tc.phase_declined_cases():
            for d in tc.descriptors(case):
                var = lib.l2s_tapgemm_variant(ctypes.byref(_lib.GemmDesc(**d)))
                if var not in tc.TILES:
                    bad += 1
                    print(f"ROUTE {part} {case['dt']} {case['name']}: variant {var}, a generic tile expected")
    return bad


def main():
    args = sys.argv[1:]
    route_only = args[0] == "--route"
    part = args[1] if route_only else args[0]
    if part not in GENERIC_PARTS:
        tile = int(args[-1])
        for name in tc.SWITCHES:            # the kernel under test, its grid and its threshold: exactly the part's switches
            assert os.environ.get(name) == tc.PART_ENV[part].get(name), (name, os.environ.get(name))
    else:
        tile = int(os.environ["L2S_FORCE_TILE"])
        assert os.environ.get("L2S_PHASEGEMM") == "0" and os.environ.get("L2S_NO_PATCHCONV") == "1", "generic kernel only"
        if part == "band":
            assert os.environ.get("L2S_BAND") == str(tc.BAND)
    lib = _lib.load()
    if route_only:
        sys.exit(1 if route(part, tile, lib) else 0)
    rep = Report(tile)
    t0 = time.time()
    cases = tc.cases_of(part, tile)
    for case in cases:
        run_case(case, lib, tile, rep)
    dt_s = time.time() - t0
    print(f"tile {tile} part {part}: {len(cases)} cases, {len(rep.fail)} failures, {dt_s:.1f} s")
    if part not in GENERIC_PARTS:                 # one line per instantiation: (type, mode, EPI) / (type, mode, CH, EPI)
        for inst in sorted({k for k, _ in rep.worst}):
            a, b = rep.worst.get((inst, "a")), rep.worst.get((inst, "b"))
            print(f"RATIO {tile} {part} " + " ".join(str(x) for x in inst) + f" (a) {a:5.3f} (b) " + ("    -" if b is None else f"{b:5.3f}"))
    else:
        print("worst err/bound   " + "  ".join(f"fam{f}" for f in range(10)))
        for dt in tc.DTYPES:
            for crit in "ab":
                cells = [rep.worst.get(((dt, f), crit)) for f in range(10)]
                print(f"RATIO {tile} {part} {dt:4s} ({crit}) " + " ".join("    -" if c is None else f"{c:5.3f}" for c in cells))
    for line in rep.fail:
        print(line)
    sys.exit(1 if rep.fail else 0)


if __name__ == "__main__":
    main()
