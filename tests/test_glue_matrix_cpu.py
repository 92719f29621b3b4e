"""The unit decoders' and layout / cast kernels' matrix, host side: the case lists of tests/_glue_cases.py reach every kernel
instantiation with the shapes, edges and refusals they claim; exactly one case per capped kernel and type passes the 8192 x 256 work
items of the capped grid, by no more than a row; the coded beams are what both the fp64 restatement and oracle/decode.py rank in
binary-expansion order; the random beams keep three quarters of their ranks; the cast data tell round-to-nearest-even from truncation
and from round-half-away; the saturated conv_post reference is saturated; every reference runs.  Nothing here needs a device."""
import importlib.util
import math
import os
import re
import subprocess
import sys

from tests import _glue_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_glue_kernels.py")
CSRC = os.path.join(ROOT, "lip2speech_unit_amd", "csrc")
_DRV = []


def _driver():
    if not _DRV:
        spec = importlib.util.spec_from_file_location("check_glue_kernels", TOOL)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _DRV.append(mod)
    return _DRV[0]


def _cases(op=None, ok=None):
    return [c for _, c in gc.all_cases() if (op is None or c["op"] == op) and (ok is None or (c["expect"] == 0) == ok)]


def test_constants_match_the_sources():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    for name, val in (("L2S_EINVAL", gc.EINVAL), ("L2S_ESHAPE", gc.ESHAPE), ("L2S_EALIGN", gc.EALIGN), ("L2S_EUNSUPPORTED", gc.EUNSUPPORTED)):
        assert f"{name} = {val}" in hdr
    misc = open(os.path.join(CSRC, "misc.hip")).read()
    assert "return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));" in misc and misc.count("grid_for(") == 10      # its definition and nine launchers
    assert (gc.GRID_CAP, gc.GRID_BLOCK, gc.CAP_ITEMS) == (8192, 256, 2097152)
    assert gc.grid_for(0) == 1 and gc.grid_for(1) == 1 and gc.grid_for(gc.CAP_ITEMS) == 8192 == gc.grid_for(gc.CAP_ITEMS + 1)
    assert not gc.takes_stride_loop(gc.CAP_ITEMS) and gc.takes_stride_loop(gc.CAP_ITEMS + 1)
    assert "constexpr int CP_TILE = 256;" in misc and "(CP_TILE + k - 1) * (C + 1) + (size_t)k * C) * sizeof(float)" in misc
    # the entry points whose f32 dtype goes to l2s_f32_rows, and those that refuse it through DISPATCH_ET
    routed = {body.split("(")[0] for body in misc.split('extern "C" int l2s_')[1:] if "l2s_f32_rows(" in body}
    assert routed == {"repeat2_cast", "cast_f32_to_16", "cast_16_to_f32", "broadcast_rows", "rows_f32_to_16_masked"}
    assert set(gc.F32_ROUTED) == {"repeat2", "cast16", "cast32", "bcast", "rows16"} and set(gc.F32_REFUSED) == {"transpose", "embedding", "embtok", "split"}
    for k, f in gc.CPU_F32_WORST.items():
        assert gc.F_of(k) == max(8.0, 8.0 * f)
    assert set(gc.CPU_F32_WORST) == {"split-gelu", "convpost", "greedy-lprob", "greedy-score", "beam-pos", "beam-score", "ctc-lp"}
    assert gc.TOL_ABS == {"convpost": 2e-5, "greedy": 1e-4, "beam": 1e-4} and gc.DELTA == 2.0 ** -6 and gc.SKIP_CAP == 0.25
    assert (gc.CANARY32, gc.CANARY16, gc.GUARD) == (0x5A5A5A5A, 0x5A5A, 3)


def test_names_are_unique_and_every_instantiation_is_reached():
    names = [(c["dt"], c["name"]) for c in _cases()]
    assert len(names) == len(set(names))
    assert {p for p, _ in gc.all_cases()} == set(gc.PARTS)
    inst = gc.instantiations()
    assert len(inst) == len(set(inst)) == 10 + 2 * (7 + 2 + 3)
    launched = [c["inst"] for c in _cases(ok=True)]
    assert set(launched) == set(inst)
    for i in inst:
        assert launched.count(i) >= 3, i
    # both template arguments of broadcast_rows_kernel, the three ACTs, both conv_post kernels, both f32 row kernels
    for dt in gc.DTYPES:
        assert {i[2] for i in launched if i[:2] == ("broadcast_rows_kernel", dt)} == {True, False}
        assert {i[2] for i in launched if i[:2] == ("split_hi_lo_kernel", dt)} == {0, 1, 2}
    assert {i[0] for i in launched if i[0].startswith("conv_post")} == {"conv_post_kernel", "conv_post16_kernel"}
    assert {i[2] for i in launched if i[0] == "rows_f32_kernel"} == {True, False}
    # l2s_f32_rows is reached through all four entry points the issue names (and cast_16_to_f32)
    assert {c["op"] for c in _cases(ok=True) if c["inst"][0] == "rows_f32_kernel"} == set(gc.F32_ROUTED)
    # the kernels of the sources are the kernels of the list
    kernels = set()
    for f, pick in (("misc.hip", None), ("decode.hip", None), ("f32_kernels.hip", {"rows_f32_kernel"}), ("ctc.hip", {"ctc_frames_kernel", "ctc_repeat_kernel"})):
        found = set(re.findall(r"__global__(?: __launch_bounds__\(\d+\))? void (\w+)\(", open(os.path.join(CSRC, f)).read()))
        kernels |= found if pick is None else found & pick
    assert kernels == {k for i in inst for k in i[0].split("+")}


def test_refusals():
    want = {("repeat2", gc.EALIGN), ("rows16", gc.EALIGN), ("rows16", gc.ESHAPE), ("bcast", gc.EINVAL), ("transpose", gc.EINVAL), ("embedding", gc.EINVAL),
            ("embedding", gc.EALIGN), ("embtok", gc.EINVAL), ("embtok", gc.ESHAPE), ("split", gc.ESHAPE), ("split", gc.EALIGN), ("split", gc.EINVAL),
            ("convpost", gc.EUNSUPPORTED), ("convpost", gc.ESHAPE), ("greedy", gc.ESHAPE), ("greedy", gc.EINVAL), ("beam", gc.EUNSUPPORTED),
            ("beam", gc.ESHAPE), ("ctcframes", gc.EUNSUPPORTED), ("ctcframes", gc.ESHAPE)}
    assert {(c["op"], c["expect"]) for c in _cases(ok=False)} == want
    ref = {c["name"].split("/")[1]: c for c in _cases(ok=False)}
    assert ref["refused-C6"]["C"] == 6 and ref["refused-col2"]["col0"] == 2 and ref["refused-ldx-odd"]["ldx"] % 2 == 1 and ref["refused-mul0"]["len_mul"] == 0
    assert ref["refused-f32-with-v16"]["dt"] == "f32" and ref["refused-f32-with-v16"]["v32"] is False
    assert ref["refused-C12"]["C"] == 12 and ref["refused-ldt-below-L"]["ldt"] < ref["refused-ldt-below-L"]["L"]
    assert ref["refused-act3"]["act"] == 3 and ref["refused-C60-k7"]["expect"] == gc.EUNSUPPORTED and ref["refused-k4"]["k"] % 2 == 0
    assert ref["refused-V4"]["V"] == 4 and ref["refused-ldl-below-V"]["ldl"] < ref["refused-ldl-below-V"]["V"] and ref["refused-temperature-0"]["temp"] == 0.0
    assert gc.greedy_lens(ref["refused-len_mul-0"]["lens"], 2, 6)[1] == 0
    assert ref["refused-V257"]["V"] == 257 and ref["refused-beam65"]["beam"] == 65
    for n in ("refused-beam-V-3", "refused-beam-V-3-small"):
        assert ref[n]["beam"] == ref[n]["V"] - 3 <= 64 and ref[n]["V"] <= 256
    assert ref["refused-workspace-one-byte-short"]["ws_short"] == 1 and ref["refused-workspace-misaligned-by-2"]["ws_off"] == 2
    assert ref["refused-V4097"]["V"] == 4097 and (ref["refused-K65"]["K"], ref["refused-K65"]["V"]) == (65, 4096) and ref["refused-K-above-V"]["K"] > ref["refused-K-above-V"]["V"]
    assert {c["dt"] for c in _cases(ok=False) if c["op"] in gc.F32_REFUSED and c["expect"] == gc.EINVAL} == {"f32"}


def test_grid_cap():
    """Every capped kernel, in every type it has: exactly one case past 8192 x 256 work items - and with one row less it is not - and cases
    below it."""
    keys = {i[:2] for i in gc.instantiations() if i[0] in gc.CAPPED}
    assert len(keys) == 2 * 8 + 2
    for key in keys:
        mine = [c for c in _cases(ok=True) if c["inst"][:2] == key]
        past = [c for c in mine if gc.takes_stride_loop(gc.items_of(c))]
        assert len(past) == 1 and len(mine) - len(past) >= 1, (key, [c["name"] for c in past])
        c = past[0]
        assert "cap" in c["name"] and gc.grid_for(gc.items_of(c)) == 8192 and gc.one_row_less(c) <= gc.CAP_ITEMS < gc.items_of(c), c["name"]
    assert all(("cap" in c["name"]) == gc.takes_stride_loop(gc.items_of(c)) for c in _cases(ok=True) if c["inst"][0] in gc.CAPPED)
    by = {(c["dt"], c["name"]): c for c in _cases()}
    assert gc.items_of(by[("f16", "cast16/coded-2049x1024-cap")]) == 2049 * 1024 and gc.items_of(by[("bf16", "repeat2/cap-rows8193-C1024")]) == 8193 * 256
    assert gc.items_of(by[("f16", "bcast/v16-cap-B2-T1025-C1024")]) == 2 * 1025 * 1024 and gc.items_of(by[("-", "splitk/cap-S2-N1024-M8193")]) == 8193 * 256


def test_case_lists_hold_what_the_issue_lists():
    for dt in gc.DTYPES:
        ok = [c for c in _cases(ok=True) if c["dt"] == dt]
        sel = lambda op: [c for c in ok if c["op"] == op]
        assert {(c["M"], c["C"]) for c in sel("cast16")} == {(1, 1), (3, 7), (37, 80), (2049, 1024)}
        assert any(c["ldx"] > c["C"] and c["ldy"] > c["C"] for c in sel("cast16")) and (64, 1024, 1032) in {(c["M"], c["C"], c["ldx"]) for c in sel("cast32")}
        assert {c["C"] for c in sel("repeat2")} == {4, 12, 512, 1024} and {(c["B"], c["T"]) for c in sel("repeat2")} == {(1, 1), (3, 13), (1, 8193)}
        r16 = sel("rows16")
        assert {c["C"] for c in r16} == {4, 80, 1024} and {c["col0"] for c in r16} == {0, 4, 128} and {c["len_mul"] for c in r16} == {1, 4}
        assert {c["lens"] for c in r16} == {"none", "mixed"} and all(c["ldx"] > c["C"] and c["ldy"] > c["C"] + c["col0"] for c in r16 if "cap" not in c["name"])
        bc = sel("bcast")
        assert {c["C"] for c in bc} == {1, 7, 128, 1024} and {c["col0"] for c in bc} == {3, 0, 4} and {c["T"] for c in bc} == {1, 33, 1025}
        assert {c["v32"] for c in bc} == {True, False} and all(c["ldv"] > c["C"] for c in bc if "cap" not in c["name"])
        tr = sel("transpose")
        assert {(c["C"], c["T"]) for c in tr} == {(80, 13), (32, 32), (33, 31), (1, 1), (31, 65)} and {c["col0"] for c in tr} == {0, 5} and {c["B"] for c in tr} == {3}
        em, et = sel("embedding"), sel("embtok")
        assert {c["C"] for c in em} == {8, 128, 1024} and {c["lens"] for c in em} == {"none", "mixed"} and all(c["ldy"] > c["C"] for c in em if "cap" not in c["name"])
        assert {c["off"] for c in et} == {0, 4} and {c["len_mul"] for c in et} == {1, 2} and all(c["ldt"] > c["L"] for c in et)
        sp = sel("split")
        assert {c["act"] for c in sp} == {0, 1, 2} and {c["C"] for c in sp} == {4, 64, 1024} and {c["len_mul"] for c in sp} == {1, 4}
        assert all(c["ldx"] > c["C"] and c["ld16"] > c["C"] for c in sp if c["C"] != 1024) and gc.SLOPE == 0.1
    for T in (1, 13, 33, 200):                            # the ragged lengths: a clip of length 0, one past T, one inside
        for m in (1, 2, 4):
            ln = gc.lens_of(5, T, m)
            assert ln[0] == 0 and ln[1] * m > T and 0 < ln[2] * m and ln[3] * m >= T
    ok = _cases(ok=True)
    lm = [c for c in ok if c["op"] == "lensmask"]
    assert {c["T"] for c in lm} == {1, 63, 64, 65, 200} and {c["B"] for c in lm} == {5} and {c["mask"] for c in lm} == {True, False}
    sk = [c for c in ok if c["op"] == "splitk"]
    assert {c["S"] for c in sk} == {1, 2, 8} and {c["N"] for c in sk} == {4, 64, 1024} and {c["M"] for c in sk} == {1, 37, 8193}
    assert all(c["ldp"] > c["S"] * c["N"] and c["ldx"] > c["N"] for c in sk if "cap" not in c["name"]) and any(c["data"] == "order" for c in sk)
    cp = [c for c in ok if c["op"] == "convpost"]
    assert {(c["C"], c["k"], c["xoff"]) for c in cp} == {(16, 7, 0), (16, 7, 1), (16, 5, 0), (32, 7, 0), (1, 1, 0), (59, 7, 0)}
    for shape in gc.CONVPOST_SHAPES:
        assert {c["T"] for c in cp if (c["C"], c["k"], c["xoff"]) == shape} >= {1, 3, 255, 256, 257, 700}
    assert {c["lens"] for c in cp} == {"none", "mixed"} and {c["len_mul"] for c in cp} == {1, 2} and {c["pcm"] for c in cp} == {True, False}
    assert {c["xoff"] for c in cp if c["data"] == "saturated"} == {0, 1}
    assert gc.convpost_smem(59, 7) <= 64 * 1024 < gc.convpost_smem(60, 7)
    cf = [c for c in ok if c["op"] == "ctcframes"]
    assert {c["V"] for c in cf} == {2, 63, 64, 65, 4095, 4096} and {c["L"] for c in cf} == {5} and all(c["ldl"] > c["V"] for c in cf)
    for V in gc.CTC_V:
        assert {c["K"] for c in cf if c["V"] == V} == {0, 1, min(V, 64)}
    assert {c["lens"] for c in cf} == {"none", "mixed"}
    cr = [c for c in ok if c["op"] == "ctcrepeat"]
    assert {c["L"] for c in cr} == {1, 63, 64, 65, 129, 200} and {c["inplace"] for c in cr} == {True, False} and {c["len_mul"] for c in cr} == {1, 2}
    assert all(c["ldx"] > c["L"] and c["ldy"] > c["L"] for c in cr) and any(c["inplace"] and c["L"] == 200 for c in cr) and any(c["inplace"] and c["L"] > 64 and c["lens"] == "mixed" for c in cr)


def test_decoder_edges():
    gr = _cases("greedy", ok=True)
    assert {c["V"] for c in gr} == {5, 63, 64, 65, 204, 256, 257, 1004} and {c["T2"] for c in gr} == {1, 2, 3, 4, 62, 63, 64, 65, 130}
    assert len(gr) == 72 and {c["B"] for c in gr} == {4}
    for V in gc.GREEDY_V:
        mine = [c for c in gr if c["V"] == V]
        assert {c["T2"] for c in mine} == set(gc.GREEDY_T2)
    assert {c["temp"] for c in gr} == {0.5, 1.0, 1.3} and {c["lenpen"] for c in gr} == {0.0, 1.0, 1.7} and {c["ldl"] - c["V"] for c in gr} == {0, 3}
    assert {c["lens"] for c in gr} == set(gc.GREEDY_LENS)
    Ls = [L for c in gr for L in gc.greedy_lens(c["lens"], c["B"], c["T2"])[2]]
    assert {64, 65} <= {L + 1 for L in Ls} and 0 in Ls and {(c["T2"] + 1) % 4 for c in gr} == {0, 1, 2, 3}
    assert any(L + 1 > 128 for L in Ls)                   # a third trip of the score loop
    for T2 in (4, 63, 130):
        lens, mul, L = gc.greedy_lens("clamp", 4, T2)
        assert any(n * mul > T2 for n in lens) and max(L) == T2
        lens, mul, L = gc.greedy_lens("mul2", 4, T2)
        assert mul == 2 and any(n * mul > T2 for n in lens) and L == [min(2 * n, T2) for n in lens]
        assert gc.greedy_lens("zero-first", 4, T2)[2][0] == 0 and gc.greedy_lens("none", 4, T2)[0] is None
    bm = _cases("beam", ok=True)
    assert {c["beam"] for c in bm} == {1, 2, 5, 50, 64} and {c["V"] for c in bm} == {5, 68, 204, 256}
    assert any(c["V"] == 256 and c["beam"] == 64 for c in bm) and any(c["beam"] == c["V"] - 4 == 64 for c in bm) and all(c["beam"] == 1 for c in bm if c["V"] == 5)
    for data in ("coded", "random"):
        assert any(c["V"] == 256 for c in bm if c["data"] == data) and any(c["beam"] == c["V"] - 4 for c in bm if c["data"] == data)
    assert {L for c in bm if c["data"] == "coded" for L in c["Ls"]} >= {0, 1, 2, 63, 64, 65, 130}
    assert {c["lens"] for c in bm} == {"lens", "none", "clamp"} and {c["len_mul"] for c in bm} == {1, 2} and {c["ldl"] - c["V"] for c in bm} == {0, 3}
    assert {c["lenpen"] for c in bm} == {0.0, 1.0, 1.7} and len({c["temp"] for c in bm}) >= 4


def test_coded_beams_rank_in_binary_expansion_order():
    """Every coded beam case, every clip, every rank: the fp64 restatement and oracle/decode.py (fp32) both return 'hypothesis h flips the
    coded steps in the binary expansion of h', the smallest gap between adjacent scores is delta / temperature, and the launch asks for
    no more ranks than the code has."""
    drv = _driver()
    coded = [c for c in _cases("beam", ok=True) if c["data"] == "coded"]
    assert len(coded) >= 8 and {c["temp"] for c in coded} >= {1.0, 0.9, 2.0}
    assert any(c["V"] == 204 and c["beam"] == 64 and 130 in c["Ls"] and c["temp"] == t for c in coded for t in (1.0,)) and \
        all(any(c["V"] == 204 and c["beam"] == 64 and 130 in c["Ls"] and c["temp"] == t for c in coded) for t in (1.0, 0.9, 2.0))
    for c in coded:
        x, code = drv.beam_data(c)
        for b, L in enumerate(c["Ls"]):
            assert L == 0 or c["beam"] <= drv.coded_ranks(c, b), (c["name"], b)
            assert len(code[b][1]) == (gc.n_coded(L) if c["V"] > 5 else 0) == len(set(code[b][1]))
        r = drv.beam_cpu(c, x, code)
        assert r["order-ok"], c["name"]
        assert r["min-gap"] >= gc.DELTA / c["temp"] * 0.99, (c["name"], r["min-gap"])
        assert r["skipped"] == 0


def test_random_beams_keep_three_quarters_of_their_ranks():
    drv = _driver()
    rnd = [c for c in _cases("beam", ok=True) if c["data"] == "random"]
    assert {c["name"] for c in rnd} == set(gc.BEAM_G) and all(g > 0 for g in gc.BEAM_G.values())
    for c in rnd:
        x, code = drv.beam_data(c)
        r = drv.beam_cpu(c, x, code)
        assert r["total"] > 0 and r["skipped"] <= gc.SKIP_CAP * r["total"], (c["name"], r["skipped"], r["total"])
        assert 16 * r["dev"] <= gc.BEAM_G[c["name"]] * 1.001, (c["name"], r["dev"])      # the stored G is 16 x the oracle's deviation


def test_greedy_oracle_agrees_with_the_restatement():
    """oracle/decode.py (fp32) against the fp64 restatement on every greedy case: the same tokens (but where two units' fp32 lprobs
    coincide), lprobs and scores within CPU_F32_WORST."""
    drv = _driver()
    worst = {"greedy-lprob": 0.0, "greedy-score": 0.0}
    for c in _cases("greedy", ok=True):
        for k, q in drv.BUILD["greedy"](c).cpuf32().items():
            worst[k] = max(worst[k], q)
    for k, q in worst.items():
        assert q <= gc.CPU_F32_WORST[k] * 1.001, (k, q)


def _wrong_casts(x, t):
    """(truncation toward zero, round half away from zero) of finite fp32 x to the 16-bit type t, by stepping the bit pattern of the
    correctly rounded value: patterns of one sign are ordered like their magnitudes."""
    import torch
    y = x.to(t)
    yb = y.view(torch.int16).to(torch.int32)
    ax, ay = x.double().abs(), y.double().abs()
    trunc = torch.where(ay > ax, yb - 1, yb)
    up = (yb + 1).to(torch.int16).view(t).double().abs()
    half = (ay < ax) & ((ax - ay) == (up - ax))
    away = torch.where(half, yb + 1, yb)
    return trunc.to(torch.int16), away.to(torch.int16)


def test_cast_data_tell_the_rounding_modes_apart():
    """Bit-exact against x.to(t16) on this data is the criterion that tells round-to-nearest-even from truncation (which differs on every
    value above a midpoint, and on the midpoints whose even neighbour is the upper one) and from round-half-away (which differs on the
    midpoints whose even neighbour is the lower one): both wrong casts, written here, differ from the reference on it."""
    import torch
    drv = _driver()
    for dt in gc.DTYPES:
        t = drv.t16(dt)
        cd = drv.cast_coded(dt)
        have = set(cd.view(torch.int32).tolist())
        top = {"f16": 0x7BFF, "bf16": 0x7F7F}[dt]
        v = torch.arange(0, top + 1, dtype=torch.int32).to(torch.int16).view(t).double()
        mid = ((v[:-1] + v[1:]) / 2).float()
        assert torch.equal(mid.double(), (v[:-1] + v[1:]) / 2)
        for s in (1.0, -1.0):
            for pts in (mid, torch.nextafter(mid, torch.tensor(math.inf)), torch.nextafter(mid, torch.tensor(-math.inf)), v.float()):
                assert set((s * pts).view(torch.int32).tolist()) <= have, dt
        assert set(torch.tensor([0.0, -0.0, math.inf, -math.inf, 2.0 ** -149, 65504.0, 65519.996, 65520.0]).view(torch.int32).tolist()) <= have
        assert torch.isnan(cd).any() and len(have) > 250000 and cd.numel() < gc.CAP_ITEMS
        fin = cd[torch.isfinite(cd) & torch.isfinite(cd.to(t).float())]
        ref = fin.to(t).view(torch.int16)
        trunc, away = _wrong_casts(fin, t)
        assert (trunc != ref).sum() > 60000 and (away != ref).sum() > 10000, dt
        assert ((trunc != ref) & (away == ref)).any() and ((away != ref) & (trunc == ref)).any()
        # the cases carry it: all of it where it fits, a stride through it elsewhere, midpoints included
        for c in (c for c in _cases("cast16", ok=True) if c["dt"] == dt):
            x = drv.coded_fill(dt, c["M"] * c["C"])
            assert c["M"] * c["C"] < cd.numel() or set(x.view(torch.int32).tolist()) == have
        x = drv.coded_fill(dt, 37 * 80)
        fin = x[torch.isfinite(x) & torch.isfinite(x.to(t).float())]
        trunc, away = _wrong_casts(fin, t)
        assert (trunc != fin.to(t).view(torch.int16)).any() and (away != fin.to(t).view(torch.int16)).any()
        # rows_f32_to_16_masked and repeat2_cast round through pack2 / from_f32 on the same midpoints
        c = next(c for c in _cases("rows16", ok=True) if c["dt"] == dt and c["C"] == 80)
        x = drv.mixed_f32(c, c["B"] * c["T"] * c["C"])
        trunc, away = _wrong_casts(x, t)
        assert (trunc != x.to(t).view(torch.int16)).any() and (away != x.to(t).view(torch.int16)).any()


def test_exact_references_see_what_they_claim():
    import torch
    drv = _driver()
    # splitk_reduce: the order case changes bits under any other order of the additions
    c = next(c for c in _cases("splitk") if c["data"] == "order")
    x, P = drv.splitk_data(c)
    up, down = drv.splitk_sum(x, P, c["S"], c["N"]), drv.splitk_sum(x, P, c["S"], c["N"], descending=True)
    assert (up != down).float().mean() > 0.1
    assert float(P[:, : c["N"]].abs().median() / P[:, c["N"]: 2 * c["N"]].abs().median()) > 2.0 ** 19
    # split_hi_lo, f16: residues that are subnormal and residues that underflow to zero
    c = next(c for c in _cases("split", ok=True) if c["dt"] == "f16" and c["act"] == 0 and c["C"] == 64)
    r = drv.BUILD["split"](c).ref()
    res = (r["y32"] - r["hi"].float()).double().abs()
    lo = r["lo"].double().abs()
    assert ((lo > 0) & (lo < 2.0 ** -14)).sum() > 20 and ((lo == 0) & (res > 0)).sum() > 20
    assert float(r["y32"].abs().max()) < 65504.0 and float(r["y32"].abs()[r["y32"] != 0].min()) < 2.0 ** -18
    c = next(c for c in _cases("split", ok=True) if c["dt"] == "bf16" and c["act"] == 1 and c["C"] == 64)
    assert float(drv.split_data(c).abs().max()) > 1e28
    # lens_from_mask: all padded, none padded, one pad at the last position
    m = drv.lensmask_rows(5, 65, torch.Generator().manual_seed(0))
    assert int(m[0].sum()) == 65 and int(m[1].sum()) == 0 and m[2].nonzero().tolist() == [[64]] and int(m[4].max()) > 1
    # ctc_repeat_labels: one label at t = 0 alone, an all-zero row, a zero-free row
    x = drv.ctcrepeat_rows(6, 200, torch.Generator().manual_seed(0))
    assert x[0].nonzero().tolist() == [[0]] and not x[1].any() and x[2].all() and x[5].nonzero().tolist() == [[63]]
    assert drv.dr.repeat_labels([0, 0, 3, 0, 0, 5, 5, 0]) == [0, 0, 3, 3, 3, 5, 5, 5]
    # embedding_tokens: the clamp at both ends inside the valid range; embedding: codes 0 and n - 1, never out of range
    for c in _cases("embtok", ok=True):
        k = drv.BUILD["embtok"](c)
        tok = k.specs["tok"].data
        assert int(tok[1, 0]) < c["off"] and int(tok[1, 1]) >= c["n"] + c["off"] and drv.lens_setup(c, c["L"])[1][1] == c["L"]
    for c in _cases("embedding", ok=True):
        code = drv.BUILD["embedding"](c).specs["code"].data
        assert int(code.min()) == 0 and int(code.max()) == c["n"] - 1 and {0, c["n"] - 1} <= set(code[1].tolist())
    # ctc_frames: a spread of 60 with p normal in fp32 down to the K-th class, a tie at the top of the first frame
    c = next(c for c in _cases("ctcframes", ok=True) if c["V"] == 4096 and c["K"] == 64)
    r = drv.BUILD["ctcframes"](c).ref()
    x = drv.ctc_data(c)
    top = x.sort(1, descending=True).values
    L = c["L"]
    assert float((top[:, 0] - top[:, 63]).min()) >= 59.0 and float(top[L, 0]) == float(top[L, 1]) and int(r["cls"][L, 0]) < int(r["cls"][L, 1])
    assert float(r["lp"][r["A"] > 0].exp().min()) > 1.2e-38 * 1e6
    # greedy: specials at +40, exact ties, -inf on losers
    c = next(c for c in _cases("greedy", ok=True) if c["V"] == 204 and c["T2"] == 130)
    x = drv.greedy_data(c)
    assert (x[:, :, :4] == 40.0).any() and torch.isinf(x[:, :, 4:]).any()
    u = x[:, :, 4:].sort(2, descending=True).values
    assert (u[:, :, 0] == u[:, :, 1]).sum() > 10


def test_conv_post_references():
    import torch
    drv = _driver()
    sat = [c for c in _cases("convpost", ok=True) if c["data"] == "saturated"]
    for c in sat:
        r = drv.BUILD["convpost"](c).ref()
        pos = torch.tensor([t for rg in drv.SAT_POS for t in rg])
        neg = torch.tensor([t for rg in drv.SAT_NEG for t in rg])
        assert float(r["acc"][:, pos].min()) > 20.0 and float(r["acc"][:, neg].max()) < -20.0
        assert (r["wav"][:, pos] == 1.0).all() and (r["wav"][:, neg] == -1.0).all()          # tanh(56) is 1 in fp64 as well
        assert 255 in pos.tolist() and 256 in pos.tolist()                                 # across the 256-sample tile boundary
        assert float(r["wav"].abs().min()) < 0.5                                           # and unsaturated samples beside them
    assert gc.convpost_smem(59, 7) == 64532 and gc.convpost_smem(60, 7) == 65608
    # the twins of the (16, 7) shape carry the same data
    a = next(c for c in _cases("convpost") if c["name"] == "convpost/C16-k7-T257-lens-none")
    b = next(c for c in _cases("convpost") if c["name"] == "convpost/C16-k7-offset-T257-lens-none")
    assert torch.equal(drv.convpost_data(a)[0], drv.convpost_data(b)[0]) and a["inst"][0] == "conv_post16_kernel" and b["inst"][0] == "conv_post_kernel"
    # lens: 0, 1, the clamp and none
    c = next(c for c in _cases("convpost") if c["lens"] == "mixed" and c["T"] == 700)
    ln, lim = drv.lens_setup(c, c["T"])
    assert ln[0] == 0 and ln[1] * c["len_mul"] > c["T"] and lim[1] == c["T"]
    assert any(1 in drv.lens_setup(c, c["T"])[1] for c in _cases("convpost", ok=True) if c["lens"] == "mixed")


def test_every_reference_runs():
    r = subprocess.run([sys.executable, TOOL, "--cpu-ref"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("CPUREF ") == len(gc.PARTS)
