"""The vocoder-convolution matrix, host side: the selection rule restated in tests/_vocconv_cases.py equals l2s_respair_variant under
every child's switches, the case lists reach all 44 kernel instantiations with the shapes, lengths and arguments they claim, the
restated LDS sizes of csrc/resblock.hip say which ResBlock launches must succeed, the tile walk under L2S_RESPAIR_SLOTS=8 is the one
the cases were sized for, the tapcode data sets are exact in 16 bits, and criterion (b) of tools/check_vocoder_convs.py rejects five
subtle errors planted into the CPU fp32 evaluation.  Nothing here needs a device."""
import importlib.util
import os
import subprocess
import sys

import pytest

from lip2speech_unit_amd import _lib
from tests import _vocconv_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_vocoder_convs.py")
# the children of the GPU matrix, and the one-sided settings of the bit mask
ROUTE_ENVS = dict(vc.ENVS, **{"phase-128-only": {"L2S_RESPAIR_PHASE": "1"}, "phase-64-only": {"L2S_RESPAIR_PHASE": "2"}})


def _driver():
    spec = importlib.util.spec_from_file_location("check_vocoder_convs", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _all_cases():
    return [(e, c) for e in vc.ENVS for c in vc.cases_of(e)]


def test_constants_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    assert "L2S_EUNSUPPORTED = -4" in hdr and vc.EUNSUPPORTED == -4
    assert "l2s_respair_variant" in hdr and "l2s_respair_variant" in _lib.SIGNATURES
    assert [getattr(_lib, n.upper()) for n in vc.DTYPES] == [0, 1]
    assert all(set(v) <= set(vc.SWITCHES) for v in vc.ENVS.values())
    assert vc.ENVS["pair192"] == {"L2S_RESPAIR_PHASE": "0"} and vc.ENVS["walk"] == {"L2S_RESPAIR_SLOTS": "8"}
    assert vc.ENVS["walk-plain"] == {"L2S_RESPAIR_SLOTS": "8", "L2S_RESPAIR_XCD": "0"}
    for (k, dt), f in vc.CPU_F32_WORST.items():
        assert vc.F_of(k, dt) == max(8.0, 8.0 * f)
    kinds = {(vc.fkind(c), c["dt"]) for e in vc.ENVS for c in vc.cases_of(e)}
    assert kinds == set(vc.CPU_F32_WORST) and len(kinds) == 13
    # a figure kept per type and width class is never above the figure of the whole operation over both types
    for op in ("pair", "final"):
        whole = max(f for (k, _), f in vc.CPU_F32_WORST.items() if k.startswith(op))
        assert all(f <= whole for (k, _), f in vc.CPU_F32_WORST.items() if k.startswith(op))


@pytest.mark.parametrize("env_name", list(ROUTE_ENVS))
def test_restated_rule_equals_the_query(env_name):
    """In a child process (the switches are read once): every C, k = 1..21, dil = 1..35 and kind, the refusals, and every pair case of
    the environment against the instantiation it claims."""
    env = {k: v for k, v in os.environ.items() if k not in vc.SWITCHES}
    env.update(ROUTE_ENVS[env_name])
    r = subprocess.run([sys.executable, TOOL, "--route", env_name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_selection_rule_at_the_points_the_issue_names():
    d, off = vc.ENVS["default"], vc.ENVS["pair192"]
    assert [vc.respair_variant(C, 11, 5, d) for C in (64, 128, 256)] == [512064, 256128, 128256]
    assert [vc.respair_variant(C, 11, 5, off) for C in (64, 128, 256)] == [192064, 192128, 128256]
    for k, dil in vc.FALLBACK_GEOS:                       # h1 = 29 .. 32: the default path falls back to respair.hip
        assert 29 <= (k - 1) // 2 * dil <= 32
        assert [vc.respair_variant(C, k, dil, d) for C in (64, 128, 256)] == [192064, 192128, vc.EUNSUPPORTED]
    assert [vc.respair_variant(C, 3, 33, e) for C in (64, 128, 256) for e in (d, off)] == [vc.EUNSUPPORTED] * 6
    assert vc.respair_variant(64, 3, 28, d) == 512064 and vc.respair_variant(64, 17, 1, d) == 512064
    assert vc.respair_variant(64, 19, 1, d) == vc.EUNSUPPORTED and vc.respair_variant(32, 3, 1, d) == vc.EUNSUPPORTED


def test_tile_walk_under_the_slot_cap():
    """L2S_RESPAIR_SLOTS = 8 with 19 tiles: in XCD order (per = 3, gx = 1) XCDs 0-5 walk three tiles, XCD 6 one, XCD 7 none; in plain
    order blocks 0-2 walk three tiles and the rest two.  Unset, the grid is the parent's."""
    w = vc.ENVS["walk"]
    assert vc.respair_grid(19, 256, w) == 8 and vc.respair_grid(19, 512, w) == 8 and vc.respair_grid(3, 256, w) == 8
    assert vc.respair_grid(19, 256, {}) == 24 and vc.respair_grid(5000, 256, {}) == 256 and vc.respair_grid(5000, 512, {}) == 512
    assert vc.respair_grid(19, 256, {"L2S_RESPAIR_SLOTS": "7"}) == 24 and vc.respair_grid(100, 256, {"L2S_RESPAIR_SLOTS": "21"}) == 16
    xcd = vc.tile_walk(19, 8, True)
    assert [len(t) for t in xcd] == [3, 3, 3, 3, 3, 3, 1, 0] and xcd[0] == [0, 1, 2] and xcd[6] == [18]
    plain = vc.tile_walk(19, 8, False)
    assert [len(t) for t in plain] == [3, 3, 3, 2, 2, 2, 2, 2] and plain[0] == [0, 8, 16]
    for walk in (xcd, plain, vc.tile_walk(21, 8, True), vc.tile_walk(21, 8, False), vc.tile_walk(300, 256, True)):
        assert sorted(t for blk in walk for t in blk) == list(range(sum(len(b) for b in walk)))
    # every walk case is one of these two tilings, and walks at least three tiles in some block
    for e in ("walk", "walk-plain", "walk192", "walk192-plain"):
        for c in vc.cases_of(e):
            ntiles = c["B"] * vc.cdiv(c["T"], c["S"])
            assert ntiles in (19, 21), (e, c["name"], ntiles)
            walk = vc.tile_walk(ntiles, vc.respair_grid(ntiles, 256, vc.ENVS[e]), vc.ENVS[e].get("L2S_RESPAIR_XCD") != "0")
            assert max(len(b) for b in walk) == 3 and min(len(b) for b in walk) < 3
            lim = vc.lims(c)
            assert 0 in lim and c["T"] in lim and any(0 < n < c["T"] for n in lim)


def test_every_instantiation_is_reached():
    cases = _all_cases()
    inst = vc.instantiations()
    assert len(inst) == len(set(inst)) == 44
    launched = [c["inst"] for _, c in cases if c["expect"] == 0]
    assert set(launched) == set(inst)
    for i in inst:
        assert launched.count(i) >= 4, i
    # the eight kernels of respair.hip: through pair192, walk192 and the fallback halos of the default child
    r192 = {(192000 + C, kind) for C in (64, 128) for kind in (0, 1)}
    for e in ("default", "pair192", "walk192", "walk192-plain"):
        for dt in vc.DTYPES:
            assert {c["inst"][2] for c in vc.pair_cases(e) if c["dt"] == dt and c["expect"] == 0} >= r192, e
    assert {c["inst"][2][0] for c in vc.pair_cases("pair192")} == {192064, 192128}
    assert {c["inst"][2][0] for c in vc.pair_cases("walk")} == {512064, 256128, 128256}
    # every pair kernel (type, C, rows) has every kind of launch, and every geometry with every kind
    per = {}
    for e, c in cases:
        if c["op"] == "pair" and c["expect"] == 0:
            per.setdefault((c["dt"], c["inst"][2][0]), set()).add((c["k"], c["dil"], c["kind"]))
    assert len(per) == 2 * 5
    for key, have in per.items():
        assert {kind for _, _, kind in have} == set(vc.KINDS), key
        geos = vc.GEOS if key[1] // 1000 != 192 else vc.GEOS + vc.FALLBACK_GEOS
        assert have >= {(k, d, kind) for k, d in geos for kind in vc.KINDS}, key
    names = [(e, c["dt"], c["op"], c["name"]) for e, c in cases]
    assert len(names) == len(set(names))
    # no case is skipped or exempted: the only fields a case may carry are the launch's arguments, its data set and its claim
    assert not any(k.startswith("skip") or k.startswith("exempt") for _, c in cases for k in c)


def test_pair_cases():
    for dt in vc.DTYPES:
        cases = [c for c in vc.pair_cases("default") if c["dt"] == dt]
        for C in (256, 128, 64):
            rm = vc.RM_PHASE[C]
            sub = [c for c in cases if c["C"] == C and c["rm"] == rm]
            for c in sub:
                assert c["S"] == rm - (c["k"] - 1)
            # per geometry: T = S + 1, lens S + 1, S, S - 1, all four kinds
            for k, dil in vc.GEOS:
                S = rm - (k - 1)
                g = [c for c in sub if (c["k"], c["dil"], c["T"]) == (k, dil, S + 1) and c["lens"] == [S + 1, S, S - 1] and c["data"] == "randn"]
                assert {c["kind"] for c in g} == set(vc.KINDS), (C, k, dil)
            # the length sweep, for the mid pair and the accumulating last pair
            for k, dil in vc.SWEEP_GEOS:
                h2 = (k - 1) // 2
                h1, S = h2 * dil, rm - 2 * h2
                for kind in ("mid", "acc"):
                    sw = [c for c in sub if (c["k"], c["dil"], c["kind"]) == (k, dil, kind) and c["data"] == "randn" and c["len_mul"] == 1 and c["lens"]]
                    assert {c["T"] for c in sw} >= {1, h1, S - 1, S, S + 1, 2 * S, 2 * S + 1}
                    drawn = {n for c in sw for n in c["lens"]}
                    assert drawn >= {0, 1, S, S + 1, S - 1, h2, h1 + 1, 2 * S + 1, 2 * S}, (C, k, sorted(drawn))
            sp = {c["name"].split("/")[1]: c for c in sub}
            assert sp["no-lens-mid"]["lens"] is None and sp["no-lens-acc"]["lens"] is None
            lm = sp["len-mul4-acc"]
            S = lm["S"]
            assert lm["len_mul"] == 4 and vc.lims(lm)[0] == S and 0 < vc.lims(lm)[1] < S and vc.lims(lm)[2] == lm["T"] < 4 * lm["lens"][2]
            assert sp["slope1-mid"]["slope"] == 1.0 and sp["slope0.01-negative-acc"]["slope"] == 0.01
            assert {c["data"] for c in sub} == {"randn", "negative", "tapcode"}
            for c in sub:
                assert c["lens"] is None or (len(c["lens"]) == c["B"] and all(0 <= n * c["len_mul"] for n in c["lens"]))
        rej = [c for c in cases if c["expect"]]
        assert {(c["C"], c["k"], c["dil"]) for c in rej} == {(256, k, d) for k, d in vc.FALLBACK_GEOS} | {(C, 3, 33) for C in (64, 128, 256)}
        assert all(c["expect"] == vc.EUNSUPPORTED and c["inst"][2][0] == vc.EUNSUPPORTED for c in rej)
        fb = [c for c in cases if c["rm"] == 192]
        assert {(c["C"], c["k"], c["dil"]) for c in fb} == {(C, k, d) for C in (64, 128) for k, d in vc.FALLBACK_GEOS}
        # pair192 repeats every C = 64 / 128 case of the default child on respair.hip's tiles
        p192 = [c for c in vc.pair_cases("pair192") if c["dt"] == dt]
        shape = lambda c: (c["k"], c["dil"], c["kind"], c["data"], c["len_mul"], c["slope"], c["lens"] is None, vc.cdiv(c["T"], c["S"]))   # noqa: E731
        for C in (64, 128):
            again, first = [c for c in p192 if c["C"] == C], [c for c in cases if c["C"] == C and c["rm"] == vc.RM_PHASE[C]]
            assert len(again) == len(first) and sorted(map(shape, again)) == sorted(map(shape, first)) and {c["rm"] for c in again} == {192}


def test_final_resblock_resstage_and_post_cases():
    for dt in vc.DTYPES:
        fin = [c for c in vc.final_cases("default") if c["dt"] == dt]
        for C in (256, 128, 64):
            sub = [c for c in fin if c["C"] == C]
            assert {c["ks"] for c in sub} >= {(11,), (3, 7), (3, 7, 11), (11, 7, 3), (1, 17, 5)}
            assert all(len(set(c["dils"])) == len(c["dils"]) for c in sub if len(c["ks"]) > 1)        # dilations differ between the ResBlocks
            assert max((k - 1) // 2 * d for c in sub for k, d in zip(c["ks"], c["dils"])) == 28
            S = vc.RM_PHASE[C] - 10
            assert {c["T"] for c in sub if c["ks"] == (3, 7, 11) and c["dils"] == (5, 3, 1)} >= {1, S - 1, S, S + 1, 2 * S + 1}
            assert any(c["lens"] is None for c in sub) and any(c["len_mul"] == 4 for c in sub) and any(c["lens"] and 0 in c["lens"] for c in sub)
        assert {c["B"] * vc.cdiv(c["T"], c["S"]) for c in vc.final_cases("walk")} == {19, 21}
        rb = [c for c in vc.resblock_cases() if c["dt"] == dt]
        for C in (16, 32):
            for k in (3, 7, 11):
                sub = [c for c in rb if (c["C"], c["k"]) == (C, k)]
                TT = vc.rb_tt(C, k)
                assert TT == {(32, 3): 384, (32, 7): 368}.get((C, k), 512)
                assert {c["dils"] for c in sub} == set(vc.RB_DILS)
                for dils in vc.RB_SWEEP:
                    assert {c["T"] for c in sub if c["dils"] == dils} >= {1, vc.rb_halo(k, dils), TT - 1, TT, TT + 1, 2 * TT + 1}
                ok = [c for c in sub if c["expect"] == 0]
                assert {(c["accumulate"], c["xl_out"]) for c in ok} == {(a, o) for a in (False, True) for o in (False, True)}
                assert all((2 * c["xl_off"]) % 16 == 8 for c in sub)                                   # 8- but not 16-byte aligned
                assert any(c["lens"] is None for c in sub) and any(c["len_mul"] == 4 for c in sub) and any(c["lens"] and 0 in c["lens"] for c in sub)
                assert {c["data"] for c in sub} == {"randn", "negative", "tapcode"}
                # which launches must succeed: all but the (5, 5, 5) set of <32, 11>, whose two 768-row buffers of 96-byte rows
                # and one conv's weights are 167 KB
                assert {c["dils"] for c in sub if c["expect"]} == ({(5, 5, 5)} if (C, k) == (32, 11) else set())
        assert vc.rb_smem(32, 11, (5, 5, 5), False) == 171008 and vc.rb_smem(32, 11, (1, 3, 5), False) <= 160 * 1024
        assert vc.rb_smem(32, 7, (1, 3, 5), True) == 162816 and not vc.rs_launches(32, vc.RS_TABLES[2]) and vc.rs_launches(32, vc.RS_TABLES[1])
        rs = [c for c in vc.resstage_cases() if c["dt"] == dt]
        for C in (16, 32):
            sub = [c for c in rs if c["C"] == C]
            assert {c["table"] for c in sub} == set(vc.RS_TABLES)
            ok = [c for c in sub if c["expect"] == 0]
            assert {c["T"] for c in ok if c["table"] == vc.RS_TABLES[1]} >= set(vc.RS_T) == {1, 511, 512, 513, 1025}
            assert {(c["xs_final"], c["xl_out"]) for c in ok} == {(True, True), (True, False), (False, True)}
            assert {c["table"] for c in sub if c["expect"]} == (set() if C == 16 else set(vc.RS_TABLES[2:4]))
            assert any(c["lens"] is None for c in ok) and any(c["len_mul"] == 4 for c in ok) and any(c["lens"] and 0 in c["lens"] for c in ok)
    post = vc.post_cases()
    assert {(c["C"], c["k"], c["x_off"]) for c in post} == set(vc.POST_SHAPES)
    assert {c["inst"][2][0] for c in post if (c["C"], c["k"], c["x_off"]) == (16, 7, 0)} == {"conv_post16_kernel"}
    assert {c["inst"][2][0] for c in post if (c["C"], c["k"]) != (16, 7) or c["x_off"]} == {"conv_post_kernel"}
    assert {(c["C"], c["k"]) for c in post if c["expect"]} == {(64, 7)} and vc.post_smem(64, 7) > 64 * 1024 >= vc.post_smem(32, 7)
    for C, k, off in vc.POST_SHAPES:
        sub = [c for c in post if (c["C"], c["k"], c["x_off"]) == (C, k, off)]
        assert {c["T"] for c in sub} >= set(vc.POST_T) and any(not c["pcm"] for c in sub) and any(c["len_mul"] == 4 for c in sub)
        assert any(c["data"] == "saturate" for c in sub) and any(c["lens"] and 0 in c["lens"] for c in sub)


def test_tapcode_and_saturate_data_sets():
    """tapcode: every tap of both convolutions sits in some channel, and the mirrored reference equals the un-mirrored one: every
    intermediate and result is exact in 16 bits, so the device result must be bit-exact.  saturate: pre-activations pass +-12."""
    import torch
    drv = _driver()
    for C, k in ((64, 11), (64, 17), (16, 11), (16, 3), (256, 3)):
        for conv in (0, 1):
            W = drv.tap_weights(C, k, conv, 2)
            assert {int(i) // C for i in W.abs().sum(0).nonzero().reshape(-1)} == set(range(min(k, C) if conv == 0 else k)) or C < k
            assert int((W != 0).sum()) == C
    seen = 0
    for c in vc.pair_cases("default") + vc.resblock_cases():
        if c["data"] != "tapcode" or c["dt"] != "bf16" or c["C"] not in (64, 16) or c["expect"]:
            continue
        a, b = drv.eval_case(c, torch.float64), drv.eval_case(c, torch.float64, mirror=False)
        for name in a:
            v = a[name][0]
            assert torch.equal(v, b[name][0]) and torch.equal(v, v.to(torch.bfloat16).double()) and float(v.abs().max()) > 1.0, (c["name"], name)
        seen += 1
    assert seen >= 6
    c = next(c for c in vc.post_cases() if c["data"] == "saturate" and (c["C"], c["k"]) == (16, 1))
    ins = drv.post_inputs(c)
    wav = drv.post_eval(c, ins, torch.float32)[0]
    assert bool((wav == 1.0).any()) and bool((wav == -1.0).any())           # tanh in fp32 is exactly +-1 there


def test_elementwise_bound_rejects_subtle_errors():
    """Criterion (b) with the measured F on the CPU fp32 evaluation: unmodified it passes; each planted error fails (b) on a case of
    its kind.  Whether the max-error criterion (a) of tests/test_kernels_gpu.py would have let the error through:
      tap-dropped          one tap of conv2 dropped at the first row of a clip's second tile                 (a) catches it too
      t1-unmasked          t1 not zeroed past the clip length (h2 rows of leaky_relu(b1 + ...) leak in)      (a) catches it too
      dilation-off-by-one  the second dilation of a ResBlock is d + 1                                        (a) catches it too
      chopped-output       the 16-bit output of a wide pair (K = 2816, bf16) chopped instead of rounded      (a) lets it through
      residual-no-inverse  the residual taken from xl without the inverse (negative values, slope 0.1)       (a) catches it too
    The first three and the last are errors of the size of a term of the sum: on random data both criteria see them.  What (b)
    adds over (a) is the chopped conversion, and - being element-wise - any error in elements quiet against the loudest sample."""
    import torch
    drv = _driver()
    f64, f32 = torch.float64, torch.float32

    def a_ratio(c, got, ref):
        worst = 0.0
        for name, (r, A, is16) in ref.items():
            tol = {"pair": drv.TOL_PAIR, "resblock": drv.TOL_RB}[c["op"]][c["dt"]] * ref[next(iter(ref))][0].abs().max().item()
            worst = max(worst, (got[name][0].to(f64) - r).abs().max().item() / tol)
        return worst

    pairs = {c["name"]: c for c in vc.pair_cases("default") if c["dt"] == "f16"}
    pairs_bf = {c["name"]: c for c in vc.pair_cases("default") if c["dt"] == "bf16"}
    rbs = {c["name"]: c for c in vc.resblock_cases() if c["dt"] == "f16"}
    plan = {
        "tap-dropped": pairs["C64-rm512/k11d5-T1005-mid"],          # T = 2 S + 1: the clips have a second tile
        "t1-unmasked": pairs["C64-rm512/k11d5-T1005-acc"],          # ragged lengths inside the tile
        "residual-no-inverse": pairs["C128-rm256/negative-mid"],
        "dilation-off-by-one": rbs["C16-k7/d135-T513"],
        # a flip of t1 moves a result by 2 u of one of its K = C k terms: only where K is large (here 2816) is that far enough
        # below half an ulp of the output for a chopped conversion to stand out, in the elements where A is under 2.8 |ref| (the
        # stage sum dominates); see profiles/vocoder_conv_matrix.md
        "chopped-output": pairs_bf["C256-rm128/k11d5-acc"],
    }
    verdict_a = {}
    for mut, c in plan.items():
        ref = drv.eval_case(c, f64)
        clean = drv.eval_case(c, f32)
        assert drv.ratio_b_of_case(c, clean, ref) <= 1.0, (mut, c["name"])
        assert a_ratio(c, clean, ref) <= 1.0
        bad = drv.eval_case(c, f32, chop=True) if mut == "chopped-output" else drv.eval_case(c, f32, mut=mut)
        verdict_a[mut] = a_ratio(c, bad, ref) <= 1.0
        if mut == "chopped-output":                       # "at least one case": the wide bf16 pairs of this geometry, every output
            worst = [drv.ratio_b_of_case(c, bad, ref)]
            for name in ("C256-rm128/k11d5-T236-acc", "C256-rm128/k11d5-T237-acc", "C256-rm128/k11d5-T237-mid"):
                c2 = pairs_bf[name]
                r2, b2 = drv.eval_case(c2, f64), drv.eval_case(c2, f32, chop=True)
                assert drv.ratio_b_of_case(c2, drv.eval_case(c2, f32), r2) <= 1.0
                verdict_a[mut] = verdict_a[mut] and a_ratio(c2, b2, r2) <= 1.0
                worst.append(drv.ratio_b_of_case(c2, b2, r2))
            assert max(worst) > 1.0, worst
            continue
        assert drv.ratio_b_of_case(c, bad, ref) > 1.0, (mut, c["name"])
    assert verdict_a == {"tap-dropped": False, "t1-unmasked": False, "residual-no-inverse": False, "dilation-off-by-one": False,
                         "chopped-output": True}
