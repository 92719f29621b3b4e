"""The lip front end's kernel matrix, host side: the rules restated in tests/_frontend_cases.py equal l2s_basicblock_variant and
l2s_stem_pool_frames under every child's switches, the case lists reach every kernel instantiation with the shapes, image counts
and data sets they claim, the walk cases give some block three tiles, the stride-loop cases exceed the capped grid, the coded data
sets are exact in 16 bits, and criterion (b) of tools/check_frontend_kernels.py rejects one wrong term of conv2 at a border position
that the max-error criterion (a) accepts.  Nothing here needs a device."""
import importlib.util
import os
import subprocess
import sys

import pytest

from lip2speech_unit_amd import _lib
from tests import _frontend_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_frontend_kernels.py")
_DRV = []


def _driver():
    if not _DRV:
        spec = importlib.util.spec_from_file_location("check_frontend_kernels", TOOL)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _DRV.append(mod)
    return _DRV[0]


def _all_cases():
    return [(e, c) for e in fc.ENVS for c in fc.cases_of(e)]


def test_constants_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    for name, val in (("L2S_BB_PADDED64", fc.PADDED64), ("L2S_BB_PHASE64", fc.PHASE64), ("L2S_BB_PHASE128", fc.PHASE128)):
        assert f"#define {name} {val}" in hdr
    assert (_lib.BB_PADDED64, _lib.BB_PHASE64, _lib.BB_PHASE128) == (576064, 512064, 256128) == (fc.PADDED64, fc.PHASE64, fc.PHASE128)
    for q, nargs in (("l2s_basicblock_variant", 6), ("l2s_stem_pool_frames", 2)):
        assert f"int {q}(" in hdr and len(_lib.SIGNATURES[q][0]) == nargs
    assert "L2S_EALIGN = -3" in hdr and "L2S_EUNSUPPORTED = -4" in hdr and (fc.EALIGN, fc.EUNSUPPORTED) == (-3, -4)
    assert all(set(v) <= set(fc.SWITCHES) for v in fc.ENVS.values())
    assert fc.ENVS["padded64"] == {"L2S_BASICBLOCK_PHASE": "0"} and fc.ENVS["default"] == fc.ENVS["default-walk-f16"] == fc.ENVS["stem-bf16"] == {}
    assert [fc.ENVS[e + "-f16"].get("L2S_STEM_FT") for e in fc.STEM_ENVS] == [None, "25", "1", "3"]
    assert len(fc.ENVS) == 3 + 2 * len(fc.PER_TYPE) and {fc.part_of(e)[0] for e in fc.ENVS} == set(fc.PARTS)
    assert fc.part_of("stem-ft3-bf16") == ("stem-ft3", "bf16") and fc.part_of("padded64") == ("padded64", None)
    for (k, dt), f in fc.CPU_F32_WORST.items():
        assert fc.F_of(k, dt) == max(8.0, 8.0 * f)
    kinds = {(fc.fkind(c), c["dt"]) for _, c in _all_cases() if c["op"] != "maxpool"}
    assert kinds == set(fc.CPU_F32_WORST)
    src = open(os.path.join(ROOT, "lip2speech_unit_amd", "csrc", "basicblock.hip")).read()
    # the launcher asks the same selection code as the query, not a copy of it
    assert src.count("bb_select(") == 3 and src.count('getenv("L2S_BASICBLOCK_PHASE")') == 1
    src = open(os.path.join(ROOT, "lip2speech_unit_amd", "csrc", "frontend.hip")).read()
    assert src.count("stem_pool_frames(B, T)") == 2 and src.count('getenv("L2S_STEM_FT")') == 1


@pytest.mark.parametrize("env_name", list(fc.PARTS))
def test_restated_rules_equal_the_queries(env_name):
    """In a child process (the switches are read once): a sweep of (N, H, W, C, n_blocks) and of (B, T) around every limit, and every
    case of the part's children against the instantiation and the frames per block it claims."""
    env = {k: v for k, v in os.environ.items() if k not in fc.SWITCHES}
    env.update(fc.PARTS[env_name])
    r = subprocess.run([sys.executable, TOOL, "--route", env_name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_rules_at_the_points_the_issue_names():
    d, off = fc.PARTS["default"], fc.PARTS["padded64"]
    v = fc.basicblock_variant
    assert v(5, 22, 22, 64, 1, d) == 512064 and v(5, 22, 22, 64, 4, d) == 512064 and v(5, 22, 22, 64, 1, off) == 576064
    assert v(5, 11, 11, 128, 1, d) == v(5, 11, 11, 128, 1, off) == 256128
    for H, W in fc.PADDED_MAPS:
        assert v(2, H, W, 64, 1, d) == 576064, (H, W)
    assert {(16, 29), (94, 4), (1, 1)} <= set(fc.PADDED_MAPS) and (16 + 2) * (29 + 2) <= 576 and (94 + 2) * (4 + 2) == 576
    assert fc.PADDED_REFUSED == ((17, 29), (5, 30), (23, 22), (95, 4))
    for H, W in fc.PADDED_REFUSED:
        assert v(2, H, W, 64, 1, d) == v(2, H, W, 64, 1, off) == fc.EUNSUPPORTED
    assert v(3, 22, 13, 64, 5, d) == v(3, 22, 22, 64, 5, d) == v(2, 11, 11, 128, 2, d) == v(2, 10, 10, 128, 1, d) == fc.EUNSUPPORTED
    assert fc.stem_ft(342, 1, d) == 25 and fc.stem_ft(341, 1, d) == 10 and fc.stem_ft(2, 26, d) == 10
    assert [fc.stem_ft(2, 26, fc.PARTS[e]) for e in fc.STEM_ENVS] == [10, 25, 1, 3]
    assert fc.grid_for(1) == 1 and fc.grid_for(8192 * 256) == 8192 == fc.grid_for(8192 * 256 + 1) and fc.grid_for(0) == 1


def test_every_instantiation_is_reached():
    inst = fc.instantiations()
    assert len(inst) == len(set(inst)) == 2 * (3 + 1 + 6 + 4) + 9
    launched = [c["inst"] for _, c in _all_cases() if c["expect"] == 0]
    assert set(launched) == set(inst)
    for i in inst:
        assert launched.count(i) >= (1 if i[0] == "stem2" else 4), i
    # the padded kernel at 22 x 22 only where the switch holds the phase kernel off
    assert {c["inst"][2] for c in fc.bb_cases("padded64")} == {576064}
    assert all((c["H"], c["W"]) != (22, 22) for c in fc.bb_cases("default") if c["inst"][2] == 576064)
    assert {c["inst"][2] for c in fc.bb_cases("default-walk")} == {576064, 512064, 256128}


def test_case_lists_hold_what_the_issue_lists():
    for dt in fc.DTYPES:
        bb = [c for e in fc.PARTS for c in fc.bb_cases(e) if c["dt"] == dt]
        ok = [c for c in bb if c["expect"] == 0]
        padded = [c for c in ok if c["inst"][2] == 576064 and c["nb"] == 1 and not c["walk"]]
        for H, W in fc.PADDED_MAPS + ((22, 22),):
            sub = [c for c in padded if (c["H"], c["W"]) == (H, W)]
            assert {c["N"] for c in sub} == {1, 2, 5} and "coded" in {c["data"] for c in sub}, (H, W)
        assert {c["data"] for c in padded} == set(fc.BB_DATA)
        assert {(c["H"], c["W"]) for c in bb if c["expect"] == fc.EUNSUPPORTED and c["C"] == 64 and c["nb"] == 1} == set(fc.PADDED_REFUSED)
        for H, W in fc.LAYER_MAPS:
            assert {c["nb"] for c in ok if (c["H"], c["W"]) == (H, W) and c["nb"] > 1 and not c["walk"]} == {2, 3, 4}
        assert any(c["nb"] == 5 and c["expect"] == fc.EUNSUPPORTED for c in bb)
        assert {c["N"] for c in ok if c["walk"] and (c["H"], c["W"]) == (5, 7)} == {257, 513}
        p64 = [c for c in ok if c["inst"][2] == 512064]
        assert {c["N"] for c in p64 if not c["walk"]} == {1, 2, 3, 255, 256, 257} and {c["nb"] for c in p64 if c["N"] <= 3} == {1, 2, 3, 4}
        assert {(c["N"], c["nb"]) for c in p64 if c["walk"]} == {(513, 1), (513, 2)} and {c["data"] for c in p64} == set(fc.BB_DATA)
        p128 = [c for c in ok if c["inst"][2] == 256128]
        assert {c["N"] for c in p128 if not c["walk"]} == {1, 2, 3, 4, 5, 511, 512, 513} and {c["N"] for c in p128 if c["walk"]} == {1025}
        assert {c["data"] for c in p128 if c["N"] <= 5} == set(fc.BB_DATA)
        assert {(c["nb"], c["H"]) for c in bb if c["C"] == 128 and c["expect"]} == {(2, 11), (1, 10)}
        tail = [c for e in fc.PARTS for c in fc.tail_cases(e) if c["dt"] == dt]
        assert {c["N"] for c in tail if c["expect"] == 0 and not c["walk"]} == {1, 2, 3, 4, 5, 511, 512, 513}
        assert {c["N"] for c in tail if c["walk"]} == {1025} and {c["data"] for c in tail if c["expect"] == 0} == set(fc.BB_DATA)
        assert {c["expect"] for c in tail} == {0, fc.EUNSUPPORTED, fc.EALIGN}
        stem = [c for c in fc.stem_cases("stem") if c["dt"] == dt]
        assert {c["T"] for c in stem} >= set(fc.STEM_T) == {1, 2, 3, 4, 5, 9, 10, 11, 20, 21, 26} and {c["B"] for c in stem} >= {2, 3}
        assert {(c["Hin"], c["Win"]) for c in stem if c["xk"] == "u8"} == set(fc.U8_HW) == {(96, 96), (88, 88), (97, 120), (89, 91)}
        assert {(c["xk"], c["slopes"]) for c in stem} >= {(x, s) for x in fc.XKS for s in fc.STEM_SLOPES}
        assert {c["wset"] for c in stem if c["data"] == "coded"} == {0, 1, 2, 3} and any(c["data"] == "negbias" for c in stem)
        assert [(c["B"], c["ft"]) for c in stem if c["pool"]] == [(342, 25), (341, 10)]
        for e in fc.STEM_ENVS:                            # every stem case runs in all four stem children
            assert [c["name"] for c in fc.stem_cases(e) if c["dt"] == dt] == [c["name"] for c in stem]
        assert {c["T"] for c in fc.stem2_cases()} == {1, 5, 11}
    pools = fc.pool_cases()
    for dt in fc.DTYPES + ("f32",):
        mp = [c for c in pools if c["op"] == "maxpool" and c["dt"] == dt]
        assert {(c["H"], c["W"], c["C"]) for c in mp if c["expect"] == 0} == set(fc.MAXPOOL_SHAPES)
        assert any(c["data"] == "negative" for c in mp) and any(c["expect"] == fc.EALIGN and c["C"] % 8 for c in mp)
        assert {(c["HW"], c["C"]) for c in pools if c["op"] == "avgpool" and c["dt"] == dt} >= set(fc.AVGPOOL_SHAPES)
        pp = [c for c in pools if c["op"] == "preproc" and c["dt"] == dt]
        assert {(c["Hin"], c["Win"]) for c in pp if c["crop"] == 88} == set(fc.U8_HW) and any(c["crop"] != 88 for c in pp)


def test_walks_and_stride_loops():
    """Some block of every walk case takes three tiles (513 tiles on 256 blocks: block 0 takes tiles 0, 256, 512), the pool of seven
    images hands a block that reads a wrong tile or a neighbouring image another image, and the grid-stride cases exceed the grid."""
    assert 512 % fc.POOL == 1 and 256 % fc.POOL != 0
    for e in fc.ENVS:
        for c in fc.cases_of(e):
            if c["op"] in ("bb", "tail") and c["expect"] == 0:
                walk = fc.tiles_per_block(fc.cdiv(c["N"], fc.images_per_tile(c["inst"][2])))
                if c["walk"]:                             # (the pool of seven images is for these; N = 257 at 5 x 7 is its two-tile twin)
                    assert max(len(b) for b in walk) == (3 if c["N"] >= 513 else 2), c["name"]
                    assert c["N"] == 257 or (walk[0] == [0, 256, 512] and len(walk[1]) == 2)
                else:
                    assert max(len(b) for b in walk) <= 2, c["name"]
    assert fc.tiles_per_block(513)[0] == [0, 256, 512] and fc.tiles_per_block(257)[0] == [0, 256]
    loops = [c for c in fc.pool_cases() if "stride-loop" in c["name"]]
    assert {(c["op"], c["dt"]) for c in loops} == {(op, dt) for op in ("maxpool", "avgpool", "preproc") for dt in fc.DTYPES + ("f32",)}
    for c in fc.pool_cases():
        if c["expect"] == 0 and c["dt"] != "f32":
            assert fc.takes_stride_loop(fc.items_of(c)) == ("stride-loop" in c["name"]), c["name"]
            assert fc.grid_for(fc.items_of(c)) == (8192 if "stride-loop" in c["name"] else fc.cdiv(fc.items_of(c), 256))
    assert fc.items_of(next(c for c in loops if c["op"] == "maxpool")) == 542 * 22 * 22 * 8 > 8192 * 256 > 541 * 22 * 22 * 8
    assert fc.items_of(next(c for c in loops if c["op"] == "avgpool")) == 32769 * 64 > 8192 * 256 >= 32768 * 64


def test_coded_sets_are_exact():
    """Every intermediate and result of a coded case is exact in 16 bits: the mirrored reference equals the un-mirrored one and its own
    bf16 rounding, the largest value stays below 256.  Every tap is named: a rich convolution reads nine different, non-diagonal input
    channels per output channel; the four stem weight sets carry the 245 taps once each."""
    import torch
    drv = _driver()
    f64 = torch.float64
    w = drv.coded_conv(64, 0, True)
    for co in (0, 1, 17, 63):
        cins = [int(w[co, t * 64: (t + 1) * 64].nonzero()) for t in range(9)]
        assert len(set(cins)) == 9 and cins.count(co) <= 1 and len({ci // 8 for ci in cins}) > 1
    assert {float(v) for v in w.unique()} == {0.0, 1.0, 2.0} and all(int((w[:, t * 64: (t + 1) * 64] != 0).sum()) == 64 for t in range(9))
    assert drv.marks_of(22, 22) == [(0, 0), (0, 11), (0, 21), (11, 0), (11, 11), (11, 21), (21, 0), (21, 11), (21, 21)]
    assert drv.marks_of(1, 1) == [(0, 0)] and len(drv.marks_of(3, 5)) == 2
    x = drv.coded_map(2, 11, 11, 128)
    assert not torch.equal(x[0], x[1])                    # the two images of a tile carry different marks
    seen = 0
    for e, c in _all_cases():
        if c.get("data") != "coded" or c["dt"] != "bf16" or c["expect"] or c["op"] not in ("bb", "tail"):
            continue
        a, b = drv.eval_case(c, f64)[0], drv.eval_case(c, f64, mirror=False)[0]
        assert torch.equal(a, b) and torch.equal(a, a.to(torch.bfloat16).double()) and 3.0 < float(a.abs().max()) < 256.0, c["name"]
        seen += 1
    assert seen >= 30
    taps = set()
    for c in fc.stem_cases("stem"):
        if c["data"] != "coded" or c["dt"] != "bf16":
            continue
        ins = drv.stem_inputs(c)
        taps |= {(c["wset"], int(co), int(t)) for co, t in ins["w"].nonzero().tolist()}
        assert float(ins["x"].max()) == 1.0 and set(ins["x"].unique().tolist()) == {0.0, 1.0} and torch.equal(ins["x"], ins["xu"])
        a, b = drv.eval_case(c, f64)[0], drv.eval_case(c, f64, mirror=False)[0]
        assert torch.equal(a, b) and torch.equal(a, a.to(torch.bfloat16).double()) and torch.equal(a, a.half().double())
        assert {float(v) for v in a.unique()} <= {0.0, 1.0, 2.0, 3.0} and float(a.max()) == 3.0
    assert sorted(t for _, _, t in taps) == list(range(245)) and all(t == co + 64 * s for s, co, t in taps)


def test_negbias_sets_pool_negative_maxima():
    import torch
    drv = _driver()
    c = next(c for c in fc.stem_cases("stem") if c["data"] == "negbias" and c["xk"] == "x16" and c["dt"] == "f16")
    y = drv.eval_case(c, torch.float64)[0]
    assert float((y < 0).double().mean()) > 0.5           # a zero-padded pool would show at the map border
    c = next(c for c in fc.bb_cases("default") if c["data"] == "negative" and c["C"] == 128)
    ins = drv.bb_inputs(c)
    pre = drv.conv3x3(ins["x"], ins["ws"][0]) + ins["bs"][0]
    assert float((pre < 0).double().mean()) > 0.5


def test_elementwise_bound_rejects_one_wrong_term_that_the_max_error_accepts():
    """Criterion (b) with the measured F on the CPU fp32 evaluation, bf16: unmodified it passes (a) and (b); with ONE term w2 t1 of
    conv2 dropped at one element of a corner position - of the four taps a corner has, a term smaller than half the tolerance of (a),
    so that (a) cannot see it, in the channel where it is largest against the element's own bound - (a) still passes and (b) fails,
    at C = 64 and at C = 128.  A term of typical size
    (1 / 24 of the output's spread at C = 64) stays below both criteria on random data (profiles/frontend_matrix.md): those are what
    the coded sets are for."""
    import torch
    drv = _driver()
    f64, f32 = torch.float64, torch.float32
    cases = {c["name"]: c for c in fc.bb_cases("default") if c["dt"] == "bf16"}
    for name in ("phase64/N1-nb1-randn", "phase128/N2-randn"):
        c = cases[name]
        assert c["nb"] == 1 and c["data"] == "randn"
        ref, A = drv.eval_case(c, f64)
        clean = drv.eval_case(c, f32)[0]
        assert drv.ratio_a_of(c, clean, ref) <= 1.0 and drv.ratio_b_of(c, clean, ref, A) <= 1.0
        cap = 0.5 * drv.TOL_BB["bf16"] * float(ref.abs().max())
        bound = drv.bound_b(ref[0, 0, 0], A[0, 0, 0], "bf16", fc.fkind(c))
        mut, size = drv.planted_term(c, drv.bb_inputs(c), 0, 0, 0, cap, bound, ref[0, 0, 0])
        assert 0.0 < size <= cap
        bad = drv.eval_case(c, f32, mut=mut)[0]
        assert drv.ratio_a_of(c, bad, ref) <= 1.0, (name, mut, size)
        assert drv.ratio_b_of(c, bad, ref, A) > 1.0, (name, mut, size)
