"""The tap-GEMM instantiation matrix, host side: the case lists of tests/_tapgemm_cases.py cover the whole product
(type, mode, tap path, epilogue family) on every tile, their schedule cases make a block walk three output tiles, and every
descriptor is one l2s_tapgemm accepts.  The same for the phase-staggered and the LDS-patch kernel: their case lists cover every
instantiation, are routed to the kernel they claim under the part's switches, and their walk / natural parts make a block walk
several output tiles.  The library's two query entries run without a device."""
import ctypes
import os
import subprocess
import sys

import pytest

from lip2speech_unit_amd import _lib
from tests import _tapgemm_cases as tc

TILES = sorted(tc.TILES)


def test_constants_match_the_binding():
    assert (tc.ACT_NONE, tc.ACT_RELU, tc.ACT_GELU, tc.ACT_SWISH, tc.ACT_PRELU, tc.ACT_LRELU, tc.ACT_TANH) == (
        _lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_SWISH, _lib.ACT_PRELU, _lib.ACT_LRELU, _lib.ACT_TANH)
    assert (tc.F_RES_PRE, tc.F_RES_POST, tc.F_ACCUM, tc.F_DUAL, tc.F_MASK, tc.F_OUT_F32, tc.F_RES_F32) == (
        _lib.F_RES_PRE, _lib.F_RES_POST, _lib.F_ACCUM, _lib.F_DUAL, _lib.F_MASK, _lib.F_OUT_F32, _lib.F_RES_F32)
    assert (tc.MODE_LINEAR, tc.MODE_CONV1D, tc.MODE_CONV2D) == (_lib.MODE_LINEAR, _lib.MODE_CONV1D, _lib.MODE_CONV2D)
    assert [getattr(_lib, n.upper()) for n in tc.DTYPES] == [0, 1]


@pytest.mark.parametrize("tile", TILES)
def test_family_cases_cover_the_product(tile):
    want = {(dt, mode, uni, fam) for dt in tc.DTYPES
            for mode, uni in ((0, False), (1, True), (1, False), (2, True), (2, False)) for fam in range(10)}
    assert len(want) == 2 * 5 * 10
    cases = tc.family_cases(tile)
    assert {(c["dt"], c["mode"], c["uni"], c["family"]) for c in cases} == want
    BM, BN = tc.TILES[tile][:2]
    for _, g in tc.base_geometries(BM, BN):
        assert g["M"] == 2 * BM + 37 and g["N"] == 2 * BN + 20 and g["N"] % 8 == 4
        assert g["uni"] == (g["mode"] != 0 and g["Cin"] % 64 == 0)
    names = [(c["dt"], c["name"]) for c in cases]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("tile,part", [(t, p) for t in TILES for p in ("families", "schedule")] + [(tc.BAND_TILE, "band")])
def test_descriptors_are_accepted_and_claim_their_family(tile, part):
    lib = _lib.load()
    for c in tc.cases_of(part, tile):
        for d in tc.descriptors(c):
            assert tc.alignment_ok(d), (c["name"], d)
            gd = _lib.GemmDesc(**d)
            assert lib.l2s_tapgemm_epilogue_family(ctypes.byref(gd)) == c["family"], c["name"]
            assert lib.l2s_tapgemm(ctypes.byref(gd), None) == -1        # null operands: refused before anything is launched
        if c["epi"]["mask"]:
            T = c["geom"]["mask_T"]
            assert tc.mask_lens(c) == [T, 0, 1, T - 1, T] and tc.cdiv(c["geom"]["M"] * c["geom"].get("out_row_mul", 1), T) <= tc.NCLIPS


def test_stream32_cases_are_the_exact_fast_path_descriptor():
    for c in tc.family_cases(256128):
        if c["name"].endswith(("/stream32", "/stream32-inplace", "/stream32-ldr")):
            (d, *_) = tc.descriptors(c)
            assert d["flags"] == tc.F_RES_POST | tc.F_RES_F32 | tc.F_OUT_F32 and d["act"] == tc.ACT_NONE
            assert (d["ldr"] == d["ldc"]) == (not c["name"].endswith("-ldr"))


@pytest.mark.parametrize("tile", TILES)
def test_schedule_cases_walk_three_tiles(tile):
    BM, BN, waves, stages = tc.TILES[tile]
    assert tc.blocks_per_cu(tile) == {128016: 4, 128032: 2, 256128: 1, 256064: 1, 128128: 2, 128064: 2, 64064: 3}[tile]
    cases = tc.schedule_cases(tile)
    assert {(c["dt"], c["geom"]["Cin"], c["family"]) for c in cases} == {(dt, K, f) for dt in tc.DTYPES for K in (64, 128, 200)
                                                                         for f in (0, 8)}
    for c in cases:
        g = c["geom"]
        ntiles, chunk, slots, my_n = tc.schedule(tile, g["M"], g["N"])
        assert ntiles > 2 * 8 * 32 * tc.blocks_per_cu(tile) and ntiles % 8 != 0 and g["M"] % BM != 0
        assert my_n >= 3


def test_band_case_has_a_short_last_band():
    BM, BN = tc.TILES[tc.BAND_TILE][:2]
    for c in tc.band_cases():
        g = c["geom"]
        assert (tc.cdiv(g["M"], BM), tc.cdiv(g["N"], BN)) == (7, 3) and 7 % tc.BAND != 0


def _driver():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_tapgemm_matrix.py")
    spec = importlib.util.spec_from_file_location("check_tapgemm_matrix", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("dt", tc.DTYPES)
def test_elementwise_bound_accepts_nearest_and_rejects_truncation(dt):
    """Criterion (b) of the driver on a result formed on the CPU the way the kernel forms it (fp32 accumulation, one rounding to
    16 bits): round-to-nearest passes, chopping the fp32 value to 16 bits fails, while the max-error criterion (a) lets both through
    - the hole (b) is there to close."""
    import torch
    drv = _driver()
    case = next(c for c in tc.family_cases(128064) if c["dt"] == dt and c["name"] == "linear/none")
    o = drv.operands(case)
    ref, _, S, _, _, _ = drv.reference(case, o)
    g = case["geom"]
    v32 = ((o["A"].float() @ o["W"][0].float().t() + o["bias"].float()) * 0.5).view(ref.shape)
    nearest = v32.to(drv.t16(dt)).double()
    shift = 13 if dt == "f16" else 16     # chop the fp32 mantissa to the type's 10 / 7 bits (these values are f16 normals)
    chopped = ((v32.view(torch.int32) >> shift) << shift).view(torch.float32).double()
    bound = drv.bound_b(ref, S, g["Cin"], dt, False)
    assert ((nearest - ref).abs() / bound).max().item() <= 1.0
    assert ((chopped - ref).abs() / bound).max().item() > 1.0
    assert (chopped - ref).abs().max().item() <= drv.TOL[dt] * ref.abs().max().item()


# ---- the phase-staggered kernel (256256) and the LDS-patch kernel (999064 / 999128) ------------------------------------------------
SPECIAL = [(part, k) for part in tc.PART_ENV for k in tc.PART_KERNELS[part]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_phase_cases_cover_every_instantiation():
    want = {(dt, mode, e) for dt in tc.DTYPES for mode in range(3) for e in tc.PHASE_EPIS}
    assert len(want) == 2 * 3 * 10
    cases = tc.cases_of("phase-families", tc.PHASE)
    assert {c["inst"] for c in cases} == want
    for c in cases:
        e = c["epi"]
        assert c["inst"][2] == (c["family"] if c["family"] < 9 else 10) and (c["family"] < 9 or tc.is_x32(e["flags"], e["act"]))
    # the ConvTranspose1d phases (negative dilation, out_row_mul) with 3 and 2 taps, N % 8 == 4 in the conv modes
    convt = {c["geom"]["s"]: tc.descriptors(c) for c in cases if c["geom"]["kind"] == "convt"}
    assert {d["ntaps"] for d in convt[4]} == {2} and {d["ntaps"] for d in convt[5]} == {3, 2}
    assert all(d["dil"] == -1 and d["out_row_mul"] == s for s, ds in convt.items() for d in ds)
    # N % 8 == 4 in the conv modes wherever the kernel admits it (G16B, S32, X32); families 0-6 need whole 8-channel groups
    assert {c["inst"] for c in cases if c["geom"]["N"] % 8 == 4} == {(dt, mode, e) for dt in tc.DTYPES for mode in (1, 2)
                                                                     for e in (7, 8, 10)}
    assert all(c["geom"]["N"] % 8 == 0 for c in cases if c["inst"][2] <= 6)
    assert {(c["dt"], c["mode"], c["family"]) for c in tc.phase_declined_cases()} == {(dt, mode, f) for dt in tc.DTYPES
                                                                                      for mode in (1, 2) for f in range(7)}
    walk = tc.cases_of("phase-walk", tc.PHASE)
    assert {c["inst"] for c in walk} == {(dt, mode, e) for dt in tc.DTYPES for mode in range(3) for e in (0, 3, 5, 6, 7, 8, 10)}


def test_patch_cases_cover_every_instantiation():
    want = {(dt, mode, ch, e) for dt in tc.DTYPES for mode in (1, 2) for ch in (64, 128) for e in tc.PATCH_EPIS}
    assert len(want) == 2 * 2 * 2 * 5
    cases = tc.cases_of("patch-families", tc.PATCH64) + tc.cases_of("patch-families", tc.PATCH128)
    assert {c["inst"] for c in cases} == want
    assert {c["epi"]["name"] for c in cases} == {e["name"] for e in tc.family_epilogues()}
    spans = set()
    for c in cases:
        for d in tc.descriptors(c):
            assert tc.patch_eligible(d), c["name"]
            if d["mode"] == tc.MODE_CONV1D:
                spans.add((abs((d["ntaps"] - 1) * d["dil"]), d["ntaps"], d["T_out"]))
    assert max(s for s, _, _ in spans) == 64 and (1, 2, 256) in spans and min(t for _, _, t in spans) == 7
    assert {(c["geom"]["H"], c["geom"]["Wi"]) for c in cases if c["mode"] == 2} == {(18, 18), (16, 29), (40, 12)}
    for ch in (64, 128):
        assert {c["inst"] for c in tc.cases_of("patch-walk", 999000 + ch)} == {i for i in want if i[2] == ch}


@pytest.mark.parametrize("part,kernel", SPECIAL)
def test_special_descriptors_are_accepted(part, kernel):
    lib = _lib.load()
    cases = tc.cases_of(part, kernel)
    names = [(c["dt"], c["name"]) for c in cases]
    assert len(names) == len(set(names))
    for c in cases:
        assert c["kernel"] == kernel
        for d in tc.descriptors(c):
            assert tc.alignment_ok(d), (c["name"], d)
            gd = _lib.GemmDesc(**d)
            assert lib.l2s_tapgemm_epilogue_family(ctypes.byref(gd)) == c["family"], c["name"]
            assert lib.l2s_tapgemm(ctypes.byref(gd), None) == -1        # null operands: refused before anything is launched
            if kernel == tc.PHASE:
                assert d["Cin"] % 64 == 0 and d["M"] >= 256 and d["N"] >= 256


@pytest.mark.parametrize("part,kernel", SPECIAL)
def test_special_cases_are_routed_to_their_kernel(part, kernel):
    """In a child process: the library reads the part's switches once per process."""
    env = {k: v for k, v in os.environ.items() if k not in tc.SWITCHES}
    env.update(tc.PART_ENV[part])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_tapgemm_matrix.py"), "--route", part, str(kernel)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_switches_unset_leave_the_dispatch_alone():
    """Without L2S_PATCH_MIN_M the small patch shapes stay on the generic tiles (this process has none of the switches set)."""
    assert not any(k in os.environ for k in tc.SWITCHES)
    lib = _lib.load()
    for c in tc.cases_of("patch-families", tc.PATCH64) + tc.cases_of("patch-walk", tc.PATCH128):
        for d in tc.descriptors(c):
            assert lib.l2s_tapgemm_variant(ctypes.byref(_lib.GemmDesc(**d))) in tc.TILES, c["name"]
    for c in tc.cases_of("patch-natural", tc.PATCH64):
        for d in tc.descriptors(c):
            assert lib.l2s_tapgemm_variant(ctypes.byref(_lib.GemmDesc(**d))) == tc.PATCH64, c["name"]


def test_phase_walk_and_natural_schedules():
    for c in tc.cases_of("phase-walk", tc.PHASE):
        g = c["geom"]
        ntiles, chunk, slots, my_n = tc.phase_schedule(g["M"], g["N"], tc.PHASE_SLOTS)
        assert (ntiles, chunk, slots) == (49, 7, 2) and my_n == [[4, 3]] * 7 + [[0, 0]]
        assert tc.phase_schedule(g["M"], g["N"])[3] == [[1] * 7] * 7 + [[0] * 7]          # without the cap: one tile per block
    assert {c["geom"]["Cin"] * c["geom"]["ntaps"] // 64 for c in tc.cases_of("phase-walk", tc.PHASE) if c["mode"] == 0} == {1, 2, 3}
    for c in tc.cases_of("phase-natural", tc.PHASE):
        g = c["geom"]
        ntiles, chunk, slots, my_n = tc.phase_schedule(g["M"], g["N"])
        assert (ntiles, chunk, slots) == (266, 34, 32) and ntiles % 8 and max(max(r) for r in my_n) == 2
        assert [r[:3] for r in my_n] == [[2, 2, 1]] * 7 + [[1, 1, 1]] and my_n[7][27:] == [1, 0, 0, 0, 0]


def test_phase_walk_has_a_short_last_band():
    bands = {}
    for c in tc.cases_of("phase-walk", tc.PHASE):
        g = c["geom"]
        ntaps = max(d["ntaps"] for d in tc.descriptors(c))
        bands[c["name"].split("/")[1]] = (tc.phase_band(g["M"], g["N"], g["Cin"], ntaps), tc.cdiv(g["M"], 256))
    assert bands["linear-K64"] == (2, 7) and bands["conv1d-k3-n1788"] == bands["conv1d-k3-n1784"] == (4, 7)
    assert bands["conv2d-7x7-n1784"] == (7, 7)
    assert sum(1 for b, tm in bands.values() if tm % b) >= 4                               # band does not divide tilesM


def test_patch_walk_and_natural_schedules():
    for ch in (64, 128):
        for c in tc.cases_of("patch-walk", 999000 + ch):
            ntiles, grid, tiles = tc.patch_schedule(c["geom"], ch, tc.PATCH_SLOTS)
            assert (ntiles, grid) == (15, 4) and [len(t) for t in tiles] == [4, 4, 4, 3]
            if c["mode"] == tc.MODE_CONV1D:      # a block's consecutive tiles lie in different clips
                assert all(a[0] != b[0] for t in tiles for a, b in zip(t, t[1:]))
            assert tc.patch_schedule(c["geom"], ch)[1] == 15                               # without the cap: one tile per block
    want = {1: (522, 10), 2: (518, 6)}
    for c in tc.cases_of("patch-natural", tc.PATCH64):
        ntiles, grid, tiles = tc.patch_schedule(c["geom"], 64)
        assert grid == 512 and (ntiles, sum(1 for t in tiles if len(t) == 2)) == want[c["mode"]]
        assert max(len(t) for t in tiles) == 2
