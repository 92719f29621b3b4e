"""The tap-GEMM instantiation matrix, host side: the case lists of tests/_tapgemm_cases.py cover the whole product
(type, mode, tap path, epilogue family) on every tile, their schedule cases make a block walk three output tiles, and every
descriptor is one l2s_tapgemm accepts.  The library's two query entries run without a device."""
import ctypes

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
