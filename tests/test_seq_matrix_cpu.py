"""The sequence-kernel matrix, host side: the selection rules restated in tests/_seq_cases.py equal the library's host-only
queries (l2s_attention_variant, l2s_layernorm_variant, l2s_glu_dwconv_tile) under every switch setting, the case lists reach every
kernel instantiation with the shapes, lengths and layouts they claim, and criterion (b) / (c) of tools/check_seq_kernels.py tells
round-to-nearest from truncation.  Nothing here needs a device."""
import importlib.util
import os
import subprocess
import sys

import pytest

from lip2speech_unit_amd import _lib
from tests import _seq_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_seq_kernels.py")
# the six children of the GPU matrix, and every switch on its own (a forced block size leaves the resident kernel its clips)
ROUTE_ENVS = dict(sc.ENVS, **{"qb64-only": {"L2S_ATTN_QB": "64"}, "qb128-only": {"L2S_ATTN_QB": "128"},
                              "all-off": {"L2S_ATTN_RESIDENT": "0", "L2S_ATTN_RESIDENT_PLAIN": "1", "L2S_LN_ROWS": "0"}})


def _driver():
    spec = importlib.util.spec_from_file_location("check_seq_kernels", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _all_cases():
    return [(e, c) for e in sc.ENVS for c in sc.cases_of(e)]


def test_constants_match_the_binding():
    assert (sc.SEQ_VARIANT_F32, sc.LN_GENERIC, sc.ATTN_RESIDENT) == (_lib.SEQ_VARIANT_F32, _lib.LN_GENERIC, _lib.ATTN_RESIDENT)
    assert [getattr(_lib, n.upper()) for n in sc.DTYPES] == [0, 1]
    assert len(sc.ENVS) == 6 and all(set(v) <= set(sc.SWITCHES) for v in sc.ENVS.values())
    for k, f in sc.CPU_F32_WORST.items():
        assert sc.F_of(k) == max(8.0, 8.0 * f)


@pytest.mark.parametrize("env_name", list(ROUTE_ENVS))
def test_restated_rules_equal_the_queries(env_name):
    """In a child process (the switches are read once): T = 1..1300 with and without pos, the LayerNorm layouts, and every case
    of the environment against the instantiation it claims."""
    env = {k: v for k, v in os.environ.items() if k not in sc.SWITCHES}
    env.update(ROUTE_ENVS[env_name])
    r = subprocess.run([sys.executable, TOOL, "--route", env_name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]


def test_selection_rules_at_the_points_the_issue_names():
    assert [sc.glu_tile(T) for T in (1, 31, 99, 100, 150, 200, 257, 1200)] == [100] * 8
    assert [sc.glu_tile(T) for T in (101, 128, 201, 250, 256, 301, 384, 501, 512)] == [128] * 9
    d = sc.ENVS["default"]
    assert sc.attention_variant(208, 8, True, d) == sc.ATTN_RESIDENT + 1 and sc.attention_variant(209, 8, True, d) == 129
    assert sc.attention_variant(224, 8, True, d) == 129 and sc.attention_variant(300, 2, True, d) == 65
    assert sc.attention_variant(208, 8, False, d) == 128 and sc.attention_variant(17, 257, True, d) == 65
    assert sc.res_layout_bytes(208, True) <= 160 * 1024
    assert sc.attention_variant(513, 1, True, sc.ENVS["qb64"]) == 65 and sc.attention_variant(65, 1, False, sc.ENVS["qb128"]) == 128


def test_every_instantiation_is_reached():
    reached = {c["inst"] for _, c in _all_cases()}
    assert reached == set(sc.instantiations()) and len(reached) == 2 * (6 + 8 + 4 + 2)
    by_env = {e: {c["inst"][2] for c in sc.cases_of(e) if c["op"] == "attn"} for e in sc.ENVS}
    assert by_env["default"] == {64, 128, 65, 129, 1001} and by_env["resident-plain"] == {1000}
    assert by_env["resident-off"] == {65, 129} and by_env["qb64"] == {64, 65} and by_env["qb128"] == {128, 129}
    assert {c["inst"][2] for c in sc.cases_of("ln-rows-off")} == {10, 11, 12, 13}
    names = [(e, c["dt"], c["name"]) for e, c in _all_cases()]
    assert len(names) == len(set(names))


def test_attention_cases():
    for dt in sc.DTYPES:
        cases = [c for c in sc.attention_cases("default") if c["dt"] == dt]
        grid = {(c["pos"], c["T"], c["H"]) for c in cases if c["B"] == 3 and c["data"] == "randn" and c["len_mul"] == 1 and c["lens"]}
        assert grid >= {(True, T, H) for T in sc.REL_RESIDENT_T + sc.REL_TILED_T for H in sc.HEADS}
        assert grid >= {(False, T, H) for T in sc.PLAIN_T for H in sc.HEADS}
        for c in cases:
            H = c["H"]
            assert c["ldq"] == 3 * H * 64 + 8 and c["ldo"] == H * 64 + 4 and c["ldp"] == 3 * H * 64 and (sc.POS_NL, sc.POS_LI) == (3, 1)
            assert c["lens"] is None or (len(c["lens"]) == c["B"] and all(0 <= n <= c["T"] for n in c["lens"]))
        # per kernel of the default child: an empty clip, a full one, a ragged one
        for inst in {c["inst"] for c in cases}:
            ks = [(n, c["T"]) for c in cases if c["inst"] == inst and c["lens"] for n in sc.klens(c)]
            assert any(n == 0 for n, _ in ks) and any(n == T for n, T in ks) and any(0 < n < T for n, T in ks), inst
        drawn = {n for c in cases if c["T"] == 193 and c["B"] == 3 for n in c["lens"]}
        assert drawn == {193, 1, 64, 65, 128, 192, 0}
        for pos in (True, False):
            sp = {c["name"].split("/")[1]: c for c in cases if c["pos"] == pos}
            assert sp["no-lens-T65"]["lens"] is None
            lm = sp["len-mul2-T100"]
            assert lm["len_mul"] == 2 and 2 * lm["lens"][0] > lm["T"] > 2 * lm["lens"][1] and sc.klens(lm)[0] == lm["T"]
            assert sp["rescale-T130"]["data"] == "rescale" and sp["rescale-T130"]["T"] == 130
        # the resident kernel's slot walk: 256 / H slots capped at B
        slots = {c["name"]: (min(256 // c["H"], c["B"]), c["B"]) for c in cases if "slots" in c["name"]}
        assert slots == {"rel/slots-H128-B5-T33": (2, 5), "rel/slots-H256-B3-T17": (1, 3)}
        assert all(c["inst"][2] == 1001 for c in cases if "slots" in c["name"])
        for qb in ("qb64", "qb128"):
            q = [c for c in sc.attention_cases(qb) if c["dt"] == dt]
            assert {(c["pos"], c["T"]) for c in q} == {(p, T) for p in (True, False) for T in sc.QB_T}
            assert all(c["inst"][2] == int(qb[2:]) + c["pos"] for c in q)
        assert {c["T"] for c in sc.attention_cases("resident-off") if c["data"] == "randn" and c["B"] == 3 and c["lens"]
                and c["len_mul"] == 1} == set(sc.REL_RESIDENT_T)
        assert {c["T"] for c in sc.attention_cases("resident-plain") if c["name"].startswith("plain/T")} == {T for T in sc.PLAIN_T if T <= 208}


def test_layernorm_cases():
    for env_name in ("default", "ln-rows-off"):
        on = env_name == "default"
        for dt in sc.DTYPES:
            cases = [c for c in sc.layernorm_cases(env_name) if c["dt"] == dt]
            rows = [c for c in cases if c["name"].startswith("rows/") and c["data"] == "randn"]
            assert {(c["C"], c["M"]) for c in rows} == {(C, M) for C in (512, 1024) for M in sc.ROWS_M}
            for c in rows:
                assert c["ldx"] == c["C"] + 4 and c["ldy"] == c["C"] + (4 if c["yf"] else 8) and c["xf"]
                assert c["inst"][2] == (c["C"] + c["yf"] if on else sc.LN_GENERIC + 2 + c["yf"])
            assert {(c["C"], c["yf"], c["inplace"]) for c in rows} == {(C, yf, ip) for C in (512, 1024)
                                                                       for yf, ip in ((True, True), (True, False), (False, False))}
            fb = [c for c in cases if c["name"].startswith("fallback/")]
            assert {(c["C"], c["ldy"] - c["C"], c["y_off"]) for c in fb} == {(C, 4, 0) for C in (512, 1024)} | {(C, 8, 4) for C in (512, 1024)}
            assert all(c["inst"][2] == sc.LN_GENERIC + 2 for c in fb)        # the generic <fp32 x, 16-bit y> kernel, rows kernel on or off
            gen = [c for c in cases if c["name"].startswith("generic/")]
            assert {c["C"] for c in gen} == set(sc.GENERIC_C)
            for v in range(4):
                sub = [c for c in gen if c["inst"][2] == sc.LN_GENERIC + v and c["data"] == "randn"]
                assert {(c["C"], c["zp"]) for c in sub} == {(C, zp) for C in sc.GENERIC_C for zp in sc.ZPS}
                assert {c["y2"] for c in sub} == {True, False} and {c["eps"] for c in sub} == {1e-5, 1e-12}
                assert all(c["ldy2"] != c["ldy"] for c in sub if c["y2"])
                assert any(c["mask"] for c in sub) and any(c["zero_row"] for c in sub) and {c["M"] for c in sub} == {1, 5, 9}
            assert sum(c["data"] == "offset" for c in cases) == 5 and all(c["skip_a"] == c["yf"] for c in cases if c["data"] == "offset") and any(c["zero_row"] and c["eps"] == 1e-12 for c in rows)
            for c in cases:
                if c["mask"]:
                    mask_T, len_mul, lens = c["mask"]
                    keep = sc.ln_keep(c)
                    assert len_mul == 2 and 0 in lens and keep[0] and not all(keep) and len(lens) == sc.cdiv(c["M"], mask_T)
                assert not c["zero_row"] or c["eps"] == 1e-12
                assert not c["skip_a"] or (c["data"] == "offset" and c["yf"])      # (a) is waived for nothing else
    for dt in sc.DTYPES:
        sk = [c for c in sc.splitk_ln_cases() if c["dt"] == dt]
        assert {(c["C"], c["M"], c["S"], c["yf"]) for c in sk} == {(C, M, S, yf) for C in (512, 1024) for M in (1, 5, 9) for S in (1, 3)
                                                                   for yf in (False, True)}
        assert all(c["ldp"] == c["S"] * c["C"] + 4 and c["inplace"] == c["yf"] for c in sk)


def test_glu_cases():
    for dt in sc.DTYPES:
        cases = [c for c in sc.glu_cases() if c["dt"] == dt]
        assert {c["T"] for c in cases if c["inst"][2] == 128} == set(sc.GLU_T128) == {101, 128, 250}
        assert {c["T"] for c in cases if c["inst"][2] == 100} == set(sc.GLU_T100) == {1, 31, 99, 100, 200, 257}
        for tile in (100, 128):
            sub = [c for c in cases if c["inst"][2] == tile]
            assert {c["C"] for c in sub} == set(sc.GLU_C) and {c["k"] for c in sub} == set(sc.GLU_K)
            assert any(c["len_mul"] == 2 and any(2 * n > c["T"] for n in c["lens"]) for c in sub)
            lens = {(c["T"], n) for c in sub if c["lens"] and c["len_mul"] == 1 for n in c["lens"]}
            big = 250 if tile == 128 else 257
            want = {tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 0, 1, 15, 16, tile + 7}
            assert {n for T, n in lens if T == big} >= {n for n in want if n <= big}, (tile, sorted(n for T, n in lens if T == big))
        assert all(c["B"] == 3 for c in cases)


@pytest.mark.parametrize("dt", sc.DTYPES)
def test_elementwise_bound_accepts_nearest_and_rejects_truncation(dt):
    """Criteria (b) / (c) of the driver on results formed on the CPU in fp32 with one rounding to 16 bits: round-to-nearest passes,
    chopping the fp32 value to 16 bits fails, while the max-error criterion (a) lets both through.  (b) does this for the conv
    kernel, (c) for LayerNorm; for attention (b) as specified cannot (see below)."""
    import torch
    drv = _driver()
    shift = 13 if dt == "f16" else 16

    def chop(v32):
        return ((v32.contiguous().view(torch.int32) >> shift) << shift).view(torch.float32).double()

    def both(v32, ref, bound, tol_abs):
        near, cut = v32.to(drv.t16(dt)).double(), chop(v32)
        assert drv.ratio_b((near - ref).abs(), bound) <= 1.0
        assert drv.ratio_b((cut - ref).abs(), bound) > 1.0
        assert (cut - ref).abs().max().item() <= tol_abs

    c = next(c for c in sc.attention_cases("default") if c["dt"] == dt and c["name"] == "rel/T65-H2")
    ins = drv.attn_inputs(c)
    ref, A = drv.attn_eval(c, *ins, torch.float64)
    v32 = drv.attn_eval(c, *ins, torch.float32)[0]
    valid = torch.zeros(c["B"], c["T"], dtype=torch.bool)
    for b, n in enumerate(sc.klens(c)):
        valid[b, :n] = True
    # Attention: (b) as specified carries 1.5 u A for P rounded to 16 bits, and A >= |ref|, so it is at least 3 u |ref| and CANNOT
    # tell a chopped output conversion (error < 2 u |ref|) from a rounded one - both pass it.  What it does catch is anything beyond
    # the two documented roundings.  Without the P term (the output's own half-ulp and the fp32 term only) the chopped output fails.
    real = drv.bound_b(ref[valid], A[valid], dt, True, "attn", attn=True)
    assert drv.ratio_b((v32[valid].to(drv.t16(dt)).double() - ref[valid]).abs(), real) <= 1.0
    assert drv.ratio_b((chop(v32[valid]) - ref[valid]).abs(), real) <= 1.0
    both(v32[valid], ref[valid], real - sc.FU * drv.U16[dt] * A[valid], drv.TOL_ATTN[dt] * ref[valid].abs().max().item())

    c = next(c for c in sc.layernorm_cases("default") if c["dt"] == dt and c["name"] == "rows/C512-M9-16")
    x, gamma, beta, _ = drv.ln_inputs(c)
    ref, A, A2 = drv.ln_eval(c, x, gamma, beta, torch.float64)
    v32 = drv.ln_eval(c, x, gamma, beta, torch.float32)[0]
    keep = torch.tensor(sc.ln_keep(c))
    both(v32[keep], ref[keep], drv.bound_b(ref[keep], A2[keep], dt, True, "ln2"), drv.TOL_LN16[dt] * ref[keep].abs().max().item())

    c = next(c for c in sc.glu_cases() if c["dt"] == dt and c["name"] == "glu/T128-C128-k31")
    ins = drv.glu_inputs(c)
    ref, A = drv.glu_eval(c, *ins, torch.float64)
    v32 = drv.glu_eval(c, *ins, torch.float32)[0]
    both(v32, ref, drv.bound_b(ref, A, dt, True, "glu"), drv.TOL_GLU[dt] * ref.abs().max().item())
