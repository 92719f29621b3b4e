"""The autoregressive decoding kernels' matrix, host side: the case lists of tests/_step_cases.py reach every shape, edge, template
instantiation and host dispatch branch they claim; every refusal line of the six launchers has a case, and a restatement of each
launcher's checks gives the code the case expects; the conditions on the inputs hold for every case (deciding gaps above
DECISIVE x the value bound or bit-exact ties, planted keys that lead by 30, a clip that finishes early in the closed loop) and a case
that loses its gap fails; tests/_step_reference.py reproduces tests/_whisper_reference.py and tests/_s2s_reference.py to 1e-12 inside
their contracts, and its CTC cases are judged by tests/_ctc_reference.py itself, pinned here to its PathTrie form.  Nothing here needs a
device.  `select_tol` and the crafted logits come from tests/test_lipread_kernels_gpu.py, the one place that defines them: that module
must stay importable without a device (it touches the device only inside its tests)."""
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import _ctc_reference as ctcr
from tests import _s2s_reference as s2s
from tests import _step_cases as sc
from tests import _step_reference as sr
from tests import _whisper_reference as whr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_step_kernels.py")
CSRC = os.path.join(ROOT, "lip2speech_unit_amd", "csrc")
_DRV = []


def _driver():
    if not _DRV:
        spec = importlib.util.spec_from_file_location("check_step_kernels", TOOL)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _DRV.append(mod)
    return _DRV[0]


def _cases(op=None, ok=None):
    ops = (op,) if isinstance(op, str) else op
    return [c for _, c in sc.all_cases() if (ops is None or c["op"] in ops) and (ok is None or (c["expect"] == 0) == ok)]


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _entry(src, name):
    """the body of an extern "C" launcher"""
    at = src.index(f'extern "C" int {name}(')
    end = src.find('extern "C"', at + 10)
    return src[at: end if end > 0 else len(src)]


def test_constants_match_the_sources():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    for name, val in (("L2S_EINVAL", sc.EINVAL), ("L2S_ESHAPE", sc.ESHAPE), ("L2S_EALIGN", sc.EALIGN), ("L2S_EUNSUPPORTED", sc.EUNSUPPORTED)):
        assert f"{name} = {val}" in hdr
    wh, s2 = _src("whisper_decode.hip"), _src("s2s_decode.hip")
    # the tile arithmetic the case lists are built on
    assert "constexpr int kAttnWaves = 16;" in wh and "constexpr int KB = 8 * kAttnWaves;" in wh and "jw += 2 * KB" in wh
    assert "kMaxCacheT = 1500, kMaxWidth = 1280, kMaxVocab = 65536" in wh and "constexpr int kVTile = 64;" in wh
    assert "const int NB = B <= 16 ? 1 : B <= 32 ? 2 : 4;" in wh and "for (int t = tid; t < n_tiles; t += 256)" in wh
    assert "for (; k0 + 256 <= d; k0 += 256)" in wh and "for (; k0 < d; k0 += 64)" in wh and "for (int b0 = 0; b0 < B; b0 += 256)" in wh
    assert "for (int j0 = 0; j0 < valid; j0 += 16)" in s2 and "slot = blockIdx.y * 4 + wave" in s2
    assert "kMaxBeam = 64, kMaxWidth = 1536, kMaxVocab = 8192" in s2 and "constexpr int kMaxLen = 32767;" in s2
    assert "if (st < 0 || st + 1 >= L) return;" in s2 and "V < 2 * beam + 2" in s2
    # the clamps the out-of-contract cases rely on, each before an address is formed from the value
    assert "valid = min(max(valid, 0), cache_T);" in wh and "const bool append = k_new && p >= 0 && p < cache_T;" in wh
    assert "if (t < 0 || t >= V) t = eot;" in wh and "if (p >= 0 && p < ld_tok)" in wh and "if (p + 1 >= 0 && p + 1 < n_ctx)" in wh
    assert s2.count("min(max((int)arow[j") == 2 and "valid = min(max(enc_lens[b], 0), T);" in s2 and "(self && (p < 0 || p >= T))" in s2
    assert "min(max(n_live ? n_live[b] : beam, 1), beam)" in s2 and "nh = min(max(nh, 0), beam);" in s2
    assert s2.count("min(max(cl[") == 3 and "min(max(ct[sNewR[j]], 0), a.V - 1)" in s2
    assert (sc.CANARY32, sc.CANARY16, sc.GUARD, sc.ATTN_F, sc.DECISIVE) == (0x5A5A5A5A, 0x5A5A, 3, 4.0, 2.0)


def test_names_are_unique_and_well_formed():
    names = [c["name"] for _, c in sc.all_cases()]
    assert len(names) == len(set(names))
    for part, c in sc.all_cases():
        assert c["name"].startswith(part + "/") and c["hits"] and c["op"] in ("kv", "ba", "va", "wa", "bs", "bd", "loop", "ct")
        assert (part == "refusals") == (c["expect"] != 0)
        if "dt" in c:
            assert c["dt"] in sc.DTS
    # both 16-bit types wherever the kernel is templated on one: every passing case has its twin
    for c in _cases(("kv", "ba", "va", "wa", "bd", "loop"), ok=True):
        other = c["name"].replace("-" + c["dt"], "-" + sc.DTS[1 - sc.DTS.index(c["dt"])])
        assert other in names, c["name"]


def _kv_valid(c):
    B, T = c["B"], c["T"]
    if c["form"] == "cross":
        return [min(max(c["n_valid"], 0), T)] * B
    pos = c["pos"] if c["stride"] == 1 else [c["pos"][0]] * B
    return [min(max(p + 1, 0), T) for p in pos]


def test_kv_attention_coverage():
    cs = _cases("kv", ok=True)
    self_ = [c for c in cs if c["form"] == "self"]
    assert {c["H"] for c in cs} >= {1, 2, 20} and {c["B"] for c in cs} >= {1, 5, 70}
    for T in (1, 8, 257, 448):
        want = {v for v in (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257, T - 1, T) if 0 <= v <= T}
        for append in (True, False):
            got = {v for c in self_ if c["T"] == T and c["append"] == append and c["value"] == "rand" for v in _kv_valid(c)}
            assert got >= want, (T, append, want - got)
    pos = {(c["T"], p) for c in self_ if c["append"] for p in c["pos"]}
    assert {(8, 8), (8, 13), (8, -1), (257, 257), (257, 262), (257, -1)} <= pos
    assert {c["stride"] for c in self_} == {0, 1}
    assert any(c["stride"] == 1 and len({min(v, 1) for v in _kv_valid(c)}) == 2 and max(c["pos"]) >= c["T"] for c in self_)      # mixed across the edges
    assert {c["n_valid"] for c in cs if c["form"] == "cross" and c["T"] == 1500 and c["H"] == 2} >= {0, 1, 128, 129, 1001, 1500}
    assert any(c["pads"] == (8, 16, 24) for c in cs) and any(c["pads"] == (0, 0, 0) for c in cs)
    assert {c["value"] for c in cs} >= {"dom:0", "dom:127", "dom:200", "dom:new", "equal", "pm60"}
    assert {c["dt"] for c in cs} == set(sc.DTS)


def test_beam_attention_coverage():
    cs = _cases("ba", ok=True)
    se, cr = [c for c in cs if c["form"] == "self"], [c for c in cs if c["form"] == "cross"]
    assert {c["hd"] for c in se} == {c["hd"] for c in cr} == {64, 128, 192}
    assert {(c["H"], c["hd"]) for c in cs} >= {(1, 64), (2, 64), (8, 192)} and any(c["H"] * c["hd"] == 1536 for c in se) and any(c["H"] * c["hd"] == 1536 for c in cr)
    assert {c["beam"] for c in cs} >= {1, 3, 4, 5, 8, 64} and {c["B"] for c in cs} >= {1, 3, 70}
    for T in (18, 40):
        assert {c["p"] for c in se if c["T"] == T} >= {p for p in (0, 1, 7, 8, 15, 16, 17, 31, 32, 33, T - 1) if p < T}, T
    assert {c["p"] - c["T"] for c in se} >= {0} and -1 in {c["p"] for c in se}
    assert {c["anc"] for c in se} >= {"identity", "one", "perm", "clamp", "rand"}
    assert any(c["anc"] == "perm" and c["p"] & 1 for c in se) and any(c["anc"] == "perm" and not c["p"] & 1 and c["p"] > 0 for c in se)
    live = {(n - c["beam"]) if n >= c["beam"] - 1 else n for c in se if c["n_live"] for n in c["n_live"]}
    assert live >= {0, 1, -1, 3} and any(c["n_live"] and 0 in c["n_live"] for c in se)
    assert any(c["finished"] and c["finished"][1] and not c["finished"][0] and not c["finished"][2] for c in se)
    assert any(c["n_live"] is None and c["finished"] is None for c in se) and any(c["n_live"] is None and c["finished"] for c in se)
    assert any(c["n_live"] and c["finished"] is None for c in se)
    assert {c["T"] for c in cr} >= {16, 200}
    for T in (16, 200):
        assert any(c["T"] == T and set(c["enc_lens"]) >= {-2, 0, 1, 15, 16, 17, T, T + 9} - ({T} if T == 16 else set()) for c in cr), T
    assert any(c["pads"] == (8, 16, 24) for c in cs) and any(c["pads"] == (0, 0, 0) for c in cs)
    # every instantiation: (type, chunks per head) in both forms
    assert {(c["dt"], c["hd"], c["form"]) for c in cs} == {(d, h, f) for d in sc.DTS for h in (64, 128, 192) for f in ("self", "cross")}


def test_vocab_argmax_coverage():
    cs = _cases("va", ok=True)
    assert {c["V"] for c in cs} >= {1, 15, 16, 17, 63, 64, 65, 333, 16385, 65536}
    assert {c["d"] for c in cs} >= {64, 128, 256, 320, 1280} and {c["B"] for c in cs} >= {1, 15, 16, 17, 32, 33, 64, 65, 130}
    assert all(c["V"] * c["d"] <= 65536 * 64 for c in cs)
    assert any(c["ldpad"] != (0, 0) for c in cs) and any(c["ldpad"] == (0, 0) for c in cs)
    tops = {(c["V"], t) for c in cs for t, _ in c["plant"]}
    assert all((V, 0) in tops and (V, V - 1) in tops for V in (15, 16, 17, 63, 64, 65, 333, 65536))
    waves = {((t % 64) // 16, (t % 16) // 4) for c in cs if "waves-and-fq" in c["name"] for t, _ in c["plant"]}
    assert waves == {(w, f) for w in range(4) for f in range(4)}
    for V in (16385, 65536):
        assert {t // 64 for c in cs if c["V"] == V for t, _ in c["plant"]} >= {0, 255, 256, (V - 1) // 64}
    ties = [(t, u) for c in cs for t, u in c["plant"] if u is not None]
    assert any(t // 4 == u // 4 for t, u in ties) and any(t // 16 == u // 16 and t // 4 != u // 4 for t, u in ties)
    assert any(t // 64 == u // 64 and t // 16 != u // 16 for t, u in ties) and any(t // 64 != u // 64 for t, u in ties)
    assert any(abs(t // 64 - u // 64) == 256 for t, u in ties)
    assert {c["mask"] for c in cs} >= {"none", "top", "all", "begin", "both"}
    assert any(c["mask"] == "begin" and c["step"] == c["first"] for c in cs) and any(c["mask"] == "begin" and c["step"] not in (None, c["first"]) for c in cs)
    # every instantiation and dispatch branch: (type, B operands), grid.y > 1, both k loops, the finish kernel's second round
    nb = lambda B: 1 if B <= 16 else 2 if B <= 32 else 4
    assert {(c["dt"], nb(c["B"])) for c in cs} == {(d, n) for d in sc.DTS for n in (1, 2, 4)}
    assert any(c["B"] > 64 for c in cs) and any(c["d"] < 256 for c in cs) and any(c["d"] >= 256 and c["d"] % 256 for c in cs) and any(c["d"] % 256 == 0 for c in cs)
    assert any((c["V"] + 63) // 64 > 256 for c in cs)


def test_whisper_advance_coverage():
    cs = _cases("wa", ok=True)
    assert {c["B"] for c in cs} >= {1, 255, 256, 257, 300} and {c["d"] for c in cs} >= {8, 384, 1280}
    assert {c["dt"] for c in cs} == set(sc.DTS)
    for c in cs:
        assert (c["ld_tok"], c["n_ctx"]) == (5, 9)
    assert {c["pos"] for c in cs} >= {-1, 0, 4, 5, 7, 8}
    assert any(c["live"] == "only256" and c["B"] > 256 for c in cs) and any(c["ldpad"] == (0, 0) for c in cs) and any(c["ldpad"] != (0, 0) for c in cs)
    drv = _driver()
    k = drv.WaKase(next(c for c in cs if c["B"] == 255))
    assert k.st["token"][0] == -1 and k.st["token"][1] == k.c["V"] and k.st["token"][2] == k.c["eot"] and k.st["done"][3] and not k.st["done"][4]


def test_beam_select_coverage():
    cs = _cases("bs", ok=True)
    cr = [c for c in cs if c["kind"] == "crafted"]
    assert {(c["beam"], c["V"]) for c in cr} >= set(sc.BS_SHAPES) and (64, 8192) in sc.BS_SHAPES
    for beam, V in sc.BS_SHAPES:
        assert {c["step"] for c in cr if (c["beam"], c["V"]) == (beam, V)} >= {0, 1, 3, 5}            # min_len 2, max_len 5 for clip 1
        assert {c["ldpad"] > 0 for c in cr if (c["beam"], c["V"]) == (beam, V)} == {True, False}
    lives = {n for c in cs if isinstance(c["n_live"], list) for n in c["n_live"]}
    assert lives >= {-1, 0, 1, 5, 10} and any(c["null_live"] for c in cs) and any(c.get("null_fin") for c in cs)
    assert any(c["pad"] == -1 and c["unk"] == -1 for c in cs)
    assert {(c["kind"], c["V"]) for c in cs} >= {("topbyte", 6), ("tierows", 36), ("tierows", 8192)}


def test_beam_advance_coverage():
    cs = _cases("bd", ok=True)
    assert {c["beam"] for c in cs} >= {1, 2, 3, 64} and {c["L"] for c in cs} >= {2, 3, 40} and {c["d"] for c in cs} >= {8, 512, 1536}
    assert {c["B"] for c in cs} >= {1, 3, 70} and {c["script"] for c in cs} == set(sc.BD_SCRIPTS)
    assert {(c["lenpen"], c["normalize"]) for c in cs} >= {(lp, n) for lp in (0.0, 1.0, 2.0) for n in (0, 1)}
    assert any(c["ldpad"] == (0, 0) for c in cs) and any(c["ldpad"] != (0, 0) for c in cs)
    assert {(c["dt"], c["script"]) for c in cs} == {(d, s) for d in sc.DTS for s in sc.BD_SCRIPTS}
    # what the scripts do, on the reference tables
    drv = _driver()
    seen = set()
    for c in cs:
        k = drv.BdKase(c)
        S = k.reference(list(range(k.B)))
        beam, st = c["beam"], int(S["step"][0])
        assert st == k.nsteps
        if c["script"] == "noroom":
            assert st + 1 > c["L"] and not S["finished"].any() and int(S["n_active"][0]) == k.B         # steps went by without room: state kept, clips unfinished
            seen.add("noroom")
        if c["script"] == "maxlen" and beam > 1:
            assert S["finished"].all() and (S["nhyp"] < beam).all() and (S["out_len"][:, -1] == 0).all()
            seen.add("maxlen")
        if c["script"] == "eos-late":
            assert S["finished"].all() and (S["hyp_len"][S["hyp_len"] > 0] == 4).all()     # nothing finalised before the step at max_len = 3
            seen.add("eos-late")
        if c["script"] == "eos-neginf":
            assert not S["finished"].any() and (S["nhyp"] == 0).all()
            seen.add("eos-neginf")
        if c["script"] == "nhyp-mid" and beam > 2:
            assert S["finished"].all() and (S["nhyp"] == beam).all() and len(set(S["out_len"][0].tolist())) == 2
            seen.add("nhyp-mid")
        if c["script"] == "equal":
            assert S["finished"].all() and (S["out_score"] == S["out_score"][:, :1]).all()
            seen.add("equal")
        if c["script"] == "outlen" and beam > 2:
            assert S["finished"].all() and len(set(S["out_len"][0][:int(S["nhyp"][0])].tolist())) >= 3
            seen.add("outlen")
        if c["script"] == "inert":
            assert S["finished"][1] and S["nhyp"][1] == 0 and np.isnan(S["x"][beam:2 * beam]).all()
            seen.add("inert")
        if c["script"] == "clamp":
            assert (k.cl < 0).any() and (k.cl >= beam).any() and (k.ct < 0).any() and (k.ct >= c["V"]).any()
            seen.add("clamp")
    assert seen == {"noroom", "maxlen", "eos-late", "eos-neginf", "nhyp-mid", "equal", "outlen", "inert", "clamp"}


def test_closed_loop_coverage():
    cs = _cases("loop", ok=True)
    assert {c["beam"] for c in cs} == {3, 8} and all(c["L"] == 20 and c["steps"] == 12 and c["B"] == 3 and len(set(c["max_len"])) == 3 for c in cs)


def test_ctc_beam_search_coverage():
    cs = _cases("ct", ok=True)
    assert {c["beam"] for c in cs} >= {1, 2, 30, 64} and {c["K"] for c in cs} >= {1, 2, 40, 64} and {c["L"] for c in cs} >= {1, 2, 50}
    assert all(any(c["beam"] == b and c["nbest"] == n for c in cs) for b in (2, 30, 64) for n in (1, b) if (b, n) != (64, 1) and (b, n) != (2, 1)) \
        and {c["nbest"] for c in cs} >= {1, 2, 30, 64}
    assert any(c["beam"] == 30 and c["K"] == 40 and c["L"] == 50 for c in cs) and any(c["beam"] == 64 and c["K"] == 64 for c in cs) and any(c["beam"] == 64 and c["L"] == 50 for c in cs)
    lens = {n - c["L"] if n >= c["L"] else n for c in cs if c["lens"] for n in c["lens"]}
    assert lens >= {0, 1, 3} and any(c["lens"] and c["L"] in c["lens"] for c in cs) and any(n < 0 for c in cs if c["lens"] for n in c["lens"])
    assert {c["len_mul"] for c in cs} >= {1, 2} and any(c["lens"] is None for c in cs)
    assert {c["kind"] for c in cs} == set(sc.CT_KINDS)
    drv = _driver()
    for c in cs:
        k = drv.CtKase(c)
        tops = k.cls[:, :, :]
        if c["kind"] == "noblank":
            assert (tops != 0).all()
        if c["kind"] == "blankfirst":
            assert (k.cls[:, :, 0] == 0).all()
        if c["kind"] == "repeat":
            assert len({int(x) for x in k.cls[:, :, 0].reshape(-1)}) == 1 and k.cls[0, 0, 0] != 0
        if c["kind"] == "ties":
            assert any(k.lp[b, t, i].tobytes() == k.lp[b, t, i + 1].tobytes() for b in range(k.B) for t in range(c["L"]) for i in range(c["K"] - 1))
        if c["kind"] == "revival":                           # the trie-less answer differs: a pruned prefix does come back
            assert any(ctcr.beam_search(k.probs[b], beam=c["beam"], cutoff_top_n=c["K"], fresh_ids=True) != k.refs[b] for b in range(k.B))
        # a beam that does not exist, somewhere in the matrix
    assert any(len(drv.CtKase(c).refs[b]) < c["nbest"] for c in cs for b in range(c["B"]))
    for B, L, beam in ((1, 1, 1), (3, 50, 30), (2, 50, 64), (1, 8191, 64), (1, 8192, 64), (1, 4, 65), (0, 4, 2)):
        per = (max(64, 1 << (2 * (beam * L + 1) - 1).bit_length()) + beam * L + 1) * 8
        assert drv.ctc_need_bytes(B, L, beam) == (B * per if 0 < beam <= 64 and B > 0 and beam * L + 1 < 1 << 19 else 0)
    src = _src("ctc.hip")
    assert "const size_t need = 2 * ((size_t)beam * L + 1);" in src and "size_t cap = 64;" in src and "(size_t)beam * L + 1 >= (1u << 19)" in src
    assert "pf_cls = (uint32_t)pf_cls < (uint32_t)kCtcMaxV ? pf_cls : 0;" in src and "if (tid < K && Lb > 0)" in src


def _line_ct(c):
    B, L, K, beam, nbest = (c.get(k + "_arg", c[k]) for k in ("B", "L", "K", "beam", "nbest"))
    drv = _driver()
    checks = [any(_null(c, n) for n in ("topk_cls", "topk_lp", "work", "labels", "lengths", "scores")), B <= 0 or L <= 0 or K < 1 or beam < 1 or nbest < 1 or nbest > beam,
              K > 64 or beam > 64, c["lens"] is not None and c["len_mul"] <= 0, drv.ctc_need_bytes(B, L, beam) == 0,
              c.get("ws_short", 0) > 0 or _al(c, "work", 7)]
    return checks, [sc.EINVAL, sc.ESHAPE, sc.EUNSUPPORTED, sc.EINVAL, sc.EUNSUPPORTED, sc.ESHAPE]


def test_ctc_reference_agrees_with_its_trie_form():
    """the cases are judged by tests/_ctc_reference.py beam_search itself; its trace argument changes nothing it returns"""
    drv = _driver()
    for c in _cases("ct", ok=True):
        if c["beam"] > 3 or c["kind"] == "ties":             # the PathTrie form leaves ties to the sort, and costs seconds at wide beams
            continue
        k = drv.CtKase(c)
        for b in range(k.B):
            p = k.probs[b][:k.frames[b]]
            trie = ctcr.beam_search_trie(p, beam=c["beam"], cutoff_top_n=c["K"])
            assert [lab for lab, _ in trie] == [lab for lab, _ in k.refs[b]] and all(abs(a[1] - z[1]) <= 1e-12 for a, z in zip(trie, k.refs[b]))
            assert ctcr.beam_search(p, beam=c["beam"], cutoff_top_n=c["K"]) == k.refs[b]


# ---- refusals: a restatement of every launcher's checks, in the source's order ---------------------------------------------------------------------
def _al(c, name, mask):
    return bool(c.get("off", {}).get(name, 0) & mask)


def _null(c, name):
    return c.get("null") == name


def _line_kv(c):
    W0 = 64 * c["H"]
    ld = {**dict(q=W0 + c["pads"][0], out=W0 + c["pads"][1], new=W0 + c["pads"][2]), **c.get("ld_arg", {})}
    B, H, T = c.get("B_arg", c["B"]), c.get("H_arg", c["H"]), c.get("T_arg", c["T"])
    self_ = c["form"] == "self"
    has_k = (self_ and c["append"] or c.get("null") in ("k_new", "v_new")) and not _null(c, "k_new")
    has_v = (self_ and c["append"] or c.get("null") in ("k_new", "v_new")) and not _null(c, "v_new")
    has_pos = self_ and not _null(c, "pos")
    W = H * 64
    checks = [any(_null(c, n) for n in ("q", "kc", "vc", "out")), has_k != has_v, has_k and not has_pos, c["stride"] not in (0, 1),
              B <= 0 or H <= 0 or T <= 0, ld["q"] < W or ld["out"] < W or (has_k and ld["new"] < W), not has_pos and not 0 <= c["n_valid"] <= T,
              c.get("dtype_arg", 0) not in (0, 1), W > 1280 or T > 1500 or B > 65535,
              bool(ld["q"] & 7 or ld["out"] & 7 or ld["new"] & 7) or any(_al(c, n, 15) for n in ("q", "kc", "vc", "k_new", "v_new", "out")) or _al(c, "pos", 3)]
    codes = [sc.EINVAL] * 4 + [sc.ESHAPE] * 3 + [sc.EUNSUPPORTED] * 2 + [sc.EALIGN]
    return checks, codes


def _line_ba(c):
    W0 = c["H"] * c["hd"]
    ld = {**dict(q=W0 + c["pads"][0], out=W0 + c["pads"][1], new=W0 + c["pads"][2]), **c.get("ld_arg", {})}
    B, H, T, beam, hd = (c.get(k + "_arg", c[k]) for k in ("B", "H", "T", "beam", "hd"))
    self_ = c["form"] == "self"
    has_k, has_v = self_ and not _null(c, "k_new"), self_ and not _null(c, "v_new")
    has_anc = (self_ or c.get("extra") == "anc") and not _null(c, "anc")
    has_step = self_ and not _null(c, "step")
    has_len = (not self_ or c.get("extra") == "enc_lens") and not _null(c, "enc_lens")
    W = H * hd
    checks = [any(_null(c, n) for n in ("q", "kc", "vc", "out")), has_k != has_v, has_k and (not has_anc or not has_step or has_len), not has_k and (not has_len or has_anc),
              B <= 0 or beam <= 0 or H <= 0 or T <= 0, hd not in (64, 128, 192), ld["q"] < W or ld["out"] < W or (has_k and ld["new"] < W),
              c.get("dtype_arg", 0) not in (0, 1), W > 1536 or beam > 64 or T > 32767 or B > 65535,
              bool(ld["q"] & 7 or ld["out"] & 7 or ld["new"] & 7) or any(_al(c, n, 15) for n in ("q", "kc", "vc", "k_new", "v_new", "out")) or _al(c, "anc", 1)
              or any(_al(c, n, 3) for n in ("step", "enc_lens", "n_live"))]
    codes = [sc.EINVAL] * 4 + [sc.ESHAPE, sc.EUNSUPPORTED, sc.ESHAPE, sc.EUNSUPPORTED, sc.EUNSUPPORTED, sc.EALIGN]
    return checks, codes


def _line_va(c):
    ld = {**dict(x=c["d"] + c["ldpad"][0], emb=c["d"] + c["ldpad"][1]), **c.get("ld_arg", {})}
    B, V, d = (c.get(k + "_arg", c[k]) for k in ("B", "V", "d"))
    checks = [any(_null(c, n) for n in ("x", "emb", "work", "token", "logprob")), c["mask"] in ("begin", "both") and c["step"] is None,
              B <= 0 or V <= 0 or d <= 0, ld["x"] < d or ld["emb"] < d, c.get("dtype_arg", 0) not in (0, 1), V > 65536 or bool(d & 63) or d > 1280,
              bool(ld["x"] & 7 or ld["emb"] & 7) or _al(c, "x", 15) or _al(c, "emb", 15) or any(_al(c, n, 3) for n in ("work", "token", "logprob", "logits", "step"))]
    return checks, [sc.EINVAL, sc.EINVAL, sc.ESHAPE, sc.ESHAPE, sc.EUNSUPPORTED, sc.EUNSUPPORTED, sc.EALIGN]


def _line_wa(c):
    ld = {**dict(x=c["d"] + c["ldpad"][0], emb=c["d"] + c["ldpad"][1]), **c.get("ld_arg", {})}
    B, V, d, ld_tok, n_ctx, eot = (c.get(k + "_arg", c[k]) for k in ("B", "V", "d", "ld_tok", "n_ctx", "eot"))
    names = ("token", "logprob", "tokens", "sum_logprob", "lengths", "done", "emb", "pos_emb", "x", "pos", "n_active")
    checks = [any(_null(c, n) for n in names), B <= 0 or V <= 0 or d <= 0 or ld_tok <= 0 or n_ctx <= 0, eot < 0 or eot >= V, ld["emb"] < d or ld["x"] < d,
              c.get("dtype_arg", 0) not in (0, 1), bool(d & 7) or d > 1280 or V > 65536,
              bool(ld["emb"] & 7 or ld["x"] & 3) or any(_al(c, n, 15) for n in ("emb", "pos_emb", "x")) or any(_al(c, n, 3) for n in names)]
    return checks, [sc.EINVAL, sc.ESHAPE, sc.EINVAL, sc.ESHAPE, sc.EUNSUPPORTED, sc.EUNSUPPORTED, sc.EALIGN]


def _line_bs(c):
    B, beam, V = (c.get(k + "_arg", c[k]) for k in ("B", "beam", "V"))
    ldl, eos, temp = c.get("ldl_arg", c["V"] + c["ldpad"]), c.get("eos_arg", 2), c.get("temp_arg", 1.25)
    served = 0 < beam <= 64 and V <= 8192 and V >= 2 * beam + 2
    checks = [any(_null(c, n) for n in ("logits", "scores", "step", "max_len", "cand_score", "cand_slot", "cand_token")), B <= 0 or beam <= 0 or V <= 0 or ldl < V,
              not temp > 0, eos < 0 or eos >= V, not served or B > 65535,
              any(_al(c, n, 3) for n in ("logits", "scores", "step", "max_len", "n_live", "cand_score", "cand_slot", "cand_token"))]
    return checks, [sc.EINVAL, sc.ESHAPE, sc.EINVAL, sc.EINVAL, sc.EUNSUPPORTED, sc.EALIGN]


def _line_bd(c):
    ld = {**dict(emb=c["d"] + c["ldpad"][0], x=c["d"] + c["ldpad"][1]), **c.get("ld_arg", {})}
    B, beam, L, V, d = (c.get(k + "_arg", c[k]) for k in ("B", "beam", "L", "V", "d"))
    eos = c.get("eos_arg", 2)
    drv = _driver()
    names = ["cand_score", "cand_slot", "cand_token"] + [n for n, _ in drv.ADV_STATE] + ["max_len", "emb", "pos_table", "x", "step", "n_active"]
    assert len(names) == 22
    checks = [any(_null(c, n) for n in names), B <= 0 or beam <= 0 or L < 2 or V <= 0 or d <= 0, eos < 0 or eos >= V or ld["emb"] < d or ld["x"] < d,
              c.get("dtype_arg", 0) not in (0, 1), beam > 64 or V > 8192 or bool(d & 7) or d > 1536 or L > 32767,
              bool(ld["emb"] & 7) or _al(c, "emb", 15) or _al(c, "anc", 1) or any(_al(c, n, 3) for n in ("pos_table", "x", "tokens", "scores", "step", "n_active"))]
    return checks, [sc.EINVAL, sc.ESHAPE, sc.ESHAPE, sc.EUNSUPPORTED, sc.EUNSUPPORTED, sc.EALIGN]


LINES = {"kv": (_line_kv, "whisper_decode.hip", "l2s_kv_attention"), "ba": (_line_ba, "s2s_decode.hip", "l2s_beam_attention"),
         "va": (_line_va, "whisper_decode.hip", "l2s_vocab_argmax"), "wa": (_line_wa, "whisper_decode.hip", "l2s_whisper_advance"),
         "bs": (_line_bs, "s2s_decode.hip", "l2s_beam_select"), "bd": (_line_bd, "s2s_decode.hip", "l2s_beam_advance"),
         "ct": (_line_ct, "ctc.hip", "l2s_ctc_beam_search")}


@pytest.mark.parametrize("op", list(LINES))
def test_every_refusal_line_has_a_case_and_every_case_its_code(op):
    fn, src, entry = LINES[op]
    body = _entry(_src(src), entry)
    in_source = re.findall(r"return (L2S_E[A-Z]+);", body)
    code_of = {"L2S_EINVAL": sc.EINVAL, "L2S_ESHAPE": sc.ESHAPE, "L2S_EALIGN": sc.EALIGN, "L2S_EUNSUPPORTED": sc.EUNSUPPORTED}
    hit = set()
    for c in _cases(op):
        checks, codes = fn(c)
        assert [code_of[s] for s in in_source] == codes, "the restatement lists the source's refusal lines in order"
        first = next((i for i, bad in enumerate(checks) if bad), None)
        assert (sc.OK if first is None else codes[first]) == c["expect"], (c["name"], first)
        if first is not None:
            hit.add(first)
    assert hit == set(range(len(codes))), (op, set(range(len(codes))) - hit)


# ---- the restatements are the ones the project already trusts ------------------------------------------------------------------------------------
def test_reference_agrees_with_the_whisper_restatement():
    r16 = lambda a: sr.round16(a, "f16")
    B, H, T = 3, 2, 70
    q, k, v, kn, vn = whr.attention_case(5, B, H, T, r16)
    flat = lambda a: a.reshape(a.shape[:-2] + (H * 64,))
    for valid, new in (((1, 64, 70), True), ((65, 2, 9), False)):
        want, wk, wv = whr.kv_attention(q, k, v, np.asarray(valid), *((kn, vn) if new else ()))
        got, gk, gv, _ = sr.kv_attention(flat(q), flat(k), flat(v), H, pos=np.asarray(valid) - 1, k_new=flat(kn) if new else None, v_new=flat(vn) if new else None)
        assert np.abs(got - flat(want)).max() <= 1e-12 and np.array_equal(gk, flat(wk)) and np.array_equal(gv, flat(wv))
    want, _, _ = whr.kv_attention(q, k, v, np.full(B, 33))
    assert np.abs(sr.kv_attention(flat(q), flat(k), flat(v), H, n_valid=33)[0] - flat(want)).max() <= 1e-12
    rng = np.random.default_rng(3)
    lg = rng.standard_normal((4, 50))
    forbid = rng.random(50) < 0.3
    ids, lp, _ = whr.masked_argmax(lg, forbid)
    gi, gl = sr.masked_argmax(lg, forbid)
    assert np.array_equal(ids, gi) and np.abs(lp - gl).max() <= 1e-12
    V, d, Bq, eot = 20, 8, 6, 7
    emb, pe = rng.standard_normal((V, d)).astype(np.float32), rng.standard_normal((5, d)).astype(np.float32)
    tok, lpv = np.array([3, 25, -1, eot, 9, 11]), -rng.random(Bq).astype(np.float32)
    tokens, slp, ln, done = rng.integers(0, V, (Bq, 4)).astype(np.int32), -rng.random(Bq).astype(np.float32), rng.integers(0, 5, Bq).astype(np.int32), np.array([0, 0, 0, 0, 1, 0], bool)
    for pos in (0, 3, 4):
        w = whr.advance(tok, lpv, tokens, slp, ln, done, emb, pe, pos, eot)
        g = sr.whisper_advance(tok, lpv, tokens, slp, ln, done, emb, pe, pos, eot, np.full((Bq, d), np.nan, np.float32))
        for key in ("token", "tokens", "sum_logprob", "lengths", "done", "pos", "n_active"):
            assert np.array_equal(np.asarray(w[key]), np.asarray(g[key])), (pos, key)
        assert (w["x_next"] is None and np.isnan(g["x_next"]).all()) or np.array_equal(w["x_next"], g["x_next"])


def test_reference_agrees_with_the_s2s_restatement():
    rng = np.random.default_rng(4)
    B, beam, L, H, W = 3, 4, 12, 2, 128
    q, kn, vn = (rng.standard_normal((B, beam, W)) for _ in range(3))
    kc, vc = rng.standard_normal((B, beam, L, W)), rng.standard_normal((B, beam, L, W))
    anc = rng.integers(0, beam, (2, B, beam, L))
    live, fin = np.array([4, 2, 4]), np.array([0, 0, 1])
    for p in (0, 5, 11):
        want = s2s.beam_attention_self(q, kc.copy(), vc.copy(), kn, vn, anc[p & 1], p, H, n_live=live, finished=fin)
        got, gk, gv = sr.beam_attention_self(q, kc, vc, kn, vn, anc, p, H, live, fin)
        assert np.abs(got - want).max() <= 1e-12
        wk = kc.copy()
        s2s.beam_attention_self(q, wk, vc.copy(), kn, vn, anc[p & 1], p, H, n_live=live, finished=fin)
        assert np.array_equal(gk, wk)
    ck, cv, lens = rng.standard_normal((B, 9, W)), rng.standard_normal((B, 9, W)), np.array([1, 9, 4])
    assert np.abs(sr.beam_attention_cross(q, ck, cv, lens, H, live, fin) - s2s.beam_attention_cross(q, ck, cv, lens, H, n_live=live, finished=fin)).max() <= 1e-12
    assert s2s.round16 is not None and all(np.array_equal(sr.round16(q, a), s2s.round16(q, b)) for a, b in (("f16", "fp16"), ("bf16", "bf16")))
    lg, cum = rng.standard_normal((beam, 30)) * 3, -rng.random(beam)
    lg[1, 4] = np.nan
    for step, ml, nl in ((0, 9, 4), (1, 9, 3), (4, 9, 4), (6, 6, 2)):
        want = s2s.beam_select(lg, cum, step, ml, beam, n_live=nl, min_len=2, temperature=1.25, unk_penalty=0.4, extra=1)
        got = sr.beam_select(lg, cum, step, ml, beam, nl, 2, 1.25, 0.4, extra=1)
        assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
        f = np.isfinite(want[0])
        assert np.array_equal(f, np.isfinite(got[0])) and (not f.any() or np.abs(want[0][f] - got[0][f]).max() <= 1e-12)
    from tests.test_lipread_kernels_gpu import select_tol
    assert all(select_tol(V, np.array([-3.0, -70.0])).tolist() == sr.select_tol(V, np.array([-3.0, -70.0])).tolist() for V in (36, 8192))


@pytest.mark.parametrize("script", ["eos-first", "eos-late", "nhyp-mid", "maxlen", "equal", "outlen", "inert"])
def test_advance_reference_agrees_with_clip_state(script):
    """the table form (both halves of every double buffer, as the device keeps them) against tests/_s2s_reference.py's ClipState"""
    drv = _driver()
    for c in [c for c in _cases("bd", ok=True) if c["script"] == script and c["dt"] == "f16"]:
        k = drv.BdKase(c)
        B, beam, L = k.B, c["beam"], c["L"]
        S = sr.advance_state(B, beam, L, c["d"], k.pre)
        refs = [s2s.ClipState(beam, L) for _ in range(B)]
        for b in range(B):
            refs[b].finished = bool(k.pre[b])
        for s in range(k.nsteps):
            sr.beam_advance(S, k.cs[s], k.cl[s], k.ct[s], k.max_len, k.emb, k.pos, drv.EMBED_SCALE, c["V"], lenpen=c["lenpen"], normalize=bool(c["normalize"]))
            nxt = (s + 1) & 1
            for b, r in enumerate(refs):
                if r.finished:
                    r.step = s + 1
                else:
                    s2s.beam_advance(r, k.cs[s, b].astype(np.float64), k.cl[s, b], k.ct[s, b], k.max_len[b], lenpen=c["lenpen"], normalize=bool(c["normalize"]))
                assert bool(S["finished"][b]) == r.finished and int(S["nhyp"][b]) == len(r.hyps), (c["name"], s, b)
                if not r.finished:
                    n = r.n_live
                    assert int(S["n_live"][b]) == n
                    assert np.array_equal(S["tokens"][nxt, b, :n, :s + 2], r.tokens[:n, :s + 2]) and np.array_equal(S["anc"][nxt, b, :n, :s + 2], r.anc[:n, :s + 2])
                    assert np.array_equal(S["scores"][nxt, b, :n], r.scores[:n].astype(np.float32)) and np.array_equal(S["parents"][b, :n], r.parents[:n])
                elif r.out is not None:
                    for i, (toks, score) in enumerate(r.out):
                        assert int(S["out_len"][b, i]) == len(toks) and S["out_tokens"][b, i].tolist() == toks + [s2s.PAD] * (L - len(toks))
                        assert abs(float(S["out_score"][b, i]) - score) <= 1e-6 * (1.0 + abs(score))
            assert int(S["n_active"][0]) == sum(0 if r.finished else 1 for r in refs)


# ---- the conditions on the inputs hold, for every case ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", list(sc.PARTS))
def test_every_reference_and_every_condition(part):
    drv = _driver()
    for c in sc.cases_of(part):
        drv.host_reference(c)                                # raises when a gap is lost, a tie is not bit-exact, a planted key does not lead


def test_a_case_that_loses_its_gap_fails():
    drv = _driver()
    c = dict(next(c for c in _cases("va", ok=True) if "ties-lane" in c["name"]))
    k = drv.VaKase(c)
    k.emb[9, 0] += 1e-9                                       # the copy is no longer bit-identical, and the gap is far below the bound
    with pytest.raises(AssertionError, match="lost its gap"):
        k.reference()
    c = dict(next(c for c in _cases("bs", ok=True) if c["kind"] == "tierows" and c["V"] == 36 and c["beam"] == 5))
    k = drv.BsKase(c)
    k.lg[0, 1, 20] += np.float32(1e-5)                        # rows no longer identical: the tie of slots 0 and 1 is not exact any more
    with pytest.raises(AssertionError, match="lost its gap"):
        k.reference(0)
    c = dict(next(c for c in _cases("ct", ok=True) if c["name"] == "ctc/beam30-K40-L50"), seed=0)          # seed 0 was tried first and is not decisive
    with pytest.raises(AssertionError, match="lost its gap"):
        drv.CtKase(c)
