"""The waveform analysis kernels' matrix, host side: the case lists of tests/_wave_cases.py reach every entry with the input and output
types, strides, pads, clip lengths and refusals they claim; a restatement of each kernel's tile arithmetic shows that the cases reach one
tile, a ragged last tile, a tile wholly past the clip and a truncated T_rows; every refusal maps to the code its launcher's source
returns; the conditions on the inputs hold (no frame within 0.01 dB of the STOI threshold, decisive gain levels, a Whisper clamp that
binds; no value is excluded from any comparison); and tests/_wave_reference.py at production parameters reproduces the restatements the
project already trusts to 1e-12.  Nothing here needs a device."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import _hifigan_mel_reference as hr
from tests import _mel_reference as mr
from tests import _spk_reference as sr
from tests import _stoi_reference as st
from tests import _units_reference as ur
from tests import _wave_cases as wc
from tests import _wave_reference as wr
from tests import _whisper_reference as whr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "check_wave_kernels.py")
CSRC = os.path.join(ROOT, "lip2speech_unit_amd", "csrc")
_DRV = []


def _driver():
    if not _DRV:
        spec = importlib.util.spec_from_file_location("check_wave_kernels", TOOL)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _DRV.append(mod)
    return _DRV[0]


def _cases(op=None, ok=None):
    ops = (op,) if isinstance(op, str) else op
    return [c for _, c in wc.all_cases() if (ops is None or c["op"] in ops) and (ok is None or (c["expect"] == 0) == ok)]


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _types(cs):
    return {t for c in cs for t in (("i16", "f32") if c["intype"] == "both" else (c["intype"],))}


def test_constants_match_the_sources():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    for name, val in (("L2S_EINVAL", wc.EINVAL), ("L2S_ESHAPE", wc.ESHAPE), ("L2S_EALIGN", wc.EALIGN), ("L2S_EUNSUPPORTED", wc.EUNSUPPORTED)):
        assert f"{name} = {val}" in hdr
    mel, spk, wh, stem, stoi, fd = (_src(f) for f in ("melspec.hip", "spkemb.hip", "whisper_logmel.hip", "wavestem.hip", "stoi.hip", "frame_dft.h"))
    assert "using Tile640 = FrameDftTile<640, 160, 64, 640>;" in mel and "using Tile1024 = FrameDftTile<1024, 256, 32, 1024>;" in mel
    assert "frame_dft::FrameSpan<400, 160, 32>" in spk and "frame_dft::FrameSpan<400, 160, 32>" in wh
    assert wc.FT == {640: 64, 1024: 32, 400: 32}
    assert "constexpr int FT = 64;" in stem and "for (int t = tid; t < L0; t += 256)" in stem and (wc.STEM_FT, wc.STEM_STAT_STRIDE) == (64, 256)
    assert "RS_OUT = 256" in stoi and "constexpr int FR_WAVES = 16;" in stoi and "const int j0 = 2 * tid, j1 = 2 * tid + 1;" in stoi
    assert (wc.RS_OUT, wc.FR_PER_THREAD, wc.FR_THREADS) == (256, 2, 16 * 64)
    assert "frame_dft::FrameDftTile<FRAME, HOP, 32, 512>" in stoi and "constexpr int SC_SEG = 32" in stoi and (wc.BT_F, wc.SC_SEG) == (32, 32)
    assert "NSAMP = 480000, NFRAME = 3000, PAD = 200" in wh and (wc.WHISPER_S, wc.WHISPER_T) == (480000, 3000)
    assert "constexpr int MAX_FRAMES = 2048;" in stoi and (wc.STOI_MAX_S, wc.STOI_MAX_FRAMES) == (419840, 2048)
    assert wc.len10k(wc.STOI_MAX_S) == 256 + 2048 * 128 and wc.stoi_frames_of(wc.len10k(wc.STOI_MAX_S)) == 2048
    # the frame rules restated in the case generator are the kernels'
    assert "return (n > pad && n + 2 * pad >= Tl::K) ? (n + 2 * pad - Tl::K) / Tl::HOP + 1 : 0;" in fd
    assert "return n >= KW ? (n - KW) / STRIDE + 1 : 0;" in stem and "return (5 * n + 7) / 8;" in stoi
    assert "return len > FRAME ? (len - FRAME - 1) / HOP + 1 : 0;" in stoi
    for n in range(0, 700):
        assert wc.stem_frames(n) == wr.stem_frames(n) and wc.len10k(n) == wr.len10k(n) and wc.stoi_frames_of(n) == wr.stoi_frames_of(n)
        assert wc.stoi_frames_of(n) == len(range(0, n - 256, 128))
        for pad, K_, hop in ((320, 640, 160), (0, 640, 160), (383, 1024, 256), (199, 400, 160)):
            assert wc.reflect_frames(n, pad, K_, hop) == wr.reflect_frames(n, pad, K_, hop)
    for pad, K_, hop in ((320, 640, 160), (1, 640, 160), (0, 640, 160), (512, 1024, 256), (120, 400, 160)):
        for T in (1, 2, 33, 65):
            n = wc.first_n(T, pad, K_, hop)
            assert wc.reflect_frames(n, pad, K_, hop) >= T and wc.reflect_frames(n - 1, pad, K_, hop) < max(T, wc.reflect_frames(n, pad, K_, hop))
    for f in (1, 2, 127, 1025, 2048):
        assert wc.stoi_frames_of(wc.len10k(wc.stoi_n(f))) == f and wc.stoi_frames_of(wc.len10k(wc.stoi_n(f) - 1)) == f - 1
    assert wc.stoi_n(2048) <= wc.STOI_MAX_S
    for k, f in wc.CPU_F32_WORST.items():
        assert k in wc.KINDS and wc.F_of(k) == max(4.0, 4.0 * f)
    assert wc.F_of("stem") == wc.F_of("gain") == wc.F_of("resample") == wc.F_of("bands") == wc.F_of("scores") == wc.F_of("stem16") == 4.0
    assert wc.F_of("whisper16") == wc.F_of("whisper")
    assert (wc.CANARY32, wc.CANARY16, wc.GUARD, wc.MARGIN_DB, wc.TOL_BANDS) == (0x5A5A5A5A, 0x5A5A, 3, 0.01, 4.0e-6)


def test_names_are_unique_and_every_entry_is_reached():
    names = [c["name"] for c in _cases()]
    assert len(names) == len(set(names))
    assert list(wc.PARTS) == ["mel640", "mel1024", "power", "whisper", "stem-gain", "stoi", "refusals"]
    for p in wc.PARTS:
        assert len(wc.cases_of(p)) > 0
    ops = {"mel", "melspec", "power", "whisper", "stem", "gain", "resample", "frames", "bands", "scores"}
    assert {c["op"] for c in _cases(ok=True)} == ops == {c["op"] for c in _cases(ok=False)} == set(_driver().BUILD)
    assert all(c["expect"] != 0 for c in wc.cases_of("refusals")) and all(c["expect"] == 0 for p in wc.PARTS if p != "refusals" for c in wc.cases_of(p))
    # one case per kernel with 70 clips, more than any test has used, at the shortest clip
    for op in ops - {"melspec"}:
        big = [c for c in _cases(op, ok=True) if len(c.get("kinds", c.get("n_kept"))) == 70]
        assert len(big) == (2 if op == "mel" else 1) and all("B70-shortest" in c["name"] for c in big), op
    assert all(len(c.get("kinds", c.get("n_kept"))) <= 7 for c in _cases(ok=True) if "B70" not in c["name"])


def test_types_strides_and_pads():
    for Kf in (640, 1024):
        cs = [c for c in _cases("mel", ok=True) if c["K"] == Kf]
        assert {c["pad"] for c in cs} == set(wc.MEL_PADS[Kf]) and {c["hop"] for c in cs} == {wc.MEL_HOP[Kf]}
        assert wc.MEL_PADS[640] == (320, 240, 1, 319, 0) and wc.MEL_PADS[1024] == (384, 512, 0, 383)
        for pad in wc.MEL_PADS[Kf]:
            mine = [c for c in cs if c["pad"] == pad]
            assert _types(mine) == {"i16", "f32"}
            assert {c["ldw"] - c["S"] for c in mine} == {0, 3} and {c["ldm"] for c in mine} == {80, 83}
            # the last n without a frame and the first with one, n = pad and n = pad + 1
            rule = [c for c in mine if c["name"].endswith("frame-rule")][0]
            n1, hop = rule["ns"][1], wc.MEL_HOP[Kf]
            assert wc.reflect_frames(n1 - 1, pad, Kf, hop) == 0 < wc.reflect_frames(n1, pad, Kf, hop) and rule["ns"] == [n1 - 1, n1, pad, pad + 1]
            # T_b either side of a tile edge in one batch; T_rows at the largest T_b, a tile beyond, and below a clip's T_b at 1, FT, FT + 1
            ft = wc.FT[Kf]
            tiles = [c for c in mine if "-tiles-" in c["name"]]
            tb = [wc.reflect_frames(n, pad, Kf, hop) for n in tiles[0]["ns"]]
            assert tb == [ft - 1, ft, ft + 1, 2 * ft + 1] == list(wc.MEL_TB[Kf])
            assert [c["T_rows"] for c in tiles] == [2 * ft + 1, 3 * ft + 1, 1, ft, ft + 1]
            hot = [c for c in mine if c["name"].endswith("one-hot")][0]
            n = hot["ns"][0]
            assert {int(k.split(":")[1]) for k in hot["kinds"]} == {0, pad, n - 1 - pad, n - 1}
            assert {k for c in mine for k in c["kinds"]} >= {"noise", "zeros", "dc", "extreme"}
        assert {c["mag_eps"] for c in cs} == {0.0, 1e-9} and {c["floor"] for c in cs} == {1e-5, 1e-10} and {c["fb"] for c in cs} == {"prod", "edge"}
        assert any(c["ns"] is None for c in cs)
        clamp = [c for c in cs if c["ns"] and any(n > c["S"] for n in c["ns"])]
        assert clamp and {n - clamp[0]["S"] for n in clamp[0]["ns"]} >= {5} and {0, -3} <= set(clamp[0]["ns"])
    twins = _cases("melspec", ok=True)
    assert len(twins) >= 6 and all((c["K"], c["pad"], c["mag_eps"]) == (640, 320, 0.0) for c in twins) and _types(twins) == {"i16", "f32"}
    assert {c["ldw"] - c["S"] for c in twins} == {0, 3} and {c["ldm"] for c in twins} == {80, 83} and any(c["ns"] is None for c in twins)
    assert {c["name"].replace("melspec/", "mel/") for c in twins} <= {c["name"] for c in _cases("mel", ok=True)}

    cs = _cases("power", ok=True)
    assert {c["pad"] for c in cs} == set(wc.POWER_PADS) == {200, 120, 0, 199}
    for pad in wc.POWER_PADS:
        mine = [c for c in cs if c["pad"] == pad]
        assert _types(mine) == {"i16", "f32"} and {c["ldw"] - c["S"] for c in mine} == {0, 3} and {c["ldm"] for c in mine} == {40, 43}
        assert {c["scale"] is None for c in mine} == {True, False}
        past = [c for c in mine if c["ns"] and any(n > c["S"] for n in c["ns"])]
        assert {c["nv"] is None for c in past} == {True, False}
        nv = [c for c in past if c["nv"] is not None][0]
        assert nv["nv"][0] == nv["ns"][0] > nv["S"] and 0 < nv["nv"][1] < nv["S"] and nv["nv"][2] == 0
        tiles = [c for c in mine if "-tiles-" in c["name"]]
        assert [wc.reflect_frames(n, pad, 400, 160) for n in tiles[0]["ns"]] == [31, 32, 33, 65] and [c["T_rows"] for c in tiles] == [65, 97, 1, 32, 33]
    assert any(c["ns"] is None for c in cs) and any(c["ns"] and min(c["ns"]) < 0 for c in cs)

    cs = _cases("whisper", ok=True)
    assert {c["ld"] for c in cs} == {80, 88, 96} and {c["f32out"] for c in cs} == {True, False} and {c["dt"] for c in cs} == {"f16", "bf16"}
    assert _types(cs) == {"i16", "f32"} and {c["ldw"] - c["S"] for c in cs} == {0, 3}
    for dt in ("f16", "bf16"):
        assert {c["f32out"] for c in cs if c["dt"] == dt} == {True, False}
    lens = {n for c in cs if c["ns"] for n in c["ns"]}
    edge = 160 * 32 - 200
    assert {0, 1, 200, 201, edge, edge + 1} <= lens and any(c["ns"] is None and c["S"] == 480000 for c in cs) and any(n > c["S"] for c in cs if c["ns"] for n in c["ns"])
    loud = [c for c in cs if "loudest" in c["name"]]
    assert len(loud) == 2 and all([int(k.split(":")[1]) for k in c["kinds"]] == [0, 1500, 2999] for c in loud)
    assert all(len({k.split(":")[2] for k in c["kinds"]}) == 3 for c in loud)         # batch mates whose maxima differ

    cs = _cases("stem", ok=True)
    assert {c["dt"] for c in cs} == {"f32", "f16", "bf16"} and _types(cs) == {"i16", "f32"}
    for dt in ("f32", "f16", "bf16"):
        mine = [c for c in cs if c["dt"] == dt]
        assert {c["ldo"] for c in mine} == {512, 514} and {c["ldw"] - c["S"] for c in mine} == {0, 3} and {c["eps"] for c in mine} == {1e-5, 1e-3}
        assert {c["T_rows"] - wc.stem_frames(c["S"]) for c in mine} == {0, 64}
        lens = [wc.clip_n(n, c["S"]) for c in mine if c["ns"] for n in c["ns"]]
        assert {9, 10, 14, 15} <= set(lens) and {0, 1, 2, 64, 65, 257} <= {wc.stem_frames(n) for n in lens}
        assert {k for c in mine for k in c["kinds"]} >= {"noise", "const", "dc"} and any(c["ns"] is None for c in mine)
    cs = _cases("gain", ok=True)
    assert _types(cs) == {"i16", "f32"} and {c["ldw"] - c["S"] for c in cs} >= {0, 3} and any(c["ns"] is None for c in cs)
    assert {k for c in cs for k in c["kinds"]} >= {"zeros", "level:+6", "level:+0.5", "level:-0.5"} and any(30000 in c["ns"] for c in cs if c["ns"])

    cs = _cases("resample", ok=True)
    assert _types(cs) == {"i16", "f32"} and {c["ldw"] - c["S"] for c in cs} >= {0, 3} and {c["ldo"] - c["R"] for c in cs} >= {0, 5}
    assert {wc.len10k(n) for c in cs if c["ns"] for n in c["ns"]} >= {0, 1, 5, 255, 256, 257, 513} and {0, 1, 8} <= {n for c in cs if c["ns"] for n in c["ns"]}
    assert any(c["R"] > wc.len10k(c["S"]) for c in cs) and any(c["ns"] is None for c in cs)
    hot = [c for c in cs if "one-hot" in c["name"]][0]
    assert {"onehot:0", f"onehot:{hot['ns'][1] - 1}"} <= set(hot["kinds"])
    cs = _cases("frames", ok=True)
    nf = {wc.stoi_frames_of(wc.len10k(wc.clip_n(n, c["S"]))) for c in cs for n in c["ns"]}
    assert {0, 1, 2, 127, 128, 129, 1023, 1024, 1025, 2048} <= nf
    assert {c["ldx"] - wc.len10k(c["S"]) for c in cs} >= {0, 5} and {c["ldk"] - wc.stoi_frames_of(wc.len10k(c["S"])) for c in cs} >= {0, 3}
    assert any("zeros" in c["kinds"] for c in cs)
    cs = _cases("bands", ok=True)
    assert {n for c in cs for n in c["n_kept"]} >= {0, 1, 2, 32, 33, 34, 66} and {c["kept"] for c in cs} == {"gaps", "outside", "all"}
    assert any(n > c["ldk"] for c in cs for n in c["n_kept"])
    assert {c["ldx"] - wc.len10k(c["S"]) for c in cs} >= {0, 5} and {c["ldk"] - 80 for c in cs} >= {0, 3} and {c["ldf"] - 79 for c in cs} >= {0, 21}
    cs = _cases("scores", ok=True)
    assert {max(n - 1, 0) for c in cs for n in c["n_kept"]} >= {0, 29, 30, 31, 64} and {k for c in cs for k in c["kinds"]} == {"rand", "same", "neg", "zeroband"}
    assert {c["lds"] - max(c["ldf"] - 29, 1) for c in cs} >= {0, 3} and {c["ldf"] for c in cs} >= {64, 69}


def _tile_classes(T_rows, Tb, ft):
    """what the blocks of one clip do: (a single tile, a ragged last live tile, a tile wholly past the clip, rows cut by T_rows)"""
    starts = range(0, T_rows, ft)
    live = [f0 for f0 in starts if f0 < Tb]
    return (len(starts) == 1, any(min(ft, T_rows - f0) > Tb - f0 or T_rows - f0 < ft for f0 in live), any(f0 >= Tb for f0 in starts), T_rows < Tb)


def test_tile_arithmetic():
    reach = {}

    def note(key, cls):
        reach[key] = tuple(a or b for a, b in zip(reach.get(key, (False,) * 4), cls))

    for c in _cases(("mel", "melspec"), ok=True):
        for n in (c["ns"] or [c["S"]]):
            note((c["op"], c["K"]), _tile_classes(c["T_rows"], wc.reflect_frames(wc.clip_n(n, c["S"]), c["pad"], c["K"], c["hop"]), wc.FT[c["K"]]))
    for c in _cases("power", ok=True):
        for n in (c["ns"] or [c["S"]]):
            note("power", _tile_classes(c["T_rows"], wc.reflect_frames(n, c["pad"], 400, 160), 32))
    assert reach[("mel", 640)] == reach[("mel", 1024)] == reach["power"] == (True, True, True, True), reach
    assert reach[("melspec", 640)][1:3] == (True, True)
    # Whisper: 94 tiles of 32 frames, the last one ragged (24); a clip's samples end in the first tile, on its edge, and in the last
    assert wc.cdiv(wc.WHISPER_T, 32) == 94 and wc.WHISPER_T - 93 * 32 == 24
    ends = {(wc.clip_n(n, c["S"]) + 200) // 160 // 32 for c in _cases("whisper", ok=True) for n in (c["ns"] or [c["S"]])}
    assert {0, 1, 93} <= ends
    # wave stem: 64 frames per block, the statistics loop's second trip, a block wholly past the clip
    cls = (False,) * 4
    for c in _cases("stem", ok=True):
        for n in (c["ns"] or [c["S"]]):
            L0 = wc.stem_frames(wc.clip_n(n, c["S"]))
            cls = tuple(a or b for a, b in zip(cls, _tile_classes(c["T_rows"], L0, wc.STEM_FT)[:3] + (L0 > wc.STEM_STAT_STRIDE,)))
    assert cls == (True, True, True, True)
    # resampler: 256 outputs per block
    cls = (False,) * 4
    for c in _cases("resample", ok=True):
        for n in (c["ns"] or [c["S"]]):
            cls = tuple(a or b for a, b in zip(cls, _tile_classes(c["R"], wc.len10k(wc.clip_n(n, c["S"])), wc.RS_OUT)))
    assert cls[:3] == (True, True, True)              # R >= ceil(5 S / 8): the launcher admits no truncation
    # kept-frame scan: a wave's share is 128 frames, the block's 2048
    share = wc.FR_PER_THREAD * 64
    nf = {wc.stoi_frames_of(wc.len10k(wc.clip_n(n, c["S"]))) for c in _cases("frames", ok=True) for n in c["ns"]}
    assert {share - 1, share, share + 1, 8 * share - 1, 8 * share, 8 * share + 1, wc.FR_PER_THREAD * wc.FR_THREADS} <= nf
    # bands: 32 frames per block, F = n_kept - 1; scores: 32 segments per block, M = F - 29
    cls = (False,) * 4
    for c in _cases("bands", ok=True):
        for n, k in zip(c["ns"], c["n_kept"]):
            K_ = max(min(k, wc.stoi_frames_of(wc.len10k(wc.clip_n(n, c["S"]))), c["ldk"]), 0)
            cls = tuple(a or b for a, b in zip(cls, _tile_classes(c["ldf"], max(K_ - 1, 0), wc.BT_F)))
    assert cls[:3] == (True, True, True)
    cls = (False,) * 4
    for c in _cases("scores", ok=True):
        for k in c["n_kept"]:
            cls = tuple(a or b for a, b in zip(cls, _tile_classes(c["lds"], max(min(max(k - 1, 0), c["ldf"]) - 29, 0), wc.SC_SEG)))
    assert cls[:3] == (True, True, True)


# refusal name -> (source file, the check that returns it); `{}` stands for the entry's own operand
REFUSAL_SOURCE = {
    "mel": ("melspec.hip", {
        "null-": "if (!wav || !basis || !fb || !fb_range || !mel) return L2S_EINVAL;", "ldw-below-S": "if (ldw < S || ldm < n_mels) return L2S_ESHAPE;",
        "ldm-below-n_mels": "if (ldw < S || ldm < n_mels) return L2S_ESHAPE;", "n_fft-": "if (!(s640 || s1024) || n_mels != NMEL) return L2S_EUNSUPPORTED;",
        "hop-": "if (!(s640 || s1024) || n_mels != NMEL) return L2S_EUNSUPPORTED;", "n_mels-": "if (!(s640 || s1024) || n_mels != NMEL) return L2S_EUNSUPPORTED;",
        "pad-": "if (pad < 0 || pad > n_fft / 2 || !(mag_eps >= 0.f)) return L2S_EUNSUPPORTED;",
        "mag_eps-": "if (pad < 0 || pad > n_fft / 2 || !(mag_eps >= 0.f)) return L2S_EUNSUPPORTED;", "basis-off": "if ((uintptr_t)basis & 15) return L2S_EALIGN;"}),
    "power": ("spkemb.hip", {
        "null-": "if (!wav || !basis || !fb || !fb_range || !mel) return L2S_EINVAL;", "ldw-below-S": "if (ldw < S || ldm < n_mels) return L2S_ESHAPE;",
        "ldm-below-n_mels": "if (ldw < S || ldm < n_mels) return L2S_ESHAPE;", "n_fft-": "if (n_fft != NFFT || hop != HOP || n_mels != NMEL) return L2S_EUNSUPPORTED;",
        "hop-": "if (n_fft != NFFT || hop != HOP || n_mels != NMEL) return L2S_EUNSUPPORTED;", "n_mels-": "if (n_fft != NFFT || hop != HOP || n_mels != NMEL) return L2S_EUNSUPPORTED;",
        "pad-": "if (pad < 0 || pad > n_fft / 2) return L2S_EUNSUPPORTED;"}),
    "whisper": ("whisper_logmel.hip", {
        "null-": "if (!wav || !basis || !fb || !fb_range || !workspace || !out) return L2S_EINVAL;", "ldw-below-S": "if (B <= 0 || S <= 0 || ldw < S || ld < NMEL) return L2S_ESHAPE;",
        "ld-72": "if (B <= 0 || S <= 0 || ldw < S || ld < NMEL) return L2S_ESHAPE;", "S-480001": "if (S > NSAMP || B > 65535) return L2S_EUNSUPPORTED;",
        "dtype-f32": "if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;", "ld-84": "if ((ld & 7) ||", "work-off": "((uintptr_t)workspace & 15)"}),
    "stem": ("wavestem.hip", {
        "null-": "if (!wav || !w || !gamma || !beta || !out || !workspace) return L2S_EINVAL;",
        "dtype-3": "if (dtype != L2S_F16 && dtype != L2S_BF16 && dtype != L2S_F32) return L2S_EINVAL;", "ldw-below-S": "if (ldw < S || ldo < C) return L2S_ESHAPE;",
        "ldo-below-C": "if (ldw < S || ldo < C) return L2S_ESHAPE;", "T_rows-below": "if (T_rows < stem_frames(S)) return L2S_ESHAPE;",
        "C-256": "if (C != 512) return L2S_EUNSUPPORTED;", "workspace-one-byte-short": "if (workspace_bytes < l2s_wave_stem_workspace(B, C)) return L2S_ESHAPE;",
        "ldo-odd": "|| (ldo & 1))\n    return L2S_EALIGN;"}),
    "gain": ("spkemb.hip", {"null-": "if (!wav || !gain) return L2S_EINVAL;", "ldw-below-S": "if (B <= 0 || S <= 0 || ldw < S) return L2S_ESHAPE;"}),
    "resample": ("stoi.hip", {
        "null-": "if (!wav || !taps || !out) return L2S_EINVAL;", "S-419841": "if (B > 65535 || !size_ok(S)) return L2S_EUNSUPPORTED;",
        "ldw-below-S": "if (ldw < S || R < len10k(S) || R > MAX_LEN10K || ldo < R) return L2S_ESHAPE;",
        "R-below": "if (ldw < S || R < len10k(S) || R > MAX_LEN10K || ldo < R) return L2S_ESHAPE;",
        "ldo-below-R": "if (ldw < S || R < len10k(S) || R > MAX_LEN10K || ldo < R) return L2S_ESHAPE;"}),
    "frames": ("stoi.hip", {
        "null-": "if (!x || !window || !kept || !n_kept) return L2S_EINVAL;", "S-419841": "if (B > 65535 || !size_ok(S)) return L2S_EUNSUPPORTED;",
        "ldx-below": "if (ldx < len10k(S) || ldk < frames_of(len10k(S))) return L2S_ESHAPE;",
        "ldk-below": "if (ldx < len10k(S) || ldk < frames_of(len10k(S))) return L2S_ESHAPE;"}),
    "bands": ("stoi.hip", {
        "null-": "if (!x || !y || !kept || !n_kept || !window || !basis || !band_edges || !bands) return L2S_EINVAL;",
        "S-419841": "if (B > 65535 || !size_ok(S) || ldf > MAX_FRAMES) return L2S_EUNSUPPORTED;", "ldf-2049": "if (B > 65535 || !size_ok(S) || ldf > MAX_FRAMES) return L2S_EUNSUPPORTED;",
        "ldx-below": "if (ldx < len10k(S) || ldk < frames_of(len10k(S)) || ldf < frames_of(len10k(S)) - 1) return L2S_ESHAPE;",
        "ldk-below": "if (ldx < len10k(S) || ldk < frames_of(len10k(S)) || ldf < frames_of(len10k(S)) - 1) return L2S_ESHAPE;",
        "ldf-below": "if (ldx < len10k(S) || ldk < frames_of(len10k(S)) || ldf < frames_of(len10k(S)) - 1) return L2S_ESHAPE;",
        "basis-off": "if ((uintptr_t)basis & 15) return L2S_EALIGN;"}),
    "scores": ("stoi.hip", {
        "null-": "if (!bands || !n_kept || !seg || !stoi || !estoi || !n_segments) return L2S_EINVAL;", "ldf-2049": "if (B > 65535 || ldf > MAX_FRAMES) return L2S_EUNSUPPORTED;",
        "lds-below": "if (lds < ldf - NSEG + 1) return L2S_ESHAPE;", "seg-off": "((uintptr_t)seg & 7)"}),
}
CODE_NAME = {wc.EINVAL: "L2S_EINVAL", wc.ESHAPE: "L2S_ESHAPE", wc.EALIGN: "L2S_EALIGN", wc.EUNSUPPORTED: "L2S_EUNSUPPORTED"}


def test_every_refusal_maps_to_the_code_its_launcher_returns():
    used = set()
    for c in _cases(ok=False):
        op = "mel" if c["op"] == "melspec" else c["op"]
        fname, table = REFUSAL_SOURCE[op]
        src = _src(fname)
        what = re.sub(r"^K\d+-", "", c["name"].split("/refused-")[1])
        if c["op"] == "stem":
            what = what.rsplit("-", 1)[0]                                 # the output type in the name
        keys = [k for k in table if what.startswith(k)]
        assert len(keys) == 1, (c["name"], keys)
        snippet = table[keys[0]]
        assert snippet in src, (c["name"], snippet)
        after = src[src.index(snippet):]
        assert re.search(r"return (L2S_E\w+);", after).group(1) == CODE_NAME[c["expect"]], c["name"]
        used.add((op, keys[0]))
        if keys[0] == "null-":
            operand = {"work": "workspace"}.get(c["null"], c["null"])
            assert f"!{operand}" in snippet, c["name"]
    assert used == {(op, k) for op, (_, t) in REFUSAL_SOURCE.items() for k in t}
    # every NULL check of every launcher has a case per operand
    for op, (_, t) in REFUSAL_SOURCE.items():
        operands = set(re.findall(r"!(\w+)", t["null-"]))
        have = {{"work": "workspace"}.get(c["null"], c["null"]) for c in _cases(ok=False) if c["op"] == op and "null" in c}
        assert have == operands, (op, have, operands)
    ref = {c["name"].split("/refused-")[1]: c for c in _cases("mel", ok=False)}
    assert ref["K640-pad-minus-1"]["pad"] == -1 and ref["K640-pad-past-half"]["pad"] == 321 and ref["K1024-pad-past-half"]["pad"] == 513
    assert ref["K640-mag_eps-negative"]["mag_eps"] < 0 and ref["K1024-mag_eps-nan"]["mag_eps"] != ref["K1024-mag_eps-nan"]["mag_eps"]
    assert ref["ldw-below-S"]["ldw"] == ref["ldw-below-S"]["S"] - 1 and ref["ldm-below-n_mels"]["ldm"] == 79 and ref["basis-off-by-4-bytes"]["off"] == {"basis": 4}
    ref = {c["name"].split("/refused-")[1]: c for c in _cases(("whisper", "resample", "stem", "power"), ok=False)}
    assert ref["S-480001"]["S"] == 480001 and ref["S-419841"]["S"] == 419841 and ref["ld-84-no-multiple-of-8"]["ld"] % 8 == 4 and ref["pad-201"]["pad"] == 201
    assert ref["T_rows-below-frames-of-S-f16"]["T_rows"] == wc.stem_frames(ref["T_rows-below-frames-of-S-f16"]["S"]) - 1 and ref["ldo-odd-f16"]["ldo"] % 2 == 1
    assert ref["workspace-one-byte-short-f16"]["ws_short"] == 1


def test_conditions_on_the_inputs():
    """Kept lists: no frame of the fp64 reference within 0.01 dB of the threshold (FramesKase.refs asserts it and returns the margin);
    gains: every level at least 0.25 dB from the target; Whisper: the clamp binds in every clip of the loudest-frame cases
    (WhisperKase.refs asserts it).  No comparison excludes a value: where the reference's scale is zero the device value must be zero."""
    drv = _driver()
    n = 0
    for c in _cases("frames", ok=True):
        for _, kept, margin, nf in drv.FramesKase(c).refs():
            assert margin > wc.MARGIN_DB and len(kept) <= nf
            n += 1
    assert n >= 80
    zeros = [c for c in _cases("frames", ok=True) if "zeros" in c["kinds"]][0]
    _, kept, margin, nf = drv.FramesKase(zeros).refs()[zeros["kinds"].index("zeros")]
    assert nf == 129 and kept.tolist() == list(range(129))             # an all-zero clip: every frame kept, by the + 2^-52 rule
    gaps = set(drv.FramesKase([c for c in _cases("frames", ok=True) if "1023-1024-1025" in c["name"]][0]).refs()[2][1].tolist())
    assert {125, 130, 253, 258, 1019} <= gaps and not gaps & ({126, 127, 128, 129} | set(range(1020, 1025)))   # gaps across the waves' shares of the scan
    # the one exact tie, decided by the header's rule in rational arithmetic: the silent frames of clip 0 sit ON the threshold
    tie = drv.FramesKase([c for c in _cases("frames", ok=True) if "threshold-tie-exact" in c["name"]][0])
    assert [c["name"] for c in _cases("frames", ok=True) if any(k.startswith("tie:") for k in c["kinds"])] == ["frames/threshold-tie-exact"]
    (k0, slack0), (k1, slack1) = (wr.stoi_kept_exact(tie.x[b, : tie.n10[b]], np.ones(256)) for b in range(2))
    assert k0.tolist() == [4, 5] and [s for j, s in enumerate(slack0) if j not in (4, 5)] == [0] * 10 and k1.tolist() == list(range(12)) and min(slack1) > 0
    assert [r[1].tolist() for r in tie.refs()] == [k0.tolist(), k1.tolist()]
    assert float(np.float32(99 * 2.0 ** -52)) == 99 * 2.0 ** -52 and (99 * 2.0 ** -52 + 2.0 ** -52) * 1e-2 == 2.0 ** -52      # exact in fp32 and in the kernel's fp64
    for c in _cases("gain", ok=True):
        k = drv.GainKase(c)
        for b in range(k.B):
            x = drv.x64_of(k.pcm[b][: k.lens[b]])
            if x.size and x.any():
                assert abs(wr.level_db(x) - c["target"]) > 0.25, (c["name"], b)
    for c in _cases("whisper", ok=True):
        if "loudest" in c["name"] and c["dt"] == "f16":
            refs = drv.WhisperKase(c).refs()
            assert [int(np.unravel_index(r[1].argmax(), r[1].shape)[0]) for r in refs] == [0, 1500, 2999]
            assert len({round(float(r[1].max()), 3) for r in refs}) == 3
    for c in _cases("bands", ok=True):
        if c["kept"] == "outside":
            k = drv.BandsKase(c)
            assert all(k.kept[b, 1] == k.nf[b] and k.kept[b, k.K[b] // 2] == -1 for b in range(k.B))


def test_every_reference_runs():
    drv = _driver()
    for c in _cases(ok=True):
        if c["op"] == "whisper" or len(c.get("kinds", c.get("n_kept"))) == 70 or c.get("S", 0) > 100000:
            continue                                                    # the long ones run in test_conditions_on_the_inputs or on the device
        for r in drv.BUILD[c["op"]](c).refs():
            assert r[1] is not None


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_the_reference_reproduces_the_trusted_restatements():
    pcm = mr.synthetic_clip(n=9000)
    x = mr.as_float64(pcm)
    n = len(x)
    ours = wr.stft_mel(x, n, 320, 640, 160, wr.hann_periodic(640), mr.slaney_filterbank(), 0.0, mr.FLOOR)
    assert ours.shape == (1 + n // 160, 80) and _rel(ours, mr.mel_f64(pcm)) < 1e-12
    ours = wr.stft_mel(x, n, hr.PAD, 1024, 256, wr.hann_periodic(1024), hr.slaney_filterbank(), hr.MAG_EPS, hr.FLOOR)
    assert ours.shape == (hr.num_frames(n), 80) and _rel(ours, hr.mel_f64(x)) < 1e-12
    ours = wr.stft_mel_power(x, n, n, 200, wr.hann_periodic(400), sr.filterbank())
    theirs = sr.mel_power(x)
    assert ours.shape == theirs.shape and float((np.abs(ours - theirs).max(0) / theirs.max(0)).max()) < 1e-12
    ours = wr.whisper_logmel(x, n, wr.hann_periodic(400), whr.mel_filters())
    assert ours.shape == (3000, 80) and _rel(ours, whr.log_mel(x)) < 1e-12
    sd = ur.init_weights(0, layers=0)
    w, g, b = (sd[f"feature_extractor.conv_layers.0.{k}"].double().numpy() for k in ("0.weight", "2.weight", "2.bias"))
    ours = wr.wave_stem(x[:3207], w.reshape(512, 10), g, b, 1e-5)
    assert _rel(ours, ur.wave_stem(sd, torch.from_numpy(x[:3207])).numpy()) < 1e-12
    assert abs(wr.gain(x, -30.0) - sr.gain(x)) < 1e-12 * sr.gain(x) and wr.gain(np.zeros(5), -30.0) == 1.0 == wr.gain(np.zeros(0), -30.0)
    y = st.add_noise(x, 5, seed=3)
    r = st.stages(x, y)
    assert np.array_equal(wr.stoi_resample(x), r["xr"]) and wr.stoi_kept(r["xr"])[0].tolist() == r["kept"].tolist() and len(r["kept"]) > 30
    for sig, key in ((r["xr"], "X"), (r["yr"], "Y")):
        assert _rel(wr.stoi_bands(sig, r["kept"], r["n_frames"]), r[key]) < 1e-12
    assert wr.stoi_scores(r["X"], r["Y"])[:2] == (r["stoi"], r["estoi"])
    # the fp32 evaluations are evaluations of the same thing
    assert _rel(wr.stoi_resample(x, wr.F32), r["xr"]) < 1e-5 and _rel(wr.stoi_bands(r["xr"], r["kept"], r["n_frames"], wr.F32), r["X"]) < 1e-5
    s32 = wr.stoi_scores(r["X"], r["Y"], wr.F32)
    assert abs(s32[0] - r["stoi"]) < 1e-5 and abs(s32[1] - r["estoi"]) < 1e-5 and s32[2] == r["n_segments"]
    assert _rel(wr.stft_mel(x, n, 320, 640, 160, wr.hann_periodic(640), mr.slaney_filterbank(), 0.0, mr.FLOOR, wr.F32, dense=True), mr.mel_f64(pcm)) < 1e-5
    assert wr.wave_stem(x[:3207], w.reshape(512, 10), g, b, 1e-5, wr.F32).dtype == np.float32
    # a kept index the clip does not have leaves a frame of zeros in its place
    kept = np.array([3, 5, 999, 8])
    z = wr.stoi_bands(r["xr"], kept, r["n_frames"])
    full = st.compact(r["xr"], np.array([3, 5, 6, 8]))
    full[256:512] -= st.window() * r["xr"][128 * 6:128 * 6 + 256]      # the third frame taken out again
    assert _rel(z, st.band_matrix(full)) < 1e-12


@pytest.mark.parametrize("pad,K_,hop", [(320, 640, 160), (1, 640, 160), (0, 640, 160), (383, 1024, 256), (120, 400, 160)])
def test_padded_clip_is_numpy_reflect(pad, K_, hop):
    x = np.random.default_rng(pad).standard_normal(3000)
    for n in (pad + 1, pad + 2, 1500):
        want = np.pad(x[:n], pad, mode="reflect") if pad else x[:n]
        assert np.array_equal(wr.padded_clip(x, n, n, pad), want)
    got = wr.padded_clip(x, 1500, 1000, pad)
    want = np.pad(np.concatenate([x[:1000], np.zeros(500)]), pad, mode="reflect") if pad else np.concatenate([x[:1000], np.zeros(500)])
    assert np.array_equal(got, want)
