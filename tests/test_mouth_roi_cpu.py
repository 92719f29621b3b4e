"""The mouth cropper, the parts that need no GPU: the float64 restatement tests/_mouth_roi_reference.py pinned against scipy
and worked examples, the host function landmarks_interpolate, the registration of the two entries and their host-side
guards, the CLI on a stubbed cropper, the dataset hook, and the condition the GPU cases must meet for `origin` to be decided
identically by any float64 evaluation."""
import ctypes
import os
import pickle
import re
from collections import deque

import numpy as np
import pytest
import torch

from tests import _mouth_roi_cases as K
from tests import _mouth_roi_reference as R


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------------
def test_closed_form_is_the_svd_umeyama_also_for_mirrored_points():
    rng = np.random.default_rng(7)
    worst = 0.0
    for i in range(200):
        n = int(rng.integers(3, 9))
        src = rng.normal(0, 40, (n, 2)) + rng.normal(0, 100, 2)
        th, s = rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 3.0)
        dst = s * src @ np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T + rng.normal(0, 50, 2)
        dst += rng.normal(0, 2.0, dst.shape)
        if i % 2:
            dst[:, 0] = -dst[:, 0]                                       # mirrored: det A < 0, the rotation stays proper
        a, b = R.umeyama_svd(src, dst), R.umeyama_closed(src, dst)
        if i % 2:
            assert np.linalg.det((dst - dst.mean(0)).T @ (src - src.mean(0))) < 0
        assert np.linalg.det(a[:2, :2]) > 0
        worst = max(worst, np.abs(a - b).max() / max(1.0, np.abs(a).max()))
    assert worst < 1e-12, worst


def test_warp_before_quantisation_is_scipy_map_coordinates():
    ndi = pytest.importorskip("scipy.ndimage")
    worst = 0.0
    for case in (K.CASES[1], K.CASES[5], K.CASES[4]):                    # gray and colour, a window that leaves the frame
        fr, lm = K.frames(case), K.landmarks(case)
        _, inv, _, origin = R.clip_transforms(lm, K.mean_face())
        for t in (0, case.T - 1):
            w = R.warp_window(fr[t], inv[t], origin[t])
            sx, sy = R.source_coords(inv[t], origin[t])
            img = (fr[t] if fr[t].ndim == 3 else fr[t][:, :, None]).astype(np.float64) / 255.0
            for c in range(img.shape[2]):
                want = ndi.map_coordinates(img[:, :, c], [sy, sx], order=1, mode="grid-constant", cval=0.0)
                worst = max(worst, np.abs(w[:, :, c] - want).max())
            assert w.min() >= 0.0 and w.max() <= 1.0 + 1e-15
    assert worst < 1e-12, worst


def test_identity_and_integer_translation_return_the_frame_itself():
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, size=(120, 160, 3), dtype=np.uint8)
    frame[8:12, 10:74, 1] = np.arange(256).reshape(4, 64)                # every level 0 .. 255 is inside the window
    eye = np.eye(3)
    roi = R.quantise(R.warp_window(frame, eye, (10, 7)))
    assert np.array_equal(roi, frame[7:7 + 96, 10:10 + 96])
    shift = np.array([[1.0, 0.0, -30.0], [0.0, 1.0, 50.0], [0.0, 0.0, 1.0]])                 # source = output + (-30, 50)
    roi = R.quantise(R.warp_window(frame, shift, (0, 0)))
    want = np.zeros((96, 96, 3), np.uint8)
    want[:70, 30:] = frame[50:120, 0:66]                                 # rows past the frame's bottom and columns left of it are 0
    assert np.array_equal(roi, want)
    gray = rng.integers(0, 256, size=(97, 131), dtype=np.uint8)
    assert np.array_equal(R.quantise(R.warp_window(gray, eye, (3, 1)))[..., 0], gray[1:97, 3:99])
    assert np.array_equal(R.bgr2gray(roi[:, :, :1]), roi[:, :, 0])
    bgr = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], np.uint8)
    assert R.bgr2gray(bgr).tolist() == [[255, 0, 29, 150, 76, 128]]      # cv2's 8-bit weights: 0.114, 0.587, 0.299


def _deque_windows(T, window_margin=12):
    """The landmark window each frame's transform is estimated from, by running align_mouth.py:140-180's queue on frame indices."""
    margin, q, out, last = min(T, window_margin), deque(), [], None
    for idx in range(T):
        q.append(idx)
        if len(q) == margin:
            last = (q[0], len(q))
            out.append(last)
            q.popleft()
        if idx == T - 1:
            while q:
                q.popleft()
                out.append(last)
    return out


def test_tail_rule_and_margin_on_worked_examples():
    assert [R.window_start(t, 1) for t in range(1)] == [(0, 1)]
    assert [R.window_start(t, 5) for t in range(5)] == [(0, 5)] * 5
    assert [R.window_start(t, 12) for t in range(12)] == [(0, 12)] * 12
    assert [R.window_start(t, 13) for t in range(13)] == [(0, 12)] + [(1, 12)] * 12
    assert [R.window_start(t, 30)[0] for t in range(30)] == list(range(18)) + [18] * 12
    for T in (1, 5, 12, 13, 30):
        assert [R.window_start(t, T) for t in range(T)] == _deque_windows(T), T
    case = K.CASES[3]                                                    # T = 13
    M, _, _, _ = R.clip_transforms(K.landmarks(case), K.mean_face())
    assert not np.array_equal(M[0], M[1]) and all(np.array_equal(M[1], M[t]) for t in range(2, 13))


# ---- landmarks_interpolate ------------------------------------------------------------------------------------------------------------
def test_landmarks_interpolate_cases():
    from lip2speech_unit_amd.mouth_roi import landmarks_interpolate
    rng = np.random.default_rng(5)
    a, b, c = (rng.normal(100, 30, (68, 2)) for _ in range(3))
    cases = {"inner gap": [a, None, None, None, b, c], "leading": [None, None, a, b], "trailing": [a, b, None, None, None],
             "both ends and a gap": [None, a, None, b, None], "complete": [a, b, c], "single": [None, a, None]}
    for name, lms in cases.items():
        got, want = landmarks_interpolate(list(lms)), R.interpolate_expected(list(lms))
        assert len(got) == len(want) == len(lms), name
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
    gap = landmarks_interpolate([a, None, None, None, b])
    assert np.allclose(gap[1], 0.75 * a + 0.25 * b) and np.allclose(gap[2], 0.5 * (a + b)) and np.allclose(gap[3], 0.25 * a + 0.75 * b)
    lead = landmarks_interpolate([None, None, a, b])
    assert np.array_equal(lead[0], a) and np.array_equal(lead[1], a) and np.array_equal(lead[3], b)
    assert landmarks_interpolate([None, None]) is None and landmarks_interpolate([]) is None
    assert R.interpolate_expected([None]) is None


# ---- registration and guards --------------------------------------------------------------------------------------------------------
ENTRIES = ("l2s_mouth_transforms", "l2s_mouth_warp")


def test_entries_are_declared_bound_and_wrapped():
    from lip2speech_unit_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lip2speech_hip.h")).read()
    for e in ENTRIES:
        m = re.search(r"\bint\s+" + e + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, e
        assert e in _lib.SIGNATURES and len(_lib.SIGNATURES[e][0]) == len(m.group(1).split(",")), e
        name = e[len("l2s_"):]
        assert ops.ENTRY_OF[name] == e and callable(getattr(ops, name)) and hasattr(torch.ops.lip2speech, name)
    assert "align_mouth.py:33-44" in hdr and "server.py:268-269" in hdr and "DESIGN.md section 19" in hdr
    assert _lib.ABI_VERSION == 16
    f64, i32 = torch.zeros(4, 68, 2, dtype=torch.float64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ops.L2SError):
        ops.mouth_transforms(f64, i32, i32, torch.zeros(68, 2, dtype=torch.float64), i32, torch.zeros(4, 6, dtype=torch.float64),
                             torch.zeros(4, 2, dtype=torch.int32), B=1)
    with pytest.raises(ops.L2SError):
        ops.mouth_warp(torch.zeros(4, 32, 32, 3, dtype=torch.uint8), torch.zeros(4, 6, dtype=torch.float64),
                       torch.zeros(4, 2, dtype=torch.int32), gray=torch.zeros(4, 96, 96, dtype=torch.uint8))
    with pytest.raises(NotImplementedError):
        torch.ops.lip2speech.mouth_warp(torch.zeros(4, 32, 32, 3, dtype=torch.uint8), torch.zeros(4, 6, dtype=torch.float64),
                                        torch.zeros(4, 2, dtype=torch.int32), gray=torch.zeros(4, 96, 96, dtype=torch.uint8))


def test_argument_guards_return_codes_without_a_device():
    from lip2speech_unit_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                       # an aligned host address: the guards return before any launch
    p = ctypes.addressof(buf)
    EINVAL, ESHAPE, EALIGN, EUNSUP = -1, -2, -3, -4
    order = ("lm", "N", "L", "first", "count", "B", "mf", "ids", "ns", "wm", "sh", "sw", "ch", "cw", "i0", "i1", "inv", "org", "st")
    good = dict(lm=p, N=10, L=68, first=p, count=p, B=1, mf=p, ids=p, ns=5, wm=12, sh=256, sw=256, ch=96, cw=96, i0=48, i1=68, inv=p,
                org=p, st=None)

    def tr(**k):
        return lib.l2s_mouth_transforms(*[{**good, **k}[a] for a in order])
    assert tr(lm=None) == EINVAL and tr(inv=None) == EINVAL and tr(org=None) == EINVAL and tr(ids=None) == EINVAL
    assert tr(N=0) == ESHAPE and tr(B=0) == ESHAPE and tr(wm=0) == ESHAPE and tr(ns=0) == ESHAPE
    assert tr(i1=69) == ESHAPE and tr(i0=68) == ESHAPE and tr(i0=-1) == ESHAPE and tr(ch=257) == ESHAPE and tr(cw=0) == ESHAPE
    assert tr(ns=17) == EUNSUP and tr(sh=1 << 21, ch=96) == EUNSUP
    assert tr(lm=p + 4) == EALIGN and tr(inv=p + 4) == EALIGN and tr(org=p + 2) == EALIGN and tr(first=p + 1) == EALIGN

    worder = ("fr", "N", "H", "W", "C", "inv", "org", "ch", "cw", "roi", "gray", "mi", "mc", "mean", "std", "st")
    wgood = dict(fr=p, N=4, H=120, W=160, C=3, inv=p, org=p, ch=96, cw=96, roi=p, gray=p, mi=p, mc=88, mean=0.421, std=0.165, st=None)

    def warp(**k):
        return lib.l2s_mouth_warp(*[{**wgood, **k}[a] for a in worder])
    assert warp(fr=None) == EINVAL and warp(inv=None) == EINVAL and warp(org=None) == EINVAL
    assert warp(roi=None, gray=None, mi=None) == EINVAL                  # no output at all
    assert warp(N=0) == ESHAPE and warp(H=0) == ESHAPE and warp(ch=0) == ESHAPE and warp(mc=97) == ESHAPE and warp(mc=0) == ESHAPE
    assert warp(std=0.0) == ESHAPE
    assert warp(C=2) == EUNSUP and warp(C=4) == EUNSUP and warp(H=40000) == EUNSUP and warp(cw=5000) == EUNSUP
    assert warp(inv=p + 4) == EALIGN and warp(roi=p + 1) == EALIGN and warp(gray=p + 2) == EALIGN and warp(mi=p + 2) == EALIGN
    assert warp(org=p + 2) == EALIGN
    assert warp(fr=p + 1, C=5) == EUNSUP                                 # frames may sit at any address: not an alignment error


def test_host_class_checks_its_arguments():
    from lip2speech_unit_amd.mouth_roi import MouthCropper
    from lip2speech_unit_amd._lib import L2SError
    mf = K.mean_face()
    crop = MouthCropper(mf)
    assert crop.crop == (96, 96) and crop.std_size == (256, 256) and crop.window_margin == 12
    assert (crop.start_idx, crop.stop_idx, crop.stable_ids) == (48, 68, (33, 36, 39, 42, 45))
    with pytest.raises(L2SError):
        crop.rois(torch.zeros(3, 64, 64, 3, dtype=torch.uint8), np.zeros((3, 68, 2)))             # host frames
    with pytest.raises(L2SError):
        crop.transforms(np.zeros((3, 68, 2)))                                                       # host landmarks, no device
    with pytest.raises(ValueError):
        MouthCropper(mf, stop_idx=69)
    with pytest.raises(ValueError):
        MouthCropper(mf, stable_ids=(33, 70))
    with pytest.raises(ValueError):
        MouthCropper(mf[:, :1])
    with pytest.raises(ValueError):
        MouthCropper._lengths([3, 4], 8)
    assert MouthCropper._lengths(None, 8) == [8]


# ---- the CLI on a stubbed cropper ----------------------------------------------------------------------------------------------------
def test_cli_end_to_end_on_a_stub(tmp_path, capsys):
    from lip2speech_unit_amd import align_mouth as cli
    a = cli.build_parser().parse_args(["--video-direc", "v", "--landmark-direc", "l", "--filename-path", "f", "--save-direc", "s",
                                       "--mean-face", "m.npy", "--ffmpeg", "/usr/bin/ffmpeg"])
    assert (a.crop_width, a.crop_height, a.start_idx, a.stop_idx, a.window_margin, a.rank, a.nshard, a.colour) == (
        96, 96, 48, 68, 12, 0, 1, False)
    rng = np.random.default_rng(0)
    vid, lmd, out = tmp_path / "video", tmp_path / "lm", tmp_path / "roi"
    (vid / "s0").mkdir(parents=True), (lmd / "s0").mkdir(parents=True)
    clips = {"s0/a": 5, "s0/b": 3, "s0/none": 4, "s0/c": 2}
    for fid, T in clips.items():
        np.save(vid / (fid + ".npy"), rng.integers(0, 256, size=(T, 40, 60, 3), dtype=np.uint8))
        lms = [None] * T if fid == "s0/none" else [rng.normal(30, 5, (68, 2)) if t != 1 else None for t in range(T)]
        with open(lmd / (fid + ".pkl"), "wb") as f:
            pickle.dump(lms, f)
    (tmp_path / "list.txt").write_text("\n".join(clips) + "\n")
    np.save(tmp_path / "mean.npy", K.mean_face())
    seen = []

    def stub(frames, landmarks, colour):
        assert landmarks.shape == (len(frames), 68, 2) and np.isfinite(landmarks).all()           # gaps are filled before the crop
        seen.append((len(frames), colour))
        T = len(frames)
        return np.full((T, 96, 96), T, np.uint8), (np.full((T, 96, 96, 3), T + 1, np.uint8) if colour else None)

    base = ["--video-direc", str(vid), "--landmark-direc", str(lmd), "--filename-path", str(tmp_path / "list.txt"),
            "--save-direc", str(out), "--mean-face", str(tmp_path / "mean.npy")]
    written = cli.main(base + ["--rank", "0", "--nshard", "2"], crop=stub)
    assert [os.path.relpath(w, out) for w in written] == ["s0/a.npy", "s0/b.npy"] and seen == [(5, False), (3, False)]
    assert not (out / "s0" / "a.bgr.npy").exists()
    written = cli.main(base + ["--colour"], crop=stub)                                             # a and b exist: skipped
    assert [os.path.relpath(w, out) for w in written] == ["s0/none.npy", "s0/c.npy"] and seen[2:] == [(2, True)]
    for fid, T in clips.items():
        g = np.load(out / (fid + ".npy"))
        assert g.shape == (T, 96, 96) and g.dtype == np.uint8
        if fid != "s0/none":
            assert (g == T).all()
    assert (np.load(out / "s0" / "c.bgr.npy") == 3).all()
    none = np.load(out / "s0" / "none.npy")                              # no landmark at all: the frames resized, on the host
    src = np.load(vid / "s0" / "none.npy")
    assert np.load(out / "s0" / "none.bgr.npy").shape == (4, 96, 96, 3)
    assert abs(float(none.mean()) - float(cli.to_gray(src).mean())) < 4.0 and none.std() > 10
    assert "resizing s0/none" in capsys.readouterr().out
    with pytest.raises(SystemExit):
        cli.main(base + ["--rank", "2", "--nshard", "2"], crop=stub)
    flat = np.full((2, 10, 20), 77, np.uint8)
    assert (cli.resize_frames(flat, 96, 96) == 77).all() and cli.resize_frames(flat, 96, 96).shape == (2, 96, 96)
    ramp = np.tile(np.arange(0, 200, 2, dtype=np.uint8), (1, 8, 1))      # [1, 8, 100] -> width 50: the mean of each pixel pair
    assert np.array_equal(cli.resize_frames(ramp, 8, 50)[0, 0], np.arange(1, 200, 4))


def test_dataset_takes_the_frames_from_the_hook(tmp_path):
    from lip2speech_unit_amd import data
    from tests._synth_dataset import make
    lab = make(str(tmp_path), frames=(6, 4))
    calls = []
    rois = np.random.default_rng(1).integers(0, 256, size=(4, 96, 96), dtype=np.uint8)

    def hook(path):
        calls.append(path)
        return rois

    plain = data.MultiTargetDataset(os.path.join(lab, "test.tsv"))
    hooked = data.MultiTargetDataset(os.path.join(lab, "test.tsv"), mouth_cropper=hook)
    assert plain.mouth_cropper is None
    s0, s1 = plain[1], hooked[1]
    assert calls == [os.path.join(str(tmp_path), plain.names[1][0])]
    assert np.array_equal(s1["video_source"].numpy(), data.normalize_frames(rois))
    assert s1["video_source"].shape == s0["video_source"].shape and not torch.equal(s0["video_source"], s1["video_source"])
    assert torch.equal(s0["mel"], s1["mel"]) and torch.equal(s0["spk_emb"], s1["spk_emb"])


# ---- the condition on the GPU cases ---------------------------------------------------------------------------------------------------
def test_gpu_cases_keep_every_window_centre_away_from_a_rounding_tie():
    """origin = rint(centre) - half: two float64 evaluations (about 1e-13 apart) agree on it when no centre lies within 1e-6 of a
    .5 tie.  Every case is checked; none may be dropped."""
    cases = K.CASES + K.RAGGED
    assert len(K.CASES) == 9 and len(K.RAGGED) == 4 and len({c.name for c in cases}) == 13
    assert sorted(c.T for c in K.RAGGED) == [1, 5, 13, 30] and [c.T for c in K.RAGGED] == [13, 1, 30, 5]
    assert {c.T for c in K.CASES} == {1, 5, 12, 13, 30} and {(c.H, c.W) for c in K.CASES} == {(120, 160), (97, 131)}
    assert {c.C for c in K.CASES} == {1, 3}
    checked, clamped, outside = 0, 0, 0
    for c in cases:
        lm = K.landmarks(c)
        assert lm.shape == (c.T, 68, 2) and (lm.dtype == np.int64) == c.integer
        _, inv, centre, origin = R.clip_transforms(lm, K.mean_face())
        frac = np.abs(centre - np.floor(centre) - 0.5)
        assert frac.min() > 1e-6, (c.name, frac.min())
        checked += c.T
        clamped += int(((centre == 48) | (centre == 208)).any())
        sx, sy = R.source_coords(inv[0], origin[0])
        outside += int(sx.min() < 0 or sy.min() < 0)
        fr = K.frames(c)
        assert fr.dtype == np.uint8 and fr.shape == ((c.T, c.H, c.W, 3) if c.C == 3 else (c.T, c.H, c.W))
    assert checked == sum(c.T for c in cases) == 170
    assert clamped >= 2 and outside >= 2                                 # the clamped and the negative-coordinate cases are what they claim
