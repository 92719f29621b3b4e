"""The mouth cropper on the MI355X against the float64 restatement tests/_mouth_roi_reference.py.

Gates: `origin` exact (tests/test_mouth_roi_cpu.py keeps every case's window centre away from a rounding tie); `inv` by the
source coordinates of the window's four corners, within 1e-9 px (float64 rounding is about 1e-13; a sample changes level at
about 1e-5 px); the ROI and its gray differ from the restatement by at most one level per sample, and the pooled share of
differing samples over all cases is at most 4 x the share the restatement's own float32 evaluation of the warp moves against
float64 on the same cases (computed here); model_input is bit-identical to data.normalize_frames of the device's own gray.

Measured on the MI355X: corner error at most 2.0e-13 px; 11 of 5 400 576 pooled samples (2.0e-6) differ
from the restatement, each by one level, against 485 (9.0e-5) for the float32 evaluation - the gate is 1 940."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

from tests import _mouth_roi_cases as K
from tests import _mouth_roi_reference as R

pytestmark = pytest.mark.gpu

GUARD = 256                                                              # bytes on either side of every output
FILL = {torch.uint8: 0xA5, torch.int32: -77, torch.float32: -7.25, torch.float64: -7.25}


def _guarded(n, dtype):
    pad = GUARD // torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((n + 2 * pad,), FILL[dtype], dtype=dtype, device="cuda")
    return buf, buf[pad:pad + n], pad


def _intact(buf, n, pad):
    fill = FILL[buf.dtype]
    return bool((buf[:pad] == fill).all()) and bool((buf[pad + n:] == fill).all())


def run_device(frames, lm, lengths, outputs=("roi", "gray", "model_in"), crop=(96, 96), mc=88):
    """Both entries through ops, every output between guard bytes; returns numpy arrays and whether all guards survived."""
    from lip2speech_unit_amd import ops
    N = frames.shape[0]
    C = frames.shape[3] if frames.ndim == 4 else 1
    dev = torch.from_numpy(frames).cuda()
    lmd = torch.from_numpy(np.ascontiguousarray(lm)).cuda().to(torch.float64)
    count = torch.tensor(lengths, dtype=torch.int32)
    first = (torch.cumsum(count, 0) - count).to(torch.int32)
    bufs = {"inv": _guarded(6 * N, torch.float64), "origin": _guarded(2 * N, torch.int32)}
    ops.mouth_transforms(lmd, first.cuda(), count.cuda(), torch.from_numpy(K.mean_face()).cuda(),
                         torch.tensor(R.STABLE_IDS, dtype=torch.int32, device="cuda"), bufs["inv"][1].view(N, 6),
                         bufs["origin"][1].view(N, 2), B=len(lengths), crop_h=crop[0], crop_w=crop[1])
    shapes = {"roi": ((N,) + crop + (C,), torch.uint8), "gray": ((N,) + crop, torch.uint8), "model_in": ((N, mc, mc), torch.float32)}
    kw = {}
    for name in outputs:
        shape, dt = shapes[name]
        bufs[name] = _guarded(int(np.prod(shape)), dt)
        kw[name] = bufs[name][1].view(shape)
    if "model_in" in kw:
        kw["model_crop"] = mc
    ops.mouth_warp(dev, bufs["inv"][1].view(N, 6), bufs["origin"][1].view(N, 2), crop_h=crop[0], crop_w=crop[1], **kw)
    torch.cuda.synchronize()
    out = {"guards": all(_intact(b, v.numel(), pad) for b, v, pad in bufs.values())}
    out["inv"], out["origin"] = bufs["inv"][1].view(N, 6).cpu().numpy(), bufs["origin"][1].view(N, 2).cpu().numpy()
    for name in outputs:
        out[name] = kw[name].cpu().numpy()
    return out


def _moved(a, b):
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    assert d.max() <= 1, int(d.max())
    return int((d != 0).sum())


@functools.lru_cache(maxsize=None)
def inputs(name):
    case = {c.name: c for c in K.CASES + K.RAGGED}[name]
    return K.frames(case), K.landmarks(case)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of one clip, and its float32 evaluation of the warp (same inverse maps and origins)."""
    fr, lm = inputs(name)
    ref = R.crop_clip(fr, lm, K.mean_face())
    roi32 = np.stack([R.quantise(R.warp_window(fr[t], ref["inv"][t], ref["origin"][t], dtype=np.float32)) for t in range(len(fr))])
    ref["roi32"], ref["gray32"] = roi32, R.bgr2gray(roi32)
    return ref


@functools.lru_cache(maxsize=None)
def device(name):
    fr, lm = inputs(name)
    return run_device(fr, lm, [len(fr)])


@functools.lru_cache(maxsize=None)
def device_ragged():
    fr = np.concatenate([inputs(c.name)[0] for c in K.RAGGED])
    lm = np.concatenate([inputs(c.name)[1] for c in K.RAGGED])
    return run_device(fr, lm, [c.T for c in K.RAGGED])


def _corner_error(inv_dev, ref, t):
    x0, y0 = ref["origin"][t]
    worst = 0.0
    m = np.vstack([inv_dev.reshape(2, 3), [0.0, 0.0, 1.0]])
    for x, y in ((x0, y0), (x0 + 95, y0), (x0, y0 + 95), (x0 + 95, y0 + 95)):
        a, b = m @ np.array([x, y, 1.0]), ref["inv"][t] @ np.array([x, y, 1.0])
        worst = max(worst, float(np.abs(a[:2] - b[:2] / b[2]).max()))
    return worst


def _check_clip(got, ref, rows, name):
    T = len(ref["origin"])
    assert np.array_equal(got["origin"][rows], ref["origin"]), name
    worst = max(_corner_error(got["inv"][rows][t], ref, t) for t in range(T))
    print(f"{name}: corner error {worst:.3e} px")
    assert worst < 1e-9, (name, worst)
    for key in ("roi", "gray"):
        d = np.abs(got[key][rows].astype(np.int64) - ref[key].astype(np.int64))
        print(f"{name}: {key} {int((d != 0).sum())} of {d.size} samples differ, max {int(d.max())}")
        assert d.max() <= 1, (name, key, int(d.max()))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_case_against_the_restatement(case):
    from lip2speech_unit_amd import data
    got, ref = device(case.name), reference(case.name)
    assert got["guards"], "an output wrote outside its buffer"
    assert got["roi"].shape == (case.T, 96, 96, case.C) and got["gray"].shape == (case.T, 96, 96)
    _check_clip(got, ref, slice(0, case.T), case.name)
    if case.C == 1:
        assert np.array_equal(got["gray"], got["roi"][..., 0])
    else:
        assert np.array_equal(got["gray"], R.bgr2gray(got["roi"]))                   # gray is taken from the truncated ROI
    want = data.normalize_frames(got["gray"])
    assert got["model_in"].dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got["model_in"].view(np.uint32), want.view(np.uint32))      # bit-identical
    assert got["roi"].any()


def test_ragged_batch_and_each_clip_alone_are_the_same_bytes():
    got = device_ragged()
    assert got["guards"]
    row = 0
    for c in K.RAGGED:
        rows = slice(row, row + c.T)
        _check_clip(got, reference(c.name), rows, c.name)
        alone = device(c.name)
        assert alone["guards"]
        for key in ("inv", "origin", "roi", "gray", "model_in"):
            assert np.array_equal(got[key][rows].view(np.uint8), alone[key].view(np.uint8)), (c.name, key)
        row += c.T


def test_pooled_share_of_moved_samples_is_within_four_times_float32s():
    moved, moved32, total = 0, 0, 0
    runs = [(device(c.name), slice(0, c.T), c) for c in K.CASES]
    row, rag = 0, device_ragged()
    for c in K.RAGGED:
        runs.append((rag, slice(row, row + c.T), c))
        row += c.T
    for got, rows, c in runs:
        ref = reference(c.name)
        for key in ("roi", "gray"):
            moved += int((got[key][rows] != ref[key]).sum())
            moved32 += int((ref[key + "32"] != ref[key]).sum())
            total += ref[key].size
    print(f"pooled: device {moved} / {total} = {moved / total:.3e}, float32 restatement {moved32} / {total} = {moved32 / total:.3e}")
    assert moved32 > 0
    assert moved <= 4 * moved32, (moved, moved32, total)


@pytest.mark.parametrize("crop,mc", [((90, 94), 80), ((96, 96), 86), ((64, 100), 64)], ids=["90x94-80", "96x96-86", "64x100-64"])
def test_other_crop_sizes_take_the_narrow_store_paths(crop, mc):
    """A crop width that is no multiple of 4 leaves by single bytes and ends rows inside a thread's 4 pixels, a stem crop whose
    offset is no multiple of 4 leaves by single floats, and heights that are no multiple of 32 leave tiles partly filled.  The
    window centres are those of the default crop (checked against rounding ties on the CPU) or clamped to integers."""
    from lip2speech_unit_amd import data
    moved, moved32 = 0, 0
    for case in (K.CASES[2], K.CASES[1], K.CASES[6]):                    # colour, gray, clamped
        fr, lm = inputs(case.name)
        got = run_device(fr, lm, [case.T], crop=crop, mc=mc)
        ref = R.crop_clip(fr, lm, K.mean_face(), crop=crop)
        assert got["guards"], case.name
        assert np.array_equal(got["origin"], ref["origin"]), case.name
        roi32 = np.stack([R.quantise(R.warp_window(fr[t], ref["inv"][t], ref["origin"][t], crop, np.float32)) for t in range(case.T)])
        moved += _moved(got["roi"], ref["roi"]) + _moved(got["gray"], ref["gray"])
        moved32 += _moved(roi32, ref["roi"]) + _moved(R.bgr2gray(roi32), ref["gray"])
        want = data.normalize_frames(got["gray"], crop=mc)
        assert got["model_in"].shape == want.shape == (case.T, mc, mc)
        assert np.array_equal(got["model_in"].view(np.uint32), want.astype(np.float32).view(np.uint32)), case.name
    print(f"crop {crop}: device moved {moved}, float32 restatement {moved32}")
    assert moved <= 4 * moved32, (moved, moved32)


def test_outputs_left_out_are_not_written_and_the_rest_are_the_same_bytes():
    case = K.CASES[2]
    fr, lm = inputs(case.name)
    full = device(case.name)
    for only in ("roi", "gray", "model_in"):
        got = run_device(fr, lm, [case.T], outputs=(only,))
        assert got["guards"], only
        assert np.array_equal(got[only].view(np.uint8), full[only].view(np.uint8)), only


def test_host_class_surfaces_and_errors():
    from lip2speech_unit_amd.mouth_roi import MouthCropper
    case = K.CASES[3]
    fr, lm = inputs(case.name)
    full = device(case.name)
    crop = MouthCropper(K.mean_face())
    dev = torch.from_numpy(fr).cuda()
    inv, origin = crop.transforms(lm, device="cuda")
    assert np.array_equal(inv.cpu().numpy(), full["inv"]) and np.array_equal(origin.cpu().numpy(), full["origin"])
    assert np.array_equal(crop.rois(dev, lm).cpu().numpy(), full["gray"])
    assert np.array_equal(crop.rois(dev, lm, gray=False).cpu().numpy(), full["roi"])
    assert np.array_equal(crop.rois(dev, torch.from_numpy(lm).cuda(), lengths=[6, 7]).cpu().numpy()[:6],
                          device_pair(case.name, 6)["gray"])
    mi = crop.model_input(dev, lm)
    assert mi.shape == (case.T, 88, 88) and mi.dtype == torch.float32 and np.array_equal(mi.cpu().numpy(), full["model_in"])
    gcase = K.CASES[1]                                                   # frames without a channel axis
    gfr, glm = inputs(gcase.name)
    g = crop.rois(torch.from_numpy(gfr).cuda(), glm, gray=False)
    assert g.shape == (gcase.T, 96, 96) and np.array_equal(g.cpu().numpy(), device(gcase.name)["gray"])
    with pytest.raises(ValueError):
        crop.rois(dev, lm[:-1])                                          # len(landmarks) != T
    with pytest.raises(ValueError):
        crop.rois(dev, lm, lengths=[5, 5])
    flat = lm.copy()
    flat[:, list(R.STABLE_IDS)] = flat[:, 33:34]                          # every stable point the same: no similarity exists
    with pytest.raises(ValueError):
        crop.transforms(flat, device="cuda")


@functools.lru_cache(maxsize=None)
def device_pair(name, n):
    fr, lm = inputs(name)
    return run_device(fr[:n], lm[:n], [n])


def test_dataset_hook_yields_the_sample_of_the_written_sidecar(tmp_path):
    from lip2speech_unit_amd import align_mouth, data
    from lip2speech_unit_amd.mouth_roi import MouthCropper, VideoMouthCropper
    from tests._synth_dataset import make
    root = str(tmp_path / "ds")
    cases = (K.RAGGED[3], K.CASES[6])                                     # 5 frames each
    lab = make(root, frames=tuple(c.T for c in cases))
    plain = data.MultiTargetDataset(os.path.join(lab, "test.tsv"))
    lmdir, saved = tmp_path / "lm", tmp_path / "roi"
    for c, fid in zip(cases, plain.ids):
        fr, lm = inputs(c.name)
        np.save(os.path.join(root, "video", fid + ".npy"), fr)           # raw BGR frames where the video is
        os.makedirs(os.path.dirname(lmdir / fid), exist_ok=True)
        lms = [lm[t] if t != 2 else None for t in range(c.T)]             # one frame without a detection
        with open(str(lmdir / fid) + ".pkl", "wb") as f:
            pickle.dump(lms, f)
    np.save(tmp_path / "mean.npy", K.mean_face())
    (tmp_path / "list.txt").write_text("\n".join(plain.ids) + "\n")
    hook = VideoMouthCropper(MouthCropper(K.mean_face()),
                             lambda p: str(lmdir / os.path.relpath(os.path.splitext(p)[0], os.path.join(root, "video"))) + ".pkl")
    hooked = data.MultiTargetDataset(os.path.join(lab, "test.tsv"), mouth_cropper=hook)
    samples = [hooked[i] for i in range(2)]
    written = align_mouth.main(["--video-direc", os.path.join(root, "video"), "--landmark-direc", str(lmdir), "--filename-path",
                                str(tmp_path / "list.txt"), "--save-direc", str(saved), "--mean-face", str(tmp_path / "mean.npy")])
    assert len(written) == 2
    for i, fid in enumerate(plain.ids):
        roi = np.load(str(saved / fid) + ".npy")
        assert roi.shape == (5, 96, 96) and roi.dtype == np.uint8 and roi.any()
        np.save(os.path.join(root, "video", fid + ".npy"), roi)           # the sidecar takes the video's place: the plain path reads it
        s = plain[i]
        assert torch.equal(s["video_source"], samples[i]["video_source"]) and s["video_source"].shape == (5, 88, 88)
        assert torch.equal(s["mel"], samples[i]["mel"])
