"""Mouth ROIs from raw frames and 68-point landmarks, on the device.

What avhubert/preparation/align_mouth.py does per frame with skimage and cv2 on the host - and the reference's server repeats
on every request (server.py:268-269) - in two launches for a whole ragged batch:

  l2s_mouth_transforms  forward-window mean of the stable landmarks -> Umeyama similarity onto the mean face -> inverse map and
                        the clamped, rounded origin of the crop window (fp64)
  l2s_mouth_warp        the 96 x 96 window of the bilinear warp (never the 256 x 256 image around it) -> uint8 ROI, cv2 gray,
                        and / or the normalised fp32 [88, 88] stem input of data.normalize_frames

Video decode and landmark detection stay outside.  The reference writes the ROI through a lossy ffmpeg encode (-crf 20) and
decodes it again; this path skips that round trip: the result is what the reference would read back from a lossless file.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import L2SError

STABLE_IDS = (33, 36, 39, 42, 45)


def landmarks_interpolate(landmarks: list) -> Optional[list]:
    """align_mouth.py:24-30, 184-205: frames without a detection (None) are filled linearly between their detected neighbours,
    the ends repeat the first / last detection; None when no frame has one.  Host code; the list is not modified."""
    valid = [i for i, v in enumerate(landmarks) if v is not None]
    if not valid:
        return None
    out = [None if v is None else np.asarray(v, dtype=np.float64) for v in landmarks]
    for a, b in zip(valid[:-1], valid[1:]):
        delta = out[b] - out[a]
        for i in range(1, b - a):
            out[a + i] = out[a] + i / float(b - a) * delta
    out[:valid[0]] = [out[valid[0]]] * valid[0]
    out[valid[-1]:] = [out[valid[-1]]] * (len(out) - valid[-1])
    return out


class MouthCropper:
    """mean_face: [L, 2] (x, y) in the std_size = (height, width) aligned image; crop = (height, width) of the ROI."""

    def __init__(self, mean_face, std_size=(256, 256), crop=(96, 96), window_margin=12, start_idx=48, stop_idx=68,
                 stable_ids: Sequence[int] = STABLE_IDS):
        mf = np.asarray(mean_face, dtype=np.float64)
        if mf.ndim != 2 or mf.shape[1] != 2:
            raise ValueError(f"mean_face must be [L, 2], got {mf.shape}")
        L = mf.shape[0]
        if not 0 <= start_idx < stop_idx <= L or not all(0 <= i < L for i in stable_ids) or len(stable_ids) < 2:
            raise ValueError("landmark indices outside the mean face (or fewer than 2 stable points)")
        if window_margin < 1 or crop[0] > std_size[0] or crop[1] > std_size[1]:
            raise ValueError("window_margin must be >= 1 and the crop no larger than std_size")
        self.mean_face = mf
        self.std_size, self.crop, self.window_margin = tuple(std_size), tuple(crop), int(window_margin)
        self.start_idx, self.stop_idx, self.stable_ids = int(start_idx), int(stop_idx), tuple(int(i) for i in stable_ids)
        self._dev = {}

    def _tables(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.mean_face).to(device),
                              torch.tensor(self.stable_ids, dtype=torch.int32, device=device))
        return self._dev[key]

    @staticmethod
    def _lengths(lengths, n):
        lengths = [n] if lengths is None else [int(v) for v in lengths]
        if any(v < 1 for v in lengths) or sum(lengths) != n:
            raise ValueError(f"clip lengths {lengths} do not add up to the {n} rows given")
        return lengths

    def transforms(self, landmarks, lengths=None, device=None):
        """landmarks: [N, L, 2] (any real dtype, host or device) for the clips of `lengths` frames laid end to end -> (inv fp64
        [N, 6], origin int32 [N, 2]) on the device.  Stable points of zero variance raise ValueError (the reference yields NaN)."""
        if not torch.is_tensor(landmarks):
            landmarks = torch.from_numpy(np.ascontiguousarray(np.asarray(landmarks)))
        if device is None:
            if not landmarks.is_cuda:
                raise L2SError("MouthCropper: landmarks are on the host and no device was given (there is no CPU path)")
            device = landmarks.device
        if landmarks.dim() != 3 or tuple(landmarks.shape[1:]) != self.mean_face.shape:
            raise ValueError(f"landmarks must be [N, {self.mean_face.shape[0]}, 2], got {tuple(landmarks.shape)}")
        N = landmarks.shape[0]
        lengths = self._lengths(lengths, N)
        lm = landmarks.to(device=device, dtype=torch.float64).contiguous()
        count = torch.tensor(lengths, dtype=torch.int32)
        first = (torch.cumsum(count, 0) - count).to(torch.int32)
        mf, ids = self._tables(device)
        inv = torch.empty(N, 6, dtype=torch.float64, device=device)
        origin = torch.empty(N, 2, dtype=torch.int32, device=device)
        ops.mouth_transforms(lm, first.to(device), count.to(device), mf, ids, inv, origin, B=len(lengths), window_margin=self.window_margin,
                             std_h=self.std_size[0], std_w=self.std_size[1], crop_h=self.crop[0], crop_w=self.crop[1],
                             start_idx=self.start_idx, stop_idx=self.stop_idx)
        if not bool(torch.isfinite(inv).all()):
            bad = int((~torch.isfinite(inv).all(dim=1)).nonzero()[0])
            raise ValueError(f"frame {bad}: the stable landmarks of its window have zero variance (or are not finite): no similarity exists")
        return inv, origin

    def _frames(self, frames, landmarks, lengths):
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise L2SError("MouthCropper: frames must be a device tensor (there is no CPU path)")
        if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or (frames.dim() == 4 and frames.shape[3] not in (1, 3)):
            raise ValueError("frames must be uint8 [N, H, W, 3] (BGR), [N, H, W, 1] or [N, H, W]")
        if len(landmarks) != frames.shape[0]:
            raise ValueError(f"{len(landmarks)} landmark sets for {frames.shape[0]} frames")
        inv, origin = self.transforms(landmarks, lengths, device=frames.device)
        return frames.contiguous(), inv, origin

    def rois(self, frames, landmarks, lengths=None, gray=True):
        """uint8 [N, ch, cw] (gray: cv2's BGR2GRAY of the colour ROI) or, gray=False, the ROI in the frames' own channels
        [N, ch, cw, C] ([N, ch, cw] for frames given without a channel axis)."""
        frames, inv, origin = self._frames(frames, landmarks, lengths)
        N, (ch, cw) = frames.shape[0], self.crop
        C = frames.shape[3] if frames.dim() == 4 else 1
        if gray:
            out = torch.empty(N, ch, cw, dtype=torch.uint8, device=frames.device)
            ops.mouth_warp(frames, inv, origin, crop_h=ch, crop_w=cw, gray=out)
        else:
            out = torch.empty((N, ch, cw, C) if frames.dim() == 4 else (N, ch, cw), dtype=torch.uint8, device=frames.device)
            ops.mouth_warp(frames, inv, origin, crop_h=ch, crop_w=cw, roi=out)
        return out

    def model_input(self, frames, landmarks, lengths=None, crop=88, mean=0.421, std=0.165):
        """fp32 [N, crop, crop]: data.normalize_frames of the gray ROI, ready for net_input.source.video."""
        frames, inv, origin = self._frames(frames, landmarks, lengths)
        out = torch.empty(frames.shape[0], crop, crop, dtype=torch.float32, device=frames.device)
        ops.mouth_warp(frames, inv, origin, crop_h=self.crop[0], crop_w=self.crop[1], model_in=out, model_crop=crop, mean=mean, std=std)
        return out


def load_frames(path_stem: str) -> np.ndarray:
    """<stem>.npy (uint8 [T, H, W, 3] BGR or [T, H, W]) or, when OpenCV is importable, <stem>.mp4 decoded to BGR frames."""
    import os
    if os.path.exists(path_stem + ".npy"):
        return np.load(path_stem + ".npy")
    try:
        import cv2  # type: ignore
    except ImportError as e:
        raise RuntimeError(f"cannot decode {path_stem}.mp4: OpenCV is not installed and no {path_stem}.npy exists") from e
    cap, out = cv2.VideoCapture(path_stem + ".mp4"), []
    while True:
        ret, frame = cap.read()
        if not ret:
            break
        out.append(frame)
    cap.release()
    if not out:
        raise ValueError(f"Unable to load {path_stem}.mp4")
    return np.stack(out)


class VideoMouthCropper:
    """The `mouth_cropper` hook of data.MultiTargetDataset: video path -> gray uint8 [T, ch, cw].  Frames come from
    <video stem>.npy / .mp4 (load_frames), landmarks from landmark_path(video path) (a pickle: list of [68, 2] arrays or None)."""

    def __init__(self, cropper: MouthCropper, landmark_path, device="cuda"):
        self.cropper, self.landmark_path, self.device = cropper, landmark_path, device

    def __call__(self, video_path: str) -> np.ndarray:
        import os
        import pickle
        frames = load_frames(os.path.splitext(video_path)[0])
        with open(self.landmark_path(video_path), "rb") as f:
            lm = landmarks_interpolate(pickle.load(f))
        if lm is None:
            raise ValueError(f"{video_path}: no frame has landmarks")
        return self.cropper.rois(torch.from_numpy(frames).to(self.device), np.stack(lm), gray=True).cpu().numpy()
