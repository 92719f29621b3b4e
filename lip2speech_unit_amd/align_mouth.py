"""python -m lip2speech_unit_amd.align_mouth: mouth ROIs for a list of clips, on the device.

The arguments are those of avhubert/preparation/align_mouth.py (:108-127).  Frames come from <video-direc>/<fid>.npy (uint8
[T, H, W, 3] BGR or [T, H, W]) or, when OpenCV is importable, from <fid>.mp4; landmarks from <landmark-direc>/<fid>.pkl (a list
of [68, 2] arrays or None).  Output: <save-direc>/<fid>.npy, uint8 [T, crop-height, crop-width] gray - the sidecar
data.load_video reads, so stage 1 runs on it unchanged (the reference writes an mp4 through a lossy ffmpeg encode instead;
--ffmpeg is accepted and ignored).  --colour also writes <fid>.bgr.npy.  A clip without a single landmark is resized to the
crop size on the host, as :239-244 does.  Existing outputs are skipped.
"""
import argparse
import math
import os
import pickle
import sys

import numpy as np

from .mouth_roi import STABLE_IDS, MouthCropper, landmarks_interpolate, load_frames


def build_parser():
    p = argparse.ArgumentParser(description="Mouth ROIs from frames and landmarks (MI355X)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--video-direc", required=True, help="raw video directory (<fid>.npy or <fid>.mp4)")
    p.add_argument("--landmark-direc", required=True, help="landmark directory (<fid>.pkl)")
    p.add_argument("--filename-path", required=True, help="list of clip ids, one per line")
    p.add_argument("--save-direc", required=True, help="the directory the mouth ROIs are written to")
    p.add_argument("--mean-face", required=True, help="reference mean face (.npy, [68, 2])")
    p.add_argument("--crop-width", default=96, type=int, help="the width of mouth ROIs")
    p.add_argument("--crop-height", default=96, type=int, help="the height of mouth ROIs")
    p.add_argument("--start-idx", default=48, type=int, help="the start of landmark index")
    p.add_argument("--stop-idx", default=68, type=int, help="the end of landmark index")
    p.add_argument("--window-margin", default=12, type=int, help="window margin for smoothed_landmarks")
    p.add_argument("--ffmpeg", type=str, default=None, help="accepted and ignored: nothing is encoded")
    p.add_argument("--rank", type=int, default=0, help="rank id")
    p.add_argument("--nshard", type=int, default=1, help="number of shards")
    p.add_argument("--colour", action="store_true", help="also write <fid>.bgr.npy, the ROI in the frames' own channels")
    return p


def to_gray(frames: np.ndarray) -> np.ndarray:
    """cv2's 8-bit BGR2GRAY of uint8 [..., 3]; frames without a channel axis are returned as they are."""
    if frames.ndim == 3:
        return frames
    if frames.shape[-1] == 1:
        return frames[..., 0]
    b, g, r = (frames[..., i].astype(np.int64) for i in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def resize_frames(frames: np.ndarray, height: int, width: int) -> np.ndarray:
    """The rare path of :239-244, on the host: cv2.resize when OpenCV is importable, else a bilinear resize on cv2's pixel grid
    (centres at (i + 0.5) scale - 0.5, edges replicated) rounded to nearest - cv2's own fixed-point rounding may differ by a level."""
    try:
        import cv2  # type: ignore
        return np.stack([cv2.resize(f, (width, height)) for f in frames])
    except ImportError:
        pass
    T, H, W = frames.shape[:3]
    ys = np.clip((np.arange(height) + 0.5) * H / height - 0.5, 0, H - 1)
    xs = np.clip((np.arange(width) + 0.5) * W / width - 0.5, 0, W - 1)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1)
    shape = (1, height, 1) + (1,) * (frames.ndim - 3), (1, 1, width) + (1,) * (frames.ndim - 3)
    dy, dx = (ys - y0).reshape(shape[0]), (xs - x0).reshape(shape[1])
    f = frames.astype(np.float64)
    top = (1 - dx) * f[:, y0][:, :, x0] + dx * f[:, y0][:, :, x1]
    bot = (1 - dx) * f[:, y1][:, :, x0] + dx * f[:, y1][:, :, x1]
    return np.rint((1 - dy) * top + dy * bot).astype(np.uint8)


def device_cropper(args):
    """(frames, landmarks, colour) -> (gray [T, ch, cw], ROI in the frames' channels or None) on cuda:0."""
    import torch
    cropper = MouthCropper(np.load(args.mean_face), crop=(args.crop_height, args.crop_width), window_margin=args.window_margin,
                           start_idx=args.start_idx, stop_idx=args.stop_idx, stable_ids=STABLE_IDS)

    def crop(frames, landmarks, colour):
        dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        gray = cropper.rois(dev, landmarks, gray=True).cpu().numpy()
        return gray, (cropper.rois(dev, landmarks, gray=False).cpu().numpy() if colour else None)
    return crop


def main(argv=None, crop=None):
    args = build_parser().parse_args(argv)
    if not 0 <= args.rank < args.nshard:
        raise SystemExit(f"--rank {args.rank} is not in [0, --nshard {args.nshard})")
    crop = crop if crop is not None else device_cropper(args)
    with open(args.filename_path) as f:
        fids = [ln.strip() for ln in f if ln.strip()]
    per = math.ceil(len(fids) / args.nshard)                                # align_mouth.py:218-220
    fids = fids[per * args.rank: per * (args.rank + 1)]
    written = []
    for fid in fids:
        dst = os.path.join(args.save_direc, fid + ".npy")
        if os.path.exists(dst):
            continue
        stem, lm_path = os.path.join(args.video_direc, fid), os.path.join(args.landmark_direc, fid + ".pkl")
        if not os.path.isfile(lm_path):
            raise SystemExit(f"File does not exist. Path input: {lm_path}")
        frames = load_frames(stem)
        with open(lm_path, "rb") as f:
            landmarks = landmarks_interpolate(pickle.load(f))
        if landmarks is None:
            print(f"resizing {fid}")
            bgr = resize_frames(frames, args.crop_height, args.crop_width)
            gray = to_gray(bgr)
        else:
            if len(landmarks) != len(frames):
                raise SystemExit(f"{fid}: {len(landmarks)} landmark sets for {len(frames)} frames")
            gray, bgr = crop(frames, np.stack(landmarks), args.colour)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        np.save(dst, np.ascontiguousarray(gray))
        if args.colour:
            np.save(dst[:-4] + ".bgr.npy", np.ascontiguousarray(bgr))
        written.append(dst)
    print(f"cropped {len(written)} of {len(fids)} clips into {args.save_direc}")
    return written


if __name__ == "__main__":
    main(sys.argv[1:])
