#!/usr/bin/env python3
"""Time of the on-device mouth cropper (mouth_roi.MouthCropper's two launches) at a batch of raw clips, and the GB/s of the bytes
it actually has to touch.  No threshold: the figures are recorded in DESIGN.md section 19.

  python tools/mouth_roi_bench.py [--clips 640] [--frames 100] [--height 224] [--width 224] [--channels 3] [--iters 10]

Frames are random bytes made on the device; landmarks are the tests' synthetic mean face under a per-clip similarity (face size
0.6 - 1.0 of the mean face, up to +-15 degrees) with 1 px of jitter.  "Touched" bytes: the distinct source pixels the windows'
bilinear taps read (counted exactly on the host for `--sample` frames and scaled), the inverse maps and origins, and the outputs
written - the roof a kernel that moves nothing twice would run at.  Each output set is timed on its own, with events around
`iters` launches after a warm-up.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _mouth_roi_cases as K  # noqa: E402
from tests import _mouth_roi_reference as R  # noqa: E402


def touched_pixels(inv, origin, H, W):
    """Distinct source pixels inside the frame among the four taps of every window pixel."""
    sx, sy = R.source_coords(np.vstack([inv.reshape(2, 3), [0, 0, 1]]), origin)
    fx, fy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    seen = np.zeros((H, W), bool)
    for dy in (0, 1):
        for dx in (0, 1):
            r, c = fy + dy, fx + dx
            ok = (r >= 0) & (r < H) & (c >= 0) & (c < W) & (sx > -1) & (sx < W) & (sy > -1) & (sy < H)
            seen[r[ok], c[ok]] = True
    return int(seen.sum())


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--clips", type=int, default=640)
    p.add_argument("--frames", type=int, default=100)
    p.add_argument("--height", type=int, default=224)
    p.add_argument("--width", type=int, default=224)
    p.add_argument("--channels", type=int, default=3)
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--sample", type=int, default=64)
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mouth_roi_bench measures the MI355X path: no GPU, no figure")
    from lip2speech_unit_amd import ops
    from lip2speech_unit_amd.mouth_roi import MouthCropper
    B, T, H, W, C = a.clips, a.frames, a.height, a.width, a.channels
    N = B * T
    rng = np.random.default_rng(0)
    mf = K.mean_face()
    th, s = np.deg2rad(rng.uniform(-15, 15, B)), rng.uniform(0.6, 1.0, B)
    rot = s[:, None, None] * np.stack([np.stack([np.cos(th), -np.sin(th)], -1), np.stack([np.sin(th), np.cos(th)], -1)], -2)
    centre = np.stack([rng.uniform(0.45, 0.55, B) * W, rng.uniform(0.4, 0.5, B) * H], -1)
    lm = np.einsum("lk,bjk->blj", mf - 128.0, rot)[:, None] + centre[:, None, None] + rng.normal(0, 1.0, (B, T, 68, 2))
    lm = lm.reshape(N, 68, 2)
    shape = (N, H, W, C) if C == 3 else (N, H, W)
    frames = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda")
    crop = MouthCropper(mf)
    lmd = torch.from_numpy(lm).cuda()
    lengths = [T] * B

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters

    inv, origin = crop.transforms(lmd, lengths)
    count = torch.full((B,), T, dtype=torch.int32, device="cuda")
    first = torch.arange(B, dtype=torch.int32, device="cuda") * T
    mfd, ids = crop._tables(lmd.device)
    t_ms = timed(lambda: ops.mouth_transforms(lmd, first, count, mfd, ids, inv, origin, B=B))
    pick = np.linspace(0, N - 1, min(a.sample, N)).astype(int)
    inv_h, org_h = inv.cpu().numpy(), origin.cpu().numpy()
    src_bytes = float(np.mean([touched_pixels(inv_h[i], org_h[i], H, W) for i in pick])) * C * N
    roi = torch.empty(N, 96, 96, C, dtype=torch.uint8, device="cuda")
    gray = torch.empty(N, 96, 96, dtype=torch.uint8, device="cuda")
    mi = torch.empty(N, 88, 88, dtype=torch.float32, device="cuda")
    out = {"clips": B, "frames_per_clip": T, "frame": [H, W, C], "transforms_ms": round(t_ms, 4),
           "source_bytes_touched_per_frame": round(src_bytes / N, 1), "frame_bytes": H * W * C}
    for name, kw in (("gray", dict(gray=gray)), ("model_in", dict(model_in=mi)), ("roi_gray_model_in", dict(roi=roi, gray=gray, model_in=mi))):
        ms = timed(lambda: ops.mouth_warp(frames, inv, origin, **kw))
        touched = src_bytes + 56.0 * N + sum(t.numel() * t.element_size() for t in kw.values())
        out[name] = {"ms": round(ms, 4), "touched_GB": round(touched / 1e9, 4), "GBps": round(touched / ms / 1e6, 1),
                     "frames_per_s": round(N / ms * 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
