"""Synthetic inputs of the mouth-cropper tests: a 68-point mean face, landmarks under a known similarity plus about 1 px of
jitter, and blocky textured frames.  Fixed seeds; nothing is read from disk (the real 20words_mean_face.npy is in neither tree)."""
import zlib
from collections import namedtuple

import numpy as np

# H, W, C, T: the clip; rot (degrees), scale (face size in the source over its size in the mean face), mirror: the known similarity;
# centre: where the mean face's middle (128, 128) lands in the frame, as fractions of (W, H); mouth_shift: the mouth points are moved
# by this much in mean-face space first (a window that has to be clamped); integer: landmarks rounded and stored as int64
Case = namedtuple("Case", "name H W C T rot scale mirror centre mouth_shift integer")

CASES = [
    Case("t1-plain", 120, 160, 3, 1, 0.0, 0.5, False, (0.5, 0.5), (0, 0), False),
    Case("t5-rot+20-s0.4-gray", 97, 131, 1, 5, 20.0, 0.4, False, (0.5, 0.5), (0, 0), False),
    Case("t12-rot-20-s0.7", 97, 131, 3, 12, -20.0, 0.7, False, (0.45, 0.5), (0, 0), False),
    Case("t13-mirrored", 120, 160, 3, 13, 7.0, 1.0, True, (0.5, 0.4), (0, 0), False),
    Case("t30-s2-leaves-frame-gray", 120, 160, 1, 30, -5.0, 2.0, False, (0.5, 0.1), (0, 0), False),
    Case("t13-corner-negative-coords", 97, 131, 3, 13, 12.0, 0.8, False, (0.1, -0.3), (0, 0), False),
    Case("t5-clamped-high", 120, 160, 3, 5, 3.0, 0.5, False, (0.5, 0.5), (90, 45), False),
    Case("t12-clamped-low-gray", 120, 160, 1, 12, -3.0, 0.5, False, (0.5, 0.5), (-100, -150), False),
    Case("t30-integer-landmarks", 97, 131, 3, 30, 10.0, 0.6, False, (0.5, 0.45), (0, 0), True),
]
RAGGED = [Case(f"ragged-{i}", 97, 131, 3, T, rot, s, False, (0.5, 0.5), (0, 0), False)
          for i, (T, rot, s) in enumerate(((13, 15.0, 0.5), (1, -8.0, 0.9), (30, 2.0, 0.45), (5, -20.0, 1.3)))]


def mean_face():
    """68 points in the 256 x 256 aligned image, laid out like the iBUG scheme: jaw 0-16, brows 17-26, nose 27-35, eyes 36-47,
    mouth 48-67 (an outer ring of 12 and an inner ring of 8 around (128, 186))."""
    p = np.zeros((68, 2))
    a = np.linspace(np.pi, 0.0, 17)
    p[0:17] = np.stack([128 - 88 * np.cos(np.pi - a), 110 + 120 * np.sin(a)], 1)
    p[17:22] = np.stack([np.linspace(62, 112, 5), 72 - 6 * np.sin(np.linspace(0, np.pi, 5))], 1)
    p[22:27] = np.stack([np.linspace(144, 194, 5), 72 - 6 * np.sin(np.linspace(0, np.pi, 5))], 1)
    p[27:31] = np.stack([np.full(4, 128.0), np.linspace(92, 130, 4)], 1)
    p[31:36] = np.stack([np.linspace(110, 146, 5), 142 + 4 * np.sin(np.linspace(0, np.pi, 5))], 1)
    for k, cx in ((36, 97.5), (42, 158.5)):
        t = np.linspace(np.pi, -np.pi, 6, endpoint=False)
        p[k:k + 6] = np.stack([cx + 12.5 * np.cos(t), 96 - 5 * np.sin(t)], 1)
    t = np.linspace(np.pi, -np.pi, 12, endpoint=False)
    p[48:60] = np.stack([128 + 30 * np.cos(t), 186 - 13 * np.sin(t)], 1)
    t = np.linspace(np.pi, -np.pi, 8, endpoint=False)
    p[60:68] = np.stack([128 + 18 * np.cos(t), 186 - 5 * np.sin(t)], 1)
    return p


def _rng(case):
    return np.random.default_rng(zlib.crc32(case.name.encode()))


def landmarks(case):
    """[T, 68, 2]: the mean face through the case's similarity into the frame, about 1 px of jitter per point and frame and a slow drift."""
    rng = _rng(case)
    mf = mean_face()
    mf[48:68] += np.asarray(case.mouth_shift, dtype=np.float64)
    if case.mirror:
        mf[:, 0] = 256.0 - mf[:, 0]
    th = np.deg2rad(case.rot)
    R = case.scale * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([case.centre[0] * case.W, case.centre[1] * case.H])
    drift = np.cumsum(rng.normal(0.0, 0.3, size=(case.T, 1, 2)), axis=0)
    lm = (mf - 128.0) @ R.T + c + drift + rng.normal(0.0, 1.0, size=(case.T, 68, 2))
    return np.rint(lm).astype(np.int64) if case.integer else lm


def frames(case):
    """uint8 [T, H, W, C] (C = 3) or [T, H, W] (C = 1): 8 x 8 blocks of random levels that shift from frame to frame, plus noise."""
    rng = _rng(case)
    rng.bit_generator.advance(1 << 20)                   # not the landmarks' stream
    C = case.C
    blocks = rng.integers(16, 240, size=(case.H // 8 + 2 + case.T, case.W // 8 + 2, C))
    out = np.empty((case.T, case.H, case.W, C), dtype=np.uint8)
    for t in range(case.T):
        tex = np.repeat(np.repeat(blocks[t:t + case.H // 8 + 2], 8, axis=0), 8, axis=1)[3:3 + case.H, 5:5 + case.W]
        out[t] = np.clip(tex + rng.integers(-12, 13, size=tex.shape), 0, 255).astype(np.uint8)
    return out if C == 3 else out[..., 0]
