"""The mouth cropper restated for the tests, independent of lip2speech_unit_amd: what
avhubert/preparation/align_mouth.py:33-44, 63-87, 130-181 computes with skimage and cv2, in plain numpy.

  umeyama_svd      skimage's `_umeyama(src, dst, estimate_scale=True)` as it is written there (SVD form)
  umeyama_closed   the 2-D closed form the device uses
  clip_transforms  the forward window of landmarks, the tail rule, cut_patch's clamps and rounding
  warp_window      tf.warp(order 1, mode 'constant', cval 0) restricted to the crop window, before quantisation
  quantise / bgr2gray / crop_clip  the uint8 steps

`dtype` evaluates the same code in another float format: the float32 run is the measuring stick of the GPU gates.  Parity
with skimage and cv2 themselves cannot be checked where they are not installed; tests/test_mouth_roi_cpu.py pins the warp
against scipy.ndimage.map_coordinates instead."""
import numpy as np

STABLE_IDS = (33, 36, 39, 42, 45)


def umeyama_svd(src, dst):
    src, dst = np.asarray(src), np.asarray(dst)
    num, dim = src.shape
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    src_demean, dst_demean = src - src_mean, dst - dst_mean
    A = dst_demean.T @ src_demean / num
    d = np.ones((dim,), dtype=src.dtype)
    if np.linalg.det(A) < 0:
        d[dim - 1] = -1
    T = np.eye(dim + 1, dtype=src.dtype)
    U, S, V = np.linalg.svd(A)
    rank = np.linalg.matrix_rank(A)
    if rank == 0:
        return np.nan * T
    elif rank == dim - 1:
        if np.linalg.det(U) * np.linalg.det(V) > 0:
            T[:dim, :dim] = U @ V
        else:
            s = d[dim - 1]
            d[dim - 1] = -1
            T[:dim, :dim] = U @ np.diag(d) @ V
            d[dim - 1] = s
    else:
        T[:dim, :dim] = U @ np.diag(d) @ V
    scale = 1.0 / src_demean.var(axis=0).sum() * (S @ d)
    T[:dim, dim] = dst_mean - scale * (T[:dim, :dim] @ src_mean.T)
    T[:dim, :dim] *= scale
    return T


def umeyama_closed(src, dst):
    src, dst = np.asarray(src), np.asarray(dst)
    n = src.shape[0]
    src_mean, dst_mean = src.mean(axis=0), dst.mean(axis=0)
    sc, dc = src - src_mean, dst - dst_mean
    A = dc.T @ sc / n
    p, q = A[0, 0] + A[1, 1], A[1, 0] - A[0, 1]
    r = np.hypot(p, q)
    R = np.array([[p, -q], [q, p]], dtype=src.dtype) / r
    s = r / sc.var(axis=0).sum()
    T = np.eye(3, dtype=src.dtype)
    T[:2, :2] = s * R
    T[:2, 2] = dst_mean - s * (R @ src_mean)
    return T


def window_start(t, T, window_margin=12):
    """The first frame of the landmark window whose transform frame t uses, and the window's length."""
    margin = min(T, window_margin)
    return min(t, T - margin), margin


def clip_transforms(landmarks, mean_face, window_margin=12, stable_ids=STABLE_IDS, start_idx=48, stop_idx=68, std_size=(256, 256),
                    crop=(96, 96), estimator=umeyama_svd, dtype=np.float64):
    """One clip: landmarks [T, L, 2] -> (M [T, 3, 3], inv [T, 3, 3], centre [T, 2] = the clamped (cx, cy), origin int [T, 2] = (x0, y0))."""
    lm = np.asarray(landmarks).astype(dtype)
    mf = np.asarray(mean_face).astype(dtype)
    T = lm.shape[0]
    ids = list(stable_ids)
    height, width = crop[0] // 2, crop[1] // 2
    Ms, invs, centres, origins = [], [], [], []
    for t in range(T):
        t0, margin = window_start(t, T, window_margin)
        smoothed = np.mean(lm[t0:t0 + margin], axis=0)
        M = estimator(smoothed[ids], mf[ids])
        pts = lm[t, start_idx:stop_idx]
        trans = np.concatenate([pts, np.ones((pts.shape[0], 1), dtype=dtype)], axis=1) @ M.T
        cx, cy = np.mean(trans[:, :2] / trans[:, 2:3], axis=0)
        if cy - height < 0:
            cy = height
        if cx - width < 0:
            cx = width
        if cy + height > std_size[0]:
            cy = std_size[0] - height
        if cx + width > std_size[1]:
            cx = std_size[1] - width
        Ms.append(M)
        invs.append(np.linalg.inv(M))
        centres.append((float(cx), float(cy)))
        origins.append((int(round(float(cx)) - round(width)), int(round(float(cy)) - round(height))))
    return np.stack(Ms), np.stack(invs), np.asarray(centres, dtype=np.float64), np.asarray(origins, dtype=np.int64)


def source_coords(inv, origin, crop=(96, 96), dtype=np.float64):
    """(sx, sy) [ch, cw] of the window's output pixels: skimage's _transform_affine, (m0 x + m1 y) + m2."""
    m = np.asarray(inv).astype(dtype)
    X, Y = np.meshgrid((origin[0] + np.arange(crop[1])).astype(dtype), (origin[1] + np.arange(crop[0])).astype(dtype))
    return (m[0, 0] * X + m[0, 1] * Y) + m[0, 2], (m[1, 0] * X + m[1, 1] * Y) + m[1, 2]


def warp_window(frame, inv, origin, crop=(96, 96), dtype=np.float64):
    """frame uint8 [H, W] or [H, W, C] -> float [ch, cw, C] in [0, 1]: the window of tf.warp's output, not yet times 255."""
    frame = np.asarray(frame)
    img = (frame if frame.ndim == 3 else frame[:, :, None]).astype(dtype) / dtype(255)
    H, W = img.shape[:2]
    sx, sy = source_coords(inv, origin, crop, dtype)
    fx, fy = np.floor(sx), np.floor(sy)
    dc, dr = (sx - fx)[..., None], (sy - fy)[..., None]
    # far outside the frame every neighbour is 0; clipping first keeps the integer conversion defined
    c0, r0 = np.clip(fx, -2, W + 1).astype(np.int64), np.clip(fy, -2, H + 1).astype(np.int64)

    def pixel(r, c):
        ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        out = np.zeros(r.shape + (img.shape[2],), dtype=dtype)
        out[ok] = img[r[ok], c[ok]]
        return out

    top = (1 - dc) * pixel(r0, c0) + dc * pixel(r0, c0 + 1)
    bottom = (1 - dc) * pixel(r0 + 1, c0) + dc * pixel(r0 + 1, c0 + 1)
    return (1 - dr) * top + dr * bottom


def quantise(warped):
    """align_mouth.py:36-37: times 255, astype('uint8') (truncation)."""
    return (warped * warped.dtype.type(255)).astype(np.uint8)


def bgr2gray(roi):
    """cv2's 8-bit COLOR_BGR2GRAY; a one-channel ROI is its own gray."""
    if roi.shape[-1] == 1:
        return roi[..., 0].copy()
    b, g, r = (roi[..., i].astype(np.int64) for i in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def crop_clip(frames, landmarks, mean_face, dtype=np.float64, warp_dtype=None, **kw):
    """frames uint8 [T, H, W(, C)] -> dict(inv, centre, origin, roi uint8 [T, ch, cw, C], gray uint8 [T, ch, cw]).  The transforms
    run in `dtype`, the warp in `warp_dtype` (default: the same)."""
    crop = kw.get("crop", (96, 96))
    _, inv, centre, origin = clip_transforms(landmarks, mean_face, dtype=dtype, **kw)
    wd = dtype if warp_dtype is None else warp_dtype
    roi = np.stack([quantise(warp_window(frames[t], inv[t], origin[t], crop, wd)) for t in range(len(frames))])
    return {"inv": inv, "centre": centre, "origin": origin, "roi": roi, "gray": bgr2gray(roi)}


# ---- align_mouth.py:24-30, 184-205 transcribed as cases: what landmarks_interpolate must return ----------------------------------
def interpolate_expected(landmarks):
    """Linear fill of inner gaps, the ends extended, None when nothing was detected."""
    valid = [i for i, v in enumerate(landmarks) if v is not None]
    if not valid:
        return None
    out = [None if v is None else np.asarray(v, dtype=np.float64) for v in landmarks]
    for a, b in zip(valid[:-1], valid[1:]):
        for i in range(a + 1, b):
            out[i] = out[a] + (i - a) / float(b - a) * (out[b] - out[a])
    for i in range(valid[0]):
        out[i] = out[valid[0]]
    for i in range(valid[-1] + 1, len(out)):
        out[i] = out[valid[-1]]
    return out
