// Mouth ROIs from raw frames and 68-point landmarks (lip2speech_unit_amd/mouth_roi.py): what
// avhubert/preparation/align_mouth.py:33-44, 63-87, 130-181 does per frame with skimage and cv2 on the host.
//
//   l2s_mouth_transforms  per frame: the similarity transform (Umeyama, closed form in 2-D) of the forward-window mean of the
//                         stable landmarks onto the mean face, its inverse map, and the clamped, rounded origin of the crop window
//   l2s_mouth_warp        per frame: the crop window of tf.warp(order 1, constant 0) - never the 256 x 256 image around it - as
//                         uint8 ROI, cv2 8-bit gray and / or the normalised fp32 stem input
//
// All geometry is fp64.  Contraction is off for the whole file: the warp follows skimage's operation order - (m0 x + m1 y) + m2,
// (1 - d) a + d b - with every product and sum rounded on its own, so that an exact case (an identity or integer-shift map, a
// half-way blend) truncates to the level the host code truncates to; a fused multiply-add would move those by one ulp.
//
// Warp.  A block of 256 threads owns a 32 x 32 tile of one frame's window; a thread owns 4 consecutive pixels of a row, so the
// ROI leaves as dwords (12 bytes of BGR, 4 of gray) and the stem input as a float4.  A pixel's two horizontal neighbours are 2 C
// consecutive source bytes at an arbitrary address: they are fetched as the 1 .. 3 aligned dwords that cover them and shifted
// into place.  Every fetched dword holds at least one byte of the frame, so no load leaves the buffer's pages.  u8 / 255.0 is a
// 256-entry fp64 table in LDS (a true division per entry, once per block) instead of 12 divisions per pixel; a reciprocal with
// one fma refinement gives the same 256 quotients without LDS and measured 1.2 x slower: the kernel is bound by its fp64 VALU work.
#include "l2s_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MAX_STABLE = 16;

__global__ __launch_bounds__(256) void mouth_transforms_kernel(const double* __restrict__ lm, const int N, const int L,
                                                               const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                               const double* __restrict__ mean_face, const int32_t* __restrict__ stable,
                                                               const int n_stable, const int window_margin, const int std_h,
                                                               const int std_w, const int half_h, const int half_w, const int i0,
                                                               const int i1, double* __restrict__ inv, int32_t* __restrict__ origin) {
  __shared__ double sDst[2 * MAX_STABLE];                // the mean face at the stable ids, centroid removed
  __shared__ int sId[MAX_STABLE];
  __shared__ double sMean[2];
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid < n_stable) sId[tid] = min(max(stable[tid], 0), L - 1);
  __syncthreads();
  if (tid == 0) {
    double mx = 0.0, my = 0.0;
    for (int j = 0; j < n_stable; ++j) {
      mx += mean_face[2 * sId[j]];
      my += mean_face[2 * sId[j] + 1];
    }
    sMean[0] = mx / n_stable;
    sMean[1] = my / n_stable;
  }
  __syncthreads();
  if (tid < n_stable) {
    sDst[2 * tid] = mean_face[2 * sId[tid]] - sMean[0];
    sDst[2 * tid + 1] = mean_face[2 * sId[tid] + 1] - sMean[1];
  }
  __syncthreads();
  const int f = min(max(first[b], 0), N);
  const int cnt = max(0, min(count[b], N - f));          // rows outside the landmark array do not exist
  const int margin = min(cnt, window_margin);
  for (int t = tid; t < cnt; t += 256) {
    const int tw = min(t, cnt - margin);                 // tail rule: the last margin - 1 frames reuse the last full window
    const double* w0 = lm + ((int64_t)(f + tw) * L) * 2;
    // src = mean over the window's frames (in frame order) of the stable points, then Umeyama's sums
    double sx = 0.0, sy = 0.0, a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0, var = 0.0;
    double px[MAX_STABLE], py[MAX_STABLE];               // unrolled below: registers, not scratch
#pragma unroll
    for (int j = 0; j < MAX_STABLE; ++j) {
      px[j] = 0.0, py[j] = 0.0;
      if (j < n_stable) {
        for (int k = 0; k < margin; ++k) {
          px[j] += w0[((int64_t)k * L + sId[j]) * 2];
          py[j] += w0[((int64_t)k * L + sId[j]) * 2 + 1];
        }
        px[j] /= margin, py[j] /= margin;
        sx += px[j], sy += py[j];
      }
    }
    sx /= n_stable, sy /= n_stable;
#pragma unroll
    for (int j = 0; j < MAX_STABLE; ++j) {
      if (j < n_stable) {
        const double cx = px[j] - sx, cy = py[j] - sy, dx = sDst[2 * j], dy = sDst[2 * j + 1];
        a00 += dx * cx, a01 += dx * cy, a10 += dy * cx, a11 += dy * cy;
        var += cx * cx + cy * cy;
      }
    }
    // A = dst^T src / n; rotation [[p, -q], [q, p]] / r; scale r / var(src): a zero variance gives NaN, which the host class reports
    const double p = (a00 + a11) / n_stable, q = (a10 - a01) / n_stable, r = hypot(p, q);
    const double s = r / (var / n_stable);
    const double ca = s * (p / r), sa = s * (q / r);     // M = [[ca, -sa, tx], [sa, ca, ty]]
    const double tx = sMean[0] - (ca * sx - sa * sy), ty = sMean[1] - (sa * sx + ca * sy);
    // the window: frame t's own mouth points through M, their mean, clamped low then high, rounded half to even
    const double* own = lm + ((int64_t)(f + t) * L) * 2;
    double mx = 0.0, my = 0.0;
    for (int j = i0; j < i1; ++j) {
      const double x = own[2 * j], y = own[2 * j + 1];
      mx += ca * x - sa * y + tx;
      my += sa * x + ca * y + ty;
    }
    mx /= (i1 - i0), my /= (i1 - i0);
    if (my - half_h < 0) my = half_h;
    if (mx - half_w < 0) mx = half_w;
    if (my + half_h > std_h) my = std_h - half_h;
    if (mx + half_w > std_w) mx = std_w - half_w;
    // rint of a NaN or of a value past int32 has no integer: such a frame gets origin 0 (its inv row is NaN, every sample 0)
    const double ry = rint(my) - half_h, rx = rint(mx) - half_w;
    const int64_t row = f + t;
    origin[2 * row] = fabs(rx) < 2147483647.0 ? (int)rx : 0;
    origin[2 * row + 1] = fabs(ry) < 2147483647.0 ? (int)ry : 0;
    // M^-1 = [[ca, sa], [-sa, ca]] / (ca^2 + sa^2), translation -M^-1 t
    const double det = ca * ca + sa * sa, ia = ca / det, ib = sa / det;
    double* o = inv + row * 6;
    o[0] = ia, o[1] = ib, o[2] = -(ia * tx + ib * ty);
    o[3] = -ib, o[4] = ia, o[5] = -(ia * ty - ib * tx);
  }
}

// the C (left) and C (right) bytes of the pixels fx, fx + 1 of one frame row, a pixel outside [0, W) as zeros; -1 <= fx <= W - 1
template <int C>
__device__ __forceinline__ uint64_t load_pair(const uint8_t* __restrict__ row, const int fx, const int W) {
  const int lo = max(fx, 0), hi = min(fx + 1, W - 1);
  const int nb = (hi - lo + 1) * C;                      // C or 2 C bytes, all inside the row
  const uintptr_t addr = (uintptr_t)(row + (int64_t)lo * C);
  const int sh = (int)(addr & 3);
  const uint32_t* p = (const uint32_t*)(addr - sh);
  const uint32_t d0 = p[0];
  const uint32_t d1 = sh + nb > 4 ? p[1] : 0u;           // a dword is fetched only if it holds one of the nb bytes
  const uint32_t d2 = sh + nb > 8 ? p[2] : 0u;
  const uint64_t lo32 = (((uint64_t)d1 << 32) | d0) >> (8 * sh), hi32 = (((uint64_t)d2 << 32) | d1) >> (8 * sh);
  uint64_t v = (lo32 & 0xffffffffull) | (hi32 << 32);
  v &= (1ull << (8 * nb)) - 1;                           // nb <= 6
  return fx < 0 ? v << (8 * C) : v;
}

constexpr int TILE = 32, PX = 4;

template <int C>
__global__ __launch_bounds__(256) void mouth_warp_kernel(const uint8_t* __restrict__ frames, const int H, const int W,
                                                         const double* __restrict__ inv, const int32_t* __restrict__ origin,
                                                         const int ch, const int cw, const int tiles_x, const int tiles,
                                                         uint8_t* __restrict__ roi, uint8_t* __restrict__ gray,
                                                         float* __restrict__ model_in, const int mc, const float mean, const float stdv,
                                                         const int wide_u8, const int wide_f32) {
  const int tid = threadIdx.x;
  __shared__ double sLevel[256];                         // u8 / 255.0, skimage's img_as_float
  sLevel[tid] = (double)tid / 255.0;
  __syncthreads();
  const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
  const int oy = (tile / tiles_x) * TILE + (tid >> 3), ox0 = (tile % tiles_x) * TILE + (tid & 7) * PX;
  if (oy >= ch || ox0 >= cw) return;
  const double m0 = inv[(int64_t)n * 6], m1 = inv[(int64_t)n * 6 + 1], m2 = inv[(int64_t)n * 6 + 2];
  const double m3 = inv[(int64_t)n * 6 + 3], m4 = inv[(int64_t)n * 6 + 4], m5 = inv[(int64_t)n * 6 + 5];
  const double x0 = (double)origin[2 * (int64_t)n], y = (double)origin[2 * (int64_t)n + 1] + (double)oy;
  const uint8_t* __restrict__ frame = frames + (int64_t)n * H * W * C;
  const int npx = min(PX, cw - ox0);

  uint32_t q[PX][C];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
#pragma unroll
    for (int c = 0; c < C; ++c) q[i][c] = 0;
    if (i >= npx) continue;
    const double x = x0 + (double)(ox0 + i);
    const double sx = (m0 * x + m1 * y) + m2, sy = (m3 * x + m4 * y) + m5;
    // floor in (-1, W) x (-1, H) leaves at least one neighbour inside; anything else (a NaN too) samples zeros only
    if (!(sx > -1.0 && sx < (double)W && sy > -1.0 && sy < (double)H)) continue;
    const double flx = floor(sx), fly = floor(sy);
    const double dc = sx - flx, dr = sy - fly;
    const int fx = (int)flx, fy = (int)fly;
    const uint64_t top = fy >= 0 ? load_pair<C>(frame + (int64_t)fy * W * C, fx, W) : 0ull;
    const uint64_t bot = fy + 1 < H ? load_pair<C>(frame + (int64_t)(fy + 1) * W * C, fx, W) : 0ull;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double tl = sLevel[(top >> (8 * c)) & 255], tr = sLevel[(top >> (8 * (C + c))) & 255];
      const double bl = sLevel[(bot >> (8 * c)) & 255], br = sLevel[(bot >> (8 * (C + c))) & 255];
      const double t = (1.0 - dc) * tl + dc * tr, u = (1.0 - dc) * bl + dc * br;
      const double v = ((1.0 - dr) * t + dr * u) * 255.0;
      q[i][c] = (uint32_t)min((int)v, 255);              // astype('uint8'): truncation
    }
  }

  uint32_t g[PX];                                        // cv2's 8-bit BGR2GRAY on the truncated ROI
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    if constexpr (C == 3) g[i] = (1868u * q[i][0] + 9617u * q[i][1] + 4899u * q[i][2] + 8192u) >> 14;
    else g[i] = q[i][0];
  }

  const int64_t pix = ((int64_t)n * ch + oy) * cw + ox0;
  if (wide_u8 && npx == PX) {                            // cw % 4 == 0: every group starts on a dword
    if (roi) {
      uint32_t* o = (uint32_t*)(roi + pix * C);
      if constexpr (C == 3) {
        o[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
        o[1] = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
        o[2] = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
      } else {
        o[0] = q[0][0] | q[1][0] << 8 | q[2][0] << 16 | q[3][0] << 24;
      }
    }
    if (gray) *(uint32_t*)(gray + pix) = g[0] | g[1] << 8 | g[2] << 16 | g[3] << 24;
  } else {
    for (int i = 0; i < npx; ++i) {
      if (roi)
        for (int c = 0; c < C; ++c) roi[(pix + i) * C + c] = (uint8_t)q[i][c];
      if (gray) gray[pix + i] = (uint8_t)g[i];
    }
  }
  if (model_in) {                                        // data.normalize_frames: /255 -> centre crop -> (x - mean) / std, fp32 divisions
    const int my = oy - (ch - mc) / 2, mx0 = ox0 - (cw - mc) / 2;
    if (my >= 0 && my < mc) {
      float z[PX];
#pragma unroll
      for (int i = 0; i < PX; ++i) z[i] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)g[i], 255.0f), mean), stdv);
      float* o = model_in + ((int64_t)n * mc + my) * mc + mx0;
      if (wide_f32 && npx == PX && mx0 >= 0 && mx0 + PX <= mc) {
        *(float4*)o = make_float4(z[0], z[1], z[2], z[3]);
      } else {
        for (int i = 0; i < npx; ++i)
          if (mx0 + i >= 0 && mx0 + i < mc) o[i] = z[i];
      }
    }
  }
}

}  // namespace

extern "C" int l2s_mouth_transforms(const double* landmarks, int N, int L, const int32_t* first, const int32_t* count, int B,
                                    const double* mean_face, const int32_t* stable_ids, int n_stable, int window_margin, int std_h,
                                    int std_w, int crop_h, int crop_w, int start_idx, int stop_idx, double* inv, int32_t* origin,
                                    void* stream) {
  if (!landmarks || !first || !count || !mean_face || !stable_ids || !inv || !origin) return L2S_EINVAL;
  if (N <= 0 || L <= 0 || B <= 0 || n_stable <= 0 || window_margin <= 0 || std_h <= 0 || std_w <= 0) return L2S_ESHAPE;
  if (crop_h <= 0 || crop_w <= 0 || crop_h > std_h || crop_w > std_w) return L2S_ESHAPE;
  if (start_idx < 0 || stop_idx <= start_idx || stop_idx > L) return L2S_ESHAPE;
  if (n_stable > MAX_STABLE || std_h > (1 << 20) || std_w > (1 << 20) || L > (1 << 20)) return L2S_EUNSUPPORTED;
  if ((((uintptr_t)landmarks | (uintptr_t)mean_face | (uintptr_t)inv) & 7) ||
      (((uintptr_t)first | (uintptr_t)count | (uintptr_t)stable_ids | (uintptr_t)origin) & 3))
    return L2S_EALIGN;
  hipLaunchKernelGGL(mouth_transforms_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, landmarks, N, L, first, count,
                     mean_face, stable_ids, n_stable, window_margin, std_h, std_w, crop_h / 2, crop_w / 2, start_idx, stop_idx, inv,
                     origin);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_mouth_warp(const uint8_t* frames, int N, int H, int W, int C, const double* inv, const int32_t* origin, int crop_h,
                              int crop_w, uint8_t* roi, uint8_t* gray, float* model_in, int model_crop, float mean, float std,
                              void* stream) {
  if (!frames || !inv || !origin || (!roi && !gray && !model_in)) return L2S_EINVAL;
  if (N <= 0 || H <= 0 || W <= 0 || crop_h <= 0 || crop_w <= 0) return L2S_ESHAPE;
  if (model_in && (model_crop <= 0 || model_crop > crop_h || model_crop > crop_w || !(std > 0.0f))) return L2S_ESHAPE;
  if (C != 1 && C != 3) return L2S_EUNSUPPORTED;
  if (H > 32768 || W > 32768 || crop_h > 4096 || crop_w > 4096) return L2S_EUNSUPPORTED;
  const int tiles_x = (crop_w + TILE - 1) / TILE, tiles = tiles_x * ((crop_h + TILE - 1) / TILE);
  if ((int64_t)N * tiles > 0x7fffffffll) return L2S_EUNSUPPORTED;
  if (((uintptr_t)inv & 7) || (((uintptr_t)origin | (uintptr_t)roi | (uintptr_t)gray | (uintptr_t)model_in) & 3)) return L2S_EALIGN;
  const int wide_u8 = crop_w % 4 == 0;
  const int wide_f32 = model_in && wide_u8 && model_crop % 4 == 0 && ((crop_w - model_crop) / 2) % 4 == 0 && !((uintptr_t)model_in & 15);
  dim3 grid((unsigned)(N * tiles)), blk(256);
  if (C == 3)
    hipLaunchKernelGGL(mouth_warp_kernel<3>, grid, blk, 0, (hipStream_t)stream, frames, H, W, inv, origin, crop_h, crop_w, tiles_x, tiles,
                       roi, gray, model_in, model_crop, mean, std, wide_u8, wide_f32);
  else
    hipLaunchKernelGGL(mouth_warp_kernel<1>, grid, blk, 0, (hipStream_t)stream, frames, H, W, inv, origin, crop_h, crop_w, tiles_x, tiles,
                       roi, gray, model_in, model_crop, mean, std, wide_u8, wide_f32);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
