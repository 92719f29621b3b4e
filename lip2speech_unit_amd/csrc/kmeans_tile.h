// The distance tile shared by l2s_kmeans_assign (kmeans.hip) and l2s_kmeans_nearest (kmeans_fit.hip).
//
// A block (4 waves) owns BM = 32 rows of x and walks the centres in passes of 128; in a pass wave w owns centres
// 128 p + 32 w .. + 31.  The products run on the f32-input matrix instruction v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma
// chain per dot product) with the CENTRES as the A operand: a lane ends with one row of x (lane & 31) and 16 centres in its
// registers, in ascending index order, so the running (best, argbest, second best) of a row is kept in-lane with a strict
// "<" - the lowest index wins a tie - and only the final merge crosses lanes (one shuffle with lane ^ 32) and waves (LDS).
// D is walked in chunks of 32: x chunk [32 k][32 + 4] and centre chunk [32 k][128 + 4] floats in LDS, k-major, written
// transposed from 16-byte global loads.  22.5 KB of LDS.  Centres past K are computed on centre K - 1 and discarded.
#pragma once
#include "l2s_common.h"
#include <math.h>

namespace kmeans_tile {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int BM = 32, BN = 128, BK = 32;
constexpr int LDX = BM + 4, LDC = BN + 4;

struct Best {
  float d, d2;
  int i;
};

struct Smem {
  float sX[BK][LDX];
  float sC[BK][LDC];
  Best sBest[4][BM];
};

// a, b: disjoint candidate sets; ties between equal distances go to the lower index
__device__ __forceinline__ Best merge(const Best a, const Best b) {
  Best r;
  if (b.d < a.d || (b.d == a.d && b.i < a.i)) {
    r.d = b.d; r.i = b.i; r.d2 = fminf(a.d, b.d2);
  } else {
    r.d = a.d; r.i = a.i; r.d2 = fminf(a.d2, b.d);
  }
  return r;
}

// The whole block calls this.  Thread tid's fetch role: row tid >> 3 of the block's 32 (xrow points at that row's floats
// 4 (tid & 7) ..), so xrow may be any gathered row.  Returns, to threads tid < BM, the (best, second best, argbest) of
// cnorm[k] - 2 x . c_k for the block's row tid; other threads get an unspecified value.  NORM: xsq receives, in every thread,
// the sum of squares of the 4 (D / 32) floats of its row that the thread itself staged, accumulated in ascending d - the eight
// threads of a row (consecutive lanes) hold its |x|^2 between them.
template <bool NORM>
__device__ __forceinline__ Best scan_centres(const float* __restrict__ xrow, const float* __restrict__ cen,
                                             const float* __restrict__ cnorm, const int D, const int K, Smem& sm, float& xsq) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  // fetch roles: x chunk = 32 rows x 8 float4 (one per thread); centre chunk = 128 rows x 8 float4 (four per thread)
  const int xr = tid >> 3, xk = (tid & 7) * 4;

  Best best;
  best.d = INFINITY; best.d2 = INFINITY; best.i = 0x7fffffff;
  if (NORM) xsq = 0.f;

  for (int n0 = 0; n0 < K; n0 += BN) {
    const int nw = n0 + 32 * wave;
    const bool wave_on = nw < K;                         // wave-uniform
    f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int d0 = 0; d0 < D; d0 += BK) {
      const float4 vx = *reinterpret_cast<const float4*>(xrow + d0);
      float4 vc[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int n = min(n0 + xr + 32 * h, K - 1);
        vc[h] = *reinterpret_cast<const float4*>(cen + (int64_t)n * D + d0 + xk);
      }
      if (NORM && n0 == 0) xsq = fmaf(vx.w, vx.w, fmaf(vx.z, vx.z, fmaf(vx.y, vx.y, fmaf(vx.x, vx.x, xsq))));
      __syncthreads();                                   // the previous chunk's fragments are read
      sm.sX[xk + 0][xr] = vx.x; sm.sX[xk + 1][xr] = vx.y; sm.sX[xk + 2][xr] = vx.z; sm.sX[xk + 3][xr] = vx.w;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int r = xr + 32 * h;
        sm.sC[xk + 0][r] = vc[h].x; sm.sC[xk + 1][r] = vc[h].y; sm.sC[xk + 2][r] = vc[h].z; sm.sC[xk + 3][r] = vc[h].w;
      }
      __syncthreads();
      if (wave_on) {
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
          const int k = 2 * s + lh;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sm.sC[k][32 * wave + lr], sm.sX[k][lr], acc, 0, 0, 0);
        }
      }
    }
    if (wave_on) {
      // register e of a lane: centre nw + 8 (e >> 2) + 4 lh + (e & 3) (ascending in e), row lr of the block
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int n = nw + 8 * (e >> 2) + 4 * lh + (e & 3);
        if (n < K) {
          const float dist = fmaf(-2.0f, acc[e], cnorm[n]);
          if (dist < best.d) { best.d2 = best.d; best.d = dist; best.i = n; }
          else best.d2 = fminf(best.d2, dist);
        }
      }
    }
  }
  {
    Best o;
    o.d = __shfl_xor(best.d, 32, 64); o.d2 = __shfl_xor(best.d2, 32, 64); o.i = __shfl_xor(best.i, 32, 64);
    best = merge(best, o);
  }
  if (lh == 0) sm.sBest[wave][lr] = best;
  __syncthreads();
  if (tid < BM) best = merge(merge(sm.sBest[0][tid], sm.sBest[1][tid]), merge(sm.sBest[2][tid], sm.sBest[3][tid]));
  return best;
}

}  // namespace kmeans_tile
