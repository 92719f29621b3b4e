// Nearest-centroid labels (l2s_kmeans_assign): the quantiser of the speech units,
//
//   ids[m] = argmin_k ( |c_k|^2 - 2 x_m . c_k )            avhubert/clustering/dump_km_label.py:26-52 (ApplyKmeans.__call__)
//
// i.e. its dist.argmin(dim=1) without the row-constant |x|^2.  One launch; the [M, K] distances never leave the chip.
//
// Tile.  A block (4 waves) owns BM = 32 rows of x and walks the centres in passes of 128; in a pass wave w owns centres
// 128 p + 32 w .. + 31.  The products run on the f32-input matrix instruction v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma
// chain per dot product) with the CENTRES as the A operand: a lane ends with one row of x (lane & 31) and 16 centres in its
// registers, in ascending index order, so the running (best, argbest, second best) of a row is kept in-lane with a strict
// "<" - the lowest index wins a tie - and only the final merge crosses lanes (one shuffle with lane ^ 32) and waves (LDS).
// One accumulator chain per wave is the instruction's full rate (its dependent latency equals its issue interval).
// D is walked in chunks of 32: x chunk [32 k][32 + 4] and centre chunk [32 k][128 + 4] floats in LDS, k-major, written
// transposed from 16-byte global loads (the layout of tapgemm_f32.hip: both the writes and the one-float-per-lane fragment
// reads are bank-conflict free).  22.5 KB of LDS.  Centres past K are computed on centre K - 1 and discarded.
// Traffic: x once per pass (K = 200: twice, from L2), the centres once per block (K D 4 bytes = 614 KB at 200 x 768, L2
// resident), 4 (+8) bytes per row out.
#include "l2s_common.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int BM = 32, BN = 128, BK = 32;
constexpr int LDX = BM + 4, LDC = BN + 4;

struct Best {
  float d, d2;
  int i;
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

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, const int ldx, const float* __restrict__ cen,
                                                            const float* __restrict__ cnorm, const int32_t* __restrict__ lens,
                                                            const int len_mul, const int M, const int T, const int D, const int K,
                                                            int32_t* __restrict__ ids, float* __restrict__ best2) {
  __shared__ float sX[BK][LDX];
  __shared__ float sC[BK][LDC];
  __shared__ Best sBest[4][BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * BM;
  const int lr = lane & 31, lh = lane >> 5;

  // fetch roles: x chunk = 32 rows x 8 float4 (one per thread); centre chunk = 128 rows x 8 float4 (four per thread)
  const int xr = tid >> 3, xk = (tid & 7) * 4;
  const float* xrow = x + (int64_t)min(m0 + xr, M - 1) * ldx + xk;

  Best best;
  best.d = INFINITY; best.d2 = INFINITY; best.i = 0x7fffffff;

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
      __syncthreads();                                   // the previous chunk's fragments are read
      sX[xk + 0][xr] = vx.x; sX[xk + 1][xr] = vx.y; sX[xk + 2][xr] = vx.z; sX[xk + 3][xr] = vx.w;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int r = xr + 32 * h;
        sC[xk + 0][r] = vc[h].x; sC[xk + 1][r] = vc[h].y; sC[xk + 2][r] = vc[h].z; sC[xk + 3][r] = vc[h].w;
      }
      __syncthreads();
      if (wave_on) {
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
          const int k = 2 * s + lh;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sC[k][32 * wave + lr], sX[k][lr], acc, 0, 0, 0);
        }
      }
    }
    if (wave_on) {
      // register e of a lane: centre nw + 8 (e >> 2) + 4 lh + (e & 3) (ascending in e), row m0 + lr
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
  if (lh == 0) sBest[wave][lr] = best;
  __syncthreads();
  if (tid < BM) {
    const int m = m0 + tid;
    if (m < M) {
      Best r = merge(merge(sBest[0][tid], sBest[1][tid]), merge(sBest[2][tid], sBest[3][tid]));
      bool keep = true;
      if (lens) {
        const int clip = m / T;
        keep = (m - clip * T) < lens[clip] * len_mul;
      }
      ids[m] = keep ? r.i : -1;
      if (best2) {
        best2[2 * (int64_t)m] = keep ? r.d : 0.f;
        best2[2 * (int64_t)m + 1] = keep ? r.d2 : 0.f;
      }
    }
  }
}

}  // namespace

extern "C" int l2s_kmeans_assign(const float* x, int ldx, const float* centers, const float* cnorm, const int32_t* lens, int len_mul,
                                 int B, int T, int D, int K, int32_t* ids, float* best2, void* stream) {
  if (!x || !centers || !cnorm || !ids) return L2S_EINVAL;
  if (B <= 0 || T <= 0 || D <= 0 || K <= 0) return L2S_ESHAPE;
  if (lens && len_mul <= 0) return L2S_EINVAL;
  if (ldx < D) return L2S_ESHAPE;
  if ((D & 31) || D > 1024 || K < 2 || K > 1024) return L2S_EUNSUPPORTED;
  const int64_t M = (int64_t)B * T;
  if (M >= ((int64_t)1 << 31) - BM) return L2S_EUNSUPPORTED;
  if ((ldx & 3) || ((uintptr_t)x & 15) || ((uintptr_t)centers & 15) || ((uintptr_t)cnorm & 3) || ((uintptr_t)ids & 3) ||
      ((uintptr_t)best2 & 3))
    return L2S_EALIGN;
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)((M + BM - 1) / BM)), dim3(256), 0, (hipStream_t)stream, x, ldx, centers, cnorm,
                     lens, len_mul, (int)M, T, D, K, ids, best2);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
