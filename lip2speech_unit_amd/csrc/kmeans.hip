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
#include "kmeans_tile.h"

namespace {

using namespace kmeans_tile;   // the tile itself: kmeans_tile.h (shared with l2s_kmeans_nearest, kmeans_fit.hip)

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, const int ldx, const float* __restrict__ cen,
                                                            const float* __restrict__ cnorm, const int32_t* __restrict__ lens,
                                                            const int len_mul, const int M, const int T, const int D, const int K,
                                                            int32_t* __restrict__ ids, float* __restrict__ best2) {
  __shared__ Smem sm;
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * BM;
  const float* xrow = x + (int64_t)min(m0 + (tid >> 3), M - 1) * ldx + (tid & 7) * 4;
  float unused;
  const Best r = scan_centres<false>(xrow, cen, cnorm, D, K, sm, unused);
  if (tid < BM) {
    const int m = m0 + tid;
    if (m < M) {
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
