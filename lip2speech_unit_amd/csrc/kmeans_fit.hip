// Mini-batch k-means fit on the device: the kernels behind lip2speech_unit_amd/kmeans_fit.py, which restates what
// avhubert/clustering/learn_kmeans.py:25-47,88-121 asks of scikit-learn's MiniBatchKMeans.  Everything fp32 in memory, every
// reduction in a fixed order (no floating-point atomics): the same bits from run to run.
//
//   l2s_kmeans_nearest  the distance tile of kmeans_tile.h (f32-input MFMA, [M, K] distances stay on chip) over a gathered batch;
//                       the row norm |x|^2 comes from the chunks the tile stages anyway: ids, dmin = max(0, |x|^2 + |c|^2 - 2 x.c)
//                       and the batch inertia (32-row block partials in fp64, then one finishing block).
//                       Traffic: the batch once per pass of 128 centres (L2 hits after the first), the centres once per block.
//   l2s_kmeans_update   stable counting sort of the batch positions by label - per-256-position histograms (integer LDS atomics:
//                       exact), one scan block, a scatter that ranks inside its 256 positions - then one block per centre sums
//                       its members in ascending batch position with 16-byte loads (thread t owns floats 4 t .. 4 t + 3 of the
//                       row, D <= 1024), applies c <- (c w + sum x) / (w + n), w <- w + n and writes |c|^2 (fp64 sum).
//                       Traffic: each batch row once more, K D floats in and out.
//   l2s_kmeans_pp_pot   k-means++ potentials of up to 16 candidate rows: a wave per row of the subset, the candidates in LDS
//                       (at most 48 KB per launch), sum (x - c)^2 directly in fp32 (exact on small integers, unlike the norm
//                       expansion it needs no cancellation), sum_i min(closest_i, d_i) in fp64: 64-row block partials, one
//                       finishing block per candidate.  With closest_out it writes the new closest of one candidate.
//   l2s_kmeans_pp_pick  one block: fp64 inclusive scan of closest (1024 contiguous segments, scanned across threads in LDS) and
//                       searchsorted(side = left) of t thresholds, clipped to m - 1.
#include "kmeans_tile.h"

namespace {

using namespace kmeans_tile;

constexpr int PP_ROWS = 64;        // rows of the subset per pp_pot block (16 per wave)
constexpr int PP_MAXC = 16;        // candidates per call
constexpr int PP_LDS_FLOATS = 12288;   // candidate floats in LDS per launch (48 KB)
constexpr int SORT_BLK = 256;      // batch positions per histogram / scatter block

__device__ __forceinline__ int64_t gather_row(const int32_t* __restrict__ rows, const int pos, const int64_t N) {
  int64_t r = rows ? (int64_t)rows[pos] : (int64_t)pos;
  return r < 0 ? 0 : (r >= N ? N - 1 : r);      // a bad index reads a valid row; it never leaves x
}

__global__ __launch_bounds__(256) void nearest_kernel(const float* __restrict__ x, const int ldx, const int64_t N,
                                                      const int32_t* __restrict__ rows, const int M, const float* __restrict__ cen,
                                                      const float* __restrict__ cnorm, const int D, const int K,
                                                      int32_t* __restrict__ ids, float* __restrict__ dmin, double* __restrict__ partial) {
  __shared__ Smem sm;
  __shared__ float sN[BM];
  __shared__ double sD[BM];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * BM;
  const float* xrow = x + gather_row(rows, min(m0 + (tid >> 3), M - 1), N) * ldx + (tid & 7) * 4;
  float xsq;
  const Best r = scan_centres<true>(xrow, cen, cnorm, D, K, sm, xsq);
  // the eight threads of a row are consecutive lanes: a butterfly gives all of them the same sum
  xsq += __shfl_xor(xsq, 1, 64);
  xsq += __shfl_xor(xsq, 2, 64);
  xsq += __shfl_xor(xsq, 4, 64);
  if ((tid & 7) == 0) sN[tid >> 3] = xsq;
  __syncthreads();
  if (tid < BM) {
    const int m = m0 + tid;
    double dv = 0.0;
    if (m < M) {
      const float d = fmaxf(0.f, sN[tid] + r.d);
      if (ids) ids[m] = r.i;
      if (dmin) dmin[m] = d;
      dv = (double)d;
    }
    sD[tid] = dv;
  }
  __syncthreads();
  if (tid == 0 && partial) {
    double s = 0.0;
    for (int i = 0; i < BM; ++i) s += sD[i];
    partial[blockIdx.x] = s;
  }
}

// out[c] = sum_i part[i * stride + c], i < n: thread-strided partial sums, then a fixed LDS tree.  One block per c.
__global__ __launch_bounds__(256) void finish_sum_kernel(const double* __restrict__ part, const int n, const int stride,
                                                         double* __restrict__ out) {
  __shared__ double s[256];
  const int tid = threadIdx.x, c = blockIdx.x;
  double a = 0.0;
  for (int i = tid; i < n; i += 256) a += part[(int64_t)i * stride + c];
  s[tid] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[c] = s[0];
}

// ---- update ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SORT_BLK) void hist_kernel(const int32_t* __restrict__ ids, const int M, const int K,
                                                        int32_t* __restrict__ offs) {
  __shared__ int h[1024];
  const int tid = threadIdx.x;
  for (int k = tid; k < K; k += SORT_BLK) h[k] = 0;
  __syncthreads();
  const int i = blockIdx.x * SORT_BLK + tid;
  if (i < M) {
    const int l = ids[i];
    if (l >= 0 && l < K) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  for (int k = tid; k < K; k += SORT_BLK) offs[(int64_t)blockIdx.x * K + k] = h[k];
}

// offs[b][k] <- members of k in blocks before b; start[k] <- members of centres before k (start[K] = all)
__global__ __launch_bounds__(1024) void scan_kernel(int32_t* __restrict__ offs, const int nb, const int K, int32_t* __restrict__ start) {
  __shared__ int s[1024];
  const int k = threadIdx.x;
  int run = 0;
  if (k < K) {
    for (int b = 0; b < nb; ++b) {
      const int64_t at = (int64_t)b * K + k;
      const int t = offs[at];
      offs[at] = run;
      run += t;
    }
  }
  s[k] = run;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int v = k >= o ? s[k - o] : 0;
    __syncthreads();
    s[k] += v;
    __syncthreads();
  }
  if (k < K) start[k] = s[k] - run;
  if (k == K - 1) start[K] = s[k];
}

__global__ __launch_bounds__(SORT_BLK) void scatter_kernel(const int32_t* __restrict__ ids, const int M, const int K,
                                                           const int32_t* __restrict__ offs, const int32_t* __restrict__ start,
                                                           int32_t* __restrict__ order) {
  __shared__ int lab[SORT_BLK];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * SORT_BLK + tid;
  int l = -1;
  if (i < M) {
    l = ids[i];
    if (l < 0 || l >= K) l = -1;
  }
  lab[tid] = l;
  __syncthreads();
  if (l >= 0) {
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += lab[j] == l;
    order[start[l] + offs[(int64_t)blockIdx.x * K + l] + rank] = i;     // < start[K] <= M
  }
}

__global__ __launch_bounds__(256) void centre_update_kernel(const float* __restrict__ x, const int ldx, const int64_t N,
                                                            const int32_t* __restrict__ rows, const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ start, const float* cen, const float* counts,
                                                            const int D, float* cen_out, float* counts_out,
                                                            float* __restrict__ cnorm_out) {
  __shared__ double sw[4];
  const int tid = threadIdx.x, k = blockIdx.x;
  const int col = 4 * tid;
  const bool on = col < D;
  const int beg = start[k], end = start[k + 1];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on) {
    int j = beg;
    for (; j + 4 <= end; j += 4) {       // four rows in flight, added in ascending batch position
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(x + gather_row(rows, order[j + u], N) * ldx + col);
#pragma unroll
      for (int u = 0; u < 4; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
    for (; j < end; ++j) {
      const float4 v = *reinterpret_cast<const float4*>(x + gather_row(rows, order[j], N) * ldx + col);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
  }
  const float w = counts[k];
  const int cnt = end - beg;
  double sq = 0.0;
  if (on) {
    float4 c = *reinterpret_cast<const float4*>(cen + (int64_t)k * D + col);
    if (cnt > 0) {
      const float alpha = 1.0f / (w + (float)cnt);
      c.x = fmaf(c.x, w, acc.x) * alpha; c.y = fmaf(c.y, w, acc.y) * alpha;
      c.z = fmaf(c.z, w, acc.z) * alpha; c.w = fmaf(c.w, w, acc.w) * alpha;
    }
    *reinterpret_cast<float4*>(cen_out + (int64_t)k * D + col) = c;
    sq = (double)c.x * c.x + (double)c.y * c.y + (double)c.z * c.z + (double)c.w * c.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
  if ((tid & 63) == 0) sw[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) {
    cnorm_out[k] = (float)((sw[0] + sw[1]) + (sw[2] + sw[3]));
    counts_out[k] = cnt > 0 ? w + (float)cnt : w;
  }
}

// ---- k-means++ ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pp_pot_kernel(const float* __restrict__ x, const int ldx, const int64_t N,
                                                     const int32_t* __restrict__ rows, const int m, const int D,
                                                     const int32_t* __restrict__ cand, const int t0, int nc,
                                                     const float* closest, const double* __restrict__ select, const int nsel,
                                                     float* closest_out, int32_t* __restrict__ chosen, double* __restrict__ partial) {
  extern __shared__ __align__(16) float sc[];          // [nc][D], read as float4
  __shared__ double sW[4][PP_MAXC];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int c0 = t0;
  if (select) {                           // np.argmin: the first of equal potentials
    int best = 0;
    double bv = select[0];
    for (int j = 1; j < nsel; ++j) {
      const double v = select[j];
      if (v < bv) { bv = v; best = j; }
    }
    c0 = best;
    nc = 1;
    if (chosen && blockIdx.x == 0 && tid == 0) chosen[0] = min(max(cand[best], 0), m - 1);
  }
  const int d4 = D >> 2;
  for (int idx = tid; idx < nc * d4; idx += 256) {
    const int t = idx / d4, q = idx - t * d4;
    const int p = min(max(cand[c0 + t], 0), m - 1);
    reinterpret_cast<float4*>(sc)[idx] = *reinterpret_cast<const float4*>(x + gather_row(rows, p, N) * ldx + 4 * q);
  }
  __syncthreads();
  double sum[PP_MAXC];
#pragma unroll
  for (int t = 0; t < PP_MAXC; ++t) sum[t] = 0.0;
  const int base = blockIdx.x * PP_ROWS + wave * (PP_ROWS / 4);
  for (int rr = 0; rr < PP_ROWS / 4; ++rr) {
    const int i = base + rr;
    if (i >= m) break;                    // wave-uniform
    const float* xr = x + gather_row(rows, i, N) * ldx;
    float acc[PP_MAXC];
#pragma unroll
    for (int t = 0; t < PP_MAXC; ++t) acc[t] = 0.f;
    for (int col = 4 * lane; col < D; col += 256) {
      const float4 v = *reinterpret_cast<const float4*>(xr + col);
#pragma unroll
      for (int t = 0; t < PP_MAXC; ++t) {
        if (t < nc) {
          const float4 c = *reinterpret_cast<const float4*>(sc + t * D + col);
          const float a = v.x - c.x, b = v.y - c.y, e = v.z - c.z, f = v.w - c.w;
          acc[t] = fmaf(f, f, fmaf(e, e, fmaf(b, b, fmaf(a, a, acc[t]))));
        }
      }
    }
    const float cl = closest ? closest[i] : INFINITY;
#pragma unroll
    for (int t = 0; t < PP_MAXC; ++t) {
      if (t < nc) {
        float a = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        const float v = fminf(cl, a);
        sum[t] += (double)v;
        if (closest_out && t == 0 && lane == 0) closest_out[i] = v;
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < PP_MAXC; ++t) sW[wave][t] = sum[t];
  }
  __syncthreads();
  if (tid < nc) partial[(int64_t)blockIdx.x * PP_MAXC + t0 + tid] = (sW[0][tid] + sW[1][tid]) + (sW[2][tid] + sW[3][tid]);
}

__global__ __launch_bounds__(1024) void pp_pick_kernel(const float* __restrict__ closest, const int m, const double* __restrict__ u,
                                                       const int t, const double* __restrict__ scale, int32_t* __restrict__ idx,
                                                       double* __restrict__ total) {
  __shared__ double s[1024];
  __shared__ int found[PP_MAXC];
  const int tid = threadIdx.x;
  const int seg = (m + 1023) / 1024;
  const int64_t b64 = (int64_t)tid * seg;
  const int beg = (int)(b64 < m ? b64 : m), end = min(beg + seg, m);
  double a = 0.0;
  for (int i = beg; i < end; ++i) a += (double)closest[i];
  s[tid] = a;
  if (tid < PP_MAXC) found[tid] = m - 1;          // beyond the total: clipped to the last index
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const double v = tid >= o ? s[tid - o] : 0.0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  const double before = tid ? s[tid - 1] : 0.0;
  const double sc = scale ? scale[0] : 1.0;
  for (int j = 0; j < t; ++j) {
    const double thr = u[j] * sc;
    double p = 0.0;
    for (int i = beg; i < end; ++i) {
      p += (double)closest[i];
      if (before + p >= thr) { atomicMin(&found[j], i); break; }
    }
  }
  __syncthreads();
  if (tid < t) idx[tid] = found[tid];
  if (tid == 0 && total) total[0] = s[1023];
}

inline bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" size_t l2s_kmeans_nearest_workspace(int M) {
  if (M <= 0 || (int64_t)M >= ((int64_t)1 << 31) - BM) return 0;
  return (size_t)((M + BM - 1) / BM) * sizeof(double);
}

extern "C" int l2s_kmeans_nearest(const float* x, int ldx, int64_t N, const int32_t* rows, int M, const float* centers,
                                  const float* cnorm, int D, int K, int32_t* ids, float* dmin, double* inertia, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!x || !centers || !cnorm || (!ids && !dmin && !inertia)) return L2S_EINVAL;
  if (inertia && !workspace) return L2S_EINVAL;
  if (N <= 0 || M <= 0 || D <= 0 || K <= 0) return L2S_ESHAPE;
  if (ldx < D || (!rows && N < M)) return L2S_ESHAPE;
  if ((D & 31) || D > 1024 || K < 2 || K > 1024) return L2S_EUNSUPPORTED;
  if ((int64_t)M >= ((int64_t)1 << 31) - BM || (rows && N > 0x7fffffffLL)) return L2S_EUNSUPPORTED;
  if (inertia && workspace_bytes < l2s_kmeans_nearest_workspace(M)) return L2S_ESHAPE;
  if ((ldx & 3) || misaligned(x, 15) || misaligned(centers, 15) || misaligned(cnorm, 3) || misaligned(rows, 3) || misaligned(ids, 3) ||
      misaligned(dmin, 3) || misaligned(inertia, 7) || misaligned(workspace, 7))
    return L2S_EALIGN;
  const int nb = (M + BM - 1) / BM;
  hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, ldx, N, rows, M, centers, cnorm, D, K, ids,
                     dmin, inertia ? (double*)workspace : (double*)nullptr);
  L2S_CHECK_LAUNCH();
  if (inertia) {
    hipLaunchKernelGGL(finish_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, nb, 1, inertia);
    L2S_CHECK_LAUNCH();
  }
  return L2S_OK;
}

extern "C" size_t l2s_kmeans_update_workspace(int M, int K) {
  if (M <= 0 || M > (1 << 24) || K < 2 || K > 1024) return 0;
  const size_t nb = (size_t)(M + SORT_BLK - 1) / SORT_BLK;
  return (nb * K + (size_t)K + 1 + (size_t)M) * sizeof(int32_t);
}

extern "C" int l2s_kmeans_update(const float* x, int ldx, int64_t N, const int32_t* rows, int M, const int32_t* ids,
                                 const float* centers, const float* counts, int D, int K, float* centers_out, float* counts_out,
                                 float* cnorm_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !ids || !centers || !counts || !centers_out || !counts_out || !cnorm_out || !workspace) return L2S_EINVAL;
  if (N <= 0 || M <= 0 || D <= 0 || K <= 0) return L2S_ESHAPE;
  if (ldx < D || (!rows && N < M)) return L2S_ESHAPE;
  if ((D & 31) || D > 1024 || K < 2 || K > 1024 || M > (1 << 24) || (rows && N > 0x7fffffffLL)) return L2S_EUNSUPPORTED;
  if (workspace_bytes < l2s_kmeans_update_workspace(M, K)) return L2S_ESHAPE;
  if ((ldx & 3) || misaligned(x, 15) || misaligned(centers, 15) || misaligned(centers_out, 15) || misaligned(counts, 3) ||
      misaligned(counts_out, 3) || misaligned(cnorm_out, 3) || misaligned(rows, 3) || misaligned(ids, 3) || misaligned(workspace, 3))
    return L2S_EALIGN;
  const int nb = (M + SORT_BLK - 1) / SORT_BLK;
  int32_t* offs = (int32_t*)workspace;
  int32_t* start = offs + (size_t)nb * K;
  int32_t* order = start + K + 1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(hist_kernel, dim3((unsigned)nb), dim3(SORT_BLK), 0, s, ids, M, K, offs);
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, s, offs, nb, K, start);
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)nb), dim3(SORT_BLK), 0, s, ids, M, K, (const int32_t*)offs, (const int32_t*)start, order);
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(centre_update_kernel, dim3((unsigned)K), dim3(256), 0, s, x, ldx, N, rows, (const int32_t*)order,
                     (const int32_t*)start, centers, counts, D, centers_out, counts_out, cnorm_out);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" size_t l2s_kmeans_pp_workspace(int m) {
  if (m <= 0 || (int64_t)m >= ((int64_t)1 << 31) - PP_ROWS) return 0;
  return (size_t)((m + PP_ROWS - 1) / PP_ROWS) * PP_MAXC * sizeof(double);
}

extern "C" int l2s_kmeans_pp_pot(const float* x, int ldx, int64_t N, const int32_t* rows, int m, int D, const int32_t* cand, int t,
                                 const float* closest, const double* select, double* pot, float* closest_out, int32_t* chosen,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !cand || !workspace || (!pot && !closest_out)) return L2S_EINVAL;
  if (select && !closest_out) return L2S_EINVAL;             // a selection is made to write its closest
  if (N <= 0 || m <= 0 || D <= 0 || t <= 0) return L2S_ESHAPE;
  if (ldx < D || (!rows && N < m)) return L2S_ESHAPE;
  if (closest_out && !select && t != 1) return L2S_ESHAPE;   // one candidate's closest: name it, or give the potentials to pick by
  if ((D & 31) || D > 1024 || t > PP_MAXC || (int64_t)m >= ((int64_t)1 << 31) - PP_ROWS || (rows && N > 0x7fffffffLL))
    return L2S_EUNSUPPORTED;
  if (workspace_bytes < l2s_kmeans_pp_workspace(m)) return L2S_ESHAPE;
  if ((ldx & 3) || misaligned(x, 15) || misaligned(rows, 3) || misaligned(cand, 3) || misaligned(closest, 3) || misaligned(select, 7) ||
      misaligned(pot, 7) || misaligned(closest_out, 3) || misaligned(chosen, 3) || misaligned(workspace, 7))
    return L2S_EALIGN;
  const int nb = (m + PP_ROWS - 1) / PP_ROWS;
  const int n_out = closest_out ? 1 : t;                     // potentials computed (and written, when pot is given)
  const int per = PP_LDS_FLOATS / D < PP_MAXC ? PP_LDS_FLOATS / D : PP_MAXC;
  hipStream_t s = (hipStream_t)stream;
  for (int t0 = 0; t0 < n_out; t0 += per) {
    const int nc = n_out - t0 < per ? n_out - t0 : per;
    hipLaunchKernelGGL(pp_pot_kernel, dim3((unsigned)nb), dim3(256), (size_t)nc * D * sizeof(float), s, x, ldx, N, rows, m, D, cand, t0,
                       nc, closest, select, t, closest_out, chosen, (double*)workspace);
    L2S_CHECK_LAUNCH();
  }
  if (pot) {
    hipLaunchKernelGGL(finish_sum_kernel, dim3((unsigned)n_out), dim3(256), 0, s, (const double*)workspace, nb, PP_MAXC, pot);
    L2S_CHECK_LAUNCH();
  }
  return L2S_OK;
}

extern "C" int l2s_kmeans_pp_pick(const float* closest, int m, const double* u, int t, const double* scale, int32_t* idx,
                                  double* total, void* stream) {
  if (!closest || !idx || (t > 0 && !u)) return L2S_EINVAL;
  if (m <= 0 || t < 0) return L2S_ESHAPE;
  if (t > PP_MAXC || m > (1 << 24)) return L2S_EUNSUPPORTED;
  if (misaligned(closest, 3) || misaligned(u, 7) || misaligned(scale, 7) || misaligned(idx, 3) || misaligned(total, 7)) return L2S_EALIGN;
  hipLaunchKernelGGL(pp_pick_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, closest, m, u, t, scale, idx, total);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
