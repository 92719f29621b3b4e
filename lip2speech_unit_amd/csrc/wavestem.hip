// Waveform stem of HuBERT-base (l2s_wave_stem): layer 0 of fairseq's ConvFeatureExtractionModel in mode="default",
//
//   y[t, c] = sum_j w[c, j] x[5 t + j]                      Conv1d(1 -> C, k = 10, stride 5, no bias)
//   n[t, c] = (y[t, c] - mean_c) * rstd_c * gamma_c + beta_c   GroupNorm(C groups, C channels): per (clip, channel) over the
//   out     = gelu(n)                                           clip's own L0 = (n_b - 10) / 5 + 1 frames, biased variance
//
// written channels-last as the rows [B * T_rows, C] the CONV1D tap-GEMM of layer 1 reads.  Two launches.
//
// Statistics (wave_stem_stats_kernel, one block per clip).  y is linear in the ten strided sub-signals x_j[t] = x[5 t + j], so
// mean_c = sum_j w[c, j] m_j and var_c = w_c^T Cov w_c with m_j the mean of x_j and Cov the 10 x 10 CENTRED second moments
// sum_t (x_j[t] - m_j)(x_k[t] - m_k) / L0: two passes over the waveform (65 numbers per clip), never over the [L0, C] output,
// and no difference of large numbers anywhere.  Both passes accumulate in fp64, a thread over frames tid, tid + 256, ... and
// then lanes (xor shuffles 32 .. 1) and waves (0 .. 3) in a fixed order: the same bits from run to run and for a clip whatever
// its batch mates.  The main kernel never sees the mean: it convolves the centred samples x[5 t + j] - fl(m_j), which is an
// exact fp32 subtraction for a clip riding on a DC offset, and the offset left by rounding m_j to fp32, sum_j w[c, j]
// (m_j - fl(m_j)), is folded in fp64 into the per-channel affine pair the statistics kernel leaves in the workspace:
//   a_c = rstd_c gamma_c,   b_c = beta_c - a_c * sum_j w[c, j] (m_j - fl(m_j)),   n = a_c z + b_c.
// Workspace per clip: fl(m_0 .. m_9), 6 floats of padding, a[C], b[C].
//
// Main kernel (wave_stem_kernel).  A block owns FT = 64 frames of one clip: their 330 centred samples go to LDS as [frame][10]
// (5 broadcast 8-byte reads per frame), a thread owns two adjacent channels with their 20 taps in registers, and a frame's
// row leaves as one contiguous 1 KB (16-bit) or 2 KB (fp32) line per block instruction.  Rows t >= L0 are zeros.  Memory-bound
// on the output by design: 10 FMAs and one GELU per element.
#include "l2s_common.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int KW = 10, STRIDE = 5, NMOM = KW * (KW + 1) / 2;
constexpr int WS_HEAD = 16;                              // floats in front of a[C], b[C]
constexpr int FT = 64;

__host__ __device__ inline int stem_frames(int n) { return n >= KW ? (n - KW) / STRIDE + 1 : 0; }

template <bool I16>
__device__ __forceinline__ float load_sample(const void* wav, int64_t i) {
  if (I16) return (float)((const int16_t*)wav)[i] * (1.0f / 32768.0f);
  return ((const float*)wav)[i];
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool I16>
__global__ __launch_bounds__(256) void wave_stem_stats_kernel(const void* __restrict__ wav, const int64_t ldw,
                                                              const int32_t* __restrict__ n_samples, const int S,
                                                              const float* __restrict__ w, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float eps, const int C,
                                                              float* __restrict__ work) {
  __shared__ double sPart[4][NMOM];
  __shared__ double sMean[KW];
  __shared__ double sCov[NMOM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  int n = n_samples ? n_samples[b] : S;
  n = n < S ? n : S;
  const int L0 = stem_frames(n);
  float* __restrict__ ws = work + (int64_t)b * (WS_HEAD + 2 * C);
  const int64_t base = (int64_t)b * ldw;

  // ---- pass 1: the ten strided means
  double acc[NMOM];
#pragma unroll
  for (int j = 0; j < KW; ++j) acc[j] = 0.0;
  for (int t = tid; t < L0; t += 256) {
#pragma unroll
    for (int j = 0; j < KW; ++j) acc[j] += (double)load_sample<I16>(wav, base + (int64_t)t * STRIDE + j);
  }
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const double s = wave_sum_f64(acc[j]);
    if (lane == 0) sPart[wave][j] = s;
  }
  __syncthreads();
  if (tid < KW) {
    const double s = ((sPart[0][tid] + sPart[1][tid]) + sPart[2][tid]) + sPart[3][tid];
    sMean[tid] = L0 > 0 ? s / (double)L0 : 0.0;
  }
  __syncthreads();
  double m[KW];
#pragma unroll
  for (int j = 0; j < KW; ++j) m[j] = sMean[j];

  // ---- pass 2: the 55 centred second moments (j <= k)
#pragma unroll
  for (int q = 0; q < NMOM; ++q) acc[q] = 0.0;
  for (int t = tid; t < L0; t += 256) {
    double d[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) d[j] = (double)load_sample<I16>(wav, base + (int64_t)t * STRIDE + j) - m[j];
    int q = 0;
#pragma unroll
    for (int j = 0; j < KW; ++j)
#pragma unroll
      for (int k = j; k < KW; ++k) acc[q++] += d[j] * d[k];
  }
#pragma unroll
  for (int q = 0; q < NMOM; ++q) {
    const double s = wave_sum_f64(acc[q]);
    if (lane == 0) sPart[wave][q] = s;
  }
  __syncthreads();
  if (tid < NMOM) {
    const double s = ((sPart[0][tid] + sPart[1][tid]) + sPart[2][tid]) + sPart[3][tid];
    sCov[tid] = L0 > 0 ? s / (double)L0 : 0.0;
  }
  __syncthreads();

  // ---- per channel: var = w^T Cov w, the affine pair of the main kernel
  if (tid < KW) ws[tid] = (float)m[tid];
  for (int c = tid; c < C; c += 256) {
    double wc[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) wc[j] = (double)w[c * KW + j];
    double var = 0.0, shift = 0.0;
    int q = 0;
#pragma unroll
    for (int j = 0; j < KW; ++j) {
      shift += wc[j] * (m[j] - (double)(float)m[j]);
#pragma unroll
      for (int k = j; k < KW; ++k) {
        const double term = wc[j] * wc[k] * sCov[q++];
        var += k == j ? term : 2.0 * term;
      }
    }
    var = var > 0.0 ? var : 0.0;
    const double a = (double)gamma[c] / sqrt(var + (double)eps);
    ws[WS_HEAD + c] = (float)a;
    ws[WS_HEAD + C + c] = (float)((double)beta[c] - a * shift);   // y - mean = z - shift
  }
}

struct OutF32 {};

template <typename OT>
__device__ __forceinline__ void store2(void* out, int64_t idx, float v0, float v1) {
  if constexpr (std::is_same<OT, OutF32>::value) {
    *reinterpret_cast<float2*>((float*)out + idx) = make_float2(v0, v1);
  } else {
    *reinterpret_cast<uint32_t*>((uint16_t*)out + idx) = OT::pack2(v0, v1);
  }
}

template <typename OT>
__device__ __forceinline__ float stem_gelu(float v) {
  if constexpr (std::is_same<OT, OutF32>::value) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
  else return l2s_gelu(v);
}

template <typename OT, bool I16>
__global__ __launch_bounds__(256) void wave_stem_kernel(const void* __restrict__ wav, const int64_t ldw,
                                                        const int32_t* __restrict__ n_samples, const int S,
                                                        const float* __restrict__ w, const float* __restrict__ work,
                                                        void* __restrict__ out, const int ldo, const int T_rows, const int C) {
  __shared__ __attribute__((aligned(8))) float sX[FT * KW];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, f0 = blockIdx.x * FT;
  int n = n_samples ? n_samples[b] : S;
  n = n < S ? n : S;
  const int L0 = stem_frames(n);
  const int rows = min(FT, T_rows - f0);                 // >= 1 by the grid
  const int live = min(max(L0 - f0, 0), rows);           // rows of this tile that carry frames
  const float* __restrict__ ws = work + (int64_t)b * (WS_HEAD + 2 * C);
  const int64_t orow0 = (int64_t)b * T_rows + f0;

  // frame f, tap j -> sample 5 (f0 + f) + j < 5 (L0 - 1) + 10 <= n for every live frame
  for (int e = tid; e < live * KW; e += 256) {
    const int f = e / KW, j = e - f * KW;
    sX[e] = load_sample<I16>(wav, (int64_t)b * ldw + (int64_t)(f0 + f) * STRIDE + j) - ws[j];
  }
  __syncthreads();

  for (int c = 2 * tid; c < C; c += 512) {
    float w0[KW], w1[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j) { w0[j] = w[c * KW + j]; w1[j] = w[(c + 1) * KW + j]; }
    const float a0 = ws[WS_HEAD + c], a1 = ws[WS_HEAD + c + 1];
    const float b0 = ws[WS_HEAD + C + c], b1 = ws[WS_HEAD + C + c + 1];
    for (int f = 0; f < live; ++f) {
      float z0 = 0.f, z1 = 0.f;
#pragma unroll
      for (int j = 0; j < KW; j += 2) {
        const float2 x = *reinterpret_cast<const float2*>(&sX[f * KW + j]);
        z0 = fmaf(w0[j], x.x, z0); z1 = fmaf(w1[j], x.x, z1);
        z0 = fmaf(w0[j + 1], x.y, z0); z1 = fmaf(w1[j + 1], x.y, z1);
      }
      store2<OT>(out, (orow0 + f) * ldo + c, stem_gelu<OT>(fmaf(a0, z0, b0)), stem_gelu<OT>(fmaf(a1, z1, b1)));
    }
    for (int f = live; f < rows; ++f) store2<OT>(out, (orow0 + f) * ldo + c, 0.f, 0.f);
  }
}

template <typename OT>
int launch_stem(const void* wav, int i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* w, const float* gamma,
                const float* beta, float eps, float* work, void* out, int ldo, int T_rows, int C, hipStream_t st) {
  dim3 grid((unsigned)((T_rows + FT - 1) / FT), (unsigned)B), blk(256);
  if (i16) {
    hipLaunchKernelGGL(wave_stem_stats_kernel<true>, dim3(B), blk, 0, st, wav, ldw, n_samples, S, w, gamma, beta, eps, C, work);
    hipLaunchKernelGGL((wave_stem_kernel<OT, true>), grid, blk, 0, st, wav, ldw, n_samples, S, w, work, out, ldo, T_rows, C);
  } else {
    hipLaunchKernelGGL(wave_stem_stats_kernel<false>, dim3(B), blk, 0, st, wav, ldw, n_samples, S, w, gamma, beta, eps, C, work);
    hipLaunchKernelGGL((wave_stem_kernel<OT, false>), grid, blk, 0, st, wav, ldw, n_samples, S, w, work, out, ldo, T_rows, C);
  }
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

}  // namespace

extern "C" size_t l2s_wave_stem_workspace(int B, int C) {
  if (B <= 0 || C <= 0) return 0;
  return (size_t)B * (size_t)(WS_HEAD + 2 * C) * sizeof(float);
}

extern "C" int l2s_wave_stem(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* w,
                             const float* gamma, const float* beta, float eps, void* out, int ldo, int T_rows, int C,
                             void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  if (!wav || !w || !gamma || !beta || !out || !workspace) return L2S_EINVAL;
  if (dtype != L2S_F16 && dtype != L2S_BF16 && dtype != L2S_F32) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || T_rows <= 0 || C <= 0) return L2S_ESHAPE;
  if (ldw < S || ldo < C) return L2S_ESHAPE;
  if (T_rows < stem_frames(S)) return L2S_ESHAPE;        // a clip of S samples would have rows that do not exist
  if (C != 512) return L2S_EUNSUPPORTED;
  if (B > 65535 || S >= (1 << 30)) return L2S_EUNSUPPORTED;   // grid.y; 32-bit sample positions
  if (workspace_bytes < l2s_wave_stem_workspace(B, C)) return L2S_ESHAPE;
  const int osz = dtype == L2S_F32 ? 4 : 2;
  if (((uintptr_t)wav & (wav_is_i16 ? 1 : 3)) || ((uintptr_t)w & 3) || ((uintptr_t)gamma & 3) || ((uintptr_t)beta & 3) ||
      ((uintptr_t)workspace & 3) || ((uintptr_t)out & (2 * osz - 1)) || (ldo & 1))
    return L2S_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  float* work = (float*)workspace;
  if (dtype == L2S_F16) return launch_stem<ElemF16>(wav, wav_is_i16, ldw, n_samples, B, S, w, gamma, beta, eps, work, out, ldo, T_rows, C, st);
  if (dtype == L2S_BF16) return launch_stem<ElemBF16>(wav, wav_is_i16, ldw, n_samples, B, S, w, gamma, beta, eps, work, out, ldo, T_rows, C, st);
  return launch_stem<OutF32>(wav, wav_is_i16, ldw, n_samples, B, S, w, gamma, beta, eps, work, out, ldo, T_rows, C, st);
}
