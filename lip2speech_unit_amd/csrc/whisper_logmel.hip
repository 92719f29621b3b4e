// Whisper's log-mel front end (l2s_whisper_logmel): what transformers' WhisperFeatureExtractor and
// openai-whisper's log_mel_spectrogram compute on the host, as two launches.
//
//   1. spectrum: the clip is zero-extended to 480 000 samples; frame t = samples [160 t - 200, 160 t + 200) for t = 0 .. 2999 (the
//      3 001st frame of the centred STFT is dropped), reflected against the 480 000-sample buffer.  The tile is l2s_stft_mel_power's
//      (csrc/spkemb.hip): a block of 4 waves owns 32 frames, stages their span through frame_dft.h's stage_span (analysis length
//      480 000, real samples n_samples[b]: positions past them are zeros and are not read), multiplies by the [400, 448] windowed-DFT
//      table on v_mfma_f32_32x32x2_f32 (k-ordered fp32 fma chains) and folds re^2 + im^2 into 80 Slaney bands, bins ascending.
//      log10(max(., 1e-10)) goes to an fp32 workspace [B, 3000, 80]; each block also writes the maximum of its 32 x 80 values.
//   2. finish: a clip's maximum = the maximum of its 94 tile maxima (a maximum is exact in any order; no floating-point atomics),
//      then max(x, clip_max - 8), (x + 4) / 4 and one rounding to the 16-bit type, written time-major as rows [B * 3000, ld] with
//      zeros in columns 80 .. ld - 1: conv1's tap-GEMM operand.
#include "frame_dft.h"
#include <math.h>

namespace {

using frame_dft::f32x16_t;
using Span = frame_dft::FrameSpan<400, 160, 32>;
constexpr int NFFT = Span::K, HOP = Span::HOP, FT = Span::FT, SLD = Span::SLD, NMEL = 80, NBIN = NFFT / 2 + 1;
constexpr int NSAMP = 480000, NFRAME = 3000, PAD = 200, NTILE = (NFRAME + FT - 1) / FT;
constexpr int NPAIR = 7, NCOL = 64 * NPAIR;              // 7 tile pairs = bins 0 .. 223
constexpr int LDG = 32 * NPAIR + 1;                      // power tile [FT][225]
constexpr int KC = 16;                                   // k per chunk: 8 MFMA steps whose table loads are issued together
static_assert(NFFT % KC == 0 && (Span::SX + FT * LDG) * 4 <= 64 * 1024, "tile shape / static LDS");

template <bool I16>
__global__ __launch_bounds__(256) void whisper_spectrum_kernel(const void* __restrict__ wav_, const int64_t ldw,
                                                               const int32_t* __restrict__ n_samples, const int S,
                                                               const float* __restrict__ basis, const float* __restrict__ fb,
                                                               const int32_t* __restrict__ fb_range, float* __restrict__ logspec,
                                                               float* __restrict__ tile_max) {
  __shared__ float sX[Span::SX];
  __shared__ float sG[FT * LDG];
  __shared__ float sMax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, f0 = blockIdx.x * FT;
  const int nv = max(0, min(n_samples ? n_samples[b] : S, S));     // the real samples; the analysis length is always NSAMP
  const int rows = min(FT, NFRAME - f0);
  frame_dft::stage_span<Span, I16>(sX, wav_, ldw, b, f0 * HOP - PAD, NSAMP, nv, nullptr);
  __syncthreads();

  const int lr = lane & 31, lh = lane >> 5;
  const bool two = wave + 4 < NPAIR;                     // wave-uniform: waves 0 .. 2 own a second tile pair
  const float* b0 = basis + 64 * wave + lr;
  const float* b1 = basis + 64 * (two ? wave + 4 : wave) + lr;
  f32x16_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[q][e] = 0.f;
  for (int k0 = 0; k0 < NFFT; k0 += KC) {
    float w[KC / 2][4];
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const int k = k0 + 2 * s + lh;
      w[s][0] = b0[k * NCOL];
      w[s][1] = b0[k * NCOL + 32];
      if (two) {
        w[s][2] = b1[k * NCOL];
        w[s][3] = b1[k * NCOL + 32];
      }
    }
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const int k = k0 + 2 * s + lh;
      const int q = k / HOP;
      const float a = sX[(lr + q) * SLD + (k - q * HOP)];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w[s][0], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w[s][1], acc[1], 0, 0, 0);
      if (two) {
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w[s][2], acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w[s][3], acc[3], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int fr = 8 * (e >> 2) + 4 * lh + (e & 3);
    sG[fr * LDG + 32 * wave + lr] = __fadd_rn(__fmul_rn(acc[0][e], acc[0][e]), __fmul_rn(acc[1][e], acc[1][e]));
    if (two) sG[fr * LDG + 32 * (wave + 4) + lr] = __fadd_rn(__fmul_rn(acc[2][e], acc[2][e]), __fmul_rn(acc[3][e], acc[3][e]));
  }
  __syncthreads();

  const int mf = tid & (FT - 1), mg = tid / FT;          // frame, band group (10 bands each)
  float mx = -INFINITY;
  if (mf < rows) {
    float* __restrict__ out = logspec + ((int64_t)b * NFRAME + f0 + mf) * NMEL;
#pragma unroll
    for (int j = 0; j < NMEL / 8; ++j) {
      const int band = mg * (NMEL / 8) + j;
      const int lo = max(fb_range[2 * band], 0), hi = min(fb_range[2 * band + 1], NBIN);
      const float* w = fb + band * NBIN;
      float m = 0.f;
      for (int k = lo; k < hi; ++k) m = fmaf(w[k], sG[mf * LDG + k], m);
      const float v = log10f(fmaxf(m, 1e-10f));
      out[band] = v;
      mx = fmaxf(mx, v);
    }
  }
  mx = wave_max(mx);
  if (lane == 0) sMax[wave] = mx;
  __syncthreads();
  if (tid == 0) tile_max[(int64_t)b * NTILE + blockIdx.x] = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
}

template <typename E>
__global__ __launch_bounds__(256) void whisper_logmel_finish_kernel(const float* __restrict__ logspec, const float* __restrict__ tile_max,
                                                                    uint16_t* __restrict__ out16, const int ld, float* __restrict__ out32) {
  __shared__ float sMax[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y;
  {
    const float* tm = tile_max + (int64_t)b * NTILE;
    float m = -INFINITY;
    for (int t = tid; t < NTILE; t += 256) m = fmaxf(m, tm[t]);
    m = wave_max(m);
    if (lane == 0) sMax[wave] = m;
    __syncthreads();
  }
  const float floor_v = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3])) - 8.0f;
  const int per = ld >> 3;                               // 8-channel chunks of an output row
  const int e = blockIdx.x * 256 + tid;
  if (e >= NFRAME * per) return;
  const int r = e / per, c = (e - r * per) * 8;
  const int64_t row = (int64_t)b * NFRAME + r;
  uint4 o = make_uint4(0, 0, 0, 0);
  if (c < NMEL) {
    const float4 v0 = *reinterpret_cast<const float4*>(logspec + row * NMEL + c), v1 = *reinterpret_cast<const float4*>(logspec + row * NMEL + c + 4);
    float y[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) y[i] = (fmaxf(y[i], floor_v) + 4.0f) * 0.25f;
    if (out32) {
      *reinterpret_cast<float4*>(out32 + row * NMEL + c) = make_float4(y[0], y[1], y[2], y[3]);
      *reinterpret_cast<float4*>(out32 + row * NMEL + c + 4) = make_float4(y[4], y[5], y[6], y[7]);
    }
    o.x = E::pack2(y[0], y[1]); o.y = E::pack2(y[2], y[3]); o.z = E::pack2(y[4], y[5]); o.w = E::pack2(y[6], y[7]);
  }
  *reinterpret_cast<uint4*>(out16 + row * ld + c) = o;
}

}  // namespace

extern "C" size_t l2s_whisper_logmel_workspace(int B) {
  if (B <= 0 || B > 65535) return 0;
  return ((size_t)B * NFRAME * NMEL + (size_t)B * NTILE) * 4;
}

extern "C" int l2s_whisper_logmel(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                                  const float* fb, const int32_t* fb_range, void* workspace, void* out, int ld, float* out_f32, int dtype,
                                  void* stream) {
  if (!wav || !basis || !fb || !fb_range || !workspace || !out) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || ldw < S || ld < NMEL) return L2S_ESHAPE;
  if (S > NSAMP || B > 65535) return L2S_EUNSUPPORTED;          // one 30-second window
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if ((ld & 7) || ((uintptr_t)wav & (wav_is_i16 ? 1 : 3)) || ((uintptr_t)basis & 3) || ((uintptr_t)fb & 3) || ((uintptr_t)fb_range & 3) ||
      ((uintptr_t)n_samples & 3) || ((uintptr_t)workspace & 15) || ((uintptr_t)out & 15) || ((uintptr_t)out_f32 & 15))
    return L2S_EALIGN;
  float* logspec = (float*)workspace;
  float* tile_max = logspec + (size_t)B * NFRAME * NMEL;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(NTILE, (unsigned)B), blk(256);
  if (wav_is_i16) hipLaunchKernelGGL(whisper_spectrum_kernel<true>, grid, blk, 0, s, wav, ldw, n_samples, S, basis, fb, fb_range, logspec, tile_max);
  else hipLaunchKernelGGL(whisper_spectrum_kernel<false>, grid, blk, 0, s, wav, ldw, n_samples, S, basis, fb, fb_range, logspec, tile_max);
  L2S_CHECK_LAUNCH();
  const dim3 grid2((unsigned)((NFRAME * (ld >> 3) + 255) / 256), (unsigned)B);
  if (dtype == L2S_F16) hipLaunchKernelGGL(whisper_logmel_finish_kernel<ElemF16>, grid2, blk, 0, s, logspec, tile_max, (uint16_t*)out, ld, out_f32);
  else hipLaunchKernelGGL(whisper_logmel_finish_kernel<ElemBF16>, grid2, blk, 0, s, logspec, tile_max, (uint16_t*)out, ld, out_f32);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
