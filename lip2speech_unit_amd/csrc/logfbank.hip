// Log filterbank features of 16 kHz waveforms in one launch (l2s_logfbank): the audio rows AV-HuBERT's audio sub-model reads -
// python_speech_features.logfbank(wav, samplerate=16000) with that library's defaults, then the stacker, the alignment to the
// video's frame count and the F.layer_norm of avhubert/hubert_dataset.py:299-315,370-372 - restated in fp32:
//
//   y[0] = x[0], y[p] = x[p] - rn(0.97 x[p-1])       pre-emphasis over the whole clip, samples at int16 scale, before framing
//   frame t = y[160 t .. 160 t + 400), zeros past the clip; n_frames = 1 if n <= 400 else 1 + ceil((n - 400) / 160); no window
//   pspec[k] = (fma(im, im, rn(re re))) / 512         512-point DFT of the 400 samples, bins 0 .. 255 (bin 256 has weight 0 in every band)
//   e[j] = sum_k fb[j][k] pspec[k] (k ascending over fb_range[j]);  feat[j] = e[j] == 0 ? float(log(2.220446049250313e-16)) : logf(e[j])
//   row r = frames stack r .. stack r + stack - 1 side by side (26 stack columns), frames at or past n_frames are 0.0 (padded AFTER the log)
//   rows at or past min(ceil(n_frames / stack), n_rows[b]) are zeros; with `normalize` every row is (x - mean) / sqrt(var + 1e-5), biased
//   variance, two passes in fp32 with the mean taken about the row's first value (an all-zero row stays zero, a constant row becomes zero)
//
//   frame  hop  frames/block FT  span samples  span rows x stride  basis pass PN  K-tile BK  passes  LDS per block
//    400   160       64             10 480        66 x 161            128 cols       16        4      59 400 B
//
// Tile, span layout, basis streaming and the barriers are frame_dft.h's (FrameDftTile<400, 160, 64, 512>); the span is filled here
// because of the pre-emphasis (a tile needs one sample before its first) and the zero tail.  A tile of 64 frames is 64 / stack whole
// stacked rows, so the stacking and the row norm happen on the LDS result tile (laid over the span, which is dead by then) and only
// the final rows reach HBM.  Every clip is analysed alone: its bits do not depend on its batch mates or on the padded length S.
#include "frame_dft.h"
#include <math.h>

namespace {

using namespace frame_dft;

constexpr int NFILT = 26, NBIN = 257, BPG = 7;           // bands; columns of a filterbank row (n_dft / 2 + 1); bands per wave (7 7 7 5)
constexpr float LOG_EPS = -36.04365338911715f;          // log(2.220446049250313e-16), numpy.finfo(float).eps: the library's stand-in for a zero band energy

using Tile = FrameDftTile<400, 160, 64, 512>;

__device__ __forceinline__ float preemph(float x, float xp) {
#pragma clang fp contract(off)
  return x - 0.97f * xp;
}

__device__ __forceinline__ int lfb_frames(int n) { return n <= 0 ? 0 : (n <= Tile::K ? 1 : 1 + (n - Tile::K + Tile::HOP - 1) / Tile::HOP); }

template <class ET, bool F32>
__device__ __forceinline__ void store_rows(void* __restrict__ out_, const float* sO, int64_t row0, int ldo, int rows, int C) {
  for (int e = threadIdx.x; e < rows * C; e += 256) {
    const int r = e / C;
    const int64_t o = (row0 + r) * ldo + (e - r * C);
    if constexpr (F32) ((float*)out_)[o] = sO ? sO[e] : 0.f;
    else ((uint16_t*)out_)[o] = sO ? ET::from_f32(sO[e]) : (uint16_t)0;
  }
}

__device__ __forceinline__ void store_tile(void* __restrict__ out, int out_dtype, const float* sO, int64_t row0, int ldo, int rows, int C) {
  if (out_dtype == L2S_F32) store_rows<ElemF16, true>(out, sO, row0, ldo, rows, C);
  else if (out_dtype == L2S_F16) store_rows<ElemF16, false>(out, sO, row0, ldo, rows, C);
  else store_rows<ElemBF16, false>(out, sO, row0, ldo, rows, C);
}

template <bool I16, int STACK>
__global__ __launch_bounds__(256, 2) void logfbank_kernel(const void* __restrict__ wav_, const int64_t ldw, const int32_t* __restrict__ n_samples,
                                                          const int S, const float* __restrict__ basis, const float* __restrict__ fb,
                                                          const int32_t* __restrict__ fb_range, const int32_t* __restrict__ n_rows,
                                                          void* __restrict__ out, const int out_dtype, const int ldo, const int T_rows,
                                                          const int normalize) {
  using Tl = Tile;
  constexpr int HOP = Tl::HOP, FT = Tl::FT, NBP = Tl::NBP, LDR = Tl::LDR;
  constexpr int RT = FT / STACK, C = NFILT * STACK;      // stacked rows of a tile; their width
  static_assert(FT % STACK == 0 && C <= 128 && 4 * BPG >= NFILT, "tile shape");
  static_assert(FT * NFILT <= Tl::SX, "the output tile reuses the span");
  __shared__ float sX[Tl::SX];
  __shared__ __attribute__((aligned(16))) float sB[Tl::SB];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, r0 = blockIdx.x * RT, f0 = blockIdx.x * FT;
  const int n = clip_len(n_samples, b, S);
  const int nf = lfb_frames(n);
  const int arows = (nf + STACK - 1) / STACK;            // the audio's own rows
  const int keep = n_rows ? min(arows, n_rows[b]) : arows;   // rows that carry features; everything past them is zeros
  const int rows = min(RT, T_rows - r0);                 // rows of this tile that exist in the output (>= 1 by the grid)
  const int64_t row0 = (int64_t)b * T_rows + r0;
  if (r0 >= keep) {                                      // block-uniform: a tile wholly past the clip's rows
    store_tile(out, out_dtype, nullptr, row0, ldo, rows, C);
    return;
  }
  // ---- the span: pre-emphasised samples f0 HOP .. of the clip, zeros at and past n
  for (int s = tid; s < Tl::SROWS * HOP; s += 256) {
    const int p = f0 * HOP + s;
    float v = 0.f;
    if (s < Tl::SPAN && p < n) {
      const int64_t i = (int64_t)b * ldw + p;
      float x, xp = 0.f;
      if (I16) {
        x = (float)((const int16_t*)wav_)[i];
        if (p > 0) xp = (float)((const int16_t*)wav_)[i - 1];
      } else {
        x = ((const float*)wav_)[i];
        if (p > 0) xp = ((const float*)wav_)[i - 1];
      }
      v = p > 0 ? preemph(x, xp) : x;
    }
    const int r = s / HOP;
    sX[r * Tl::SLD + (s - r * HOP)] = v;
  }

  const int mf = tid % FT;                               // the frame whose band sums this thread keeps; its bands: BPG wave ..
  float m[BPG];
#pragma unroll
  for (int j = 0; j < BPG; ++j) m[j] = 0.f;

  pass_loop<Tl>(
      sX, sB, basis,
      [&](int pass, int e, float re, float im) { return power(re, im) * (1.0f / 512.0f); },
      [&](int pass, const float* sG) {                   // the power spectrum's bins NBP pass .. into the band sums, bins ascending
        const int c0 = pass * NBP;
#pragma unroll
        for (int j = 0; j < BPG; ++j) {
          const int band = wave * BPG + j;
          if (band < NFILT) {
            const int lo = max(fb_range[2 * band], c0), hi = min(min(fb_range[2 * band + 1], c0 + NBP), NBIN - 1);
            const float* w = fb + band * NBIN;
            for (int k = lo; k < hi; ++k) m[j] = fmaf(w[k], sG[mf * LDR + (k - c0)], m[j]);
          }
        }
      });

  // ---- log, the 0.0 of frames past the clip's last; frame mf's bands are columns NFILT (mf % STACK) .. of row mf / STACK
  float* sO = sX;
#pragma unroll
  for (int j = 0; j < BPG; ++j) {
    const int band = wave * BPG + j;
    if (band < NFILT) {
      const float v = m[j] == 0.f ? LOG_EPS : logf(m[j]);
      sO[mf * NFILT + band] = f0 + mf < nf ? v : 0.f;
    }
  }
  __syncthreads();
  // ---- rows at or past `keep` are zeros; the row norm, a wave per row, two passes
  for (int r = wave; r < RT; r += 4) {
    const bool live = r0 + r < keep;                     // wave-uniform
    const float x0 = lane < C ? sO[r * C + lane] : 0.f, x1 = lane + 64 < C ? sO[r * C + lane + 64] : 0.f;
    float y0 = live ? x0 : 0.f, y1 = live ? x1 : 0.f;
    if (live && normalize) {
      // the mean as x[0] + mean(x - x[0]): a constant row (digital silence) has deviations of exactly 0, whatever C is
      const float xf = sO[r * C];
      const float mean = xf + wave_sum((lane < C ? x0 - xf : 0.f) + (lane + 64 < C ? x1 - xf : 0.f)) * (1.0f / C);
      const float d0 = lane < C ? x0 - mean : 0.f, d1 = lane + 64 < C ? x1 - mean : 0.f;
      const float var = wave_sum(fmaf(d0, d0, d1 * d1)) * (1.0f / C);
      const float rstd = 1.0f / sqrtf(var + 1e-5f);
      y0 = d0 * rstd;
      y1 = d1 * rstd;
    }
    if (lane < C) sO[r * C + lane] = y0;
    if (lane + 64 < C) sO[r * C + lane + 64] = y1;
  }
  __syncthreads();
  store_tile(out, out_dtype, sO, row0, ldo, rows, C);
}

template <bool I16, int STACK>
void launch(const void* wav, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis, const float* fb, const int32_t* fb_range,
            const int32_t* n_rows, void* out, int out_dtype, int ldo, int T_rows, int normalize, hipStream_t st) {
  constexpr int RT = Tile::FT / STACK;
  dim3 grid((unsigned)((T_rows + RT - 1) / RT), (unsigned)B), blk(256);
  hipLaunchKernelGGL((logfbank_kernel<I16, STACK>), grid, blk, 0, st, wav, ldw, n_samples, S, basis, fb, fb_range, n_rows, out, out_dtype, ldo,
                     T_rows, normalize);
}

}  // namespace

extern "C" int l2s_logfbank(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                            const float* fb, const int32_t* fb_range, const int32_t* n_rows, void* out, int out_dtype, int ldo, int T_rows,
                            int stack, int normalize, void* stream) {
  if (!wav || !basis || !fb || !fb_range || !out) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || T_rows <= 0 || stack <= 0) return L2S_ESHAPE;
  if (ldw < S || ldo < (int64_t)NFILT * stack) return L2S_ESHAPE;
  if (stack != 1 && stack != 4) return L2S_EUNSUPPORTED;
  if (out_dtype != L2S_F16 && out_dtype != L2S_BF16 && out_dtype != L2S_F32) return L2S_EUNSUPPORTED;
  if (B > 65535 || S >= (1 << 30) || T_rows > (1 << 22) / stack) return L2S_EUNSUPPORTED;   // grid.y; 32-bit sample positions
  if ((uintptr_t)basis & 15) return L2S_EALIGN;
  if (((uintptr_t)wav & (wav_is_i16 ? 1 : 3)) || ((uintptr_t)out & (out_dtype == L2S_F32 ? 3 : 1)) || ((uintptr_t)fb & 3) ||
      ((uintptr_t)fb_range & 3) || ((uintptr_t)n_samples & 3) || ((uintptr_t)n_rows & 3))
    return L2S_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (stack == 4) {
    if (wav_is_i16) launch<true, 4>(wav, ldw, n_samples, B, S, basis, fb, fb_range, n_rows, out, out_dtype, ldo, T_rows, normalize, st);
    else launch<false, 4>(wav, ldw, n_samples, B, S, basis, fb, fb_range, n_rows, out, out_dtype, ldo, T_rows, normalize, st);
  } else {
    if (wav_is_i16) launch<true, 1>(wav, ldw, n_samples, B, S, basis, fb, fb_range, n_rows, out, out_dtype, ldo, T_rows, normalize, st);
    else launch<false, 1>(wav, ldw, n_samples, B, S, basis, fb, fb_range, n_rows, out, out_dtype, ldo, T_rows, normalize, st);
  }
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
