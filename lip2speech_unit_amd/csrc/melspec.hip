// Log-mel analysis of waveforms in one launch (l2s_stft_mel, and l2s_mel_spectrogram as its 640 / 160 / pad 320 / eps 0 case):
// the TacotronSTFT recipe of the vocoder's conditioning and the HiFi-GAN mel_spectrogram of the vocoder's validation loss
//
//   frame t of clip b = samples [t*hop - pad, t*hop - pad + n_fft) of the clip, reflect-padded against the clip's OWN length
//   re/im[k] = sum_n x[n] * basis,   mag = sqrtf((re^2 + im^2) + mag_eps),   m[j] = sum_k fb[j,k] * mag[k],   out = logf(max(m, floor))
//
// as a dense windowed DFT on the f32-input matrix instruction v_mfma_f32_32x32x2_f32: every re / im is a k-ordered fp32 fma
// chain over the n_fft samples of the frame, which is the arithmetic of the F.conv1d with a dense Fourier basis that TacotronSTFT
// itself runs - not an approximation of it.  One kernel template over the sizes (the tables are data):
//
//   n_fft  hop  frames/block FT  span samples  span rows x stride  basis pass PN  K-tile BK  passes  LDS per block
//    640   160       64             10 720        67 x 161            128 cols       16        5      60 304 B
//   1024   256       32              8 960        35 x 257            256 cols        8        4      52 752 B
//
// Tile.  A block (4 waves) owns FT consecutive frames of one clip.  It stages the tile's contiguous sample span,
// (FT - 1) * hop + n_fft samples, into LDS once, applying the reflection and the int16 -> fp32 conversion there; the
// frame matrix never exists in HBM.  The span is kept in hop-sized rows with a padded stride of hop + 1 floats: frame i,
// sample k sits at [(i + k / hop)][k % hop], so the 32 frames of an MFMA A fragment are hop + 1 floats apart (161 = 33 banks,
// 257 = 1 bank: odd, all distinct) instead of hop (160 = 32 mod 64: two banks; 256: one bank for all).  The n_fft x n_fft basis is
// walked in passes of PN columns; its K-tiles ([BK][PN] floats = 8 KB, contiguous rows of the table) stream global -> registers
// -> LDS double buffered under the MFMAs.  The four waves split the tile as FT / 32 frame halves x (PN / 64) column pairs: wave
// (fh, pp) owns frames 32 fh .. + 31 and the column pair pp: accumulator tile 0 is re, tile 1 is im of the same 32 bins, in the
// same lane and register, so the magnitude needs no cross-lane traffic.  Two blocks per CU give every SIMD four independent
// accumulator chains - the instruction's dependent latency equals its issue interval - and cover each other's barriers.
//
// After a pass's K loop the FT x PN/2 magnitudes go to LDS (over the idle basis buffers) and every thread folds them into the
// 80 * FT / 256 mel sums it keeps in registers (frame tid % FT, bands (80 FT / 256) (tid / FT) ..), bin by bin in ascending order
// over the band's non-zero range fb_range[j] (the filterbank's sparse triangular form; at FT = 64 a wave shares its bands and the
// weights come through the scalar cache).  Bin n_fft/2 lives in pass 0 and is added last.  Then clamp, logf, and the tile's rows
// leave through LDS as contiguous 320-byte rows.  The spectrum is never written to HBM.  Rows t >= T_b are zeros; tiles wholly
// past T_b skip the K loop.
#include "l2s_common.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int NMEL = 80;

template <int NFFT_, int HOP_, int FT_>
struct MelTile {
  static constexpr int NFFT = NFFT_, HOP = HOP_, FT = FT_, NBIN = NFFT / 2 + 1;
  static constexpr int SPAN = (FT - 1) * HOP + NFFT;                 // samples a tile's frames cover
  static constexpr int SROWS = SPAN / HOP, SLD = HOP + 1;            // the span as hop-sized rows, padded stride
  static constexpr int FH = FT / 32, NPP = 4 / FH;                   // waves = frame halves x column pairs
  static constexpr int PN = 64 * NPP, LDB = PN + 4;                  // basis columns per pass; K-tile row stride
  static constexpr int BK = 2048 / PN;                               // K-tile [BK][PN]: two float4 per thread
  static constexpr int KT_PASS = NFFT / BK, NPASS = NFFT / PN;
  static constexpr int NBP = PN / 2, LDG = NBP + 1;                  // bins per pass; magnitude tile [FT][NBP + 1]
  static constexpr int MG = 256 / FT, BPG = NMEL / MG;               // mel sums: thread groups per frame set, bands per group
  static_assert(SPAN % HOP == 0 && NFFT % PN == 0 && NFFT % BK == 0 && NMEL % MG == 0 && (FT == 32 || FT == 64), "tile shape");
  static_assert(FT * LDG <= 2 * BK * LDB, "the magnitude tile reuses the basis buffers");
  static_assert(FT * NMEL <= SROWS * SLD, "the output tile reuses the span");
  static_assert((SROWS * SLD + 2 * BK * LDB + FT) * 4 <= 64 * 1024, "static LDS");
};

template <class Tl, bool I16>
__global__ __launch_bounds__(256, 2) void melspec_kernel(const void* __restrict__ wav_, const int64_t ldw, const int32_t* __restrict__ n_samples,
                                                         const int S, const float* __restrict__ basis, const float* __restrict__ fb,
                                                         const int32_t* __restrict__ fb_range, float* __restrict__ mel, const int ldm,
                                                         const int T_rows, const float floor_, const int pad, const float mag_eps) {
  constexpr int NFFT = Tl::NFFT, HOP = Tl::HOP, FT = Tl::FT, NBIN = Tl::NBIN, SPAN = Tl::SPAN, SROWS = Tl::SROWS, SLD = Tl::SLD;
  constexpr int FH = Tl::FH, PN = Tl::PN, LDB = Tl::LDB, BK = Tl::BK, KT_PASS = Tl::KT_PASS, NPASS = Tl::NPASS, NBP = Tl::NBP;
  constexpr int LDG = Tl::LDG, BPG = Tl::BPG;
  __shared__ float sX[SROWS * SLD];
  __shared__ __attribute__((aligned(16))) float sB[2 * BK * LDB];
  __shared__ float sNyq[FT];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, f0 = blockIdx.x * FT;
  int n = n_samples ? n_samples[b] : S;
  n = n < S ? n : S;
  const int Tb = (n > pad && n + 2 * pad >= NFFT) ? (n + 2 * pad - NFFT) / HOP + 1 : 0;   // no valid reflect padding: no frames
  const int rows = min(FT, T_rows - f0);                 // rows of this tile that exist in the output (>= 1 by the grid)
  float* __restrict__ out = mel + ((int64_t)b * T_rows + f0) * ldm;
  if (f0 >= Tb) {                                        // block-uniform: a tile wholly past the clip's end
    for (int e = tid; e < rows * NMEL; e += 256) {
      const int r = e / NMEL;
      out[(int64_t)r * ldm + (e - r * NMEL)] = 0.f;
    }
    return;
  }

  // ---- stage the sample span: position p of the clip, reflected once at either end; frames past T_b may reach further and read 0
  {
    const int p0 = f0 * HOP - pad;
    for (int s = tid; s < SPAN; s += 256) {
      int p = p0 + s;
      p = p < 0 ? -p : p;
      p = p >= n ? 2 * (n - 1) - p : p;
      float v = 0.f;
      if ((unsigned)p < (unsigned)n) {
        if (I16) v = (float)((const int16_t*)wav_)[(int64_t)b * ldw + p] * (1.0f / 32768.0f);
        else v = ((const float*)wav_)[(int64_t)b * ldw + p];
      }
      const int r = s / HOP;
      sX[r * SLD + (s - r * HOP)] = v;
    }
  }

  // ---- basis fetch: thread -> rows tid / (PN/4) and that + BK/2 of the K-tile, columns 4 (tid % (PN/4)) .. + 3
  const int ld_k = tid / (PN / 4), ld_c = (tid % (PN / 4)) * 4;
  float4 rb0, rb1;
  auto fetch = [&](int t) {                              // t: flat K-tile index, pass = t / KT_PASS
    const int pass = t / KT_PASS, k0 = (t - pass * KT_PASS) * BK;
    const float* src = basis + (int64_t)(k0 + ld_k) * NFFT + pass * PN + ld_c;
    rb0 = *reinterpret_cast<const float4*>(src);
    rb1 = *reinterpret_cast<const float4*>(src + (BK / 2) * NFFT);
  };
  auto stage = [&](int buf) {
    *reinterpret_cast<float4*>(&sB[(buf * BK + ld_k) * LDB + ld_c]) = rb0;
    *reinterpret_cast<float4*>(&sB[(buf * BK + ld_k + BK / 2) * LDB + ld_c]) = rb1;
  };

  const int fh = wave % FH, pp = wave / FH;
  const int lr = lane & 31, lh = lane >> 5;
  const int arow = (32 * fh + lr) * SLD;
  const int mf = tid % FT;                               // the frame whose mel sums this thread keeps
  const int mg = FT == 64 ? wave : tid / FT;             // ... and its band group (wave-uniform at FT = 64)
  float m[BPG];
#pragma unroll
  for (int j = 0; j < BPG; ++j) m[j] = 0.f;
  f32x16_t acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }

  constexpr int NT = NPASS * KT_PASS;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int t = 0; t < NT; ++t) {
    const int buf = t & 1;
    const int pass = t / KT_PASS, kt = t - pass * KT_PASS;
    if (t + 1 < NT) fetch(t + 1);
    const float* bt = &sB[buf * BK * LDB + 64 * pp + lr];
#pragma unroll
    for (int s = 0; s < BK / 2; ++s) {
      const int k = kt * BK + 2 * s + lh;
      const int q = k / HOP;
      const float a = sX[arow + q * SLD + (k - q * HOP)];
      const float w0 = bt[(2 * s + lh) * LDB], w1 = bt[(2 * s + lh) * LDB + 32];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w1, acc[1], 0, 0, 0);
    }
    if (kt + 1 < KT_PASS) {
      stage(buf ^ 1);
      __syncthreads();
      continue;
    }
    // ---- end of a pass: magnitudes of bins NBP pass .. + NBP - 1 -> LDS -> the mel sums
    __syncthreads();                                     // every wave is done with the basis buffers
    float* sG = sB;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int fr = 32 * fh + 8 * (e >> 2) + 4 * lh + (e & 3);
      const float re = acc[0][e], im = acc[1][e];
      float g;
      if (pass == 0 && pp == 0 && lr == 0) {             // column 0 of the first pair: re[0] | re[n_fft/2], both real-only
        g = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), 0.f), mag_eps));
        sNyq[fr] = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(im, im), 0.f), mag_eps));
      } else {
        g = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), mag_eps));
      }
      sG[fr * LDG + 32 * pp + lr] = g;
      acc[0][e] = 0.f;
      acc[1][e] = 0.f;
    }
    __syncthreads();
    const int c0 = pass * NBP;
#pragma unroll
    for (int j = 0; j < BPG; ++j) {
      const int band = mg * BPG + j;
      const int lo = max(fb_range[2 * band], c0), hi = min(min(fb_range[2 * band + 1], c0 + NBP), NBIN - 1);
      const float* w = fb + band * NBIN;
      for (int k = lo; k < hi; ++k) m[j] = fmaf(w[k], sG[mf * LDG + (k - c0)], m[j]);
    }
    __syncthreads();                                     // the magnitude tile is read: the buffers go back to the basis
    if (t + 1 < NT) {
      stage(buf ^ 1);
      __syncthreads();
    }
  }

  // ---- bin n_fft/2, clamp, log; the tile's rows leave through LDS (over the span, which is dead now) as contiguous rows
  float* sO = sX;
#pragma unroll
  for (int j = 0; j < BPG; ++j) {
    const int band = mg * BPG + j;
    float v = m[j];
    if (fb_range[2 * band + 1] == NBIN) v = fmaf(fb[band * NBIN + NBIN - 1], sNyq[mf], v);
    v = logf(fmaxf(v, floor_));
    sO[mf * NMEL + band] = f0 + mf < Tb ? v : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < rows * NMEL; e += 256) {
    const int r = e / NMEL;
    out[(int64_t)r * ldm + (e - r * NMEL)] = sO[e];
  }
}

using Tile640 = MelTile<640, 160, 64>;
using Tile1024 = MelTile<1024, 256, 32>;

template <class Tl>
void launch(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis, const float* fb,
            const int32_t* fb_range, float* mel, int ldm, int T_rows, float floor_, int pad, float mag_eps, hipStream_t st) {
  dim3 grid((unsigned)((T_rows + Tl::FT - 1) / Tl::FT), (unsigned)B), blk(256);
  if (wav_is_i16)
    hipLaunchKernelGGL((melspec_kernel<Tl, true>), grid, blk, 0, st, wav, ldw, n_samples, S, basis, fb, fb_range, mel, ldm, T_rows, floor_, pad, mag_eps);
  else
    hipLaunchKernelGGL((melspec_kernel<Tl, false>), grid, blk, 0, st, wav, ldw, n_samples, S, basis, fb, fb_range, mel, ldm, T_rows, floor_, pad, mag_eps);
}

// the checks of both entries, in one order; wide: the sizes l2s_stft_mel serves beyond (640, 160)
int stft_mel(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis, const float* fb,
             const int32_t* fb_range, float* mel, int ldm, int T_rows, int n_fft, int hop, int n_mels, int pad, float mag_eps, float floor_,
             void* stream, bool wide) {
  if (!wav || !basis || !fb || !fb_range || !mel) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || T_rows <= 0 || n_fft <= 0 || hop <= 0 || n_mels <= 0) return L2S_ESHAPE;
  if (ldw < S || ldm < n_mels) return L2S_ESHAPE;
  const bool s640 = n_fft == 640 && hop == 160, s1024 = wide && n_fft == 1024 && hop == 256;
  if (!(s640 || s1024) || n_mels != NMEL) return L2S_EUNSUPPORTED;
  if (pad < 0 || pad > n_fft / 2 || !(mag_eps >= 0.f)) return L2S_EUNSUPPORTED;
  if (B > 65535 || S >= (1 << 30) || T_rows > (1 << 22)) return L2S_EUNSUPPORTED;   // grid.y; 32-bit sample positions
  if ((uintptr_t)basis & 15) return L2S_EALIGN;
  if (((uintptr_t)wav & (wav_is_i16 ? 1 : 3)) || ((uintptr_t)mel & 3) || ((uintptr_t)fb & 3) || ((uintptr_t)fb_range & 3)) return L2S_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (s640) launch<Tile640>(wav, wav_is_i16, ldw, n_samples, B, S, basis, fb, fb_range, mel, ldm, T_rows, floor_, pad, mag_eps, st);
  else launch<Tile1024>(wav, wav_is_i16, ldw, n_samples, B, S, basis, fb, fb_range, mel, ldm, T_rows, floor_, pad, mag_eps, st);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

}  // namespace

extern "C" int l2s_stft_mel(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                            const float* fb, const int32_t* fb_range, float* mel, int ldm, int T_rows, int n_fft, int hop, int n_mels,
                            int pad, float mag_eps, float floor_, void* stream) {
  return stft_mel(wav, wav_is_i16, ldw, n_samples, B, S, basis, fb, fb_range, mel, ldm, T_rows, n_fft, hop, n_mels, pad, mag_eps, floor_,
                  stream, true);
}

extern "C" int l2s_mel_spectrogram(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S,
                                   const float* basis, const float* fb, const int32_t* fb_range, float* mel, int ldm, int T_rows,
                                   int n_fft, int hop, int n_mels, float floor_, void* stream) {
  return stft_mel(wav, wav_is_i16, ldw, n_samples, B, S, basis, fb, fb_range, mel, ldm, T_rows, n_fft, hop, n_mels, n_fft / 2, 0.f, floor_,
                  stream, false);
}
