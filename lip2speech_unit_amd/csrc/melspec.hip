// Log-mel analysis of waveforms in one launch (l2s_stft_mel, and l2s_mel_spectrogram as its 640 / 160 / pad 320 / eps 0 case):
// the TacotronSTFT recipe of the vocoder's conditioning and the HiFi-GAN mel_spectrogram of the vocoder's validation loss
//
//   frame t of clip b = samples [t*hop - pad, t*hop - pad + n_fft) of the clip, reflect-padded against the clip's OWN length
//   re/im[k] = sum_n x[n] * basis,   mag = sqrtf(fma(im, im, rn(re re)) + mag_eps),   m[j] = sum_k fb[j,k] * mag[k],   out = logf(max(m, floor))
//
// as a dense windowed DFT on the f32-input matrix instruction v_mfma_f32_32x32x2_f32: every re / im is a k-ordered fp32 fma
// chain over the n_fft samples of the frame, which is the arithmetic of the F.conv1d with a dense Fourier basis that TacotronSTFT
// itself runs - not an approximation of it.  One kernel template over the sizes (the tables are data):
//
//   n_fft  hop  frames/block FT  span samples  span rows x stride  basis pass PN  K-tile BK  passes  LDS per block
//    640   160       64             10 720        67 x 161            128 cols       16        5      60 304 B
//   1024   256       32              8 960        35 x 257            256 cols        8        4      52 752 B
//
// Tile, span layout, basis streaming and the barriers are frame_dft.h's (FrameDftTile<n_fft, hop, FT, n_fft>); two blocks per CU give
// every SIMD four independent accumulator chains - the instruction's dependent latency equals its issue interval - and cover each
// other's barriers.  This file holds the epilogue: after a pass's K loop the FT x PN/2 magnitudes are in the result tile and every
// thread folds them into the 80 * FT / 256 mel sums it keeps in registers (frame tid % FT, bands (80 FT / 256) (tid / FT) ..), bin by
// bin in ascending order over the band's non-zero range fb_range[j] (the filterbank's sparse triangular form; at FT = 64 a wave
// shares its bands and the weights come through the scalar cache).  Bin n_fft/2 lives in pass 0 and is added last.  Then clamp,
// logf, and the tile's rows leave through LDS as contiguous 320-byte rows.  The spectrum is never written to HBM.  Rows t >= T_b
// are zeros; tiles wholly past T_b skip the K loop.
#include "frame_dft.h"
#include <math.h>

namespace {

using namespace frame_dft;

constexpr int NMEL = 80;

template <class Tl, bool I16>
__global__ __launch_bounds__(256, 2) void melspec_kernel(const void* __restrict__ wav_, const int64_t ldw, const int32_t* __restrict__ n_samples,
                                                         const int S, const float* __restrict__ basis, const float* __restrict__ fb,
                                                         const int32_t* __restrict__ fb_range, float* __restrict__ mel, const int ldm,
                                                         const int T_rows, const float floor_, const int pad, const float mag_eps) {
  constexpr int NFFT = Tl::K, HOP = Tl::HOP, FT = Tl::FT, NBIN = NFFT / 2 + 1, FH = Tl::FH, NBP = Tl::NBP, LDR = Tl::LDR;
  constexpr int MG = 256 / FT, BPG = NMEL / MG;          // mel sums: thread groups per frame set, bands per group
  static_assert(Tl::NCOL == NFFT && Tl::SPAN % HOP == 0 && NMEL % MG == 0, "tile shape");
  static_assert(FT * NMEL <= Tl::SX, "the output tile reuses the span");
  static_assert((Tl::SX + Tl::SB + FT) * 4 <= 64 * 1024, "static LDS");
  __shared__ float sX[Tl::SX];
  __shared__ __attribute__((aligned(16))) float sB[Tl::SB];
  __shared__ float sNyq[FT];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, f0 = blockIdx.x * FT;
  const int n = clip_len(n_samples, b, S);
  const int Tb = reflect_frames<Tl>(n, pad);
  const int rows = min(FT, T_rows - f0);                 // rows of this tile that exist in the output (>= 1 by the grid)
  float* __restrict__ out = mel + ((int64_t)b * T_rows + f0) * ldm;
  if (f0 >= Tb) {                                        // block-uniform: a tile wholly past the clip's end
    zero_tile(out, rows, NMEL, ldm);
    return;
  }
  stage_span<Tl, I16>(sX, wav_, ldw, b, f0 * HOP - pad, n, n, nullptr);   // frames past T_b may reach past the clip and read 0

  const int fh = wave % FH, lh = lane >> 5;
  const bool nyq = wave / FH == 0 && (lane & 31) == 0;   // column 0 of pass 0's first pair: re[0] | re[n_fft/2], both real-only
  const int mf = tid % FT;                               // the frame whose mel sums this thread keeps
  const int mg = FT == 64 ? wave : tid / FT;             // ... and its band group (wave-uniform at FT = 64)
  float m[BPG];
#pragma unroll
  for (int j = 0; j < BPG; ++j) m[j] = 0.f;

  pass_loop<Tl>(
      sX, sB, basis,
      [&](int pass, int e, float re, float im) {         // magnitudes of bins NBP pass .. + NBP - 1
        if (pass == 0 && nyq) {
          sNyq[32 * fh + 8 * (e >> 2) + 4 * lh + (e & 3)] = sqrtf(__builtin_fmaf(im, im, mag_eps));
          return sqrtf(add_rn(power(re, 0.f), mag_eps));
        }
        return sqrtf(add_rn(power(re, im), mag_eps));
      },
      [&](int pass, const float* sG) {                   // ... into the mel sums, bins ascending
        const int c0 = pass * NBP;
#pragma unroll
        for (int j = 0; j < BPG; ++j) {
          const int band = mg * BPG + j;
          const int lo = max(fb_range[2 * band], c0), hi = min(min(fb_range[2 * band + 1], c0 + NBP), NBIN - 1);
          const float* w = fb + band * NBIN;
          for (int k = lo; k < hi; ++k) m[j] = fmaf(w[k], sG[mf * LDR + (k - c0)], m[j]);
        }
      });

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

using Tile640 = FrameDftTile<640, 160, 64, 640>;
using Tile1024 = FrameDftTile<1024, 256, 32, 1024>;

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
