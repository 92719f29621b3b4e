// The framed windowed DFT shared by the log-mel (melspec.hip) and STOI band (stoi.hip) kernels; the power-mel kernel (spkemb.hip)
// takes the span, the clip preamble and stage_span from here and keeps a K loop of its own.
//
// Tile.  A block (4 waves) owns FT consecutive frames (K samples every HOP) of one signal and multiplies them by a [K, NCOL] fp32
// table on the f32-input matrix instruction v_mfma_f32_32x32x2_f32: every output is a k-ordered fp32 fma chain over the frame.
//
//   span    The frames' contiguous samples, (FT - 1) HOP + K of them, sit in LDS once as hop-sized rows with a padded stride of
//           HOP + 1 floats: frame i, sample k is [(i + k / HOP)][k % HOP], so the 32 frames of an A fragment are HOP + 1 floats
//           apart (161 = 33 banks, 129 and 257 = 1 bank: odd, all distinct).  K need not be a multiple of HOP; the last row is
//           then partly unused.  stage_span fills it from a reflect-padded waveform; a kernel may fill it its own way.
//   table   Column c -> tile q = c / 32, lane l = c % 32; tiles 2 p and 2 p + 1 hold the real (w cos) and imaginary (-w sin) parts
//           of the same 32 bins.  It is walked in NPASS passes of PN columns; a pass's K-tiles ([BK][PN] floats = 8 KB, contiguous
//           rows of the table) stream global -> registers -> LDS double buffered under the MFMAs.
//   waves   FT / 32 frame halves x PN / 64 column pairs: wave (fh, pp) owns frames 32 fh .. + 31 and the tile pair pp of the
//           pass, so re and im of a bin end in the same lane and register and |.|^2 needs no cross-lane traffic.
//   result  After a pass's K loop each (frame, bin) value - what the kernel's `cell` makes of (re, im) - goes to an LDS tile
//           [FT][NBP + 1] laid over the idle basis buffers, and the kernel's `fold` reads it (frame tid % FT is conflict free).
//
// Barrier contract of pass_loop, which holds every __syncthreads() of this choreography:
//   - on entry the caller has WRITTEN the span (and anything else `cell` / `fold` read from LDS) and not yet synchronised: the
//     barrier that publishes K-tile 0 publishes the span with it;
//   - inside a pass one barrier per K-tile: it publishes tile t + 1 in buffer (t + 1) & 1 and retires the reads of tile t;
//   - at the end of a pass: barrier (every wave is done with both basis buffers: they ARE the result tile from here), `cell`
//     values written, barrier, `fold`, barrier (the result tile is read: the buffers go back to the basis), then the next pass's
//     first K-tile - fetched under the last MFMAs - is stored and published;
//   - on return every thread has passed the barrier that follows the last `fold`: the span and the buffers are free for reuse.
// `cell` and `fold` must not synchronise and must be reached by all 256 threads.
#pragma once
#include "l2s_common.h"

namespace frame_dft {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

template <int K_, int HOP_, int FT_>
struct FrameSpan {
  static constexpr int K = K_, HOP = HOP_, FT = FT_;
  static constexpr int SPAN = (FT - 1) * HOP + K;                    // samples a tile's frames cover
  static constexpr int SROWS = (SPAN + HOP - 1) / HOP, SLD = HOP + 1;   // the span as hop-sized rows, padded stride
  static constexpr int SX = SROWS * SLD;                             // floats of the span
};

template <int K_, int HOP_, int FT_, int NCOL_>
struct FrameDftTile : FrameSpan<K_, HOP_, FT_> {
  static constexpr int NCOL = NCOL_;
  static constexpr int FH = FT_ / 32, NPP = 4 / FH;                  // waves = frame halves x column pairs
  static constexpr int PN = 64 * NPP, LDB = PN + 4;                  // table columns per pass; K-tile row stride
  static constexpr int BK = 2048 / PN;                               // K-tile [BK][PN]: two float4 per thread
  static constexpr int KT_PASS = K_ / BK, NPASS = NCOL / PN;
  static constexpr int NBP = PN / 2, LDR = NBP + 1;                  // bins per pass; result tile [FT][NBP + 1]
  static constexpr int SB = 2 * BK * LDB;                            // floats of the two basis buffers
  static_assert((FT_ == 32 || FT_ == 64) && K_ % BK == 0 && NCOL % PN == 0, "tile shape");
  static_assert(FT_ * LDR <= SB, "the result tile reuses the basis buffers");
  static_assert((FrameSpan<K_, HOP_, FT_>::SX + SB) * 4 <= 64 * 1024, "static LDS");
};

// ---- clip preamble ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int clip_len(const int32_t* __restrict__ n_samples, int b, int S) {   // at most the buffer; may be <= 0
  const int n = n_samples ? n_samples[b] : S;
  return n < S ? n : S;
}

// frames of a clip of n samples with `pad` reflected on each side; none unless the reflection is valid and one whole frame fits
template <class Tl>
__device__ __forceinline__ int reflect_frames(int n, int pad) {
  return (n > pad && n + 2 * pad >= Tl::K) ? (n + 2 * pad - Tl::K) / Tl::HOP + 1 : 0;
}

template <bool I16>
__device__ __forceinline__ float wav_sample(const void* __restrict__ wav, int64_t idx) {
  if (I16) return (float)((const int16_t*)wav)[idx] * (1.0f / 32768.0f);
  return ((const float*)wav)[idx];
}

// zeros over out[r * ld + c], r < nr, c < nc: the block-uniform answer of a tile wholly past its clip's end
__device__ __forceinline__ void zero_tile(float* __restrict__ out, int nr, int nc, int64_t ld) {
  for (int e = threadIdx.x; e < nr * nc; e += 256) {
    const int r = e / nc;
    out[r * ld + (e - r * nc)] = 0.f;
  }
}

// ---- a^2 + b^2 as fma(b, b, rn(a a)) and a rounded sum, fenced from the compiler's fp contraction: left to it, which product is
// rounded and which is fused is chosen per call site (the log-mel kernel had rounded re re, the STOI kernel im im; each caller
// passes its arguments in the order that keeps its bits), and a kernel's bits would depend on the code around the expression
__device__ __forceinline__ float power(float a, float b) {
#pragma clang fp contract(off)
  return __builtin_fmaf(b, b, a * a);
}

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// ---- span staging: clip positions p0 .. of a waveform of analysis length n, reflected once at either end; positions at or past
// n_valid (<= the buffer) are zeros and are not read; `scale` (or null) multiplies the clip by scale[b]
template <class Tl, bool I16>
__device__ __forceinline__ void stage_span(float* sX, const void* __restrict__ wav, int64_t ldw, int b, int p0, int n, int n_valid,
                                           const float* __restrict__ scale) {
  const float g = scale ? scale[b] : 1.0f;
  for (int s = threadIdx.x; s < Tl::SROWS * Tl::HOP; s += 256) {
    int p = p0 + s;
    p = p < 0 ? -p : p;
    p = p >= n ? 2 * (n - 1) - p : p;
    float v = 0.f;
    if (s < Tl::SPAN && (unsigned)p < (unsigned)n_valid) {
      v = wav_sample<I16>(wav, (int64_t)b * ldw + p);
      if (scale) v = __fmul_rn(v, g);
    }
    const int r = s / Tl::HOP;
    sX[r * Tl::SLD + (s - r * Tl::HOP)] = v;
  }
}

// ---- the pass loop.  cell(pass, e, re, im) -> the value of accumulator element e (frame 32 fh + 8 (e / 4) + 4 (lane / 32) + e % 4,
// bin NBP pass + 32 pp + lane % 32); fold(pass, sR) reads the result tile sR[frame * LDR + bin - NBP pass].
template <class Tl, class Cell, class Fold>
__device__ __forceinline__ void pass_loop(const float* sX, float* sB, const float* __restrict__ basis, Cell cell, Fold fold) {
  constexpr int HOP = Tl::HOP, SLD = Tl::SLD, FH = Tl::FH, PN = Tl::PN, LDB = Tl::LDB, BK = Tl::BK, KT_PASS = Tl::KT_PASS;
  constexpr int NCOL = Tl::NCOL, LDR = Tl::LDR, NT = Tl::NPASS * KT_PASS;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // basis fetch: thread -> rows tid / (PN/4) and that + BK/2 of the K-tile, columns 4 (tid % (PN/4)) .. + 3
  const int ld_k = tid / (PN / 4), ld_c = (tid % (PN / 4)) * 4;
  float4 rb0, rb1;
  auto fetch = [&](int t) {                                // t: flat K-tile index, pass = t / KT_PASS
    const int pass = t / KT_PASS, k0 = (t - pass * KT_PASS) * BK;
    const float* src = basis + (int64_t)(k0 + ld_k) * NCOL + pass * PN + ld_c;
    rb0 = *reinterpret_cast<const float4*>(src);
    rb1 = *reinterpret_cast<const float4*>(src + (BK / 2) * NCOL);
  };
  auto stage = [&](int buf) {
    *reinterpret_cast<float4*>(&sB[(buf * BK + ld_k) * LDB + ld_c]) = rb0;
    *reinterpret_cast<float4*>(&sB[(buf * BK + ld_k + BK / 2) * LDB + ld_c]) = rb1;
  };
  const int fh = wave % FH, pp = wave / FH;
  const int lr = lane & 31, lh = lane >> 5;
  const int arow = (32 * fh + lr) * SLD;
  f32x16_t acc[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }

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
    __syncthreads();
    float* sR = sB;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int fr = 32 * fh + 8 * (e >> 2) + 4 * lh + (e & 3);
      sR[fr * LDR + 32 * pp + lr] = cell(pass, e, acc[0][e], acc[1][e]);
      acc[0][e] = 0.f;
      acc[1][e] = 0.f;
    }
    __syncthreads();
    fold(pass, sR);
    __syncthreads();
    if (t + 1 < NT) {
      stage(buf ^ 1);
      __syncthreads();
    }
  }
}

}  // namespace frame_dft
