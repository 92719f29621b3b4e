// STOI (Taal, Hendriks, Heusdens, Jensen, IEEE TASL 19(7), 2011) and ESTOI (Jensen, Taal, IEEE/ACM TASLP 24(11), 2016) of a batch of
// clip pairs, on the device.  DESIGN.md section 17 holds the definition; the four entries are its stages, each observable:
//
//   l2s_stoi_resample  16 kHz -> 10 kHz, up 5 / down 8, the Octave-compatible 581-tap Kaiser low-pass as a polyphase FIR
//   l2s_stoi_frames    windowed frame norms of the clean signal, the 40 dB mask, the kept-frame list by an exclusive scan
//   l2s_stoi_bands     kept frames overlap-added in LDS, windowed 512-point DFT of bins 7..218 on v_mfma_f32_32x32x2_f32, third-octave
//                      band magnitudes [B, 2, 15, F]
//   l2s_stoi_scores    every 30-frame segment's STOI and ESTOI term, and their per-clip means
//
// Nothing here uses an atomic: every sum has one fixed order, so a clip's results are the same bytes from run to run and whatever
// its batch mates are.  Samples, spectra and normalisations are fp32; sums of squares that decide the mask and the sums over
// bands, frames and segments are carried in fp64.
#include "frame_dft.h"
#include <math.h>

namespace {

constexpr int FRAME = 256, HOP = 128, NBAND = 15, NSEG = 30;
constexpr int BIN0 = 7, BIN1 = 219;                      // the bins the 15 bands cover: [7, 219)
constexpr int MAX_FRAMES = 2048;                         // analysis frames per clip (24 s are 1 873)
constexpr int MAX_LEN10K = FRAME + MAX_FRAMES * HOP;     // resampled samples that give MAX_FRAMES frames
constexpr int MAX_SAMPLES = MAX_LEN10K / 5 * 8;          // 419 840: the longest 16 kHz clip, ceil(5 n / 8) <= MAX_LEN10K
constexpr float EPS32 = 2.220446049250313e-16f;          // 2^-52
constexpr double EPS64 = 2.220446049250313e-16;

__host__ __device__ __forceinline__ int len10k(int n) { return (5 * n + 7) / 8; }                     // ceil(5 n / 8)
__host__ __device__ __forceinline__ int frames_of(int len) { return len > FRAME ? (len - FRAME - 1) / HOP + 1 : 0; }   // i < len - 256
static_assert(MAX_LEN10K % 5 == 0 && (5 * MAX_SAMPLES + 7) / 8 == MAX_LEN10K && (5 * (MAX_SAMPLES + 1) + 7) / 8 > MAX_LEN10K, "cap");
inline bool size_ok(int S) { return S > 0 && S <= MAX_SAMPLES; }

__device__ __forceinline__ int clip_samples(const int32_t* n_samples, int b, int S) { return max(frame_dft::clip_len(n_samples, b, S), 0); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- 1. resample ------------------------------------------------------------------------------------------------------------------
// out[m] = 5 sum_j w[j] xup[8 m + 290 - j], xup = x zero-stuffed by 5: only j = p + 5 q with p = 3 m mod 5 meet a sample, which is
// x[(8 m + 290 - p) / 5 - q].  taps: [5][117] = 5 w[p + 5 q] (0 where p + 5 q > 580); the sum runs q = 0 .. 116 as one fma chain.
// A block makes 256 consecutive outputs of one clip from a 528-sample span staged in LDS (zeros outside the clip).
constexpr int RS_PH = 5, RS_Q = 117, RS_HALF = 290, RS_OUT = 256, RS_SPAN = 528;

template <bool I16>
__global__ __launch_bounds__(RS_OUT) void stoi_resample_kernel(const void* __restrict__ wav_, const int64_t ldw,
                                                               const int32_t* __restrict__ n_samples, const int S,
                                                               const float* __restrict__ taps, float* __restrict__ out, const int64_t ldo,
                                                               const int R) {
  __shared__ float sX[RS_SPAN];
  __shared__ float sT[RS_PH * RS_Q];
  const int tid = threadIdx.x, b = blockIdx.y, m0 = blockIdx.x * RS_OUT;
  const int n = clip_samples(n_samples, b, S);
  const int n_out = len10k(n);
  const int m = m0 + tid;
  float* __restrict__ o = out + (int64_t)b * ldo;
  if (m0 >= n_out) {                                     // block-uniform: wholly past the clip
    if (m < R) o[m] = 0.f;
    return;
  }
  const int lo = (8 * m0 + RS_HALF - 4) / 5 - (RS_Q - 1);   // first sample any output of the block can touch
  for (int s = tid; s < RS_SPAN; s += RS_OUT) {
    const int p = lo + s;
    float v = 0.f;
    if ((unsigned)p < (unsigned)n) v = frame_dft::wav_sample<I16>(wav_, (int64_t)b * ldw + p);
    sX[s] = v;
  }
  for (int s = tid; s < RS_PH * RS_Q; s += RS_OUT) sT[s] = taps[s];
  __syncthreads();
  if (m >= R) return;
  float acc = 0.f;
  if (m < n_out) {
    const int p = (3 * m) % 5;
    const int base = (8 * m + RS_HALF - p) / 5 - lo;     // in [116, 525]
    const float* t = &sT[p * RS_Q];
#pragma unroll 9
    for (int q = 0; q < RS_Q; ++q) acc = fmaf(t[q], sX[base - q], acc);
  }
  o[m] = acc;
}

// ---- 2. kept frames ---------------------------------------------------------------------------------------------------------------
// One block of 16 waves per clip.  Wave w takes frames w, w + 16, ...: 4 samples per lane, fp32 product with the window, squares
// summed in fp64 (lane order, then the xor butterfly).  Frame j is kept iff norm_j + EPS > (norm_max + EPS) 10^-2.
constexpr int FR_WAVES = 16;

__global__ __launch_bounds__(FR_WAVES * 64) void stoi_frames_kernel(const float* __restrict__ x, const int64_t ldx,
                                                                    const int32_t* __restrict__ n_samples, const int S,
                                                                    const float* __restrict__ window, int32_t* __restrict__ kept,
                                                                    const int ldk, int32_t* __restrict__ n_kept) {
  __shared__ double sN[MAX_FRAMES];
  __shared__ double sMax[FR_WAVES];
  __shared__ int sCnt[FR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  const int nf = min(frames_of(len10k(clip_samples(n_samples, b, S))), min(MAX_FRAMES, ldk));
  const float* __restrict__ xb = x + (int64_t)b * ldx;
  float w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = window[lane + 64 * i];
  for (int j = wave; j < nf; j += FR_WAVES) {
    const float* p = xb + (int64_t)j * HOP;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v = __fmul_rn(w[i], p[lane + 64 * i]);
      acc += (double)v * (double)v;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) sN[j] = sqrt(acc);
  }
  __syncthreads();
  double mx = 0.0;
  for (int j = tid; j < nf; j += FR_WAVES * 64) mx = fmax(mx, sN[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) sMax[wave] = mx;
  __syncthreads();
  mx = sMax[0];
#pragma unroll
  for (int i = 1; i < FR_WAVES; ++i) mx = fmax(mx, sMax[i]);
  const double thr = (mx + EPS64) * 1e-2;
  const int j0 = 2 * tid, j1 = 2 * tid + 1;
  const int f0 = j0 < nf && sN[j0] + EPS64 > thr, f1 = j1 < nf && sN[j1] + EPS64 > thr;
  const int c = f0 + f1;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) sCnt[wave] = incl;
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int i = 0; i < FR_WAVES; ++i) {
    off += i < wave ? sCnt[i] : 0;
    total += sCnt[i];
  }
  int32_t* __restrict__ kb = kept + (int64_t)b * ldk;
  const int e = off + incl - c;                          // exclusive position; e + c <= total <= nf <= ldk
  if (f0) kb[e] = j0;
  if (f1) kb[e + f0] = j1;
  for (int k = total + tid; k < ldk; k += FR_WAVES * 64) kb[k] = -1;
  if (tid == 0) n_kept[b] = total;
}

// ---- 3. band matrices -------------------------------------------------------------------------------------------------------------
// The compacted signal z (kept windowed frames overlap-added at hop 128) is chunk c = samples [128 c, 128 c + 128):
//   z[128 c + r] = W[128 + r] x[128 g(c-1) + 128 + r] + W[r] x[128 g(c) + r],   g(k) = the k-th kept frame, terms outside 0 <= k < K drop.
// Frame f of the second analysis is chunks f, f + 1; there are F = K - 1 of them.  A block owns 32 consecutive frames of one signal
// of one clip: it gathers their 33 chunks into the span rows of frame_dft.h (rows of 128 with stride 129) and that header's pass
// loop multiplies [32 x 256] by the basis [256 x 512] - the second window folded in, column map in the ABI header - in two passes
// of 256 columns: wave pp owns the re and im tiles of bins 7 + 128 pass + 32 pp .. + 31.  After a pass the 32 x 128 powers are in
// the result tile and thread (frame tid % 32, band group tid / 32) adds its bands' bins in ascending order.
using BandTile = frame_dft::FrameDftTile<FRAME, HOP, 32, 512>;
constexpr int BT_F = BandTile::FT, BT_CH = BandTile::SROWS;

__global__ __launch_bounds__(256, 2) void stoi_bands_kernel(const float* __restrict__ x, const float* __restrict__ y, const int64_t ldx,
                                                            const int32_t* __restrict__ n_samples, const int S,
                                                            const int32_t* __restrict__ kept, const int ldk,
                                                            const int32_t* __restrict__ n_kept, const float* __restrict__ window,
                                                            const float* __restrict__ basis, const int32_t* __restrict__ band_edges,
                                                            float* __restrict__ bands, const int ldf) {
  constexpr int LDZ = BandTile::SLD, NBP = BandTile::NBP, LDP = BandTile::LDR;
  __shared__ float sZ[BandTile::SX];
  __shared__ __attribute__((aligned(16))) float sB[BandTile::SB];
  __shared__ int sG[BT_CH + 1];
  const int tid = threadIdx.x;
  const int f0 = blockIdx.x * BT_F, sig = blockIdx.y, b = blockIdx.z;
  const int nf = min(frames_of(len10k(clip_samples(n_samples, b, S))), MAX_FRAMES);
  const int K = max(min(min(n_kept[b], nf), ldk), 0);
  const int F = min(max(K - 1, 0), ldf);
  const int rows = min(BT_F, ldf - f0);                  // columns of this tile that exist in the output (>= 1 by the grid)
  float* __restrict__ out = bands + ((int64_t)(b * 2 + sig) * NBAND) * ldf + f0;
  if (f0 >= F) {                                         // block-uniform: a tile wholly past the clip's frames
    frame_dft::zero_tile(out, NBAND, rows, ldf);
    return;
  }

  // ---- the kept frames behind chunks f0 - 1 .. f0 + 32 (-1: none), then the chunks themselves
  if (tid < BT_CH + 1) {
    const int c = f0 - 1 + tid;
    int g = (c >= 0 && c < K) ? kept[(int64_t)b * ldk + c] : -1;
    sG[tid] = (unsigned)g < (unsigned)nf ? g : -1;       // a frame index the clip does not have is not read
  }
  __syncthreads();
  {
    const float* __restrict__ src = (sig ? y : x) + (int64_t)b * ldx;
    for (int e = tid; e < BT_CH * HOP; e += 256) {
      const int ci = e / HOP, r = e - ci * HOP;
      const int g0 = sG[ci], g1 = sG[ci + 1];
      float v = g0 >= 0 ? __fmul_rn(window[HOP + r], src[(int64_t)g0 * HOP + HOP + r]) : 0.f;
      if (g1 >= 0) v = fmaf(window[r], src[(int64_t)g1 * HOP + r], v);
      sZ[ci * LDZ + r] = v;
    }
  }

  const int mf = tid % BT_F, mg = tid / BT_F;            // the frame and the band group (bands mg, mg + 8) of this thread's sums
  int e_lo[2], e_hi[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int band = mg + 8 * j;
    e_lo[j] = band < NBAND ? max(band_edges[band], BIN0) : BIN1;
    e_hi[j] = band < NBAND ? min(band_edges[band + 1], BIN1) : BIN1;
  }
  float m[2] = {0.f, 0.f};
  frame_dft::pass_loop<BandTile>(
      sZ, sB, basis,
      [](int, int, float re, float im) { return frame_dft::power(im, re); },   // powers of bins 7 + 128 pass ..: fma(re, re, rn(im im))
      [&](int pass, const float* sP) {                   // ... into the band sums, bins ascending
        const int c0 = BIN0 + pass * NBP;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int lo = max(e_lo[j], c0), hi = min(e_hi[j], c0 + NBP);
          for (int k = lo; k < hi; ++k) m[j] += sP[mf * LDP + (k - c0)];
        }
      });

  if (mf < rows) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int band = mg + 8 * j;
      if (band < NBAND) out[(int64_t)band * ldf + mf] = f0 + mf < F ? sqrtf(m[j]) : 0.f;
    }
  }
}

// ---- 4. scores --------------------------------------------------------------------------------------------------------------------
// Segment s covers frames [s, s + 30).  A block takes 32 consecutive segments of one clip: their 61 columns of X and Y in LDS.
// Step 1, thread = (segment, band): the clipped-and-scaled correlation of STOI and the row statistics (mean, 1 / (norm + EPS)) that
// ESTOI's first normalisation needs.  Step 2, thread = (segment, frame): ESTOI's column normalisation over the 15 bands and the
// column's inner product.  Step 3, thread = segment: the 15 band terms and the 30 column terms summed in index order in fp64 ->
// seg[b][0][s], seg[b][1][s].  A second kernel (one block per clip) sums the segments: strided fp64 partials, then a fixed tree.
constexpr int SC_SEG = 32, SC_COLS = SC_SEG + NSEG - 1, SC_LDC = SC_COLS + 2;

__global__ __launch_bounds__(256) void stoi_segments_kernel(const float* __restrict__ bands, const int ldf,
                                                            const int32_t* __restrict__ n_kept, double* __restrict__ seg, const int lds) {
  __shared__ float sX[NBAND * SC_LDC], sY[NBAND * SC_LDC];
  __shared__ float sMuX[SC_SEG * NBAND], sIvX[SC_SEG * NBAND], sMuY[SC_SEG * NBAND], sIvY[SC_SEG * NBAND], sCorr[SC_SEG * NBAND];
  __shared__ float sE[SC_SEG * NSEG];
  const int tid = threadIdx.x, s0 = blockIdx.x * SC_SEG, b = blockIdx.y;
  const int F = min(max(n_kept[b] - 1, 0), ldf);
  const int M = min(max(F - NSEG + 1, 0), lds);
  if (s0 >= M) return;                                   // block-uniform; the finishing kernel reads segments < M only
  const float* __restrict__ X = bands + (int64_t)(b * 2) * NBAND * ldf;
  const float* __restrict__ Y = X + (int64_t)NBAND * ldf;
  for (int e = tid; e < NBAND * SC_COLS; e += 256) {
    const int j = e / SC_COLS, c = e - j * SC_COLS;
    const bool in = s0 + c < F;
    sX[j * SC_LDC + c] = in ? X[(int64_t)j * ldf + s0 + c] : 0.f;
    sY[j * SC_LDC + c] = in ? Y[(int64_t)j * ldf + s0 + c] : 0.f;
  }
  __syncthreads();
  const float clip = 1.0f + 5.623413251903491f;          // 1 + 10^(15/20)
  for (int e = tid; e < SC_SEG * NBAND; e += 256) {
    const int i = e % SC_SEG, j = e / SC_SEG;
    const float* xs = &sX[j * SC_LDC + i];
    const float* ys = &sY[j * SC_LDC + i];
    float sxx = 0.f, syy = 0.f, sx = 0.f, sy = 0.f;
#pragma unroll
    for (int n = 0; n < NSEG; ++n) {
      sxx = fmaf(xs[n], xs[n], sxx);
      syy = fmaf(ys[n], ys[n], syy);
      sx += xs[n];
      sy += ys[n];
    }
    const float c = sqrtf(sxx) / (sqrtf(syy) + EPS32);
    float sp = 0.f;
#pragma unroll
    for (int n = 0; n < NSEG; ++n) sp += fminf(c * ys[n], xs[n] * clip);
    const float mx = sx * (1.0f / NSEG), my = sy * (1.0f / NSEG), mp = sp * (1.0f / NSEG);
    float vx = 0.f, vy = 0.f, vp = 0.f, xp = 0.f;
#pragma unroll
    for (int n = 0; n < NSEG; ++n) {
      const float dx = xs[n] - mx, dy = ys[n] - my, dp = fminf(c * ys[n], xs[n] * clip) - mp;
      vx = fmaf(dx, dx, vx);
      vy = fmaf(dy, dy, vy);
      vp = fmaf(dp, dp, vp);
      xp = fmaf(dx, dp, xp);
    }
    const float ivx = 1.0f / (sqrtf(vx) + EPS32), ivy = 1.0f / (sqrtf(vy) + EPS32), ivp = 1.0f / (sqrtf(vp) + EPS32);
    sCorr[i * NBAND + j] = xp * ivx * ivp;
    sMuX[i * NBAND + j] = mx;
    sIvX[i * NBAND + j] = ivx;
    sMuY[i * NBAND + j] = my;
    sIvY[i * NBAND + j] = ivy;
  }
  __syncthreads();
  for (int e = tid; e < SC_SEG * NSEG; e += 256) {
    const int i = e % SC_SEG, n = e / SC_SEG;
    float xn[NBAND], yn[NBAND];
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int j = 0; j < NBAND; ++j) {
      xn[j] = (sX[j * SC_LDC + i + n] - sMuX[i * NBAND + j]) * sIvX[i * NBAND + j];
      yn[j] = (sY[j * SC_LDC + i + n] - sMuY[i * NBAND + j]) * sIvY[i * NBAND + j];
      sx += xn[j];
      sy += yn[j];
    }
    const float mx = sx * (1.0f / NBAND), my = sy * (1.0f / NBAND);
    float vx = 0.f, vy = 0.f, xy = 0.f;
#pragma unroll
    for (int j = 0; j < NBAND; ++j) {
      const float dx = xn[j] - mx, dy = yn[j] - my;
      vx = fmaf(dx, dx, vx);
      vy = fmaf(dy, dy, vy);
      xy = fmaf(dx, dy, xy);
    }
    sE[i * NSEG + n] = xy / ((sqrtf(vx) + EPS32) * (sqrtf(vy) + EPS32));
  }
  __syncthreads();
  if (tid < SC_SEG && s0 + tid < M) {
    double d = 0.0, e = 0.0;
    for (int j = 0; j < NBAND; ++j) d += (double)sCorr[tid * NBAND + j];
    for (int n = 0; n < NSEG; ++n) e += (double)sE[tid * NSEG + n];
    seg[(int64_t)(b * 2) * lds + s0 + tid] = d;
    seg[(int64_t)(b * 2 + 1) * lds + s0 + tid] = e * (1.0 / NSEG);
  }
}

__global__ __launch_bounds__(256) void stoi_finish_kernel(const double* __restrict__ seg, const int lds, const int ldf,
                                                          const int32_t* __restrict__ n_kept, float* __restrict__ stoi,
                                                          float* __restrict__ estoi, int32_t* __restrict__ n_segments) {
  __shared__ double sD[256], sE[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = min(max(n_kept[b] - 1, 0), ldf);
  const int M = min(max(F - NSEG + 1, 0), lds);
  double d = 0.0, e = 0.0;
  for (int s = tid; s < M; s += 256) {
    d += seg[(int64_t)(b * 2) * lds + s];
    e += seg[(int64_t)(b * 2 + 1) * lds + s];
  }
  sD[tid] = d;
  sE[tid] = e;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sD[tid] += sD[tid + o];
      sE[tid] += sE[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    n_segments[b] = M;
    stoi[b] = M > 0 ? (float)(sD[0] / ((double)NBAND * M)) : 1e-5f;   // no segment: the value the published code returns
    estoi[b] = M > 0 ? (float)(sE[0] / (double)M) : 1e-5f;
  }
}

}  // namespace

extern "C" int l2s_stoi_resample(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* taps,
                                 float* out, int64_t ldo, int R, void* stream) {
  if (!wav || !taps || !out) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || R <= 0) return L2S_ESHAPE;
  if (B > 65535 || !size_ok(S)) return L2S_EUNSUPPORTED;
  if (ldw < S || R < len10k(S) || R > MAX_LEN10K || ldo < R) return L2S_ESHAPE;
  if (((uintptr_t)wav & (wav_is_i16 ? 1 : 3)) || ((uintptr_t)taps & 3) || ((uintptr_t)out & 3)) return L2S_EALIGN;
  dim3 grid((unsigned)((R + RS_OUT - 1) / RS_OUT), (unsigned)B), blk(RS_OUT);
  hipStream_t st = (hipStream_t)stream;
  if (wav_is_i16) hipLaunchKernelGGL((stoi_resample_kernel<true>), grid, blk, 0, st, wav, ldw, n_samples, S, taps, out, ldo, R);
  else hipLaunchKernelGGL((stoi_resample_kernel<false>), grid, blk, 0, st, wav, ldw, n_samples, S, taps, out, ldo, R);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_stoi_frames(const float* x, int64_t ldx, const int32_t* n_samples, int B, int S, const float* window, int32_t* kept,
                               int ldk, int32_t* n_kept, void* stream) {
  if (!x || !window || !kept || !n_kept) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || ldk <= 0) return L2S_ESHAPE;
  if (B > 65535 || !size_ok(S)) return L2S_EUNSUPPORTED;
  if (ldx < len10k(S) || ldk < frames_of(len10k(S))) return L2S_ESHAPE;
  if (((uintptr_t)x & 3) || ((uintptr_t)window & 3) || ((uintptr_t)kept & 3) || ((uintptr_t)n_kept & 3)) return L2S_EALIGN;
  hipLaunchKernelGGL(stoi_frames_kernel, dim3((unsigned)B), dim3(FR_WAVES * 64), 0, (hipStream_t)stream, x, ldx, n_samples, S, window, kept,
                     ldk, n_kept);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_stoi_bands(const float* x, const float* y, int64_t ldx, const int32_t* n_samples, int B, int S, const int32_t* kept,
                              int ldk, const int32_t* n_kept, const float* window, const float* basis, const int32_t* band_edges,
                              float* bands, int ldf, void* stream) {
  if (!x || !y || !kept || !n_kept || !window || !basis || !band_edges || !bands) return L2S_EINVAL;
  if (B <= 0 || S <= 0 || ldk <= 0 || ldf <= 0) return L2S_ESHAPE;
  if (B > 65535 || !size_ok(S) || ldf > MAX_FRAMES) return L2S_EUNSUPPORTED;
  if (ldx < len10k(S) || ldk < frames_of(len10k(S)) || ldf < frames_of(len10k(S)) - 1) return L2S_ESHAPE;
  if ((uintptr_t)basis & 15) return L2S_EALIGN;
  if (((uintptr_t)x & 3) || ((uintptr_t)y & 3) || ((uintptr_t)kept & 3) || ((uintptr_t)n_kept & 3) || ((uintptr_t)window & 3) ||
      ((uintptr_t)band_edges & 3) || ((uintptr_t)bands & 3))
    return L2S_EALIGN;
  dim3 grid((unsigned)((ldf + BT_F - 1) / BT_F), 2u, (unsigned)B);
  hipLaunchKernelGGL(stoi_bands_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, y, ldx, n_samples, S, kept, ldk, n_kept, window, basis,
                     band_edges, bands, ldf);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_stoi_scores(const float* bands, int ldf, const int32_t* n_kept, int B, double* seg, int lds, float* stoi, float* estoi,
                               int32_t* n_segments, void* stream) {
  if (!bands || !n_kept || !seg || !stoi || !estoi || !n_segments) return L2S_EINVAL;
  if (B <= 0 || ldf <= 0 || lds <= 0) return L2S_ESHAPE;
  if (B > 65535 || ldf > MAX_FRAMES) return L2S_EUNSUPPORTED;
  if (lds < ldf - NSEG + 1) return L2S_ESHAPE;
  if (((uintptr_t)bands & 3) || ((uintptr_t)n_kept & 3) || ((uintptr_t)seg & 7) || ((uintptr_t)stoi & 3) || ((uintptr_t)estoi & 3) ||
      ((uintptr_t)n_segments & 3))
    return L2S_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((lds + SC_SEG - 1) / SC_SEG), (unsigned)B);
  hipLaunchKernelGGL(stoi_segments_kernel, grid, dim3(256), 0, st, bands, ldf, n_kept, seg, lds);
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, seg, lds, ldf, n_kept, stoi, estoi, n_segments);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
