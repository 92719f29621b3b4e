// fp32 tap-GEMM (desc.dtype = L2S_F32): the reference-precision form of tapgemm.hip's contraction
//
//   C[o(m), n] = epi( sum_tap sum_c A[src(m,tap), c] * W[n, tap*Cin + c] )        A, W, C, C2, R all fp32
//
// on the f32-input matrix instruction v_mfma_f32_32x32x2_f32: every result is a k-ordered fp32 fma chain (one rounding per
// product, no wider internal sum), so only the order of the additions separates it from an fp32 reference.  One tile shape:
// 4 waves, block tile 128 x 128, K-tile 16; a wave owns 64 x 64 = 2 x 2 blocks of 32 x 32, i.e. four independent
// accumulators (the instruction's dependent latency equals its issue interval, so four chains keep the pipe full with one wave
// per SIMD; two blocks per CU cover the barrier).  Operands travel global -> registers -> LDS (k-major, [16][128 + 4] floats:
// the transposing writes and the one-float-per-lane fragment reads are both bank-conflict free), double buffered with the next
// K-tile's global loads in flight under the current tile's MFMAs.  The im2col gather (CONV1D / CONV2D taps, zero padding),
// groups (blockIdx.z), the output-row remap and the lens row mask follow tapgemm_kernel.h.  The MFMA is issued with the
// activations as the A operand: a lane ends with ONE output channel (lane & 31) of 16 rows, so every store / residual load of
// a wave instruction covers 128 contiguous bytes of a row and N needs no multiple-of-4 tail handling inside a tile.
// The epilogue uses erff / expf / tanhf and IEEE division (no v_rcp, no polynomial): at 1/16 of the 16-bit MFMA rate their
// cost does not show.
#include "l2s_common.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int LDT = BM + 4;   // LDS row stride in floats (k-major tiles): 4*LDT = 16 mod 64 banks

template <int MODE>
__global__ __launch_bounds__(256, 2) void tapgemm_f32_kernel(const l2s_gemm_desc p, const int tiles_n) {
  __shared__ float sA[2][BK][LDT];
  __shared__ float sW[2][BK][LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = blockIdx.z;
  const int tile_m = blockIdx.x / tiles_n, tile_n = blockIdx.x - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int Cin = p.Cin, Ktot = p.Cin * p.ntaps;
  const float* __restrict__ A = (const float*)p.A + (int64_t)grp * p.a_gstride;
  const float* __restrict__ W = (const float*)p.W + (int64_t)grp * p.w_gstride;

  // ---- operand fetch: thread -> rows (tid >> 2) and (tid >> 2) + 64 of both tiles, k chunk (tid & 3) * 4 ------------
  const int ld_row = tid >> 2, ld_k = (tid & 3) * 4;
  const float* a_base[2];
  int a_t[2], a_x[2];
  const float* w_ptr[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    int m = m0 + ld_row + 64 * h;
    m = m < p.M ? m : p.M - 1;          // rows past M are computed on a valid row and never stored
    a_t[h] = 0; a_x[h] = 0;
    if (MODE == L2S_MODE_LINEAR) {
      a_base[h] = A + (int64_t)m * p.lda;
    } else if (MODE == L2S_MODE_CONV1D) {
      const int b = m / p.T_out, t = m - b * p.T_out;
      a_base[h] = A + (int64_t)b * p.T_in * p.lda;
      a_t[h] = t * p.stride + p.off;
    } else {
      const int hw = p.Ho * p.Wo;
      const int img = m / hw, rem = m - img * hw;
      const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
      a_base[h] = A + (int64_t)img * p.Hi * p.Wi * p.lda;
      a_t[h] = oy * p.stride - p.pad;
      a_x[h] = ox * p.stride - p.pad;
    }
    int n = n0 + ld_row + 64 * h;
    n = n < p.N ? n : p.N - 1;
    w_ptr[h] = W + (int64_t)n * Ktot;
  }
  float4 ra[2], rw[2];
  auto fetch = [&](int kt) {
    const int kk = kt * BK + ld_k;       // Cin % 4 == 0: the four k of a chunk share one tap
    const bool kok = kk < Ktot;
    int tap = 0, cc = kk;
    if (MODE != L2S_MODE_LINEAR) { tap = kk / Cin; cc = kk - tap * Cin; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bool ok = kok;
      int64_t off;
      if (MODE == L2S_MODE_LINEAR) {
        off = kk;
      } else if (MODE == L2S_MODE_CONV1D) {
        const int st = a_t[h] + tap * p.dil;
        ok = ok && ((unsigned)st < (unsigned)p.T_in);
        off = (int64_t)st * p.lda + cc;
      } else {
        const int ky = tap / p.KW, kx = tap - ky * p.KW;
        const int iy = a_t[h] + ky, ix = a_x[h] + kx;
        ok = ok && ((unsigned)iy < (unsigned)p.Hi) && ((unsigned)ix < (unsigned)p.Wi);
        off = ((int64_t)iy * p.Wi + ix) * p.lda + cc;
      }
      ra[h] = ok ? *reinterpret_cast<const float4*>(a_base[h] + off) : make_float4(0.f, 0.f, 0.f, 0.f);
      rw[h] = kok ? *reinterpret_cast<const float4*>(w_ptr[h] + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = ld_row + 64 * h;
      sA[buf][ld_k + 0][r] = ra[h].x; sA[buf][ld_k + 1][r] = ra[h].y;
      sA[buf][ld_k + 2][r] = ra[h].z; sA[buf][ld_k + 3][r] = ra[h].w;
      sW[buf][ld_k + 0][r] = rw[h].x; sW[buf][ld_k + 1][r] = rw[h].y;
      sW[buf][ld_k + 2][r] = rw[h].z; sW[buf][ld_k + 3][r] = rw[h].w;
    }
  };

  // ---- main loop ---------------------------------------------------------------------------------------------------
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  const int lr = lane & 31, lh = lane >> 5;
  const bool wave_on = (n0 + wn < p.N) && (m0 + wm < p.M);   // wave-uniform: a sub-tile wholly outside the matrix idles
  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  const int nk = (Ktot + BK - 1) / BK;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) fetch(kt + 1);
    if (wave_on) {
#pragma unroll
      for (int s = 0; s < BK / 2; ++s) {
        const int k = 2 * s + lh;
        const float a0 = sA[buf][k][wm + lr], a1 = sA[buf][k][wm + 32 + lr];
        const float w0 = sW[buf][k][wn + lr], w1 = sW[buf][k][wn + 32 + lr];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w1, acc[1][1], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) stage(buf ^ 1);
    __syncthreads();
  }
  if (!wave_on) return;

  // ---- epilogue: v = alpha*(acc + bias) [+R] -> act -> [+R] [+C] -> mask -> C (and C2 = leaky_relu(v, slope2)) --------
  // block (i, j), register e of a lane: row wm + 32 i + 8 (e >> 2) + 4 lh + (e & 3), channel wn + 32 j + lr
  const int flags = p.flags, act = p.act;
  const float alpha = p.alpha;
  float* __restrict__ C = (float*)p.C;
  float* __restrict__ C2 = (float*)p.C2;
  const float* __restrict__ R = (const float*)p.R;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 32 * j + lr;
    if (n >= p.N) continue;
    const float bv = p.bias ? p.bias[grp * p.N + n] : 0.f;
    const float sv = act == L2S_ACT_PRELU ? p.slope[grp * p.N + n] : (act == L2S_ACT_LRELU ? p.act_slope : 0.f);
    const int col = grp * p.c_gstride + n;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm + 32 * i + 8 * (e >> 2) + 4 * lh + (e & 3);
        if (m >= p.M) continue;
        const int64_t o = (int64_t)m * p.out_row_mul + p.out_row_add;
        float v = acc[i][j][e] + bv;
        if (alpha != 1.f) v *= alpha;
        float rv = 0.f;
        if (flags & (L2S_F_RES_PRE | L2S_F_RES_POST)) rv = R[o * p.ldr + col];
        if (flags & L2S_F_RES_PRE) v += rv;
        switch (act) {
          case L2S_ACT_RELU: v = fmaxf(v, 0.f); break;
          case L2S_ACT_GELU: v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); break;
          case L2S_ACT_SWISH: v = v / (1.0f + expf(-v)); break;
          case L2S_ACT_PRELU:
          case L2S_ACT_LRELU: v = v >= 0.f ? v : v * sv; break;
          case L2S_ACT_TANH: v = tanhf(v); break;
          default: break;
        }
        if (flags & L2S_F_RES_POST) v += rv;
        if (flags & L2S_F_ACCUM) v += C[o * p.ldc + col];
        if (flags & L2S_F_MASK) {
          const int clip = (int)(o / p.mask_T);
          const int t = (int)(o - (int64_t)clip * p.mask_T);
          if (!(t < p.lens[clip] * p.mask_mul)) v = 0.f;
        }
        C[o * p.ldc + col] = v;
        if (flags & L2S_F_DUAL) C2[o * p.ldc2 + col] = v >= 0.f ? v : v * p.slope2;
      }
    }
  }
}

}  // namespace

// called by l2s_tapgemm (tapgemm.hip) after the checks every dtype shares
int l2s_tapgemm_f32_launch(const l2s_gemm_desc& d, hipStream_t st) {
  if (d.ktab) return L2S_EUNSUPPORTED;                 // the K-block table belongs to the phase-staggered 16-bit kernel
  if (d.mode < 0 || d.mode > 2) return L2S_EINVAL;
  // 16-byte operand chunks of four fp32 along K (a chunk never straddles a tap)
  if ((d.Cin & 3) || (d.lda & 3) || (d.a_gstride & 3) || (d.w_gstride & 3)) return L2S_EALIGN;
  const int64_t tiles_m = ((int64_t)d.M + BM - 1) / BM, tiles_n = (d.N + BN - 1) / BN;
  if (tiles_m * tiles_n >= ((int64_t)1 << 31) || d.groups > 65535) return L2S_EUNSUPPORTED;
  dim3 grid((unsigned)(tiles_m * tiles_n), 1, (unsigned)d.groups), blk(256);
  if (d.mode == L2S_MODE_LINEAR) hipLaunchKernelGGL(tapgemm_f32_kernel<L2S_MODE_LINEAR>, grid, blk, 0, st, d, (int)tiles_n);
  else if (d.mode == L2S_MODE_CONV1D) hipLaunchKernelGGL(tapgemm_f32_kernel<L2S_MODE_CONV1D>, grid, blk, 0, st, d, (int)tiles_n);
  else hipLaunchKernelGGL(tapgemm_f32_kernel<L2S_MODE_CONV2D>, grid, blk, 0, st, d, (int)tiles_n);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
