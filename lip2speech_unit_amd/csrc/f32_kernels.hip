// fp32 (L2S_F32) forms of the non-GEMM kernels of the stage-1 path: attention, LayerNorm, the conformer conv core, the
// stem, the pools, the frame preprocessing and the row utilities.  They exist for reference precision, not speed: every
// value is an fp32 load, the arithmetic is plain fp32 with erff / expf and IEEE division and square root, and each kernel is
// the shortest correct form (the tap-GEMMs carry > 95 % of an fp32 step's time).  Entry points are the l2s_f32_* functions
// at the bottom, called from the extern "C" wrappers of the 16-bit translation units after their argument checks.
#include "l2s_common.h"
#include <math.h>

namespace {

inline int grid_for(int64_t total, int block) {
  int64_t g = (total + block - 1) / block;
  return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// ---- LayerNorm: one wave per row, the row in registers, two-pass statistics ------------------------------------------------
constexpr int MAXV4 = 8;  // float4 per lane -> C <= 2048

__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float* __restrict__ y,
                                                            int ldy, float* __restrict__ y2, int ldy2, int M, int C, int zp,
                                                            const int32_t* __restrict__ lens, int len_mul, int mask_T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= M) return;
  bool keep = true;
  if (lens) {
    const int clip = row / mask_T;
    keep = (row - clip * mask_T) < lens[clip] * len_mul;
  }
  const int nv = C >> 2;
  float4 v[MAXV4];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV4; ++i) {
    const int gi = i * 64 + lane;
    v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gi < nv) {
      v[i] = *reinterpret_cast<const float4*>(x + (int64_t)row * ldx + gi * 4);
      sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float ctot = (float)(C + zp);
  const float mean = wave_sum(sum) / ctot;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV4; ++i) {
    const int gi = i * 64 + lane;
    if (gi < nv) {
      const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
      sq += (a * a + b * b) + (c * c + d * d);
    }
  }
  sq = wave_sum(sq) + (float)zp * mean * mean;
  const float rstd = 1.0f / sqrtf(sq / ctot + eps);
  auto store4 = [&](int col, float4 o) {
    if (!keep) o = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(y + (int64_t)row * ldy + col) = o;
    if (y2) *reinterpret_cast<float4*>(y2 + (int64_t)row * ldy2 + col) = o;
  };
  const float z = -mean * rstd;   // the zero prefix of hubert.py:706-720
  for (int gi = lane; gi < (zp >> 2); gi += 64) {
    const float4 g = *reinterpret_cast<const float4*>(gamma + gi * 4);
    const float4 bt = *reinterpret_cast<const float4*>(beta + gi * 4);
    store4(gi * 4, make_float4(z * g.x + bt.x, z * g.y + bt.y, z * g.z + bt.z, z * g.w + bt.w));
  }
#pragma unroll
  for (int i = 0; i < MAXV4; ++i) {
    const int gi = i * 64 + lane;
    if (gi < nv) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + zp + gi * 4);
      const float4 bt = *reinterpret_cast<const float4*>(beta + zp + gi * 4);
      store4(zp + gi * 4, make_float4((v[i].x - mean) * rstd * g.x + bt.x, (v[i].y - mean) * rstd * g.y + bt.y,
                                      (v[i].z - mean) * rstd * g.z + bt.z, (v[i].w - mean) * rstd * g.w + bt.w));
    }
  }
}

// ---- attention: one wave per query row, online softmax over 64-key chunks ------------------------------------------------------
// Scores: lane = key (each lane walks its key's 64-float row, and its position row P[(T-1) - (i-j)]); output: lane = head
// dimension, the chunk's probabilities broadcast lane by lane.  No LDS, no barrier: any T.
template <bool REL>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ qkv, int ldq, float* __restrict__ out, int ldo,
                                                            const float* __restrict__ pos, int ldp,
                                                            const float* __restrict__ bias_u, const float* __restrict__ bias_v,
                                                            const int32_t* __restrict__ lens, int len_mul, int T, int H) {
  constexpr int D = 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave, h = blockIdx.y, b = blockIdx.z;
  if (i >= T) return;
  int klen = lens ? lens[b] * len_mul : T;
  klen = klen < T ? klen : T;
  float* orow = out + ((int64_t)b * T + i) * ldo + h * D;
  if (klen <= 0) { orow[lane] = 0.f; return; }
  const float* qrow = qkv + ((int64_t)b * T + i) * ldq + h * D;
  const float* kbase = qkv + (int64_t)b * T * ldq + H * D + h * D;
  const float* vbase = qkv + (int64_t)b * T * ldq + 2 * H * D + h * D;
  // q (+ u, + v) of this row: lane d holds element d; read back per d through readlane
  const float qd = qrow[lane];
  const float qu = REL ? qd + bias_u[h * D + lane] : qd;
  const float qv = REL ? qd + bias_v[h * D + lane] : 0.f;
  float mx = -INFINITY, l = 0.f, o = 0.f;
  for (int j0 = 0; j0 < klen; j0 += 64) {
    const int j = j0 + lane;
    const bool valid = j < klen;
    const int jc = valid ? j : klen - 1;
    const float4* kr = reinterpret_cast<const float4*>(kbase + (int64_t)jc * ldq);
    const float4* pr = REL ? reinterpret_cast<const float4*>(pos + (int64_t)(T - 1 - i + jc) * ldp + h * D) : nullptr;
    float s = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < D / 4; ++d4) {
      const float4 kv = kr[d4];
      s = fmaf(__shfl(qu, 4 * d4 + 0), kv.x, s);
      s = fmaf(__shfl(qu, 4 * d4 + 1), kv.y, s);
      s = fmaf(__shfl(qu, 4 * d4 + 2), kv.z, s);
      s = fmaf(__shfl(qu, 4 * d4 + 3), kv.w, s);
    }
    if (REL) {
      float sp = 0.f;
#pragma unroll
      for (int d4 = 0; d4 < D / 4; ++d4) {
        const float4 pv = pr[d4];
        sp = fmaf(__shfl(qv, 4 * d4 + 0), pv.x, sp);
        sp = fmaf(__shfl(qv, 4 * d4 + 1), pv.y, sp);
        sp = fmaf(__shfl(qv, 4 * d4 + 2), pv.z, sp);
        sp = fmaf(__shfl(qv, 4 * d4 + 3), pv.w, sp);
      }
      s += sp;
    }
    if (!valid) s = -INFINITY;
    const float mnew = fmaxf(mx, wave_max(s));
    const float corr = expf(mx - mnew);          // first chunk: exp(-inf) = 0
    const float pj = valid ? expf(s - mnew) : 0.f;
    l = l * corr + wave_sum(pj);
    o *= corr;
    const int nj = (klen - j0) < 64 ? (klen - j0) : 64;
    for (int jj = 0; jj < nj; ++jj) o = fmaf(__shfl(pj, jj), vbase[(int64_t)(j0 + jj) * ldq + lane], o);
    mx = mnew;
  }
  orow[lane] = o / l;
}

// ---- conformer conv core: GLU -> depthwise conv (BatchNorm folded) -> Swish, one thread per output -------------------------
__global__ void glu_dwconv_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                      float* __restrict__ y, const int32_t* __restrict__ lens, int len_mul, int B, int T, int C, int k) {
  const int64_t total = (int64_t)B * T * C;
  const int half = (k - 1) / 2;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    const int64_t r = idx / C;
    const int b = (int)(r / T), t = (int)(r - (int64_t)b * T);
    int lim = lens ? lens[b] * len_mul : T;
    lim = lim < T ? lim : T;
    float acc = bias[c];
    for (int j = 0; j < k; ++j) {
      const int tt = t + j - half;
      if (tt < 0 || tt >= lim) continue;        // zero padding, and rows past the clip's length read as zero
      const float* rp = x + ((int64_t)b * T + tt) * (2 * C) + c;
      const float g = rp[0] * (1.0f / (1.0f + expf(-rp[C])));
      acc += g * w[j * C + c];
    }
    acc = acc / (1.0f + expf(-acc));
    y[idx] = t < lim ? acc : 0.f;
  }
}

// ---- stem: Conv3d(1->64, k(5,7,7), s(1,2,2), p(2,3,3)) + folded BatchNorm3d + PReLU / Swish -------------------------------------
// One block = one frame x 4 conv rows; the 5-frame x 13-row input window and the transposed weights live in LDS; lane =
// output channel, a wave owns one conv row (44 accumulators per lane), taps summed in (dt, dy, dx) order.
constexpr int SH = 88, SW = 88, SHO = 44, SWO = 44, SROWS_B = 4, SWIN = 2 * SROWS_B + 5, SCOLS = 96;

__global__ __launch_bounds__(256) void stem_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ slope, float* __restrict__ y, int B, int T) {
  extern __shared__ float smem[];
  float* sx = smem;                          // [5][SWIN][SCOLS], column xg stored at xg + 3
  float* sw = smem + 5 * SWIN * SCOLS;       // [245][64]
  const int tid = threadIdx.x, c = tid & 63, wave = tid >> 6;
  const int bt = blockIdx.y, b = bt / T, t = bt - b * T;
  const int oy0 = blockIdx.x * SROWS_B;
  const int ylo = 2 * oy0 - 3;
  for (int idx = tid; idx < 5 * SWIN * SCOLS; idx += 256) {
    const int col = idx % SCOLS, rr = idx / SCOLS;
    const int row = rr % SWIN, f = rr / SWIN;
    const int tt = t + f - 2, gy = ylo + row, gx = col - 3;
    float v = 0.f;
    if (tt >= 0 && tt < T && gy >= 0 && gy < SH && gx >= 0 && gx < SW) v = x[(((int64_t)b * T + tt) * SH + gy) * SW + gx];
    sx[idx] = v;
  }
  for (int idx = tid; idx < 245 * 64; idx += 256) {   // packed [64][288], k = (dt*7 + dy)*8 + dx  ->  [(dt*7 + dy)*7 + dx][64]
    const int ch = idx & 63, q = idx >> 6;
    const int dx = q % 7, r = q / 7;
    sw[idx] = w[ch * 288 + r * 8 + dx];
  }
  __syncthreads();
  const int oy = oy0 + wave;
  if (oy >= SHO) return;
  float acc[SWO];
#pragma unroll
  for (int px = 0; px < SWO; ++px) acc[px] = 0.f;
  for (int r = 0; r < 35; ++r) {             // r = dt*7 + dy
    const int dt = r / 7, dy = r - dt * 7;
    const float* xr = sx + (dt * SWIN + 2 * wave + dy) * SCOLS;
#pragma unroll
    for (int dx = 0; dx < 7; ++dx) {
      const float wv = sw[(r * 7 + dx) * 64 + c];
#pragma unroll
      for (int px = 0; px < SWO; ++px) acc[px] = fmaf(xr[2 * px + dx], wv, acc[px]);
    }
  }
  const float bs = bias[c];
  const float sl = slope ? slope[c] : 0.f;
  float* yo = y + (((int64_t)bt * SHO + oy) * SWO) * 64 + c;
#pragma unroll
  for (int px = 0; px < SWO; ++px) {
    float v = acc[px] + bs;
    if (slope) v = v >= 0.f ? v : v * sl;
    else v = v / (1.0f + expf(-v));           // espnet conv3d_extractor.py:63-64 (relu_type 'swish')
    yo[px * 64] = v;
  }
}

__global__ void maxpool_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo) {
  const int64_t total = (int64_t)N * Ho * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    int64_t r = i / C;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int64_t n = r / Ho;
    float m = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = 2 * ox - 1 + dx;
        if (ix < 0 || ix >= W) continue;
        m = fmaxf(m, x[((n * H + iy) * W + ix) * C + c]);
      }
    }
    y[i] = m;
  }
}

__global__ void avgpool_f32_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int HW, int C) {
  const int64_t total = (int64_t)N * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t n = i / C;
    float s = 0.f, comp = 0.f;                 // compensated (Kahan) sum: the mean is good to an ulp at any HW
    for (int p = 0; p < HW; ++p) {
      const float v = x[(n * HW + p) * C + c] - comp;
      const float t = s + v;
      comp = (t - s) - v;
      s = t;
    }
    y[i] = s / (float)HW;
  }
}

__global__ void preprocess_f32_kernel(const uint8_t* __restrict__ f, float* __restrict__ y, int64_t nframes, int Hin, int Win, int crop,
                                      float mean, float std) {
  const int dy = (Hin - crop) / 2, dx = (Win - crop) / 2;  // utils.py:90-91: int(round(h - th) / 2.) truncates
  const int64_t total = nframes * crop * crop;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % crop);
    const int yy = (int)((i / crop) % crop);
    const int64_t n = i / ((int64_t)crop * crop);
    const float v = (float)f[(n * Hin + yy + dy) * Win + xx + dx];
    y[i] = (v / 255.0f - mean) / std;          // hubert_dataset.py:242-245 as written: two IEEE divisions
  }
}

// y[(r * rep + k) * ldy + col0 + c] = keep(r) ? x[src(r) * ldx + c] : 0   with src(r) = r (row copy) or r / T (per-clip broadcast)
template <bool BCAST>
__global__ void rows_f32_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int col0,
                                const int32_t* __restrict__ lens, int len_mul, int64_t rows, int T, int C, int rep) {
  const int64_t total = rows * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t r = i / C;
    const int64_t b = r / T;
    const int t = (int)(r - b * T);
    float v = x[(BCAST ? b : r) * ldx + c];
    if (lens && t >= lens[b] * len_mul) v = 0.f;
    for (int k = 0; k < rep; ++k) y[(r * rep + k) * ldy + col0 + c] = v;
  }
}

}  // namespace

int l2s_f32_layernorm(const void* x, int ldx, const float* gamma, const float* beta, float eps, void* y, int ldy, void* y2, int ldy2,
                      int M, int C, int zp, const int32_t* lens, int len_mul, int mask_T, hipStream_t st) {
  if (C > MAXV4 * 64 * 4) return L2S_EUNSUPPORTED;
  if (((uintptr_t)x & 15) || ((uintptr_t)y & 15) || ((uintptr_t)y2 & 15)) return L2S_EALIGN;
  hipLaunchKernelGGL(layernorm_f32_kernel, dim3((M + 3) / 4), dim3(256), 0, st, (const float*)x, ldx, gamma, beta, eps, (float*)y, ldy,
                     (float*)y2, ldy2, M, C, zp, lens, len_mul, mask_T);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_attention(const void* qkv, int ldq, void* out, int ldo, const void* pos, int ldp, const float* bias_u, const float* bias_v,
                      const int32_t* lens, int len_mul, int B, int T, int H, hipStream_t st) {
  if (H > 65535 || B > 65535) return L2S_EUNSUPPORTED;
  if ((ldq & 3) || (pos && (ldp & 3))) return L2S_EALIGN;
  dim3 grid((T + 3) / 4, H, B), blk(256);
  if (pos) hipLaunchKernelGGL(attention_f32_kernel<true>, grid, blk, 0, st, (const float*)qkv, ldq, (float*)out, ldo, (const float*)pos, ldp,
                              bias_u, bias_v, lens, len_mul, T, H);
  else hipLaunchKernelGGL(attention_f32_kernel<false>, grid, blk, 0, st, (const float*)qkv, ldq, (float*)out, ldo, (const float*)pos, ldp,
                          bias_u, bias_v, lens, len_mul, T, H);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_glu_dwconv_swish(const void* x, const float* w, const float* bias, void* y, const int32_t* lens, int len_mul, int B, int T,
                             int C, int k, hipStream_t st) {
  hipLaunchKernelGGL(glu_dwconv_f32_kernel, dim3(grid_for((int64_t)B * T * C, 256)), dim3(256), 0, st, (const float*)x, w, bias, (float*)y,
                     lens, len_mul, B, T, C, k);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_stem_conv3d(const void* x, const void* w, const float* bias, const float* slope, void* y, int B, int T, hipStream_t st) {
  constexpr int bytes = (5 * SWIN * SCOLS + 245 * 64) * 4;   // 87 680 B
  static L2sSmemOptIn opt_in;
  if (int e = l2s_smem_opt_in(stem_f32_kernel, bytes, opt_in)) return e;
  hipLaunchKernelGGL(stem_f32_kernel, dim3(SHO / SROWS_B, B * T), dim3(256), bytes, st, (const float*)x, (const float*)w, bias, slope,
                     (float*)y, B, T);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_maxpool2d_3x3s2(const void* x, void* y, int N, int H, int W, int C, hipStream_t st) {
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  hipLaunchKernelGGL(maxpool_f32_kernel, dim3(grid_for((int64_t)N * Ho * Wo * C, 256)), dim3(256), 0, st, (const float*)x, (float*)y, N, H,
                     W, C, Ho, Wo);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_avgpool_hw(const void* x, void* y, int N, int HW, int C, hipStream_t st) {
  hipLaunchKernelGGL(avgpool_f32_kernel, dim3(grid_for((int64_t)N * C, 256)), dim3(256), 0, st, (const float*)x, (float*)y, N, HW, C);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

int l2s_f32_preprocess_frames(const uint8_t* frames, void* y, int64_t nframes, int Hin, int Win, int crop, float mean, float std,
                              hipStream_t st) {
  hipLaunchKernelGGL(preprocess_f32_kernel, dim3(grid_for(nframes * crop * crop, 256)), dim3(256), 0, st, frames, (float*)y, nframes, Hin,
                     Win, crop, mean, std);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

// row copy (rep = 1: masked copy / cast; rep = 2: the x2 time repeat) or per-clip broadcast of fp32 rows
int l2s_f32_rows(const float* x, int ldx, void* y, int ldy, int col0, const int32_t* lens, int len_mul, int64_t rows, int T, int C, int rep,
                 int bcast, hipStream_t st) {
  dim3 g(grid_for(rows * C, 256)), blk(256);
  if (bcast) hipLaunchKernelGGL(rows_f32_kernel<true>, g, blk, 0, st, x, ldx, (float*)y, ldy, col0, lens, len_mul, rows, T, C, rep);
  else hipLaunchKernelGGL(rows_f32_kernel<false>, g, blk, 0, st, x, ldx, (float*)y, ldy, col0, lens, len_mul, rows, T, C, rep);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
