// One autoregressive decoder step against a key/value cache: l2s_kv_attention, l2s_vocab_argmax,
// l2s_whisper_advance.  Everything that changes from step to step (the position, the valid cache length, "is this the first
// sampled position") is READ FROM DEVICE MEMORY, never passed by value, so a step is a fixed launch sequence that a captured
// graph can replay.  No kernel here uses an atomic, and every reduction runs in a fixed order: a clip's bytes do not depend on
// its batch mates or on the run.
//
// l2s_kv_attention - a block (16 waves) per (head, clip).  The head's 64 channels are 128 bytes of a cache row: a lane loads 16
//   bytes (8 channels), 8 consecutive lanes cover one row, a wave covers 8 keys per load instruction and the block 128; key j
//   belongs to lane group (j mod 128).  Two iterations' K and V rows (4 x 16 bytes per lane) are issued before the first is used.
//   Each 8-lane group keeps its own fp32 online softmax (running maximum, denominator, 8 output channels per lane); the 128
//   partials are merged at the end: 3 shuffle steps inside a wave, then the 16 waves in LDS in ascending order.  Rows at or past
//   the valid length are never loaded.  With k_new / v_new the block first stores its head's 2 x 128 bytes at row `pos` of the
//   caches and takes that key from the new rows themselves.  Traffic: 2 x valid x 128 bytes per (head, clip), read once.
//   16 waves, not 4: at one clip there are only H blocks, and a block's time is its count of dependent iterations (1 500 keys:
//   6 instead of 24 double iterations); at 64 clips either shape fills the chip.
//
// l2s_vocab_argmax - logits = x . E^T on v_mfma_f32_16x16x32 with E as the A operand (16 vocabulary rows per wave, 64 per
//   block) and up to 64 clips as 1, 2 or 4 B operands, both fragments loaded straight from global memory (every byte of E is
//   used once per block: an LDS round trip would buy nothing), k ascending in steps of 32.  The accumulator puts a clip on
//   lane & 15 and 4 vocabulary rows in a lane's registers, so the masked (maximum, first index, sum of exponentials) of a tile
//   needs two shuffles per clip and one LDS merge over the 4 waves.  Partials [tiles, B] go to the workspace; the finishing
//   kernel (a block per clip) merges them in a fixed order.  The [B, V] logits are written only when asked for.
//
// l2s_whisper_advance - one block: resolves the step's tokens (eot once a clip is done), books them, writes the next input row
//   of the fp32 residual stream, then one thread advances the device position and writes the count of unfinished clips.
#include "l2s_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int kHead = 64;            // channels per head (Whisper at every size)
constexpr int kMaxCacheT = 1500, kMaxWidth = 1280, kMaxVocab = 65536;
constexpr int kVTile = 64;           // vocabulary rows per block of the tile kernel
constexpr int kAttnWaves = 16;       // waves of an attention block: 8 keys each per load instruction, 128 per block

// ---- l2s_kv_attention -------------------------------------------------------------------------------------------------------------

struct Soft {        // an online-softmax partial of one lane: 8 output channels
  float m, l, acc[8];
};

__device__ __forceinline__ void soft_merge(Soft& a, const float bm, const float bl, const float (&bacc)[8]) {
  const float M = fmaxf(a.m, bm);
  const float fa = a.m == -INFINITY ? 0.f : __expf(a.m - M);
  const float fb = bm == -INFINITY ? 0.f : __expf(bm - M);
  a.l = a.l * fa + bl * fb;
#pragma unroll
  for (int c = 0; c < 8; ++c) a.acc[c] = a.acc[c] * fa + bacc[c] * fb;
  a.m = M;
}

template <typename E>
__device__ __forceinline__ void soft_step(Soft& st, const uint4 qv, const uint4 kv, const uint4 vv, const bool on, const int lane) {
  frag16 fq, fk, fv;
  fq.u = qv; fk.u = kv; fv.u = vv;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) s = fmaf(E::to_f32(fq.s[c]), E::to_f32(fk.s[c]), s);
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  if (on) {
    const float mn = fmaxf(st.m, s);
    const float sc = __expf(st.m - mn);      // st.m = -inf on the first key: exp(-inf) = 0
    const float p = __expf(s - mn);
    st.l = st.l * sc + p;
#pragma unroll
    for (int c = 0; c < 8; ++c) st.acc[c] = fmaf(p, E::to_f32(fv.s[c]), st.acc[c] * sc);
    st.m = mn;
  }
}

template <typename E>
__global__ __launch_bounds__(64 * kAttnWaves) void kv_attention_kernel(const uint16_t* __restrict__ q, const int ldq, uint16_t* kc, uint16_t* vc,
                                                           const int cache_T, const uint16_t* __restrict__ k_new,
                                                           const uint16_t* __restrict__ v_new, const int ld_new,
                                                           const int32_t* __restrict__ pos, const int pos_stride, const int n_valid,
                                                           const int H, uint16_t* __restrict__ out, const int ldo) {
  __shared__ float sPart[kAttnWaves][8][10];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.y;
  const int grp = lane >> 3, ch = (lane & 7) * 8;
  const int ld = H * kHead;
  int valid = n_valid, p = -1;
  if (pos) {
    p = pos[(int64_t)b * pos_stride];
    valid = p + 1;
  }
  valid = min(max(valid, 0), cache_T);
  const bool append = k_new && p >= 0 && p < cache_T;
  const int64_t cbase = (int64_t)b * cache_T * ld + h * kHead;
  const uint16_t* knew = k_new + (int64_t)b * ld_new + h * kHead;
  const uint16_t* vnew = v_new + (int64_t)b * ld_new + h * kHead;
  if (append && tid < 16) {                  // this head's 64 channels of the new K row (threads 0-7) and V row (8-15)
    const int c = (tid & 7) * 8;
    const uint4 v = *reinterpret_cast<const uint4*>((tid < 8 ? knew : vnew) + c);
    *reinterpret_cast<uint4*>((tid < 8 ? kc : vc) + cbase + (int64_t)p * ld + c) = v;
  }
  const uint4 qv = *reinterpret_cast<const uint4*>(q + (int64_t)b * ldq + h * kHead + ch);

  Soft st;
  st.m = -INFINITY; st.l = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) st.acc[c] = 0.f;

  const uint4 zero = make_uint4(0, 0, 0, 0);
  constexpr int KB = 8 * kAttnWaves;                              // keys the block covers per load instruction
  for (int jw = 8 * wave; jw < valid; jw += 2 * KB) {             // a wave-uniform bound: every lane takes part in the shuffles
    const int ja = jw + grp, jb = ja + KB;
    const bool ona = ja < valid, onb = jb < valid;
    uint4 ka = zero, va = zero, kb = zero, vb = zero;
    if (ona) {
      const bool nw = append && ja == p;
      ka = *reinterpret_cast<const uint4*>((nw ? knew : kc + cbase + (int64_t)ja * ld) + ch);
      va = *reinterpret_cast<const uint4*>((nw ? vnew : vc + cbase + (int64_t)ja * ld) + ch);
    }
    if (onb) {
      const bool nw = append && jb == p;
      kb = *reinterpret_cast<const uint4*>((nw ? knew : kc + cbase + (int64_t)jb * ld) + ch);
      vb = *reinterpret_cast<const uint4*>((nw ? vnew : vc + cbase + (int64_t)jb * ld) + ch);
    }
    soft_step<E>(st, qv, ka, va, ona, lane);
    soft_step<E>(st, qv, kb, vb, onb, lane);
  }
  // the 8 lane groups of a wave
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    const float om = __shfl_xor(st.m, o, 64), ol = __shfl_xor(st.l, o, 64);
    float oacc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) oacc[c] = __shfl_xor(st.acc[c], o, 64);
    // both partners must reach the same bytes: merge the lower group's partial first
    if (lane & o) {
      Soft t;
      t.m = om; t.l = ol;
#pragma unroll
      for (int c = 0; c < 8; ++c) t.acc[c] = oacc[c];
      soft_merge(t, st.m, st.l, st.acc);
      st = t;
    } else {
      soft_merge(st, om, ol, oacc);
    }
  }
  if (lane < 8) {
    sPart[wave][lane][0] = st.m;
    sPart[wave][lane][1] = st.l;
#pragma unroll
    for (int c = 0; c < 8; ++c) sPart[wave][lane][2 + c] = st.acc[c];
  }
  __syncthreads();
  if (tid < 8) {
#pragma unroll
    for (int w = 1; w < kAttnWaves; ++w) {
      float oacc[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) oacc[c] = sPart[w][tid][2 + c];
      soft_merge(st, sPart[w][tid][0], sPart[w][tid][1], oacc);
    }
    const float inv = st.l > 0.f ? 1.0f / st.l : 0.f;       // no valid key: zeros
    uint4 o;
    o.x = E::pack2(st.acc[0] * inv, st.acc[1] * inv);
    o.y = E::pack2(st.acc[2] * inv, st.acc[3] * inv);
    o.z = E::pack2(st.acc[4] * inv, st.acc[5] * inv);
    o.w = E::pack2(st.acc[6] * inv, st.acc[7] * inv);
    *reinterpret_cast<uint4*>(out + (int64_t)b * ldo + h * kHead + ch) = o;
  }
}

// ---- l2s_vocab_argmax -------------------------------------------------------------------------------------------------------------

struct Pick {        // a partial of the masked softmax: maximum, its first index, sum of exp(logit - maximum)
  float m, s;
  int i;
};

__device__ __forceinline__ Pick pick_merge(const Pick a, const Pick b) {
  const float M = fmaxf(a.m, b.m);
  Pick r;
  if (b.m > a.m || (b.m == a.m && b.i < a.i)) { r.m = b.m; r.i = b.i; } else { r.m = a.m; r.i = a.i; }
  const float sa = a.m == -INFINITY ? 0.f : a.s * __expf(a.m - M);
  const float sb = b.m == -INFINITY ? 0.f : b.s * __expf(b.m - M);
  r.s = sa + sb;
  return r;
}

template <typename E, int NB, int STEPS>
__device__ __forceinline__ void vocab_k_block(const uint16_t* __restrict__ e, const uint16_t* (&xrow)[NB], const int k0,
                                              f32x4_t (&acc)[NB]) {
  frag16 a[STEPS];
#pragma unroll
  for (int s = 0; s < STEPS; ++s) a[s].u = *reinterpret_cast<const uint4*>(e + 32 * s);
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      frag16 bb;
      bb.u = *reinterpret_cast<const uint4*>(xrow[n] + k0 + 32 * s);
      acc[n] = E::mfma(a[s], bb, acc[n]);
    }
  }
}

template <typename E, int NB>
__global__ __launch_bounds__(256) void vocab_tile_kernel(const uint16_t* __restrict__ x, const int ldx, const uint16_t* __restrict__ emb,
                                                         const int lde, const int B, const int V, const int d,
                                                         const uint8_t* __restrict__ suppress, const uint8_t* __restrict__ begin_suppress,
                                                         const int32_t* __restrict__ step, const int first_step, float* __restrict__ logits,
                                                         float* __restrict__ pm, float* __restrict__ ps, int32_t* __restrict__ pi) {
  __shared__ float sM[4][16 * NB];
  __shared__ float sS[4][16 * NB];
  __shared__ int sI[4][16 * NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int tile = blockIdx.x, b0 = blockIdx.y * (16 * NB);
  const int v0 = tile * kVTile + 16 * wave;
  const uint16_t* erow = emb + (int64_t)min(v0 + fr, V - 1) * lde + fq * 8;       // rows past V: row V - 1, discarded below
  const uint16_t* xrow[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) xrow[n] = x + (int64_t)min(b0 + 16 * n + fr, B - 1) * ldx + fq * 8;
  f32x4_t acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  // 8 k-steps' fragments of E (8 x 16 bytes per lane) are in flight before the first product; d = 64 i leaves a tail of 2 i' steps
  int k0 = 0;
  for (; k0 + 256 <= d; k0 += 256) vocab_k_block<E, NB, 8>(erow + k0, xrow, k0, acc);
  for (; k0 < d; k0 += 64) vocab_k_block<E, NB, 2>(erow + k0, xrow, k0, acc);
  // acc[n][r]: clip b0 + 16 n + fr, vocabulary row v0 + 4 fq + r
  const bool begin = begin_suppress && step && *step == first_step;
  bool ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = v0 + 4 * fq + r;
    ok[r] = v < V && !(suppress && suppress[v]) && !(begin && begin_suppress[v]);
  }
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    const int b = b0 + 16 * n + fr;
    float bm = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = v0 + 4 * fq + r;
      if (logits && v < V && b < B) logits[(int64_t)b * V + v] = acc[n][r];
      if (ok[r] && acc[n][r] > bm) { bm = acc[n][r]; bi = v; }
    }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float om = __shfl_xor(bm, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (om > bm || (om == bm && oi < bi)) { bm = om; bi = oi; }
    }
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ok[r]) s += __expf(acc[n][r] - bm);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (fq == 0) { sM[wave][16 * n + fr] = bm; sS[wave][16 * n + fr] = s; sI[wave][16 * n + fr] = bi; }
  }
  __syncthreads();
  if (tid < 16 * NB && b0 + tid < B) {
    Pick r;
    r.m = sM[0][tid]; r.s = sS[0][tid]; r.i = sI[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      Pick o;
      o.m = sM[w][tid]; o.s = sS[w][tid]; o.i = sI[w][tid];
      r = pick_merge(r, o);
    }
    const int64_t at = (int64_t)tile * B + b0 + tid;
    pm[at] = r.m; ps[at] = r.s; pi[at] = r.i;
  }
}

__global__ __launch_bounds__(256) void vocab_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                           const int32_t* __restrict__ pi, const int n_tiles, const int B,
                                                           int32_t* __restrict__ token, float* __restrict__ logprob) {
  __shared__ Pick sP[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  Pick r;
  r.m = -INFINITY; r.s = 0.f; r.i = INT_MAX;
  for (int t = tid; t < n_tiles; t += 256) {
    Pick o;
    o.m = pm[(int64_t)t * B + b]; o.s = ps[(int64_t)t * B + b]; o.i = pi[(int64_t)t * B + b];
    r = pick_merge(r, o);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Pick q;
    q.m = __shfl_xor(r.m, o, 64); q.s = __shfl_xor(r.s, o, 64); q.i = __shfl_xor(r.i, o, 64);
    r = (lane & o) ? pick_merge(q, r) : pick_merge(r, q);
  }
  if (lane == 0) sP[wave] = r;
  __syncthreads();
  if (tid == 0) {
    r = pick_merge(pick_merge(sP[0], sP[1]), pick_merge(sP[2], sP[3]));
    token[b] = r.i == INT_MAX ? -1 : r.i;                   // every id suppressed: -1 (l2s_whisper_advance reads it as eot)
    logprob[b] = r.i == INT_MAX ? -INFINITY : -logf(r.s);   // log softmax at the maximum = -log sum exp(logit - maximum)
  }
}

// ---- l2s_whisper_advance ----------------------------------------------------------------------------------------------------------

template <typename E>
__global__ __launch_bounds__(256) void whisper_advance_kernel(int32_t* token, const float* __restrict__ logprob, int32_t* __restrict__ tokens,
                                                              const int ld_tok, float* __restrict__ sum_logprob, int32_t* __restrict__ lengths,
                                                              uint8_t* __restrict__ done, const uint16_t* __restrict__ tok_emb, const int lde,
                                                              const float* __restrict__ pos_emb, const int n_ctx, float* __restrict__ x_next,
                                                              const int ldx, int32_t* pos, int32_t* __restrict__ n_active, const int B,
                                                              const int V, const int d, const int eot) {
  const int tid = threadIdx.x;
  const int p = *pos;
  int active = 0;
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + tid;
    int live = 0;
    if (b < B) {
      const bool was = done[b] != 0;
      int t = was ? eot : token[b];
      if (t < 0 || t >= V) t = eot;
      token[b] = t;
      if (p >= 0 && p < ld_tok) tokens[(int64_t)b * ld_tok + p] = t;
      if (!was) {
        sum_logprob[b] += logprob[b];
        if (t != eot) lengths[b] += 1;
      }
      const bool now = was || t == eot;
      done[b] = now ? 1 : 0;
      live = now ? 0 : 1;
    }
    active += __syncthreads_count(live);
  }
  __syncthreads();                           // every thread has read *pos, and the resolved tokens are visible to the block
  if (p + 1 >= 0 && p + 1 < n_ctx) {
    const int per = d >> 3;
    const float* pe = pos_emb + (int64_t)(p + 1) * d;
    for (int e = tid; e < B * per; e += 256) {
      const int b = e / per, c = (e - b * per) * 8;
      frag16 te;
      te.u = *reinterpret_cast<const uint4*>(tok_emb + (int64_t)token[b] * lde + c);
      const float4 p0 = *reinterpret_cast<const float4*>(pe + c), p1 = *reinterpret_cast<const float4*>(pe + c + 4);
      float4 o0, o1;
      o0.x = E::to_f32(te.s[0]) + p0.x; o0.y = E::to_f32(te.s[1]) + p0.y; o0.z = E::to_f32(te.s[2]) + p0.z; o0.w = E::to_f32(te.s[3]) + p0.w;
      o1.x = E::to_f32(te.s[4]) + p1.x; o1.y = E::to_f32(te.s[5]) + p1.y; o1.z = E::to_f32(te.s[6]) + p1.z; o1.w = E::to_f32(te.s[7]) + p1.w;
      float* xr = x_next + (int64_t)b * ldx + c;
      *reinterpret_cast<float4*>(xr) = o0;
      *reinterpret_cast<float4*>(xr + 4) = o1;
    }
  }
  if (tid == 0) {
    *pos = p + 1;
    *n_active = active;
  }
}

}  // namespace

extern "C" int l2s_kv_attention(const void* q, int ldq, void* k_cache, void* v_cache, int cache_T, const void* k_new, const void* v_new,
                                int ld_new, const int32_t* pos, int pos_stride, int n_valid, int B, int H, void* out, int ldo, int dtype,
                                void* stream) {
  if (!q || !k_cache || !v_cache || !out) return L2S_EINVAL;
  if ((k_new == nullptr) != (v_new == nullptr)) return L2S_EINVAL;
  if (k_new && !pos) return L2S_EINVAL;                     // an appended row needs the device position
  if (pos_stride != 0 && pos_stride != 1) return L2S_EINVAL;
  if (B <= 0 || H <= 0 || cache_T <= 0) return L2S_ESHAPE;
  const int W = H * kHead;
  if (ldq < W || ldo < W || (k_new && ld_new < W)) return L2S_ESHAPE;
  if (!pos && (n_valid < 0 || n_valid > cache_T)) return L2S_ESHAPE;
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if (W > kMaxWidth || cache_T > kMaxCacheT || B > 65535) return L2S_EUNSUPPORTED;
  if ((ldq & 7) || (ldo & 7) || (ld_new & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) ||
      ((uintptr_t)k_new & 15) || ((uintptr_t)v_new & 15) || ((uintptr_t)out & 15) || ((uintptr_t)pos & 3))
    return L2S_EALIGN;
  const dim3 grid((unsigned)H, (unsigned)B);
  if (dtype == L2S_F16)
    hipLaunchKernelGGL(kv_attention_kernel<ElemF16>, grid, dim3(64 * kAttnWaves), 0, (hipStream_t)stream, (const uint16_t*)q, ldq, (uint16_t*)k_cache,
                       (uint16_t*)v_cache, cache_T, (const uint16_t*)k_new, (const uint16_t*)v_new, ld_new, pos, pos_stride, n_valid, H,
                       (uint16_t*)out, ldo);
  else
    hipLaunchKernelGGL(kv_attention_kernel<ElemBF16>, grid, dim3(64 * kAttnWaves), 0, (hipStream_t)stream, (const uint16_t*)q, ldq, (uint16_t*)k_cache,
                       (uint16_t*)v_cache, cache_T, (const uint16_t*)k_new, (const uint16_t*)v_new, ld_new, pos, pos_stride, n_valid, H,
                       (uint16_t*)out, ldo);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" size_t l2s_vocab_argmax_workspace(int V, int B) {
  if (V <= 0 || V > kMaxVocab || B <= 0) return 0;
  return (size_t)((V + kVTile - 1) / kVTile) * (size_t)B * 12;
}

namespace {
template <typename E, int NB>
void launch_vocab_tiles(const dim3 grid, hipStream_t s, const void* x, int ldx, const void* emb, int lde, int B, int V, int d,
                        const uint8_t* suppress, const uint8_t* begin_suppress, const int32_t* step, int first_step, float* logits,
                        float* pm, float* ps, int32_t* pi) {
  hipLaunchKernelGGL((vocab_tile_kernel<E, NB>), grid, dim3(256), 0, s, (const uint16_t*)x, ldx, (const uint16_t*)emb, lde, B, V, d,
                     suppress, begin_suppress, step, first_step, logits, pm, ps, pi);
}
}  // namespace

extern "C" int l2s_vocab_argmax(const void* x, int ldx, const void* emb, int lde, int B, int V, int d, const uint8_t* suppress,
                                const uint8_t* begin_suppress, const int32_t* step, int first_step, void* workspace, int32_t* token,
                                float* logprob, float* logits, int dtype, void* stream) {
  if (!x || !emb || !workspace || !token || !logprob) return L2S_EINVAL;
  if (begin_suppress && !step) return L2S_EINVAL;
  if (B <= 0 || V <= 0 || d <= 0) return L2S_ESHAPE;
  if (ldx < d || lde < d) return L2S_ESHAPE;
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if (V > kMaxVocab || (d & 63) || d > kMaxWidth || B > 65535 * 16) return L2S_EUNSUPPORTED;
  if ((ldx & 7) || (lde & 7) || ((uintptr_t)x & 15) || ((uintptr_t)emb & 15) || ((uintptr_t)workspace & 3) || ((uintptr_t)token & 3) ||
      ((uintptr_t)logprob & 3) || ((uintptr_t)logits & 3) || ((uintptr_t)step & 3))
    return L2S_EALIGN;
  const int n_tiles = (V + kVTile - 1) / kVTile;
  float* pm = (float*)workspace;
  float* ps = pm + (size_t)n_tiles * B;
  int32_t* pi = (int32_t*)(ps + (size_t)n_tiles * B);
  const int NB = B <= 16 ? 1 : B <= 32 ? 2 : 4;
  const dim3 grid((unsigned)n_tiles, (unsigned)((B + 16 * NB - 1) / (16 * NB)));
  hipStream_t s = (hipStream_t)stream;
#define L2S_VT(E, N) launch_vocab_tiles<E, N>(grid, s, x, ldx, emb, lde, B, V, d, suppress, begin_suppress, step, first_step, logits, pm, ps, pi)
  if (dtype == L2S_F16) {
    if (NB == 1) L2S_VT(ElemF16, 1); else if (NB == 2) L2S_VT(ElemF16, 2); else L2S_VT(ElemF16, 4);
  } else {
    if (NB == 1) L2S_VT(ElemBF16, 1); else if (NB == 2) L2S_VT(ElemBF16, 2); else L2S_VT(ElemBF16, 4);
  }
#undef L2S_VT
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(vocab_finish_kernel, dim3((unsigned)B), dim3(256), 0, s, pm, ps, pi, n_tiles, B, token, logprob);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_whisper_advance(int32_t* token, const float* logprob, int32_t* tokens, int ld_tok, float* sum_logprob, int32_t* lengths,
                                   uint8_t* done, const void* tok_emb, int lde, const float* pos_emb, int n_ctx, float* x_next, int ldx,
                                   int32_t* pos, int32_t* n_active, int B, int V, int d, int eot, int dtype, void* stream) {
  if (!token || !logprob || !tokens || !sum_logprob || !lengths || !done || !tok_emb || !pos_emb || !x_next || !pos || !n_active)
    return L2S_EINVAL;
  if (B <= 0 || V <= 0 || d <= 0 || ld_tok <= 0 || n_ctx <= 0) return L2S_ESHAPE;
  if (eot < 0 || eot >= V) return L2S_EINVAL;
  if (lde < d || ldx < d) return L2S_ESHAPE;
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if ((d & 7) || d > kMaxWidth || V > kMaxVocab || B > 65535) return L2S_EUNSUPPORTED;
  if ((lde & 7) || (ldx & 3) || ((uintptr_t)tok_emb & 15) || ((uintptr_t)pos_emb & 15) || ((uintptr_t)x_next & 15) ||
      ((uintptr_t)token & 3) || ((uintptr_t)logprob & 3) || ((uintptr_t)tokens & 3) || ((uintptr_t)sum_logprob & 3) ||
      ((uintptr_t)lengths & 3) || ((uintptr_t)pos & 3) || ((uintptr_t)n_active & 3))
    return L2S_EALIGN;
  if (dtype == L2S_F16)
    hipLaunchKernelGGL(whisper_advance_kernel<ElemF16>, dim3(1), dim3(256), 0, (hipStream_t)stream, token, logprob, tokens, ld_tok,
                       sum_logprob, lengths, done, (const uint16_t*)tok_emb, lde, pos_emb, n_ctx, x_next, ldx, pos, n_active, B, V, d, eot);
  else
    hipLaunchKernelGGL(whisper_advance_kernel<ElemBF16>, dim3(1), dim3(256), 0, (hipStream_t)stream, token, logprob, tokens, ld_tok,
                       sum_logprob, lengths, done, (const uint16_t*)tok_emb, lde, pos_emb, n_ctx, x_next, ldx, pos, n_active, B, V, d, eot);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
