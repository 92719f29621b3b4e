// One LSTM layer's recurrence (l2s_lstm_layer), hidden size 256, fp32 throughout: the time loop of the GE2E speaker encoder
//
//   gates[s, t] = xproj[row_off[s] + t] + h[s, t-1] . W_hh^T          (i, f, g, o; xproj already holds x W_ih^T + b_ih + b_hh)
//   c = sigmoid(f) c + sigmoid(i) tanh(g),   h = sigmoid(o) tanh(c)     from h = c = 0
//
// A workgroup (8 waves) owns a tile of 16 sequences for all T steps and never talks to another workgroup: no cooperative launch,
// no flag in global memory, nothing to wait for but its own barrier.  h of the tile lives in LDS ([16][256 + 4] floats), c in
// registers.  Wave w owns hidden units 32 w .. 32 w + 31 of ALL FOUR gates: two column tiles x four gate accumulators of
// v_mfma_f32_16x16x4_f32 (rows = sequences, columns = units) that share one lane map, so a lane ends a step holding i, f, g, o of
// the same (sequence, unit) in the same register index and the cell update needs no cross-lane traffic.  Eight independent
// chains per wave and two waves per SIMD keep the matrix pipe issued.
//
// Tile height.  The height trades W_hh traffic per flop against busy CUs: 2560 sequences are 80 workgroups at 32 rows
// (v_mfma_f32_32x32x2_f32, Tile<32>) and 160 at 16 rows.  Measured on the MI355X at S = 2560, T = 160: 6.6 ms per layer at 32,
// 4.4 ms at 16 - 16 is built; -DL2S_LSTM_TILE=32 builds the other (tools/build_variant.sh).  The height
// is a compile-time constant because the k order of a chain differs between the two instructions: a sequence's bits must not
// depend on S.
//
// Operand layouts (built once at pack time, speaker_encoder.pack_lstm_layer) make every global access of a lane one 16-byte
// load that serves all four gates: the gate axis is innermost.
//   xproj column 4 u + g,   w_hh_p[k][u][g] = W_hh[256 g + u][k].
// W_hh is 1 MiB: it cannot stay in LDS and streams from L2 every step, each wave reading only its own 128 KiB slice
// (32 units x 16 B = 512 contiguous bytes per k).  The loads of K-group j + 2 are issued before the MFMAs of group j, the first
// two groups of the next step and the next step's xproj rows before the cell update, which covers them.
//
// k order of a chain, fixed: with KI lane groups (k per instruction: 4 at 16 rows, 2 at 32) a K-group is 4 KI wide, lane group q
// holds k = 4 KI j + 4 q .. + 3 of it (one ds_read_b128 of its sequence's h row), and instruction i = 0 .. 3 of group j sums
// k = 4 KI j + 4 q + i over q ascending.  A sequence's chain reads its own LDS row and its own xproj rows only: its bits do not
// depend on its tile mates, its place in the tile, or S.
#include "l2s_common.h"
#include <math.h>

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

#ifndef L2S_LSTM_TILE
#define L2S_LSTM_TILE 16   // sequences per workgroup: 16 (v_mfma_f32_16x16x4_f32) or 32 (v_mfma_f32_32x32x2_f32); A/B: tools/build_variant.sh
#endif

constexpr int H = 256, LDH = H + 4, NWAVE = 8;

// The two tile heights differ in the matrix instruction and its lane maps only.  KI: k per instruction = lane groups; a lane group
// q reads 4 consecutive k of every K-group (one ds_read_b128), so a K-group is GK = 4 KI wide and instruction i of a group
// covers k = GK j + 4 q + i over q.  NE: accumulator registers; register e of lane group q is sequence seq(e, q).  NCT: column
// tiles of TS units that make up the wave's 32 units.
template <int TS_>
struct Tile;
template <>
struct Tile<32> {
  static constexpr int TS = 32, KI = 2, NE = 16, NCT = 1;
  typedef f32x16_t acc_t;
  static __device__ __forceinline__ int seq(int e, int q) { return 8 * (e >> 2) + 4 * q + (e & 3); }
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
template <>
struct Tile<16> {
  static constexpr int TS = 16, KI = 4, NE = 4, NCT = 2;
  typedef f32x4_t acc_t;
  static __device__ __forceinline__ int seq(int e, int q) { return 4 * q + e; }
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
};

#ifdef L2S_LSTM_FAST_ACT   // A/B only (4.0 instead of 4.4 ms per layer): v_exp_f32 / v_rcp_f32 forms, ~1 ulp each
__device__ __forceinline__ float sigmoid_f32(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_f32(float x) { return fmaf(2.0f, sigmoid_f32(2.0f * x), -1.0f); }
#else
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_f32(float x) { return tanhf(x); }
#endif

template <class Tl>
constexpr bool tile_ok = Tl::TS * Tl::KI == 64 && Tl::NE * 64 == Tl::TS * Tl::TS && Tl::NCT * Tl::TS == 32;
static_assert(tile_ok<Tile<16>> && tile_ok<Tile<32>>, "a wave is TS rows x KI lane groups, NE registers cover TS x TS, NCT tiles cover 32 units");

template <class Tl>
__global__ __launch_bounds__(64 * NWAVE, 1) void lstm_layer_kernel(const float* __restrict__ xproj, const int ldx, const int n_rows,
                                                                  const int32_t* __restrict__ row_off,
                                                                  const float4* __restrict__ w_hh_p, const int S, const int T,
                                                                  float* __restrict__ h_seq, float* __restrict__ h_last) {
  constexpr int TS = Tl::TS, KI = Tl::KI, NE = Tl::NE, NCT = Tl::NCT, GK = 4 * KI, NJ = H / GK;
  static_assert(NJ % 4 == 0, "the ring of four K-groups wraps at a step's end");
  typedef typename Tl::acc_t acc_t;
  __shared__ __attribute__((aligned(16))) float sH[TS * LDH];
  __shared__ int32_t sRow[TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & (TS - 1), lq = lane / TS;
  const int s0 = blockIdx.x * TS;
  const int u = wave * 32 + lr;                          // + TS ct: the hidden unit of this lane's accumulator column in tile ct

  for (int e = tid; e < TS * LDH; e += 64 * NWAVE) sH[e] = 0.f;
  if (tid < TS) {                                        // rows past S run on the last sequence's rows and are never stored
    const int s = min(s0 + tid, S - 1);
    sRow[tid] = min(max(row_off[s], 0), n_rows - 1);
  }
  __syncthreads();

  auto xrow = [&](int e, int t) -> const float4* {
    const int r = min(sRow[Tl::seq(e, lq)] + t, n_rows - 1);   // a row past the projection reads its last row: never out of bounds
    return reinterpret_cast<const float4*>(xproj + (int64_t)r * ldx) + u;
  };
  float4 xn[NCT][NE];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int e = 0; e < NE; ++e) xn[ct][e] = xrow(e, 0)[TS * ct];

  const float4* wl = w_hh_p + (int64_t)(4 * lq) * H + u;  // + (GK j + i) * H + TS ct: W_hh[., k = GK j + 4 lq + i], four gates
  float4 wr[4][4][NCT];                                  // ring of four K-groups, filled two groups ahead of their use
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) wr[g][i][ct] = wl[(GK * g + i) * H + TS * ct];

  float c[NCT][NE];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int e = 0; e < NE; ++e) c[ct][e] = 0.f;
  const float* arow = &sH[lr * LDH + 4 * lq];

  for (int t = 0; t < T; ++t) {
    acc_t acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        acc[ct][0][e] = xn[ct][e].x;
        acc[ct][1][e] = xn[ct][e].y;
        acc[ct][2][e] = xn[ct][e].z;
        acc[ct][3][e] = xn[ct][e].w;
      }
#pragma unroll 1   // a rolled loop of four groups: the ring slots are static, and the loads stay two groups ahead, no further
    for (int j = 0; j < NJ; j += 4) {
#pragma unroll
      for (int cur = 0; cur < 4; ++cur) {
        const int jn = (j + cur + 2) & (NJ - 1);         // the last two groups fetch groups 0 and 1 for the next step
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) wr[(cur + 2) & 3][i][ct] = wl[(GK * jn + i) * H + TS * ct];
        __builtin_amdgcn_sched_barrier(0);               // issue the loads first; the MFMAs below wait for older loads only
        const float4 a = *reinterpret_cast<const float4*>(arow + GK * (j + cur));
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            acc[ct][0] = Tl::mfma(av[i], wr[cur][i][ct].x, acc[ct][0]);
            acc[ct][1] = Tl::mfma(av[i], wr[cur][i][ct].y, acc[ct][1]);
            acc[ct][2] = Tl::mfma(av[i], wr[cur][i][ct].z, acc[ct][2]);
            acc[ct][3] = Tl::mfma(av[i], wr[cur][i][ct].w, acc[ct][3]);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (t + 1 < T) {                                     // the next step's projection rows travel under the cell update
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < NE; ++e) xn[ct][e] = xrow(e, t + 1)[TS * ct];
    }
    __syncthreads();                                     // every wave has read h[t-1]: the tile may be overwritten
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int sq = Tl::seq(e, lq), uu = u + TS * ct;
        const float ig = sigmoid_f32(acc[ct][0][e]), fg = sigmoid_f32(acc[ct][1][e]), gg = tanh_f32(acc[ct][2][e]),
                    og = sigmoid_f32(acc[ct][3][e]);
        c[ct][e] = fg * c[ct][e] + ig * gg;
        const float hv = og * tanh_f32(c[ct][e]);
        sH[sq * LDH + uu] = hv;
        const int sg = s0 + sq;
        if (sg < S) {
          if (h_seq) h_seq[((int64_t)sg * T + t) * H + uu] = hv;
          if (h_last && t == T - 1) h_last[(int64_t)sg * H + uu] = hv;
        }
      }
    __syncthreads();
  }
}

using LstmTile = Tile<L2S_LSTM_TILE>;

}  // namespace

extern "C" int l2s_lstm_layer(const float* xproj, int ldx, int64_t n_rows, const int32_t* row_off, const float* w_hh_p, int S, int T,
                              int hidden, float* h_seq, float* h_last, void* stream) {
  if (!xproj || !row_off || !w_hh_p || (!h_seq && !h_last)) return L2S_EINVAL;
  if (S <= 0 || T <= 0 || hidden <= 0 || n_rows <= 0 || ldx <= 0) return L2S_ESHAPE;
  if (hidden != H) return L2S_EUNSUPPORTED;
  if (ldx < 4 * H || n_rows < T) return L2S_ESHAPE;
  if (n_rows >= ((int64_t)1 << 31) - T || S > (1 << 30)) return L2S_EUNSUPPORTED;   // 32-bit row arithmetic in the kernel
  if ((ldx & 3) || ((uintptr_t)xproj & 15) || ((uintptr_t)w_hh_p & 15)) return L2S_EALIGN;
  if (((uintptr_t)row_off & 3) || ((uintptr_t)h_seq & 3) || ((uintptr_t)h_last & 3)) return L2S_EALIGN;
  dim3 grid((unsigned)((S + LstmTile::TS - 1) / LstmTile::TS)), blk(64 * NWAVE);
  hipLaunchKernelGGL(lstm_layer_kernel<LstmTile>, grid, blk, 0, (hipStream_t)stream, xproj, ldx, (int)n_rows, row_off,
                     reinterpret_cast<const float4*>(w_hh_p), S, T, h_seq, h_last);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
