// The phase-staggered weight stream shared by the fused conv-pair kernels (respair_phase.hip: respair_phase_kernel,
// respair_final_kernel) and the fused BasicBlock kernel (basicblock_phase.hip), each piece once:
//   * LDS accessors that carry their own wait;
//   * the block -> tiles map of the pair kernels (XCD-aware or plain), also used by respair.hip;
//   * the per-lane addressing of a weight quarter's fragments (paired or plain row order);
//   * the PHASE STEP: 8 waves of 64 x 64 (MI = NI = 4), a four-slot ring of weight quarters fed by LDS-DMA, one quarter = 16 MFMAs
//     per wave between two raw barriers, the upper wave row one barrier behind the lower one (respair_phase.hip's header comment
//     describes the schedule).
// Everything is a forced-inline template: a kernel built from these pieces compiles to what it was with the text written out.
#pragma once
#include "tapgemm_common.h"

namespace l2s {

__device__ __forceinline__ void lds_write_u4(uint32_t addr, u32x4_t v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write_u2(uint32_t addr, u32x2_t v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// Reads whose results must survive a long stretch of code (the residual rows: held across the whole second convolution) carry
// their own wait: after an asm LDS read without one the compiler believes the destination is valid at once, and under
// register pressure it may spill the register BEFORE the separate s_waitcnt - the spill slot then holds the stale contents
// (seen with the last-pair epilogue: garbage in exactly the spilled (row group, block) entries).
__device__ __forceinline__ void lds_read4_u2_sync(u32x2_t (&v)[4], const uint32_t (&ad)[4]) {
  asm volatile("ds_read_b64 %0, %4\n\tds_read_b64 %1, %5\n\tds_read_b64 %2, %6\n\tds_read_b64 %3, %7\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
               : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]));
}
__device__ __forceinline__ void lds_read8_u4_sync(u32x4_t (&v)[4][2], const uint32_t (&ad)[4][2]) {
  asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %9\n\tds_read_b128 %2, %10\n\tds_read_b128 %3, %11\n\t"
               "ds_read_b128 %4, %12\n\tds_read_b128 %5, %13\n\tds_read_b128 %6, %14\n\tds_read_b128 %7, %15\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(v[0][0]), "=&v"(v[0][1]), "=&v"(v[1][0]), "=&v"(v[1][1]), "=&v"(v[2][0]), "=&v"(v[2][1]), "=&v"(v[3][0]), "=&v"(v[3][1])
               : "v"(ad[0][0]), "v"(ad[0][1]), "v"(ad[1][0]), "v"(ad[1][1]), "v"(ad[2][0]), "v"(ad[2][1]), "v"(ad[3][0]), "v"(ad[3][1]));
}
__device__ __forceinline__ void lds_read4_f4_sync(f32x4_t (&v)[4], const uint32_t (&ad)[4]) {
  asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
               : "v"(ad[0]), "v"(ad[1]), "v"(ad[2]), "v"(ad[3]));
}

// Tiles of a block.  Plain: tile blockIdx + i * gridDim.  XCD-aware: blocks b and b + 8 share an XCD (and its L2), so each XCD walks
// ONE contiguous range [xcd * per, min((xcd + 1) * per, ntiles)) of the tile list with stride gridDim / 8 from offset b / 8, and
// the blocks of an XCD work on neighbouring tiles at the same time - the halo rows two neighbours share are then fetched from
// HBM once instead of once per XCD (speed only: any order is correct).  The grid is a multiple of 8.
struct TileWalk {
  int n;                                       // tiles of this block
  int xcd_order, xcd, bx, gx, per;
  __device__ __forceinline__ TileWalk(int ntiles, int xcd_order_) : n(0), xcd_order(xcd_order_) {
    xcd = blockIdx.x & 7, bx = blockIdx.x >> 3, gx = (gridDim.x + 7) >> 3, per = (ntiles + 7) >> 3;
    if (!xcd_order) {
      n = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    } else {
      const int lo = xcd * per;
      int hi = lo + per;
      hi = hi < ntiles ? hi : ntiles;
      if (lo + bx < hi) n = (hi - lo - bx + gx - 1) / gx;
    }
  }
  __device__ __forceinline__ int tile(int i) const {
    return xcd_order ? xcd * per + bx + i * gx : (int)blockIdx.x + i * (int)gridDim.x;
  }
  // the block's i-th tile as (clip, global time of its conv row 0): a clip is cut into tiles of S output rows with `halo` rows in front
  __device__ __forceinline__ void origin(int i, int tiles_per_clip, int S, int halo, int& unit, int& g0) const {
    const int L = tile(i);
    unit = L / tiles_per_clip;
    g0 = (L - unit * tiles_per_clip) * S - halo;
  }
};

// ET: element type; Q_B: bytes of a weight quarter (32 rows x 128 B per wave column); DPW: LDS-DMA instructions per staging wave
// and quarter; PAIRED: the weight rows' order inside a quarter (tapgemm_common.h: paired_w_off).
template <typename ET, int Q_B, int DPW, bool PAIRED>
struct PhaseStream {
  static constexpr int MI = 4, NI = 4, NSLOT = 4;
  // fragments: two per-lane bases for W (A's belong to the kernel), everything else is an immediate offset.
  // W quarter, this wave column's 32 rows (4 KB).  plain order: block s, k-step ks at  s*2048 + lm*128 + ((4ks + lg) ^ (lm & 7))*16;
  // paired order (paired_w_off): row 8 (lm >> 2) + 4 s + (lm & 3), chunk (lg ^ key0) ^ 4 (ks ^ s): with c0 = lg ^ key0 the four
  // fragments sit at P, Q (ks = 1), Q + 512 (s = 1), P + 512 (s = 1, ks = 1) for P = row0 + c0*16, Q = row0 + (c0 ^ 4)*16
  uint32_t wP, wQ;
  frag16 fa[MI][2], fb[2][2];

  __device__ __forceinline__ void init(uint32_t wring, int wc, int lm, int lg) {
    const int row0 = PAIRED ? 8 * (lm >> 2) + (lm & 3) : lm;
    const int c0 = lg ^ (PAIRED ? paired_w_key(row0) : (lm & 7));
    wP = wring + (uint32_t)(wc * 4096 + row0 * 128 + (c0 << 4));
    wQ = wring + (uint32_t)(wc * 4096 + row0 * 128 + ((c0 ^ 4) << 4));
  }
  template <int SLOT>
  __device__ __forceinline__ void read_b() {
    constexpr int SO = SLOT * Q_B;
    if constexpr (PAIRED) {
      lds_read_b128<SO>(fb[0][0], wP); lds_read_b128<SO + 512>(fb[1][0], wQ);
      lds_read_b128<SO>(fb[0][1], wQ); lds_read_b128<SO + 512>(fb[1][1], wP);
    } else {
      lds_read_b128<SO>(fb[0][0], wP); lds_read_b128<SO + 2048>(fb[1][0], wP);
      lds_read_b128<SO>(fb[0][1], wQ); lds_read_b128<SO + 2048>(fb[1][1], wQ);
    }
  }
  // one phase = one quarter (ring slot SLOT, a compile-time constant): half H of the wave's 64 columns x all 64 rows x K = 64.
  // read_a(): the K-tile's 8 A fragments into fa (first half only);  stage_one(slot tag, half tag): exactly DPW LDS-DMA
  // instructions per wave of the quarter two ahead.  -DL2S_PAIR_ABL_NOREAD / _NOMFMA (diagnostic builds, timing only: the results
  // are wrong) act here, so they reach every kernel built on this step: respair_phase_kernel, respair_final_kernel and
  // basicblock_phase_kernel, whichever of their files is compiled with the flag.
  template <int H, int SLOT, typename RA, typename ST>
  __device__ __forceinline__ void step(f32x4_t (&acc)[MI][NI], RA&& read_a, ST&& stage_one) {
#ifndef L2S_PAIR_ABL_NOREAD    // no fragment reads
    read_b<SLOT>();
    if (H == 0) { __builtin_amdgcn_sched_barrier(0); read_a(); }
#endif
    stage_one(std::integral_constant<int, (SLOT + 2) & (NSLOT - 1)>{}, std::integral_constant<int, H>{});   // quarter g+2 (the same half) -> the slot of quarter g-2
    __builtin_amdgcn_sched_barrier(0);         // (the staging cursor's bookkeeping stays in front of the wait, off the MFMA path)
    wait_vmcnt<DPW>();                         // quarter g+1 (staged one phase ago) has landed: read one barrier from now
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    lds_wait();
    __builtin_amdgcn_s_setprio(1);
#ifndef L2S_PAIR_ABL_NOMFMA    // no matrix instructions
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        acc[i][2 * H + s2] = ET::mfma(fb[s2][0], fa[i][0], acc[i][2 * H + s2]);
        acc[i][2 * H + s2] = ET::mfma(fb[s2][1], fa[i][1], acc[i][2 * H + s2]);
      }
#endif
    __builtin_amdgcn_s_setprio(0);
    // nothing may sit between the last MFMA and the barrier: the partner wave of this SIMD starts its MFMAs behind it.  Without the
    // second fence hipcc hoists the next phase's address arithmetic (16 SALU / VALU instructions, ~80 cycles) above the barrier
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
};

}  // namespace l2s
