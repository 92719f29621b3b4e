// One beam-search step of the AV-HuBERT seq2seq lip reader: l2s_beam_attention, l2s_beam_select,
// l2s_beam_advance.  As in whisper_decode.hip everything that changes from step to step (the position, which half of the double
// buffers is current, the live slots, the finished clips) is READ FROM DEVICE MEMORY, so a step is a fixed launch sequence that a
// captured graph can replay.  No floating-point atomic anywhere, every reduction runs in a fixed order, and a block never reads
// another clip's data: a clip's bytes do not depend on its batch mates or on the run.
//
// l2s_beam_attention - a wave per (clip, beam slot, head), four slots of one (clip, head) per block.  A head of hd = 64 NC
//   channels is NC 128-byte chunks of a cache row: an 8-lane group owns a key, a lane loads 16 bytes (8 channels) of each chunk,
//   so a wave covers 8 keys per load instruction and every load of a group is one full 128-byte line; two keys per group are in
//   flight per iteration.  Each group keeps its own fp32 online softmax (8 NC output channels per lane: 24 registers at hd = 192);
//   the 8 partials are merged by three shuffle steps, lower group first.  There is no LDS and no barrier: the 50 x 8 x 8 queries
//   of a batch-8 step are 3 200 independent waves, and a query's keys (<= a few hundred) never need more than one wave.  The
//   beams of a clip read the same cross cache rows; the 2 x T_enc x W bytes of a clip stay in L2 between them.  Self form: key
//   t < p comes from row (b, anc[b, slot, t], t), key p from k_new itself, which the wave also stores at (b, slot, p).
//
// l2s_beam_select - a block (16 waves) per clip.  Pass 1: a wave per row computes the row's maximum and log-sum-exp (lane-strided
//   partial sums, xor butterfly).  Then every candidate (slot, token) is a 64-bit key = (order-preserving bits of its fp32 score,
//   ~flat index): all keys differ, the K-th largest is found by a radix select (8 bits per pass over a 256-bin LDS histogram of
//   INTEGER counts, ending as soon as the bucket holds exactly the candidates still needed - four passes unless scores tie at the
//   boundary), the K survivors are collected and ranked against each other.  Scores are recomputed from the logits in every pass
//   by one function, so each pass sees the same bits.
//
// l2s_beam_advance - a block per clip: thread 0 walks the K candidates (finalise eos among the first `beam`, take the first `beam`
//   others as the new slots), then the block copies token and ancestor rows into the other half of the double buffers, writes the
//   next input rows and, when the clip finishes, its hypotheses sorted by score.  A second one-block kernel advances the device
//   step and counts the unfinished clips.
#include "l2s_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int kMaxBeam = 64, kMaxWidth = 1536, kMaxVocab = 8192, kMaxK = 2 * kMaxBeam;
constexpr int kMaxLen = 32767;      // ancestor tables are int16 and hold slots; positions index rows of at most this many
constexpr int kSelThreads = 1024;

// ---- l2s_beam_attention -----------------------------------------------------------------------------------------------------------

template <int NC>
struct BSoft {       // an online-softmax partial of one lane: 8 output channels of each of the head's NC chunks
  float m, l, acc[8 * NC];
};

template <int NC>
__device__ __forceinline__ void bsoft_merge(BSoft<NC>& a, const BSoft<NC>& b) {
  const float M = fmaxf(a.m, b.m);
  const float fa = a.m == -INFINITY ? 0.f : __expf(a.m - M);
  const float fb = b.m == -INFINITY ? 0.f : __expf(b.m - M);
  a.l = a.l * fa + b.l * fb;
#pragma unroll
  for (int c = 0; c < 8 * NC; ++c) a.acc[c] = a.acc[c] * fa + b.acc[c] * fb;
  a.m = M;
}

template <typename E, int NC>
__device__ __forceinline__ void bsoft_step(BSoft<NC>& st, const uint4 (&qv)[NC], const uint4 (&kv)[NC], const uint4 (&vv)[NC], const bool on) {
  float s = 0.f;
#pragma unroll
  for (int n = 0; n < NC; ++n) {
    frag16 fq, fk;
    fq.u = qv[n]; fk.u = kv[n];
#pragma unroll
    for (int c = 0; c < 8; ++c) s = fmaf(E::to_f32(fq.s[c]), E::to_f32(fk.s[c]), s);
  }
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  if (on) {
    const float mn = fmaxf(st.m, s);
    const float sc = __expf(st.m - mn);        // st.m = -inf on the first key: exp(-inf) = 0
    const float p = __expf(s - mn);
    st.l = st.l * sc + p;
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      frag16 fv;
      fv.u = vv[n];
#pragma unroll
      for (int c = 0; c < 8; ++c) st.acc[8 * n + c] = fmaf(p, E::to_f32(fv.s[c]), st.acc[8 * n + c] * sc);
    }
    st.m = mn;
  }
}

template <typename E, int NC>
__global__ __launch_bounds__(256) void beam_attention_kernel(const uint16_t* __restrict__ q, const int ldq, uint16_t* kc, uint16_t* vc,
                                                             const int T, const uint16_t* __restrict__ k_new,
                                                             const uint16_t* __restrict__ v_new, const int ld_new,
                                                             const int16_t* __restrict__ anc, const int32_t* __restrict__ step,
                                                             const int32_t* __restrict__ enc_lens, const int32_t* __restrict__ n_live,
                                                             const uint8_t* __restrict__ finished, const int B, const int beam,
                                                             const int H, uint16_t* __restrict__ out, const int ldo) {
  constexpr int HD = 64 * NC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x, slot = blockIdx.y * 4 + wave, b = blockIdx.z;
  if (slot >= beam) return;                    // no barrier in this kernel: a wave may leave
  const int grp = lane >> 3, c8 = (lane & 7) * 8;
  const int W = H * HD;
  const int64_t row = (int64_t)b * beam + slot;
  uint16_t* orow = out + row * ldo + h * HD;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  const bool self = k_new != nullptr;
  int p = -1, valid;
  if (self) {
    p = *step;
    valid = p + 1;
  } else {
    valid = min(max(enc_lens[b], 0), T);
  }
  const bool dead = (finished && finished[b]) || (n_live && slot >= n_live[b]) || (self && (p < 0 || p >= T));
  if (dead) {
    if (grp == 0) {
#pragma unroll
      for (int n = 0; n < NC; ++n) *reinterpret_cast<uint4*>(orow + 64 * n + c8) = zero;
    }
    return;
  }
  uint4 qv[NC];
#pragma unroll
  for (int n = 0; n < NC; ++n) qv[n] = *reinterpret_cast<const uint4*>(q + row * ldq + h * HD + 64 * n + c8);
  const uint16_t *knew = nullptr, *vnew = nullptr;
  const int16_t* arow = nullptr;
  if (self) {
    knew = k_new + row * ld_new + h * HD;
    vnew = v_new + row * ld_new + h * HD;
    // the half of the ancestor double buffer that is current at step p
    arow = anc + ((int64_t)(p & 1) * B * beam + row) * T;
    if (grp < 2) {                             // group 0 stores the head's part of the new K row, group 1 of the new V row
      const uint16_t* src = grp == 0 ? knew : vnew;
      uint16_t* dst = (grp == 0 ? kc : vc) + (row * T + p) * W + h * HD;
#pragma unroll
      for (int n = 0; n < NC; ++n)
        *reinterpret_cast<uint4*>(dst + 64 * n + c8) = *reinterpret_cast<const uint4*>(src + 64 * n + c8);
    }
  }

  BSoft<NC> st;
  st.m = -INFINITY; st.l = 0.f;
#pragma unroll
  for (int c = 0; c < 8 * NC; ++c) st.acc[c] = 0.f;

  for (int j0 = 0; j0 < valid; j0 += 16) {     // a wave-uniform bound: every lane takes part in the shuffles
    const int ja = j0 + grp, jb = ja + 8;
    const bool ona = ja < valid, onb = jb < valid;
    uint4 ka[NC], va[NC], kb[NC], vb[NC];
#pragma unroll
    for (int n = 0; n < NC; ++n) ka[n] = va[n] = kb[n] = vb[n] = zero;
    if (ona) {
      const uint16_t *kr, *vr;
      if (self && ja == p) { kr = knew; vr = vnew; }
      else {
        const int64_t r = self ? ((int64_t)b * beam + min(max((int)arow[ja], 0), beam - 1)) * T + ja : (int64_t)b * T + ja;
        kr = kc + r * W + h * HD; vr = vc + r * W + h * HD;
      }
#pragma unroll
      for (int n = 0; n < NC; ++n) {
        ka[n] = *reinterpret_cast<const uint4*>(kr + 64 * n + c8);
        va[n] = *reinterpret_cast<const uint4*>(vr + 64 * n + c8);
      }
    }
    if (onb) {
      const uint16_t *kr, *vr;
      if (self && jb == p) { kr = knew; vr = vnew; }
      else {
        const int64_t r = self ? ((int64_t)b * beam + min(max((int)arow[jb], 0), beam - 1)) * T + jb : (int64_t)b * T + jb;
        kr = kc + r * W + h * HD; vr = vc + r * W + h * HD;
      }
#pragma unroll
      for (int n = 0; n < NC; ++n) {
        kb[n] = *reinterpret_cast<const uint4*>(kr + 64 * n + c8);
        vb[n] = *reinterpret_cast<const uint4*>(vr + 64 * n + c8);
      }
    }
    bsoft_step<E, NC>(st, qv, ka, va, ona);
    bsoft_step<E, NC>(st, qv, kb, vb, onb);
  }
  // the 8 lane groups of the wave; both partners must reach the same bytes: the lower group's partial is merged first
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    BSoft<NC> t;
    t.m = __shfl_xor(st.m, o, 64); t.l = __shfl_xor(st.l, o, 64);
#pragma unroll
    for (int c = 0; c < 8 * NC; ++c) t.acc[c] = __shfl_xor(st.acc[c], o, 64);
    if (lane & o) {
      bsoft_merge<NC>(t, st);
      st = t;
    } else {
      bsoft_merge<NC>(st, t);
    }
  }
  if (grp == 0) {
    const float inv = st.l > 0.f ? 1.0f / st.l : 0.f;        // no valid key: zeros
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      uint4 o;
      o.x = E::pack2(st.acc[8 * n + 0] * inv, st.acc[8 * n + 1] * inv);
      o.y = E::pack2(st.acc[8 * n + 2] * inv, st.acc[8 * n + 3] * inv);
      o.z = E::pack2(st.acc[8 * n + 4] * inv, st.acc[8 * n + 5] * inv);
      o.w = E::pack2(st.acc[8 * n + 6] * inv, st.acc[8 * n + 7] * inv);
      *reinterpret_cast<uint4*>(orow + 64 * n + c8) = o;
    }
  }
}

// ---- l2s_beam_select --------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t ord32(const float f) {   // a < b  <=>  ord32(a) < ord32(b) for non-NaN floats
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord32(const uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct SelArgs {
  const float* logits;
  int ldl, V, beam, pad, unk, eos, min_len;
  float inv_temp, unk_penalty;
};

// the score of candidate (slot, v): the same instructions in every pass
__device__ __forceinline__ float cand_score(const SelArgs& a, const float* __restrict__ lrow, const int v, const float m, const float lg,
                                            const float cum, const int st, const int max_len) {
  float lp = (lrow[v] * a.inv_temp - m) - lg;
  if (!(lp == lp)) lp = -INFINITY;
  if (v == a.pad) lp = -INFINITY;
  if (v == a.unk) lp -= a.unk_penalty;
  if (st >= max_len && v != a.eos) lp = -INFINITY;
  if (st < a.min_len && v == a.eos) lp = -INFINITY;
  return (lp + cum) + 0.0f;                    // + 0: one zero, so equal scores have equal keys
}

__global__ __launch_bounds__(kSelThreads) void beam_select_kernel(const SelArgs a, const float* __restrict__ scores, const int32_t* __restrict__ step,
                                                                  const int32_t* __restrict__ max_len, const int32_t* __restrict__ n_live,
                                                                  const uint8_t* __restrict__ finished, const int B,
                                                                  float* __restrict__ cand_score_out, int32_t* __restrict__ cand_slot,
                                                                  int32_t* __restrict__ cand_token) {
  __shared__ float sM[kMaxBeam], sLg[kMaxBeam], sCum[kMaxBeam];
  __shared__ uint32_t sHist[256];
  __shared__ unsigned long long sKeys[kMaxK];
  __shared__ unsigned long long sPrefix;
  __shared__ int sNeed, sDone, sCount;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
  if (finished && finished[b]) return;
  const int st = *step, V = a.V, beam = a.beam, K = 2 * beam;
  const int ml = max_len[b];
  int ns = st <= 0 ? 1 : min(max(n_live ? n_live[b] : beam, 1), beam);   // step 0: every slot holds the same bos, only slot 0 counts
  const float* lbase = a.logits + (int64_t)b * beam * a.ldl;
  const float* cum = scores + ((int64_t)(st & 1) * B + b) * beam;         // the current half of the score double buffer
  for (int r = wave; r < ns; r += kSelThreads / 64) {
    const float* lrow = lbase + (int64_t)r * a.ldl;
    float m = -INFINITY;
    for (int v = lane; v < V; v += 64) m = fmaxf(m, lrow[v] * a.inv_temp);
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane; v < V; v += 64) s += expf(lrow[v] * a.inv_temp - m);   // a NaN logit makes the sum, and so the row, NaN
    s = wave_sum(s);
    if (lane == 0) { sM[r] = m; sLg[r] = logf(s); sCum[r] = st <= 0 ? 0.f : cum[r]; }
  }
  if (tid == 0) { sPrefix = 0ull; sNeed = K; sDone = 0; sCount = 0; }
  __syncthreads();
  const int N = ns * V;
  unsigned long long thr = 0ull;
  for (int byte = 7; byte >= 0; --byte) {
    if (tid < 256) sHist[tid] = 0u;
    __syncthreads();
    const unsigned long long prefix = sPrefix;
    for (int e = tid; e < N; e += kSelThreads) {
      const int r = e / V, v = e - r * V;
      const float sc = cand_score(a, lbase + (int64_t)r * a.ldl, v, sM[r], sLg[r], sCum[r], st, ml);
      const unsigned long long key = ((unsigned long long)ord32(sc) << 32) | (uint32_t)(0xffffffffu - (uint32_t)e);
      if (byte == 7 || (key >> (8 * (byte + 1))) == prefix) atomicAdd(&sHist[(uint32_t)(key >> (8 * byte)) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int need = sNeed, d = 255;
      for (; d > 0; --d) {
        const int c = (int)sHist[d];
        if (c >= need) break;
        need -= c;
      }
      sNeed = need;
      sPrefix = (prefix << 8) | (unsigned long long)d;
      if ((int)sHist[d] == need || byte == 0) sDone = 1;     // the bucket holds exactly what is still needed: take all of it
    }
    __syncthreads();
    if (sDone) {
      thr = sPrefix << (8 * byte);
      break;
    }
  }
  for (int e = tid; e < N; e += kSelThreads) {
    const int r = e / V, v = e - r * V;
    const float sc = cand_score(a, lbase + (int64_t)r * a.ldl, v, sM[r], sLg[r], sCum[r], st, ml);
    const unsigned long long key = ((unsigned long long)ord32(sc) << 32) | (uint32_t)(0xffffffffu - (uint32_t)e);
    if (key >= thr) {
      const int at = atomicAdd(&sCount, 1);
      if (at < kMaxK) sKeys[at] = key;
    }
  }
  __syncthreads();
  const int got = min(sCount, K);
  if (tid < got) {
    const unsigned long long key = sKeys[tid];
    int rank = 0;
    for (int i = 0; i < got; ++i) rank += sKeys[i] > key ? 1 : 0;   // all keys differ: a permutation
    const uint32_t e = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
    const int64_t o = (int64_t)b * K + rank;
    cand_score_out[o] = unord32((uint32_t)(key >> 32));
    cand_slot[o] = (int)(e / (uint32_t)V);
    cand_token[o] = (int)(e % (uint32_t)V);
  }
}

// ---- l2s_beam_advance -------------------------------------------------------------------------------------------------------------

struct AdvArgs {
  const float* cand_score;
  const int32_t* cand_slot;
  const int32_t* cand_token;
  int32_t* tokens;       // [2, B, beam, L]
  int16_t* anc;          // [2, B, beam, L]
  float* scores;         // [2, B, beam]
  int32_t* n_live;
  uint8_t* finished;
  int32_t* parents;      // [B, beam]
  int32_t* hyp_tokens;   // [B, beam, L] in finalisation order
  int32_t* hyp_len;
  float* hyp_score;
  int32_t* nhyp;
  int32_t* out_tokens;   // [B, beam, L] best first, written when the clip finishes
  int32_t* out_len;
  float* out_score;
  const int32_t* max_len;
  const uint16_t* emb;
  const float* pos_table;
  float* x_next;
  const int32_t* step;
  int lde, ldx, B, beam, L, V, d, eos, pad, normalize;
  float lenpen, embed_scale;
};

template <typename E>
__global__ __launch_bounds__(256) void beam_advance_kernel(const AdvArgs a) {
  __shared__ int sFinR[kMaxBeam], sFinDst[kMaxBeam], sNewR[kMaxBeam], sRank[kMaxBeam];
  __shared__ float sHyp[kMaxBeam];
  __shared__ int sNfin, sNnew, sNh, sFin;
  const int tid = threadIdx.x, b = blockIdx.x;
  if (a.finished[b]) return;                   // inert: nothing of a finished clip changes
  const int st = *a.step, beam = a.beam, K = 2 * beam, L = a.L;
  if (st < 0 || st + 1 >= L) return;           // no room for another token: the host sizes L so that this never happens
  const int cur = st & 1, nxt = cur ^ 1;
  const float* cs = a.cand_score + (int64_t)b * K;
  const int32_t* cl = a.cand_slot + (int64_t)b * K;
  const int32_t* ct = a.cand_token + (int64_t)b * K;
  const int64_t half = (int64_t)a.B * beam * L;
  const int32_t* tok_cur = a.tokens + cur * half + (int64_t)b * beam * L;
  int32_t* tok_nxt = a.tokens + nxt * half + (int64_t)b * beam * L;
  const int16_t* anc_cur = a.anc + cur * half + (int64_t)b * beam * L;
  int16_t* anc_nxt = a.anc + nxt * half + (int64_t)b * beam * L;
  int32_t* hyp = a.hyp_tokens + (int64_t)b * beam * L;
  if (tid == 0) {
    int nh = a.nhyp[b], nfin = 0, nnew = 0;
    nh = min(max(nh, 0), beam);
    for (int i = 0; i < nh; ++i) sHyp[i] = a.hyp_score[(int64_t)b * beam + i];
    const float denom = a.normalize ? powf((float)(st + 1), a.lenpen) : 1.0f;
    for (int r = 0; r < K; ++r) {
      const int tk = ct[r];
      const float sc = cs[r];
      if (tk == a.eos) {
        if (r < beam && sc > -INFINITY && nh < beam) {
          sFinR[nfin] = r; sFinDst[nfin] = nh;
          sHyp[nh] = sc / denom;
          ++nfin; ++nh;
        }
      } else if (nnew < beam) {
        sNewR[nnew++] = r;
      }
    }
    const int fin = (nh >= beam || st >= a.max_len[b]) ? 1 : 0;
    if (fin) {                                  // score descending, ties in finalisation order
      for (int i = 0; i < nh; ++i) {
        int rank = 0;
        for (int k = 0; k < nh; ++k) rank += (sHyp[k] > sHyp[i] || (sHyp[k] == sHyp[i] && k < i)) ? 1 : 0;
        sRank[i] = rank;
      }
    }
    sNfin = nfin; sNnew = nnew; sNh = nh; sFin = fin;
  }
  __syncthreads();
  const int nfin = sNfin, nnew = sNnew, nh = sNh, fin = sFin;
  // finalised hypotheses: positions 1 .. st of the parent, then eos, pad behind
  for (int e = tid; e < nfin * L; e += 256) {
    const int f = e / L, t = e - f * L;
    const int parent = min(max(cl[sFinR[f]], 0), beam - 1);
    hyp[(int64_t)sFinDst[f] * L + t] = t < st ? tok_cur[(int64_t)parent * L + t + 1] : (t == st ? a.eos : a.pad);
  }
  if (tid < nfin) {
    a.hyp_len[(int64_t)b * beam + sFinDst[tid]] = st + 1;
    a.hyp_score[(int64_t)b * beam + sFinDst[tid]] = sHyp[sFinDst[tid]];
  }
  if (!fin) {
    for (int e = tid; e < nnew * L; e += 256) {
      const int j = e / L, t = e - j * L;
      const int r = sNewR[j];
      const int parent = min(max(cl[r], 0), beam - 1);
      if (t <= st) {
        tok_nxt[(int64_t)j * L + t] = tok_cur[(int64_t)parent * L + t];
        anc_nxt[(int64_t)j * L + t] = anc_cur[(int64_t)parent * L + t];
      } else if (t == st + 1) {
        tok_nxt[(int64_t)j * L + t] = ct[r];
        anc_nxt[(int64_t)j * L + t] = (int16_t)j;
      }
    }
    if (tid < nnew) {
      const int r = sNewR[tid];
      a.scores[((int64_t)nxt * a.B + b) * beam + tid] = cs[r];
      a.parents[(int64_t)b * beam + tid] = min(max(cl[r], 0), beam - 1);
    }
    // the next step's rows of the residual stream
    const int per = a.d >> 3;
    const float* pe = a.pos_table + (int64_t)(st + 1) * a.d;
    for (int e = tid; e < nnew * per; e += 256) {
      const int j = e / per, c = (e - j * per) * 8;
      const int tk = min(max(ct[sNewR[j]], 0), a.V - 1);
      frag16 te;
      te.u = *reinterpret_cast<const uint4*>(a.emb + (int64_t)tk * a.lde + c);
      float* xr = a.x_next + ((int64_t)b * beam + j) * a.ldx + c;
#pragma unroll
      for (int i = 0; i < 8; ++i) xr[i] = fmaf(a.embed_scale, E::to_f32(te.s[i]), pe[c + i]);
    }
  }
  __syncthreads();                             // the hypothesis rows written above are read below
  if (fin) {
    int32_t* out = a.out_tokens + (int64_t)b * beam * L;
    for (int e = tid; e < nh * L; e += 256) {
      const int i = e / L, t = e - i * L;
      out[(int64_t)sRank[i] * L + t] = hyp[(int64_t)i * L + t];
    }
    if (tid < nh) {
      a.out_len[(int64_t)b * beam + sRank[tid]] = tid < nh - nfin ? a.hyp_len[(int64_t)b * beam + tid] : st + 1;
      a.out_score[(int64_t)b * beam + sRank[tid]] = sHyp[tid];
    }
  }
  if (tid == 0) {
    a.nhyp[b] = nh;
    a.n_live[b] = fin ? 0 : nnew;
    if (fin) a.finished[b] = 1;
  }
}

__global__ __launch_bounds__(256) void beam_step_kernel(const uint8_t* __restrict__ finished, const int B, int32_t* step, int32_t* n_active) {
  int active = 0;
  for (int b0 = 0; b0 < B; b0 += 256) {
    const int b = b0 + threadIdx.x;
    active += __syncthreads_count(b < B && !finished[b]);
  }
  if (threadIdx.x == 0) {
    *step = *step + 1;
    *n_active = active;
  }
}

template <typename E, int NC>
void launch_beam_attention(const dim3 grid, hipStream_t s, const void* q, int ldq, void* kc, void* vc, int T, const void* k_new, const void* v_new,
                           int ld_new, const int16_t* anc, const int32_t* step, const int32_t* enc_lens, const int32_t* n_live,
                           const uint8_t* finished, int B, int beam, int H, void* out, int ldo) {
  hipLaunchKernelGGL((beam_attention_kernel<E, NC>), grid, dim3(256), 0, s, (const uint16_t*)q, ldq, (uint16_t*)kc, (uint16_t*)vc, T,
                     (const uint16_t*)k_new, (const uint16_t*)v_new, ld_new, anc, step, enc_lens, n_live, finished, B, beam, H,
                     (uint16_t*)out, ldo);
}

}  // namespace

extern "C" int l2s_beam_attention(const void* q, int ldq, void* k_cache, void* v_cache, int T, const void* k_new, const void* v_new,
                                  int ld_new, const int16_t* anc, const int32_t* step, const int32_t* enc_lens, const int32_t* n_live,
                                  const uint8_t* finished, int B, int beam, int H, int hd, void* out, int ldo, int dtype, void* stream) {
  if (!q || !k_cache || !v_cache || !out) return L2S_EINVAL;
  if ((k_new == nullptr) != (v_new == nullptr)) return L2S_EINVAL;
  if (k_new && (!anc || !step || enc_lens)) return L2S_EINVAL;        // self form: ancestors and the device position
  if (!k_new && (!enc_lens || anc)) return L2S_EINVAL;                // cross form: per-clip valid lengths
  if (B <= 0 || beam <= 0 || H <= 0 || T <= 0) return L2S_ESHAPE;
  if (hd != 64 && hd != 128 && hd != 192) return L2S_EUNSUPPORTED;
  const int W = H * hd;
  if (ldq < W || ldo < W || (k_new && ld_new < W)) return L2S_ESHAPE;
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if (W > kMaxWidth || beam > kMaxBeam || T > kMaxLen || B > 65535) return L2S_EUNSUPPORTED;
  if ((ldq & 7) || (ldo & 7) || (ld_new & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15) ||
      ((uintptr_t)k_new & 15) || ((uintptr_t)v_new & 15) || ((uintptr_t)out & 15) || ((uintptr_t)anc & 1) || ((uintptr_t)step & 3) ||
      ((uintptr_t)enc_lens & 3) || ((uintptr_t)n_live & 3))
    return L2S_EALIGN;
  const dim3 grid((unsigned)H, (unsigned)((beam + 3) / 4), (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define L2S_BA(E, N) launch_beam_attention<E, N>(grid, s, q, ldq, k_cache, v_cache, T, k_new, v_new, ld_new, anc, step, enc_lens, n_live, finished, B, beam, H, out, ldo)
  const int NC = hd / 64;
  if (dtype == L2S_F16) {
    if (NC == 1) L2S_BA(ElemF16, 1); else if (NC == 2) L2S_BA(ElemF16, 2); else L2S_BA(ElemF16, 3);
  } else {
    if (NC == 1) L2S_BA(ElemBF16, 1); else if (NC == 2) L2S_BA(ElemBF16, 2); else L2S_BA(ElemBF16, 3);
  }
#undef L2S_BA
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" size_t l2s_beam_select_workspace(int V, int beam) {
  // the selection keeps its state in LDS; the query tells a caller whether a size is served (0 = unsupported) in the form the
  // other entries use, and reserves 16 bytes so that callers can allocate what it returns
  if (beam <= 0 || beam > kMaxBeam || V > kMaxVocab || V < 2 * beam + 2) return 0;
  return 16;
}

extern "C" int l2s_beam_select(const float* logits, int ldl, const float* scores, const int32_t* step, const int32_t* max_len,
                               const int32_t* n_live, const uint8_t* finished, int B, int beam, int V, int pad, int unk, int eos,
                               int min_len, float temperature, float unk_penalty, float* cand_score, int32_t* cand_slot,
                               int32_t* cand_token, void* stream) {
  if (!logits || !scores || !step || !max_len || !cand_score || !cand_slot || !cand_token) return L2S_EINVAL;
  if (B <= 0 || beam <= 0 || V <= 0 || ldl < V) return L2S_ESHAPE;
  if (!(temperature > 0.f)) return L2S_EINVAL;
  if (eos < 0 || eos >= V) return L2S_EINVAL;
  if (l2s_beam_select_workspace(V, beam) == 0 || B > 65535) return L2S_EUNSUPPORTED;
  if (((uintptr_t)logits & 3) || ((uintptr_t)scores & 3) || ((uintptr_t)step & 3) || ((uintptr_t)max_len & 3) || ((uintptr_t)n_live & 3) ||
      ((uintptr_t)cand_score & 3) || ((uintptr_t)cand_slot & 3) || ((uintptr_t)cand_token & 3))
    return L2S_EALIGN;
  SelArgs a;
  a.logits = logits; a.ldl = ldl; a.V = V; a.beam = beam; a.pad = pad; a.unk = unk; a.eos = eos; a.min_len = min_len;
  a.inv_temp = 1.0f / temperature; a.unk_penalty = unk_penalty;
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)B), dim3(kSelThreads), 0, (hipStream_t)stream, a, scores, step, max_len, n_live, finished,
                     B, cand_score, cand_slot, cand_token);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_beam_advance(const float* cand_score, const int32_t* cand_slot, const int32_t* cand_token, int32_t* tokens, int16_t* anc,
                                float* scores, int32_t* n_live, uint8_t* finished, int32_t* parents, int32_t* hyp_tokens, int32_t* hyp_len,
                                float* hyp_score, int32_t* nhyp, int32_t* out_tokens, int32_t* out_len, float* out_score,
                                const int32_t* max_len, const void* emb, int lde, const float* pos_table, float embed_scale, float* x_next,
                                int ldx, int32_t* step, int32_t* n_active, int B, int beam, int L, int V, int d, int eos, int pad,
                                float lenpen, int normalize_scores, int dtype, void* stream) {
  if (!cand_score || !cand_slot || !cand_token || !tokens || !anc || !scores || !n_live || !finished || !parents || !hyp_tokens ||
      !hyp_len || !hyp_score || !nhyp || !out_tokens || !out_len || !out_score || !max_len || !emb || !pos_table || !x_next || !step ||
      !n_active)
    return L2S_EINVAL;
  if (B <= 0 || beam <= 0 || L < 2 || V <= 0 || d <= 0) return L2S_ESHAPE;
  if (eos < 0 || eos >= V || lde < d || ldx < d) return L2S_ESHAPE;
  if (dtype != L2S_F16 && dtype != L2S_BF16) return L2S_EUNSUPPORTED;
  if (beam > kMaxBeam || V > kMaxVocab || (d & 7) || d > kMaxWidth || L > kMaxLen || B > 65535) return L2S_EUNSUPPORTED;
  if ((lde & 7) || ((uintptr_t)emb & 15) || ((uintptr_t)pos_table & 3) || ((uintptr_t)x_next & 3) || ((uintptr_t)tokens & 3) ||
      ((uintptr_t)anc & 1) || ((uintptr_t)scores & 3) || ((uintptr_t)step & 3) || ((uintptr_t)n_active & 3))
    return L2S_EALIGN;
  AdvArgs a;
  a.cand_score = cand_score; a.cand_slot = cand_slot; a.cand_token = cand_token; a.tokens = tokens; a.anc = anc; a.scores = scores;
  a.n_live = n_live; a.finished = finished; a.parents = parents; a.hyp_tokens = hyp_tokens; a.hyp_len = hyp_len; a.hyp_score = hyp_score;
  a.nhyp = nhyp; a.out_tokens = out_tokens; a.out_len = out_len; a.out_score = out_score; a.max_len = max_len;
  a.emb = (const uint16_t*)emb; a.pos_table = pos_table; a.x_next = x_next; a.step = step; a.lde = lde; a.ldx = ldx; a.B = B; a.beam = beam;
  a.L = L; a.V = V; a.d = d; a.eos = eos; a.pad = pad; a.normalize = normalize_scores; a.lenpen = lenpen; a.embed_scale = embed_scale;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == L2S_F16)
    hipLaunchKernelGGL(beam_advance_kernel<ElemF16>, dim3((unsigned)B), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(beam_advance_kernel<ElemBF16>, dim3((unsigned)B), dim3(256), 0, s, a);
  L2S_CHECK_LAUNCH();
  hipLaunchKernelGGL(beam_step_kernel, dim3(1), dim3(256), 0, s, (const uint8_t*)finished, B, step, n_active);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
