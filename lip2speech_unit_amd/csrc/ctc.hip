// CTC text decoding of the text-supervised conformer (TEXT_SUPERVISION=1).
// multi_target_lip2speech/sequence_generator.py:141-171 takes softmax(encoder_out_text) and either the framewise argmax
// or ctcdecode's CTCBeamDecoder (beam_width 30, cutoff_top_n 40, cutoff_prob 1, blank 0, no LM, probabilities in).
//  * l2s_ctc_frames: one wavefront per frame - fp32 softmax, framewise argmax, the frame's top-K classes with log(p + FLT_MIN)
//    (ctcdecode get_pruned_log_probs).
//  * l2s_ctc_beam_search: ctcdecode's DecoderState::next / PathTrie restated, one workgroup per clip, serial over frames.
//    Prefix identity is the trie's: a per-clip hash (parent node, char) -> node in the workspace, nodes never deleted, so a
//    pruned prefix that comes back merges into whatever beam later extends the same string (PathTrie::get_path_trie).
#include <float.h>
#include "l2s_common.h"

namespace {

constexpr int kCtcMaxV = 4096;      // class ids fit the LDS rank map and the 13-bit character field of a sort key
constexpr int kCtcMaxBeam = 64;
constexpr int kCtcMaxK = 64;
constexpr int kCtcThreads = 256;
constexpr int kCtcMaxCand = kCtcMaxBeam * (kCtcMaxK + 1);   // per beam member: itself + one extension per top-K class
constexpr unsigned long long kEmpty = ~0ull;

// p = softmax(x) per frame; argmax (ties -> first index) and the top-K (p descending, ties -> smaller index)
__global__ __launch_bounds__(256) void ctc_frames_kernel(const float* __restrict__ logits, int ldl,
                                                         const int32_t* __restrict__ lens, int len_mul, int L, int V,
                                                         int K, int32_t* __restrict__ labels,
                                                         int32_t* __restrict__ topk_cls, float* __restrict__ topk_lp) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x * 4 + wave;
  if (t >= L) return;
  int Lb = lens ? lens[b] * len_mul : L;
  Lb = Lb < L ? Lb : L;
  const int64_t fr = (int64_t)b * L + t;
  if (t >= Lb) {   // padded frame: label 0, no candidates
    if (lane == 0) labels[fr] = 0;
    if (lane < K) {
      topk_cls[fr * K + lane] = 0;
      topk_lp[fr * K + lane] = -FLT_MAX;
    }
    return;
  }
  const float* row = logits + fr * ldl;
  float p[kCtcMaxV / 64];
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < kCtcMaxV / 64; ++r) {
    const int v = lane + 64 * r;
    p[r] = v < V ? row[v] : -INFINITY;
    mx = fmaxf(mx, p[r]);
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int r = 0; r < kCtcMaxV / 64; ++r) {
    p[r] = lane + 64 * r < V ? expf(p[r] - mx) : 0.f;
    se += p[r];
  }
  se = wave_sum(se);
  // local best of this lane; a taken or out-of-range class is -1 (below every probability)
  float bv = -1.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int r = 0; r < kCtcMaxV / 64; ++r) {
    p[r] = lane + 64 * r < V ? p[r] / se : -1.f;
    if (p[r] > bv) { bv = p[r]; bi = lane + 64 * r; }
  }
  const int rounds = K > 0 ? K : 1;
  int my_cls = 0;
  float my_p = 0.f;
  for (int k = 0; k < rounds; ++k) {
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (ov > wv || (ov == wv && oi < wi)) { wv = ov; wi = oi; }
    }
    if (k == 0 && lane == 0) labels[fr] = wi;
    if (lane == k) { my_cls = wi; my_p = wv; }
    if ((wi & 63) == lane) {   // the winner's lane drops it and rescans its own classes
      bv = -1.f;
      bi = 0x7fffffff;
#pragma unroll
      for (int r = 0; r < kCtcMaxV / 64; ++r) {
        if (lane + 64 * r == wi) p[r] = -1.f;
        if (p[r] > bv) { bv = p[r]; bi = lane + 64 * r; }
      }
    }
  }
  if (lane < K) {
    topk_cls[fr * K + lane] = my_cls;
    topk_lp[fr * K + lane] = logf(my_p + FLT_MIN);
  }
}

// REPEAT_TEXT_LABELS (multi_input_vocoder/dataset_multi_input.py:23-38 `repeat`): y[t] = x[j] for the last j <= t with
// x[j] != 0, else 0 (the fill is seeded with label 0); frames t >= lens[b]*len_mul get 0.  One wave per clip, 64 frames a
// round: an inclusive scan with `a o b = b != 0 ? b : a` (associative), carried across rounds.  In place is allowed.
__global__ __launch_bounds__(64) void ctc_repeat_kernel(const int32_t* x, int ldx, const int32_t* __restrict__ lens,
                                                        int len_mul, int L, int32_t* y, int ldy) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int Lb = lens ? lens[b] * len_mul : L;
  Lb = Lb < L ? Lb : L;
  int carry = 0;
  for (int t0 = 0; t0 < L; t0 += 64) {
    const int t = t0 + lane;
    int v = t < Lb ? x[(int64_t)b * ldx + t] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o && v == 0) v = u;
    }
    if (v == 0) v = carry;
    carry = __shfl(v, 63, 64);
    if (t < L) y[(int64_t)b * ldy + t] = t < Lb ? v : 0;
  }
}

// ctcdecode's log_sum_exp: -FLT_MAX is its minus infinity
__device__ __forceinline__ float ctc_lse(float x, float y) {
  if (x <= -FLT_MAX) return y;
  if (y <= -FLT_MAX) return x;
  const float m = fmaxf(x, y);
  return logf(expf(x - m) + expf(y - m)) + m;
}

// Sort key of a candidate, larger = better: prefix_compare (score descending, then the smaller last character; the root's
// character is -1) and, where ctcdecode's nth_element leaves the order unspecified, the smaller slot.  0 = no candidate.
__device__ __forceinline__ unsigned long long ctc_key(float score, int ch, int slot) {
  uint32_t u = __float_as_uint(score);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const uint32_t lo = ((8191u - (uint32_t)(ch + 1)) << 13) | (8191u - (uint32_t)slot);
  return ((unsigned long long)u << 32) | lo;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
  const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ uint32_t ctc_hash(uint32_t k) { return k * 2654435761u; }

struct CtcBeam {   // beam state, double buffered across the step
  int node[2][kCtcMaxBeam], par[2][kCtcMaxBeam], chr[2][kCtcMaxBeam], dep[2][kCtcMaxBeam];
  float bp[2][kCtcMaxBeam], nbp[2][kCtcMaxBeam], sc[2][kCtcMaxBeam];
};

// One workgroup per clip.  Per frame (DecoderState::next without a scorer): every beam member p and every top-K class c
//   c == blank            : b(p)  += lp_c + score(p)
//   c == last(p)          : nb(p) += lp_c + nb_prev(p);  child p+c gets lp_c + b_prev(p) (only if b_prev(p) > -FLT_MAX)
//   otherwise             : child p+c gets lp_c + score(p)
// (+= is log_sum_exp).  A child that is itself a beam member is merged into it; every other child is a candidate with fresh
// masses.  The best `beam` of the beam members and the children survive (one radix select over the keys, then a 64-lane
// sort of the survivors).  Every accumulation has at most two terms, and two-term log_sum_exp is symmetric, so the
// result does not depend on ctcdecode's (unspecified) prefix order.
__global__ __launch_bounds__(kCtcThreads) void ctc_beam_kernel(const int32_t* __restrict__ topk_cls,
                                                               const float* __restrict__ topk_lp,
                                                               const int32_t* __restrict__ lens, int len_mul, int L,
                                                               int K, int beam, int nbest, unsigned long long* ws_hash,
                                                               int hash_cap, size_t clip_words,
                                                               int32_t* __restrict__ out_labels,
                                                               int32_t* __restrict__ out_len, float* __restrict__ out_score) {
  __shared__ unsigned long long keys[kCtcMaxCand];
  __shared__ unsigned long long sel[kCtcMaxBeam];
  __shared__ unsigned long long mmask[kCtcMaxBeam];   // bit k: the child (member i, k-th class) merged into a member
  __shared__ CtcBeam bs;
  __shared__ float bcur[kCtcMaxBeam], nbcur[kCtcMaxBeam];
  __shared__ int tk_cls[kCtcMaxK];
  __shared__ float tk_lp[kCtcMaxK];
  __shared__ int hist[256];
  __shared__ int ctl[8];
  __shared__ int8_t rank_of[kCtcMaxV];   // class -> top-K rank of the current frame, -1 if absent

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int Lb = lens ? lens[b] * len_mul : L;
  Lb = Lb < L ? Lb : L;
  unsigned long long* tab = ws_hash + (size_t)b * clip_words;
  int2* nodes = (int2*)(tab + hash_cap);
  for (int i = tid; i < hash_cap; i += kCtcThreads) tab[i] = kEmpty;
  for (int i = tid; i < kCtcMaxV; i += kCtcThreads) rank_of[i] = -1;
  hist[tid] = 0;
  if (tid == 0) {   // the root: empty prefix, b = 0, nb = -FLT_MAX
    bs.node[0][0] = 0; bs.par[0][0] = -1; bs.chr[0][0] = -1; bs.dep[0][0] = 0;
    bs.bp[0][0] = 0.f; bs.nbp[0][0] = -FLT_MAX; bs.sc[0][0] = 0.f;
  }
  __threadfence();   // the table is cleared in L2 before any atomic below touches it
  __syncthreads();

  const int K1 = K + 1;
  int nb = 1, cb = 0;
  int pf_cls = 0, old_cls = 0;
  float pf_lp = 0.f;
  if (tid < K && Lb > 0) {
    pf_cls = topk_cls[(size_t)b * L * K + tid];
    pf_lp = topk_lp[(size_t)b * L * K + tid];
  }
  for (int t = 0; t < Lb; ++t) {
    // A: this frame's candidates classes, rank map, counters; prefetch the next frame
    if (tid < K) {
      pf_cls = (uint32_t)pf_cls < (uint32_t)kCtcMaxV ? pf_cls : 0;   // l2s_ctc_frames writes ids < V <= kCtcMaxV
      tk_cls[tid] = pf_cls;
      tk_lp[tid] = pf_lp;
      rank_of[pf_cls] = (int8_t)tid;
      old_cls = pf_cls;
      if (t + 1 < Lb) {
        pf_cls = topk_cls[((size_t)b * L + t + 1) * K + tid];
        pf_lp = topk_lp[((size_t)b * L + t + 1) * K + tid];
      }
    }
    if (tid < kCtcMaxBeam) mmask[tid] = 0;
    if (tid < 8) ctl[tid] = 0;
    __syncthreads();
    // B: each member's own masses, and the merge of its parent's extension into it
    if (tid < nb) {
      const int j = tid;
      const float scj = bs.sc[cb][j];
      const int kb = rank_of[0];
      const int cj = bs.chr[cb][j];
      const int kc = cj >= 0 ? rank_of[cj] : -1;
      const float bcv = kb >= 0 ? tk_lp[kb] + scj : -FLT_MAX;
      float nbv = -FLT_MAX;
      if (kc >= 0) {
        nbv = ctc_lse(nbv, tk_lp[kc] + bs.nbp[cb][j]);
        const int pn = bs.par[cb][j];
        int pi = -1;
        for (int i = 0; i < nb; ++i)
          if (bs.node[cb][i] == pn) pi = i;
        if (pi >= 0) {
          const float lp = tk_lp[kc];
          float lpx;
          if (cj == bs.chr[cb][pi]) lpx = bs.bp[cb][pi] > -FLT_MAX ? lp + bs.bp[cb][pi] : -FLT_MAX;
          else lpx = lp + bs.sc[cb][pi];
          nbv = ctc_lse(nbv, lpx);
          atomicOr(&mmask[pi], 1ull << kc);
        }
      }
      bcur[j] = bcv;
      nbcur[j] = nbv;
    }
    __syncthreads();
    // C: keys of every candidate
    if (tid < K) rank_of[old_cls] = -1;   // read for the last time in B
    const int nslot = nb * K1;
    int nvalid = 0;
    for (int s = tid; s < nslot; s += kCtcThreads) {
      const int i = s / K1, r = s - i * K1;
      unsigned long long key = 0;
      if (r == 0) {
        key = ctc_key(ctc_lse(bcur[i], nbcur[i]), bs.chr[cb][i], s);
      } else {
        const int k = r - 1, c = tk_cls[k];
        if (c != 0 && !((mmask[i] >> k) & 1)) {
          const float lp = tk_lp[k];
          float lpx;
          if (c == bs.chr[cb][i]) lpx = bs.bp[cb][i] > -FLT_MAX ? lp + bs.bp[cb][i] : -FLT_MAX;
          else lpx = lp + bs.sc[cb][i];
          key = ctc_key(lpx, c, s);   // score = log_sum_exp(-FLT_MAX, nb) = nb
        }
      }
      keys[s] = key;
      nvalid += key != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nvalid += __shfl_xor(nvalid, o, 64);
    if (lane == 0) atomicAdd(&ctl[0], nvalid);
    __syncthreads();
    nvalid = ctl[0];
    const int nsel = nvalid < beam ? nvalid : beam;
    // D: threshold = key of the beam-th best candidate (MSB-first radix select, 8 bits a pass, stops once the bin that
    // holds it is taken whole)
    unsigned long long thr = 1;
    if (nvalid > beam) {
      unsigned long long prefix = 0;
      int need = beam;
      for (int shift = 56; shift >= 0; shift -= 8) {
        for (int s = tid; s < nslot; s += kCtcThreads) {
          const unsigned long long key = keys[s];
          if (key != 0 && (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))))
            atomicAdd(&hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (wave == 0) {   // lane l holds bins 255-4l .. 252-4l: an inclusive scan from the top bin down
          int h[4], tot = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            h[q] = hist[255 - 4 * lane - q];
            hist[255 - 4 * lane - q] = 0;
            tot += h[q];
          }
          int inc = tot;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (lane >= o) inc += v;
          }
          int run = inc - tot;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (run < need && run + h[q] >= need) {
              ctl[1] = 255 - 4 * lane - q;
              ctl[2] = need - run;
              ctl[3] = h[q];
            }
            run += h[q];
          }
        }
        __syncthreads();
        const int d = ctl[1], cnt = ctl[3];
        need = ctl[2];
        prefix |= (unsigned long long)d << shift;
        if (cnt == need) break;
        __syncthreads();   // ctl is rewritten by the next pass
      }
      thr = prefix;
    }
    // E: compact the survivors
    for (int s = tid; s < nslot; s += kCtcThreads) {
      const unsigned long long key = keys[s];
      if (key != 0 && key >= thr) {
        const int pos = atomicAdd(&ctl[4], 1);
        if (pos < kCtcMaxBeam) sel[pos] = key;
      }
    }
    __syncthreads();
    // F: sort them (64-lane bitonic, descending), commit their trie nodes, write the next beam
    if (wave == 0) {
      unsigned long long v = lane < nsel ? sel[lane] : 0ull;
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const unsigned long long o = shfl_xor_u64(v, j);
          const bool keep_max = ((lane & j) == 0) == ((lane & k) == 0);
          v = keep_max ? (v > o ? v : o) : (v < o ? v : o);
        }
      }
      if (lane < nsel) {
        const int s = 8191 - (int)(v & 8191u);
        const int i = s / K1, r = s - i * K1;
        const int nx = cb ^ 1;
        float bv, nbv;
        int node, par, ch, dep;
        if (r == 0) {
          node = bs.node[cb][i]; par = bs.par[cb][i]; ch = bs.chr[cb][i]; dep = bs.dep[cb][i];
          bv = bcur[i]; nbv = nbcur[i];
        } else {
          const int k = r - 1;
          ch = tk_cls[k];
          par = bs.node[cb][i];
          dep = bs.dep[cb][i] + 1;
          const float lp = tk_lp[k];
          if (ch == bs.chr[cb][i]) nbv = bs.bp[cb][i] > -FLT_MAX ? lp + bs.bp[cb][i] : -FLT_MAX;
          else nbv = lp + bs.sc[cb][i];
          bv = -FLT_MAX;
          // get_path_trie: the node of (parent, ch) if it was ever made, else a new one (id = 1 + t*beam + lane)
          const uint32_t hk = (uint32_t)par * 8192u + (uint32_t)ch;
          const int fresh = 1 + t * beam + lane;
          const unsigned long long want = ((unsigned long long)hk << 32) | (uint32_t)fresh;
          uint32_t pos = ctc_hash(hk) & (uint32_t)(hash_cap - 1);
          while (true) {
            const unsigned long long old = atomicCAS(&tab[pos], kEmpty, want);
            if (old == kEmpty) {
              node = fresh;
              nodes[fresh] = make_int2(par, ch);
              break;
            }
            if ((uint32_t)(old >> 32) == hk) {
              node = (int)(uint32_t)old;
              break;
            }
            pos = (pos + 1) & (uint32_t)(hash_cap - 1);
          }
        }
        bs.node[nx][lane] = node; bs.par[nx][lane] = par; bs.chr[nx][lane] = ch; bs.dep[nx][lane] = dep;
        bs.bp[nx][lane] = bv; bs.nbp[nx][lane] = nbv; bs.sc[nx][lane] = ctc_lse(bv, nbv);
      }
    }
    __syncthreads();
    nb = nsel;
    cb ^= 1;
  }
  // the surviving prefixes, best first; beams that do not exist get length 0 and score FLT_MAX
  __threadfence();
  if (wave == 0 && lane < nbest) {
    int32_t* lab = out_labels + ((size_t)b * nbest + lane) * L;
    int n = 0;
    float score = FLT_MAX;
    if (lane < nb) {
      n = bs.dep[cb][lane];
      int node = bs.node[cb][lane];
      for (int q = n - 1; q >= 0; --q) {
        const int2 e = nodes[node];
        lab[q] = e.y;
        node = e.x;
      }
      score = -bs.sc[cb][lane];
    }
    for (int q = n; q < L; ++q) lab[q] = 0;
    out_len[(size_t)b * nbest + lane] = n;
    out_score[(size_t)b * nbest + lane] = score;
  }
}

int ctc_hash_cap(int L, int beam) {
  const size_t need = 2 * ((size_t)beam * L + 1);
  size_t cap = 64;
  while (cap < need) cap <<= 1;
  return (int)cap;
}

size_t ctc_clip_words(int L, int beam) {   // 8-byte words per clip: hash table, then the node pool
  return (size_t)ctc_hash_cap(L, beam) + (size_t)beam * L + 1;
}

}  // namespace

extern "C" size_t l2s_ctc_beam_workspace(int B, int L, int beam) {
  if (B <= 0 || L <= 0 || beam <= 0 || beam > kCtcMaxBeam || (size_t)beam * L + 1 >= (1u << 19)) return 0;
  return (size_t)B * ctc_clip_words(L, beam) * sizeof(unsigned long long);
}

extern "C" int l2s_ctc_frames(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int L, int V, int K,
                              int32_t* labels, int32_t* topk_cls, float* topk_lp, void* stream) {
  if (!logits || !labels || (K > 0 && (!topk_cls || !topk_lp))) return L2S_EINVAL;
  if (B <= 0 || L <= 0 || V < 2 || ldl < V || K < 0 || K > V) return L2S_ESHAPE;
  if (V > kCtcMaxV || K > kCtcMaxK) return L2S_EUNSUPPORTED;
  if (lens && len_mul <= 0) return L2S_EINVAL;
  hipLaunchKernelGGL(ctc_frames_kernel, dim3((L + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, logits, ldl, lens, len_mul,
                     L, V, K, labels, topk_cls, topk_lp);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_ctc_beam_search(const int32_t* topk_cls, const float* topk_lp, const int32_t* lens, int len_mul, int B,
                                   int L, int K, int beam, int nbest, void* workspace, size_t workspace_bytes,
                                   int32_t* labels, int32_t* lengths, float* scores, void* stream) {
  if (!topk_cls || !topk_lp || !workspace || !labels || !lengths || !scores) return L2S_EINVAL;
  if (B <= 0 || L <= 0 || K < 1 || beam < 1 || nbest < 1 || nbest > beam) return L2S_ESHAPE;
  if (K > kCtcMaxK || beam > kCtcMaxBeam) return L2S_EUNSUPPORTED;
  if (lens && len_mul <= 0) return L2S_EINVAL;
  const size_t need = l2s_ctc_beam_workspace(B, L, beam);
  if (need == 0) return L2S_EUNSUPPORTED;
  if (workspace_bytes < need || ((uintptr_t)workspace & 7)) return L2S_ESHAPE;
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(kCtcThreads), 0, (hipStream_t)stream, topk_cls, topk_lp, lens, len_mul,
                     L, K, beam, nbest, (unsigned long long*)workspace, ctc_hash_cap(L, beam),
                     ctc_clip_words(L, beam), labels, lengths, scores);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_ctc_repeat_labels(const int32_t* x, int ldx, const int32_t* lens, int len_mul, int B, int L, int32_t* y,
                                     int ldy, void* stream) {
  if (!x || !y) return L2S_EINVAL;
  if (B <= 0 || L <= 0 || ldx < L || ldy < L) return L2S_ESHAPE;
  if (lens && len_mul <= 0) return L2S_EINVAL;
  hipLaunchKernelGGL(ctc_repeat_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, x, ldx, lens, len_mul, L, y, ldy);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
