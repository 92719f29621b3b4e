// Forward (scoring) half of the `multi_target` criterion (multi_target_lip2speech/criterion.py): label-smoothed cross-entropy and
// accuracy over the unit logits, the masked L1 / spectral-convergence sums of the mel head and the CTC negative log-likelihood of
// the text head.  No log-probability tensor is ever written: a row of logits is read once and reduced in registers.
//
// Every reduction is deterministic and a clip's results depend on that clip's rows alone: one workgroup owns one clip, waves
// and lanes take elements in a fixed pattern, partials meet through wave shuffles and an in-order LDS fold, per-clip results
// leave with ordinary vector stores (no atomics).  Elementwise arithmetic is fp32 (what the reference computes in); what is
// ACCUMULATED across lanes, rows and time steps is carried in fp64, so a clip's result is the fp32 terms' sum rounded once.
#include "l2s_common.h"

namespace {

constexpr int CE_WAVES = 8;        // unit_ce: waves per clip, wave w takes rows w, w + 8, ...
constexpr int MEL_THREADS = 256;
constexpr int CTC_MAX_S = 511;     // 2 S + 1 <= 1023 extended labels, one lane each
constexpr int MAX_V = 4096;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

struct RowStats {
  double lse;      // log sum_v exp(x_v)
  double sum;      // sum_v x_v
  int argmax;      // first index of the maximum
};

// One wave reduces one row of V fp32 logits in a single pass: per lane an online (max, sum exp) pair, the plain sum and the
// running arg-max; lanes are combined at the end.  Every lane returns the same values.
template <bool WITH_SUM_ARGMAX>
__device__ __forceinline__ RowStats row_stats(const float* __restrict__ x, int V, bool vec4, int lane) {
  float m = -INFINITY, s = 0.f, sx = 0.f, best = -INFINITY;
  int bi = 0x7fffffff;
  auto take4 = [&](float a, float b, float c, float d, int i) {
    const float m4 = fmaxf(fmaxf(a, b), fmaxf(c, d));
    if (m4 > m) {
      s *= expf(m - m4);          // exp(-inf) = 0 on the first visit
      m = m4;
    }
    s += (expf(a - m) + expf(b - m)) + (expf(c - m) + expf(d - m));
    if (WITH_SUM_ARGMAX) {
      sx += (a + b) + (c + d);
      if (a > best) { best = a; bi = i; }
      if (b > best) { best = b; bi = i + 1; }
      if (c > best) { best = c; bi = i + 2; }
      if (d > best) { best = d; bi = i + 3; }
    }
  };
  auto take1 = [&](float a, int i) {
    if (a > m) {
      s *= expf(m - a);
      m = a;
    }
    s += expf(a - m);
    if (WITH_SUM_ARGMAX) {
      sx += a;
      if (a > best) { best = a; bi = i; }
    }
  };
  if (vec4) {
    const int V4 = V >> 2;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int i = lane; i < V4; i += 64) {
      const float4 v = x4[i];
      take4(v.x, v.y, v.z, v.w, 4 * i);
    }
    for (int i = (V4 << 2) + lane; i < V; i += 64) take1(x[i], i);
  } else {
    for (int i = lane; i < V; i += 64) take1(x[i], i);
  }
  const float M = wave_max(m);
  // a lane that saw nothing has m = -inf, s = 0; M = -inf only for a row of -inf (lse = -inf, as log_softmax gives nan there)
  const double se = wave_sum_f64(m == -INFINITY ? 0.0 : (double)s * (double)expf(m - M));
  RowStats r;
  r.lse = (double)M + log(se);
  r.sum = 0.0;
  r.argmax = 0;
  if (WITH_SUM_ARGMAX) {
    r.sum = wave_sum_f64((double)sx);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    r.argmax = bi;
  }
  return r;
}

// ---- label-smoothed cross-entropy + accuracy ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CE_WAVES * 64) void unit_ce_kernel(
    const float* __restrict__ logits, int ldl, const int32_t* __restrict__ target, int ldt, const int32_t* __restrict__ lens,
    int len_mul, int T2, int V, int pad_idx, bool vec4, float* __restrict__ nll, float* __restrict__ smooth,
    int32_t* __restrict__ n_correct, int32_t* __restrict__ n_tok) {
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int rows = min(T2, ldt);
  if (lens) rows = min(rows, max(lens[b], 0) * len_mul);
  const int32_t* tg = target + (int64_t)b * ldt;
  double a_nll = 0.0, a_sm = 0.0;
  int a_ok = 0, a_n = 0;
  for (int t = wave; t < rows; t += CE_WAVES) {
    const int y = tg[t];                                   // wave-uniform
    if (y == pad_idx || y < 0 || y >= V) continue;         // a label outside the classes scores nothing (torch would raise)
    const float* x = logits + ((int64_t)b * T2 + t) * ldl;
    const RowStats r = row_stats<true>(x, V, vec4, lane);
    a_nll += r.lse - (double)x[y];                         // -lprob[target]
    a_sm += (double)V * r.lse - r.sum;                     // -sum_v lprob[v]
    a_ok += r.argmax == y;
    a_n += 1;
  }
  __shared__ double s_nll[CE_WAVES], s_sm[CE_WAVES];
  __shared__ int s_ok[CE_WAVES], s_n[CE_WAVES];
  if (lane == 0) {
    s_nll[wave] = a_nll;
    s_sm[wave] = a_sm;
    s_ok[wave] = a_ok;
    s_n[wave] = a_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double q = 0.0, u = 0.0;
    int ok = 0, n = 0;
    for (int w = 0; w < CE_WAVES; ++w) {
      q += s_nll[w];
      u += s_sm[w];
      ok += s_ok[w];
      n += s_n[w];
    }
    nll[b] = (float)q;
    smooth[b] = (float)u;
    n_correct[b] = ok;
    n_tok[b] = n;
  }
}

// ---- masked L1 / spectral-convergence sums -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(MEL_THREADS) void mel_l1_sc_kernel(
    const float* __restrict__ pred, int Tp, const float* __restrict__ targ, int Tt, const int32_t* __restrict__ lens, int len_mul,
    int crop_len, int C, bool vec4, float* __restrict__ l1, float* __restrict__ sq, float* __restrict__ tsq,
    int32_t* __restrict__ n_rows) {
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int rows = min(min(crop_len, Tp), Tt);
  if (lens) rows = min(rows, max(lens[b], 0) * len_mul);
  rows = max(rows, 0);
  // rows are C wide with no gap: the clip's counted region is one flat run of rows * C floats in either tensor
  const float* p = pred + (int64_t)b * Tp * C;
  const float* q = targ + (int64_t)b * Tt * C;
  const int n = rows * C;
  double a1 = 0.0, a2 = 0.0, a3 = 0.0;
  auto take = [&](float x, float y) {
    const float d = x - y;
    a1 += (double)fabsf(d);
    a2 += (double)d * (double)d;
    a3 += (double)y * (double)y;
  };
  if (vec4) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* q4 = reinterpret_cast<const float4*>(q);
    for (int i = tid; i < (n >> 2); i += MEL_THREADS) {
      const float4 x = p4[i], y = q4[i];
      take(x.x, y.x);
      take(x.y, y.y);
      take(x.z, y.z);
      take(x.w, y.w);
    }
  } else {
    for (int i = tid; i < n; i += MEL_THREADS) take(p[i], q[i]);
  }
  a1 = wave_sum_f64(a1);
  a2 = wave_sum_f64(a2);
  a3 = wave_sum_f64(a3);
  __shared__ double sh[3][MEL_THREADS / 64];
  if (lane == 0) {
    sh[0][wave] = a1;
    sh[1][wave] = a2;
    sh[2][wave] = a3;
  }
  __syncthreads();
  if (tid == 0) {
    double r[3];
    for (int k = 0; k < 3; ++k) {
      r[k] = 0.0;
      for (int w = 0; w < MEL_THREADS / 64; ++w) r[k] += sh[k][w];
    }
    l1[b] = (float)r[0];
    sq[b] = (float)r[1];
    tsq[b] = (float)r[2];
    n_rows[b] = rows;
  }
}

// ---- CTC ---------------------------------------------------------------------------------------------------------------------------
// Phase A, one wave per frame: log-sum-exp over the V classes, then the log-probabilities of the blank and of the clip's S labels
// go to the compact row ws[b][t][0 .. S] (0 = blank, 1 + j = label j).  A label outside [0, V) poisons the clip with NaN.
__global__ __launch_bounds__(256) void ctc_gather_kernel(
    const float* __restrict__ logits, int ldl, const int32_t* __restrict__ lens, int len_mul, int B, int L, int V, int blank,
    const int32_t* __restrict__ targets, const int32_t* __restrict__ tgt_lens, const int32_t* __restrict__ tgt_offs, int S_max,
    bool vec4, float* __restrict__ ws) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= (int64_t)B * L) return;
  const int b = (int)(row / L), t = (int)(row - (int64_t)b * L);
  const int Tb = min(lens ? max(lens[b], 0) * len_mul : L, L);
  const int S = tgt_lens[b];
  if (t >= Tb || S < 0 || S > S_max) return;
  const float* x = logits + row * ldl;
  const RowStats r = row_stats<false>(x, V, vec4, lane);
  float* out = ws + row * (S_max + 1);
  const int32_t* lab = targets + tgt_offs[b];
  for (int j = lane; j <= S; j += 64) {
    const int c = j == 0 ? blank : lab[j - 1];
    out[j] = (c >= 0 && c < V) ? (float)((double)x[c] - r.lse) : __builtin_nanf("");
  }
}

__device__ __forceinline__ double log_add3(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  if (m == -INFINITY) return -INFINITY;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// Phase B, one workgroup per clip, lane s = extended label s of blank, l_0, blank, l_1, ..., blank: the alpha recursion in log
// space, alpha double-buffered in LDS (fp64: over a thousand frames the running value reaches magnitudes whose fp32 spacing
// would dominate the result), one barrier per frame, the next frame's log-probability fetched ahead of it.
__global__ __launch_bounds__(1024) void ctc_alpha_kernel(
    const float* __restrict__ ws, const int32_t* __restrict__ lens, int len_mul, int L, const int32_t* __restrict__ targets,
    const int32_t* __restrict__ tgt_lens, const int32_t* __restrict__ tgt_offs, int S_max, float* __restrict__ nll) {
  __shared__ double alpha[2][2 * CTC_MAX_S + 2];
  const int b = blockIdx.x, s = threadIdx.x;
  const int Tb = min(lens ? max(lens[b], 0) * len_mul : L, L);
  const int S = tgt_lens[b];
  if (S < 0 || S > S_max) {                  // the caller sized the workspace for S_max labels: refuse loudly
    if (s == 0) nll[b] = __builtin_nanf("");
    return;
  }
  if (Tb <= 0) {                             // no frame: no alignment (and nothing to read)
    if (s == 0) nll[b] = 0.f;
    return;
  }
  const int E = 2 * S + 1;
  const bool live = s < E;
  const int col = (s & 1) ? 1 + (s >> 1) : 0;
  bool skip = false;                         // may alpha[s - 2] flow in: a label that differs from the previous label
  if (live && (s & 1) && s >= 3) {
    const int32_t* lab = targets + tgt_offs[b];
    skip = lab[s >> 1] != lab[(s >> 1) - 1];
  }
  const float* w = ws + (int64_t)b * L * (S_max + 1) + col;
  float lp = live ? w[0] : 0.f;
  if (live) alpha[0][s] = s < 2 ? (double)lp : -INFINITY;
  int cur = 0;
  for (int t = 1; t < Tb; ++t) {
    lp = live ? w[(int64_t)t * (S_max + 1)] : 0.f;
    __syncthreads();
    if (live) {
      const double* a = alpha[cur];
      const double v = log_add3(a[s], s >= 1 ? a[s - 1] : -INFINITY, skip ? a[s - 2] : -INFINITY);
      alpha[cur ^ 1][s] = v + (double)lp;
    }
    cur ^= 1;
  }
  __syncthreads();
  if (s == 0) {
    const double* a = alpha[cur];
    const double ll = log_add3(a[E - 1], E >= 2 ? a[E - 2] : -INFINITY, -INFINITY);
    const float v = (float)(-ll);
    nll[b] = v == INFINITY ? 0.f : v;        // zero_infinity=True
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int l2s_unit_ce(const float* logits, int ldl, const int32_t* target, int ldt, const int32_t* lens, int len_mul, int B,
                           int T2, int V, int pad_idx, int ignore_prefix, float* nll, float* smooth, int32_t* n_correct,
                           int32_t* n_tok, void* stream) {
  if (!logits || !target || !nll || !smooth || !n_correct || !n_tok) return L2S_EINVAL;
  if (B <= 0 || T2 <= 0 || V <= 0 || ldt <= 0 || ldl < V || len_mul <= 0) return L2S_ESHAPE;
  if (V > MAX_V || ignore_prefix != 0) return L2S_EUNSUPPORTED;
  if (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)nll | (uintptr_t)smooth | (uintptr_t)n_correct | (uintptr_t)n_tok) & 3)
    return L2S_EALIGN;
  const bool vec4 = aligned16(logits) && (ldl & 3) == 0;
  hipLaunchKernelGGL(unit_ce_kernel, dim3((unsigned)B), dim3(CE_WAVES * 64), 0, (hipStream_t)stream, logits, ldl, target, ldt, lens,
                     len_mul, T2, V, pad_idx, vec4, nll, smooth, n_correct, n_tok);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" int l2s_mel_l1_sc(const float* pred, int Tm_pred, const float* targ, int Tm_targ, const int32_t* lens, int len_mul, int B,
                             int n_mels, int crop_len, float* l1, float* sq, float* tsq, int32_t* n_rows, void* stream) {
  if (!pred || !targ || !l1 || !sq || !tsq || !n_rows) return L2S_EINVAL;
  if (B <= 0 || Tm_pred <= 0 || Tm_targ <= 0 || n_mels <= 0 || len_mul <= 0 || crop_len < 0) return L2S_ESHAPE;
  if ((int64_t)min(Tm_pred, Tm_targ) * n_mels >= (1ll << 31)) return L2S_EUNSUPPORTED;    // a clip's run is indexed in 32 bits
  if (((uintptr_t)pred | (uintptr_t)targ | (uintptr_t)l1 | (uintptr_t)sq | (uintptr_t)tsq | (uintptr_t)n_rows) & 3) return L2S_EALIGN;
  // float4 loads need every clip's run to start on 16 bytes in both tensors
  const bool vec4 = aligned16(pred) && aligned16(targ) && (n_mels & 3) == 0;
  hipLaunchKernelGGL(mel_l1_sc_kernel, dim3((unsigned)B), dim3(MEL_THREADS), 0, (hipStream_t)stream, pred, Tm_pred, targ, Tm_targ,
                     lens, len_mul, crop_len, n_mels, vec4, l1, sq, tsq, n_rows);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}

extern "C" size_t l2s_ctc_loss_workspace(int B, int L, int S_max) {
  if (B <= 0 || L <= 0 || S_max < 0 || S_max > CTC_MAX_S) return 0;
  return (size_t)B * (size_t)L * (size_t)(S_max + 1) * sizeof(float);
}

extern "C" int l2s_ctc_loss(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int L, int V, int blank,
                            const int32_t* targets, const int32_t* tgt_lens, const int32_t* tgt_offs, int S_max, void* workspace,
                            size_t workspace_bytes, float* nll, void* stream) {
  if (!logits || !tgt_lens || !tgt_offs || !workspace || !nll) return L2S_EINVAL;
  if (!targets && S_max > 0) return L2S_EINVAL;
  if (B <= 0 || L <= 0 || V <= 0 || ldl < V || len_mul <= 0 || S_max < 0 || blank < 0 || blank >= V) return L2S_ESHAPE;
  if (V > MAX_V || S_max > CTC_MAX_S) return L2S_EUNSUPPORTED;
  if ((int64_t)B * L > (int64_t)0x7fffffff * 4) return L2S_EUNSUPPORTED;
  const size_t need = l2s_ctc_loss_workspace(B, L, S_max);
  if (need == 0 || workspace_bytes < need) return L2S_ESHAPE;
  if (((uintptr_t)logits | (uintptr_t)workspace | (uintptr_t)nll | (uintptr_t)tgt_lens | (uintptr_t)tgt_offs | (uintptr_t)targets) & 3)
    return L2S_EALIGN;
  const bool vec4 = aligned16(logits) && (ldl & 3) == 0;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)(((int64_t)B * L + 3) / 4);
  hipLaunchKernelGGL(ctc_gather_kernel, dim3(blocks), dim3(256), 0, st, logits, ldl, lens, len_mul, B, L, V, blank, targets, tgt_lens,
                     tgt_offs, S_max, vec4, (float*)workspace);
  L2S_CHECK_LAUNCH();
  const int threads = max(64, (2 * S_max + 1 + 63) / 64 * 64);
  hipLaunchKernelGGL(ctc_alpha_kernel, dim3((unsigned)B), dim3(threads), 0, st, (const float*)workspace, lens, len_mul, L, targets,
                     tgt_lens, tgt_offs, S_max, nll);
  L2S_CHECK_LAUNCH();
  return L2S_OK;
}
