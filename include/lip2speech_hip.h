/*
 * lip2speech_hip.h — C ABI of liblip2speech_hip.so (gfx950 / MI355X only).
 *
 * Drop-in boundary for the lip->speech inference hot path of
 * DomhnallBoyle/lip2speech-unit.  The reference has no FFI of its own (every op
 * is a torch.nn call); each entry point below names the reference call site(s)
 * (path:line relative to the reference repo) whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *    the comment says host; `stream` is a hipStream_t passed as void*.
 *  - nothing allocates, frees or synchronises: all calls are asynchronous on
 *    `stream` and are safe to capture into a hipGraph.
 *  - activations are channels-last ("rows x channels"): row = (clip, time) or
 *    (frame, y, x); 16-bit storage (fp16 or bf16 selected by `dtype`), fp32
 *    accumulation; the fp32 residual stream of the transformers is fp32.
 *  - return value: 0 on success, negative L2S_E* on a rejected argument
 *    (nothing launched), positive = hipError_t of a failed launch.
 */
#ifndef LIP2SPEECH_HIP_H
#define LIP2SPEECH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2S_ABI_VERSION 16

/* element type of the operands: fp16 / bf16 storage with fp32 accumulation, or L2S_F32 (ABI 16) = the reference's default
 * precision: operands, activations and accumulation all fp32.  With L2S_F32 every pointer documented as "16-bit" below is an
 * fp32 pointer (leading dimensions stay in elements) and L2S_F_OUT_F32 / L2S_F_RES_F32 / x_is_f32 / y_is_f32 / v_is_f32 are
 * implied.  Served in fp32: l2s_tapgemm (all modes, activations and flags; no ktab), l2s_attention, l2s_layernorm,
 * l2s_glu_dwconv_swish, l2s_stem_conv3d, l2s_maxpool2d_3x3s2, l2s_avgpool_hw, l2s_preprocess_frames, l2s_repeat2_cast,
 * l2s_broadcast_rows, l2s_rows_f32_to_16_masked and the two casts (plain copies).  The fused / resident forms
 * (l2s_stem_pool_fused*, l2s_basicblock_fused, l2s_basiclayer_fused, l2s_basicstage128_tail_fused,
 * l2s_splitk_reduce_layernorm, a ktab descriptor) and the vocoder kernels answer L2S_EUNSUPPORTED or L2S_EINVAL.
 * fp32 epilogues use erff / expf / tanhf and IEEE division: only the summation order separates them from an fp32 reference. */
enum { L2S_F16 = 0, L2S_BF16 = 1, L2S_F32 = 2 };

/* error codes */
enum { L2S_OK = 0, L2S_EINVAL = -1, L2S_ESHAPE = -2, L2S_EALIGN = -3, L2S_EUNSUPPORTED = -4 };

/* epilogue activations */
enum {
  L2S_ACT_NONE = 0,
  L2S_ACT_RELU = 1,   /* espnet positionwise_feed_forward.py:30 */
  L2S_ACT_GELU = 2,   /* erf GELU: fairseq gelu, model_avhubert.py:234, models_multi_input.py:41 */
  L2S_ACT_SWISH = 3,  /* espnet convolution.py:68-73 */
  L2S_ACT_PRELU = 4,  /* per-channel slope, avhubert/resnet.py:47-48 */
  L2S_ACT_LRELU = 5,  /* speech-resynthesis/models.py:36-38,101,110 */
  L2S_ACT_TANH = 6    /* speech-resynthesis/models.py:112 */
};

/* epilogue flags */
enum {
  L2S_F_RES_PRE  = 1 << 0, /* v += R before the activation (BasicBlock: resnet.py:71-72) */
  L2S_F_RES_POST = 1 << 1, /* v += R after the activation (x + f(x) residuals) */
  L2S_F_ACCUM    = 1 << 2, /* v += previous contents of C (sum of ResBlocks, models.py:105-108) */
  L2S_F_DUAL     = 1 << 3, /* also store C2 = leaky_relu(v, slope2) as 16-bit */
  L2S_F_MASK     = 1 << 4, /* zero output rows whose time index >= lens[clip]*mask_mul */
  L2S_F_OUT_F32  = 1 << 5, /* C is fp32 (else 16-bit `dtype`) */
  L2S_F_RES_F32  = 1 << 6  /* R is fp32 (else 16-bit `dtype`) */
};

/* A-row addressing modes of the tap-GEMM */
enum {
  L2S_MODE_LINEAR = 0, /* src_row = m                                   (nn.Linear, 1x1 conv) */
  L2S_MODE_CONV1D = 1, /* rows = (clip, t): src_t = t*stride + tap*dil + off   (Conv1d / one phase of ConvTranspose1d) */
  L2S_MODE_CONV2D = 2  /* rows = (img, y, x): iy = y*stride + ky - pad, ix likewise (Conv2d) */
};

/*
 * Tap-GEMM: C[o(m), n] = epi( sum_{tap<ntaps} sum_{c<Cin} A[src(m,tap), c] * W[n, tap*Cin + c] )
 * with out-of-range source rows reading as zero (= the conv's zero padding).
 * One kernel family serves every dense contraction of the path:
 *   nn.Linear            avhubert/hubert.py:327,727 ; fairseq q/k/v/out_proj, fc1, fc2 (hubert.py:739) ;
 *                        espnet attention.py:50-53,257 ; positionwise_feed_forward.py:28-30 ;
 *                        model_avhubert.py:258,273,285 ; models_multi_input.py:70,80
 *   nn.Conv2d 3x3 / 1x1  avhubert/resnet.py:15-24,61-74 (BatchNorm folded into W and bias)
 *   nn.Conv1d            fairseq pos_conv (hubert.py:399, groups=16 via `groups`) ; model_avhubert.py:231-241 ;
 *                        espnet convolution.py:26-45 (pointwise) ; speech-resynthesis/models.py:19-31,78-79
 *   nn.ConvTranspose1d   speech-resynthesis/models.py:84-86, models_multi_input.py:40 — one call per output phase
 */
typedef struct l2s_gemm_desc {
  const void* A;      /* [rows_in, lda] 16-bit */
  const void* W;      /* [N, Ktot] 16-bit, Ktot = ntaps*Cin, K contiguous */
  void* C;            /* [rows_out, ldc] 16-bit or fp32 (L2S_F_OUT_F32) */
  void* C2;           /* [rows_out, ldc2] 16-bit, L2S_F_DUAL only */
  const float* bias;  /* [N] fp32 or NULL */
  const float* slope; /* [N] fp32 PReLU slopes (L2S_ACT_PRELU) or NULL */
  const void* R;      /* residual [rows_out, ldr] or NULL */
  const int32_t* lens;/* [clips] valid base-time units per clip (L2S_F_MASK) */
  int32_t M, N, Cin, ntaps;
  int32_t lda, ldc, ldc2, ldr;
  int32_t mode;
  /* CONV1D */
  int32_t T_out, T_in, stride, dil, off;
  /* CONV2D */
  int32_t Ho, Wo, Hi, Wi, KW, pad;
  /* output row remap: o = m*out_row_mul + out_row_add (ConvTranspose1d phases) */
  int32_t out_row_mul, out_row_add;
  /* row mask: clip = o / mask_T, t = o % mask_T, valid iff t < lens[clip]*mask_mul */
  int32_t mask_T, mask_mul;
  int32_t act, flags, dtype;
  float alpha;        /* v = alpha*(acc + bias) */
  float act_slope;    /* L2S_ACT_LRELU slope */
  float slope2;       /* leaky slope of the C2 copy */
  /* grouped conv (blockIdx.z): per-group element offsets added to A cols, W, C cols, bias */
  int32_t groups, a_gstride, c_gstride;
  int64_t w_gstride;
  /* K-block table (L2S_MODE_LINEAR only; NULL = none): the launch is `groups` problems over the same A [M, lda] and W [N, Ktot =
   * ntaps*Cin].  Problem g computes C[:, g*c_gstride + n] = epilogue(sum over j < nblk of A[:, a_off[j] .. + Cin) . W[n, w_off[j] ..
   * + Cin)) - a K that is a LIST of Cin-wide column blocks.  With an H x W map stored as ONE row of A ([images, H*W*Cin]) this is a
   * convolution on a small map in which output position g sums only the taps that fall inside the map (avhubert/resnet.py:15-24
   * conv3x3 with padding 1 on the 6 x 6 / 3 x 3 maps of layer3 / layer4: 21 / 40 % of the taps are padding).
   * ktab: device int32 [groups][2 + 2*L2S_KTAB_MAX] = {nblk, 0, a_off[L2S_KTAB_MAX], w_off[L2S_KTAB_MAX]}, element offsets that
   * are multiples of 8; bias / slope are indexed [g*N + n] (as for grouped convolutions); R is addressed like C.  Served by the
   * phase-staggered kernel for the bias + linear-activation families with or without a 16-bit residual; else L2S_EUNSUPPORTED. */
  const int32_t* ktab;
} l2s_gemm_desc;
#define L2S_KTAB_MAX 9

int l2s_abi_version(void);
const char* l2s_build_info(void);

int l2s_tapgemm(const l2s_gemm_desc* host_desc, void* stream);
/* block tile the launcher picks for this descriptor, as BM*1000+BN (profiling aid: names the kernel instantiation);
 * 256256 = the phase-staggered kernel, 999064 / 999128 = the patch conv kernel at 64 / 128 channels,
 * L2S_VARIANT_F32 = the fp32 kernel (128 x 128 tile on v_mfma_f32_32x32x2_f32, csrc/tapgemm_f32.hip) */
#define L2S_VARIANT_F32 2128128
int l2s_tapgemm_variant(const l2s_gemm_desc* host_desc);
/* epilogue family (0..9) of the kernel instantiation the launcher picks: every kernel is built once per family of
 * (flags, activation) so that a launch carries one epilogue's code only (profiling aid, names the instantiation);
 * L2S_EPI_FAMILY_F32 for an fp32 descriptor (one run-time epilogue) */
#define L2S_EPI_FAMILY_F32 32
int l2s_tapgemm_epilogue_family(const l2s_gemm_desc* host_desc);

/*
 * Stem: Conv3d(1->64,k(5,7,7),s(1,2,2),p(2,3,3)) + BatchNorm3d(eval, folded) + PReLU
 * avhubert/resnet.py:137-140.  x: [B,T,88,88] (fp32 when x_is_f32 else 16-bit); w: [64, 288] 16-bit packed
 * (k = (dt*7+dy)*8+dx, dx==7 zero); y: [B*T, Ho, Wo, 64] 16-bit channels-last.  Frames t >= lens[b] read as zero.
 * slope: [64] fp32 PReLU slopes (zeros = ReLU); NULL selects Swish, the stem of ESPnet's Conv3dResNet
 * (espnet/nets/pytorch_backend/backbones/conv3d_extractor.py:57-78, used by the `multi_target` model, model.py:184-228).
 */
int l2s_stem_conv3d(const void* x, int x_is_f32, const void* w, const float* bias, const float* slope,
                    void* y, int B, int T, int H, int W, int dtype, void* stream);

/*
 * Fused stem + pool: Conv3d + BatchNorm3d + PReLU + MaxPool3d(k(1,3,3),s(1,2,2),p(0,1,1)), avhubert/resnet.py:137-141, in one
 * launch: frame window in an LDS ring, conv tile pooled out of LDS, the [44,44,64] conv activation never reaches HBM.
 * Same x / w / bias / slope as l2s_stem_conv3d (x 16-byte aligned); y: [B*T, 22, 22, 64] 16-bit channels-last.  With all
 * slopes >= 0 the kernel pools the raw conv tile and applies the PReLU to the pooled values (PReLU is then non-decreasing and
 * commutes with the maximum); any negative slope, and Swish, keep the activation in front of the pool as written in the
 * reference.  DEVIATION of the all-slopes->= 0 path from l2s_stem_conv3d + l2s_maxpool2d_3x3s2 (and from the reference's
 * order, fp32 PReLU then ONE rounding): the conv value is rounded to 16 bits before the pool and the activated value again
 * after it, so NEGATIVE outputs are round16(s * round16(a)) instead of round16(s * a) - one 16-bit ulp at most from that;
 * the fused kernel also sums the taps in another order than l2s_stem_conv3d (different tiles), worth one more ulp on a small
 * share of the outputs of either sign (tests/test_kernels_gpu.py::test_stem_pool_fused_vs_two_step_launches: <= 2 ulp, < 2 %
 * of the outputs differ at T = 7, both dtypes).  The share follows the share of negative outputs - 4.2 % at T = 1 with that test's
 * bias - and an output that has cancelled to less than the fp32 accumulation error of its 245 terms has no meaningful ulp: the two
 * kernels then agree to that error, not to 2 ulp of the tiny value (profiles/frontend_matrix.md, Findings 1 and 2).
 */
int l2s_stem_pool_fused(const void* x, int x_is_f32, const void* w, const float* bias, const float* slope,
                        void* y, int B, int T, int H, int W, int dtype, void* stream);

/*
 * The same fused stem, fed by the raw decoder output: frames [B,T,Hin,Win] uint8 grayscale.  The centre crop to
 * crop x crop (= 88) and the (x/255 - mean)/std normalisation (avhubert/hubert_dataset.py:242-245, utils.py:56-95:
 * CenterCrop offsets truncate) are applied while the frame window is staged into LDS, in l2s_preprocess_frames'
 * arithmetic (results are bit-identical to l2s_preprocess_frames followed by l2s_stem_pool_fused); the normalised
 * frames never exist in HBM.
 */
int l2s_stem_pool_fused_u8(const uint8_t* frames, int Hin, int Win, int crop, float mean, float std, const void* w,
                           const float* bias, const float* slope, void* y, int B, int T, int dtype, void* stream);
/* l2s_stem_pool_frames (host-only: nothing is launched): the consecutive frames one block of the two fused stems above walks for
 * B clips of T frames - 10, or 25 once 6 * ceil(T / 25) * B >= 2048 blocks remain, or L2S_STEM_FT of this process (any value
 * >= 1: chunks shorter than the 5-frame window are fine, a block stages the whole window of its first frame); L2S_ESHAPE for
 * B or T <= 0.  The chunking only decides which block computes a frame: results are bit-identical for every value. */
int l2s_stem_pool_frames(int B, int T);

/* MaxPool3d(k(1,3,3),s(1,2,2),p(0,1,1)) on channels-last frames, avhubert/resnet.py:141.  x:[N,H,W,C] -> y:[N,Ho,Wo,C] */
int l2s_maxpool2d_3x3s2(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);

/* AdaptiveAvgPool2d(1) over HW, avhubert/resnet.py:127-128.  x:[N,HW,C] 16-bit -> y:[N,C] 16-bit */
int l2s_avgpool_hw(const void* x, void* y, int N, int HW, int C, int dtype, void* stream);

/*
 * LayerNorm over the last dim with fp32 statistics (wavefront reduction).
 *   fairseq LayerNorm eps 1e-5: hubert.py:400,720 and every transformer layer ; espnet layer_norm.py:12-33 eps 1e-12.
 * x: [M, ldx] (fp32 if x_is_f32 else 16-bit); y: [M, ldy] (fp32 if y_is_f32 else 16-bit), C columns.
 * zero_prefix > 0 reproduces hubert.py:706-720 (video-only fuse): the normalised vector is [zeros(zero_prefix) ‖ x]
 * of width zero_prefix + C; gamma/beta then have zero_prefix + C entries and y gets zero_prefix + C columns.
 * y2 (optional, 16-bit, ldy2) receives a second copy (used to feed the mel head concat buffer).
 * lens (optional): rows with (row % mask_T) >= lens[row / mask_T]*len_mul are written as zero (the zero padding a
 * clip run alone would see in the temporal convs that follow, SURVEY.md section 7 "Batching semantics").
 */
int l2s_layernorm(const void* x, int x_is_f32, int ldx, const float* gamma, const float* beta, float eps,
                  void* y, int y_is_f32, int ldy, void* y2, int ldy2, int M, int C, int zero_prefix,
                  const int32_t* lens, int len_mul, int mask_T, int dtype, void* stream);
/* Host-only queries (nothing launched, no pointer dereferenced; pointers count for null / alignment only): the kernel
 * instantiation the launcher runs for these arguments, or the error code the launch would answer.  L2S_SEQ_VARIANT_F32 for an
 * fp32 launch.
 * l2s_layernorm_variant: L2S_LN_GENERIC + 2 x_is_f32 + y_is_f32 = the one-row-per-wave kernel (any C, zero_prefix, y2);
 * 512 + y_is_f32 / 1024 + y_is_f32 = the rows kernel of that width (fp32 x, no y2, no zero_prefix; a 16-bit y needs 16-byte
 * alignment and ldy % 8 == 0, else the generic kernel runs). */
#define L2S_SEQ_VARIANT_F32 2000
#define L2S_LN_GENERIC 10
int l2s_layernorm_variant(const void* x, int x_is_f32, int ldx, const float* gamma, const float* beta, const void* y, int y_is_f32,
                          int ldy, const void* y2, int ldy2, int M, int C, int zero_prefix, const int32_t* lens, int len_mul,
                          int mask_T, int dtype);

/*
 * Fused multi-head self-attention with key-padding mask, fp32 online softmax.
 *   fairseq MultiheadAttention (hubert.py:739-743; q pre-scaled by d^-0.5 at pack time) when pos == NULL;
 *   espnet RelPositionMultiHeadedAttention (attention.py:240-280,59-90) when pos != NULL:
 *   score[i,j] = (q_i+u).k_j + (q_i+v).P[i-j], P = pos[(T-1)-(i-j)] (rel_shift folded into the index).
 * qkv: [B*T, ldq] 16-bit with q at col 0, k at col H*64, v at col 2*H*64 (head h at +h*64); out: [B*T, ldo] 16-bit.
 * pos: [2T-1, ldp] 16-bit (row k <-> relative position T-1-k), head h at col h*64; bias_u/bias_v: [H,64] fp32.
 * lens: [B] valid keys per clip scaled by len_mul (keys >= lens[b]*len_mul get zero probability).
 */
int l2s_attention(const void* qkv, int ldq, void* out, int ldo, const void* pos, int ldp,
                  const float* bias_u, const float* bias_v, const int32_t* lens, int len_mul,
                  int B, int T, int H, int dtype, void* stream);
/* l2s_attention_variant (host-only, as l2s_layernorm_variant): 64 + rel / 128 + rel = the tiled kernel on 64- / 128-row query
 * blocks, L2S_ATTN_RESIDENT + rel = the sequence-resident kernel; rel = 1 with a position table. */
#define L2S_ATTN_RESIDENT 1000
int l2s_attention_variant(const void* qkv, int ldq, const void* out, int ldo, const void* pos, int ldp, const float* bias_u,
                          const float* bias_v, const int32_t* lens, int len_mul, int B, int T, int H, int dtype);

/*
 * Conformer conv-module core: GLU(dim=C) -> depthwise Conv1d(k, pad (k-1)/2, groups=C) -> BatchNorm1d(eval, folded)
 * -> Swish.  espnet convolution.py:57-62.  x: [B*T, 2C] 16-bit (pointwise_cov1 output); w: [k, C] fp32 (BN folded);
 * bias: [C] fp32; y: [B*T, C] 16-bit.  Rows t >= lens[b]*len_mul are treated as zero padding and written as zero.
 */
int l2s_glu_dwconv_swish(const void* x, const float* w, const float* bias, void* y, const int32_t* lens,
                         int len_mul, int B, int T, int C, int k, int dtype, void* stream);
/* l2s_glu_dwconv_tile (host-only): the time steps per block the launcher picks, 100 or 128 (L2S_SEQ_VARIANT_F32 for fp32), or
 * the launch's error code for these shapes. */
int l2s_glu_dwconv_tile(int B, int T, int C, int k, int dtype);

/*
 * Greedy unit decode == hypothesis 0 of the reference beam search (multi_target_lip2speech/sequence_generator.py:235-494):
 * per step t < 2*src_len: token = argmax over ids [4, V) of logits/temperature (pad,bos,eos,unk excluded :274-282),
 * lprob = log_softmax over all V ; step t == 2*src_len emits EOS (id 2) with lprob 0 (:286-298).
 * logits: [B*T2, ldl] fp32; tokens: [B, T2+1] int32 (pad id 1 after EOS); lprobs: [B, T2+1] fp32; score: [B] fp32
 * = sum(lprobs)/(L+1)^lenpen (avhubert/sequence_generator.py:650-651).
 */
int l2s_greedy_decode(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int T2, int V,
                      float temperature, float lenpen, int32_t* tokens, float* lprobs, float* score, void* stream);

/*
 * n-best unit decode: the reference's beam search itself (multi_target_lip2speech/sequence_generator.py:235-494 with fairseq
 * BeamSearch.step at :337-343 and finalize_hypos avhubert/sequence_generator.py:605-721), one wavefront per clip.  Step scores are
 * history-independent (:253-256), so the search is an exact top-`beam` over sequences; hypothesis 0 equals l2s_greedy_decode.
 * beam <= 64, V <= 256.  tokens / pos_scores: [B, beam, T2+1] (hypotheses in finalisation order = descending score; EOS at
 * position L, pad id 1 / 0.0 behind it); score: [B, beam] = cumulative score / (L+1)^lenpen; nhyp: [B] hypotheses produced
 * (beam, or 1 for an empty clip).  workspace: l2s_beam_decode_workspace(B, T2, beam) bytes of device memory.
 */
int l2s_beam_decode(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int T2, int V, float temperature,
                    float lenpen, int beam, void* workspace, size_t workspace_bytes, int32_t* tokens, float* pos_scores,
                    float* score, int32_t* nhyp, void* stream);
size_t l2s_beam_decode_workspace(int B, int T2, int beam);

/*
 * CTC text head outputs (TEXT_SUPERVISION=1, multi_target_lip2speech/sequence_generator.py:141-171), per frame t < lens[b]*len_mul
 * of logits [B*L, ldl] fp32 (V classes, blank = 0): p = softmax in fp32, labels[b, t] = argmax p (ties: first index; 0 on
 * padded frames); topk_cls / topk_lp [B, L, K]: the K most probable classes, p descending (ties: smaller index), with
 * log(p + FLT_MIN) (ctcdecode get_pruned_log_probs); padded frames hold class 0 / -FLT_MAX.  K = 0 writes labels only.
 * V <= 4096, K <= 64, K <= V.
 */
int l2s_ctc_frames(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int L, int V, int K, int32_t* labels,
                   int32_t* topk_cls, float* topk_lp, void* stream);

/*
 * CTC prefix beam search over l2s_ctc_frames' top-K (ctcdecode CTCBeamDecoder without a language model: DecoderState::next /
 * PathTrie, alpha = beta = 0, cutoff_prob = 1), one workgroup per clip over its lens[b]*len_mul frames.  beam <= 64, K <= 64,
 * nbest <= beam.  labels [B, nbest, L] int32 (collapsed label ids, 0 behind the length), lengths [B, nbest], scores [B, nbest] =
 * -(log probability of the prefix), best first; a beam that does not exist has length 0 and score FLT_MAX.
 * workspace: l2s_ctc_beam_workspace(B, L, beam) bytes (8-byte aligned); 0 from the query = unsupported size.
 */
int l2s_ctc_beam_search(const int32_t* topk_cls, const float* topk_lp, const int32_t* lens, int len_mul, int B, int L, int K,
                        int beam, int nbest, void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* lengths,
                        float* scores, void* stream);
size_t l2s_ctc_beam_workspace(int B, int L, int beam);
/*
 * REPEAT_TEXT_LABELS forward fill of framewise labels (multi_input_vocoder/dataset_multi_input.py:23-38): y[b, t] = x[b, j] for
 * the last j <= t with x[b, j] != 0, else 0; frames t >= lens[b]*len_mul get 0.  x [B, ldx], y [B, ldy] int32; y == x allowed.
 */
int l2s_ctc_repeat_labels(const int32_t* x, int ldx, const int32_t* lens, int len_mul, int B, int L, int32_t* y, int ldy,
                          void* stream);

/* time-major frame duplication x2 (sequence_generator.py:130-131) fused with a cast: x:[B*T, C] fp32 -> y:[B*2T, C] 16-bit */
int l2s_repeat2_cast(const float* x, void* y, int B, int T, int C, int dtype, void* stream);

/*
 * Split-K tail of a small-M residual-stream Linear (the one-clip-per-request path, multi_target_lip2speech/inference.py:161):
 * with M of 100-500 rows a 64 x 64-tile GEMM fills 32 of the 256 CUs for K / 64 serial K-tiles.  The host then runs the layer
 * as ONE grouped l2s_tapgemm launch (groups = S slices of K: a_gstride = K / S columns of A, the weight pre-packed as
 * [S][N][K / S], c_gstride = N, fp32 partial products P [M, S*N], bias in slice 0 only) and this kernel folds them into the
 * fp32 residual stream: x[m, n] += sum_{s < S} P[m, s*N + n], s ascending (deterministic; fairseq fc2 / out_proj + residual,
 * hubert.py:739; espnet positionwise_feed_forward.py:30 + encoder_layer.py:95).
 */
int l2s_splitk_reduce(const float* P, int ldp, int S, float* x, int ldx, int M, int N, void* stream);

/* l2s_splitk_reduce followed by l2s_layernorm of the updated stream, in one launch (C = 1024 or 512; the pre-LN encoder / conformer
 * layers put a LayerNorm behind every residual update: hubert.py:739-743, encoder_layer.py:89-141): x[m] += sum_s P[m, s*C ..],
 * y[m] = LayerNorm(x[m]) (16-bit, or fp32 when y_is_f32; y == x in fp32 = in place, the un-normalised sum is then not stored).
 * The stream update is bit-identical to l2s_splitk_reduce's, the LayerNorm equal to l2s_layernorm's to fp32 rounding. */
int l2s_splitk_reduce_layernorm(const float* P, int ldp, int S, float* x, int ldx, const float* gamma, const float* beta, float eps,
                                void* y, int y_is_f32, int ldy, int M, int C, const int32_t* lens, int len_mul, int mask_T,
                                int dtype, void* stream);

/* generic cast / layout helpers */
int l2s_cast_f32_to_16(const float* x, int ldx, void* y, int ldy, int M, int C, int dtype, void* stream);
int l2s_cast_16_to_f32(const void* x, int ldx, float* y, int ldy, int M, int C, int dtype, void* stream);
/* y[b*T + t, col0 + c] = v[b, c] for t < T (speaker-embedding time tiling: model_avhubert.py:269, models.py:158-177);
 * rows t >= lens[b]*len_mul are zeroed when lens != NULL */
int l2s_broadcast_rows(const void* v, int ldv, void* y, int ldy, int col0, const int32_t* lens, int len_mul,
                       int B, int T, int C, int v_is_f32, int dtype, void* stream);
/* y[b*T + t, col0 + c] = x[b, c, t] (fp32 [B,C,T] mel -> channels-last 16-bit; models_multi_input.py:65,73) */
int l2s_transpose_ct_to_tc(const float* x, void* y, int ldy, int col0, const int32_t* lens, int len_mul,
                           int B, int C, int T, int dtype, void* stream);
/* y[b*L + l, :] = table[code[b,l], :] (nn.Embedding, models_multi_input.py:67); rows l >= lens[b] zeroed */
int l2s_embedding(const int32_t* code, const void* table, void* y, int ldy, const int32_t* lens,
                  int B, int L, int C, int dtype, void* stream);
/*
 * In-memory stage 1 -> stage 2 hand-off (replaces the file round trip multi_target_lip2speech/inference.py:267-274 ->
 * create_dataset.py:366-428 -> multi_input_vocoder/dataset_multi_input.py:41-110,198-291), all on the caller's stream:
 *  l2s_embedding_tokens: the generator's token rows (tok[b*ldt + l], fairseq ids: unit u is token u + token_offset, 4 specials
 *    first) -> nn.Embedding rows y[b*L + l, :] = table[clamp(tok - token_offset, 0, n_rows-1), :]; rows l >= lens[b]*len_mul zero.
 *  l2s_rows_f32_to_16_masked: time-major fp32 rows x[(b*T + t)*ldx + c] (the mel head's output, model_avhubert.py:276) ->
 *    16-bit y[(b*T + t)*ldy + col0 + c] (the vocoder's concat buffer, models_multi_input.py:65,73); rows t >= lens[b]*len_mul zero.
 *  l2s_lens_from_mask: src_lengths of sequence_generator.py:64-65: lens[b] = T - sum_t mask[b,t] (mask: bool bytes, True = pad;
 *    NULL = no padding).
 */
int l2s_embedding_tokens(const int32_t* tok, int ldt, int token_offset, const void* table, int n_rows, void* y, int ldy,
                         const int32_t* lens, int len_mul, int B, int L, int C, int dtype, void* stream);
int l2s_rows_f32_to_16_masked(const float* x, int ldx, void* y, int ldy, int col0, const int32_t* lens, int len_mul,
                              int B, int T, int C, int dtype, void* stream);
int l2s_lens_from_mask(const uint8_t* mask, int32_t* lens, int B, int T, void* stream);
/*
 * Reference-precision switch of the vocoder (the reference's MelCodeGenerator runs in fp32, multi_input_vocoder/inference.py:
 * 73-82, speech-resynthesis/models.py:98-114): y = act(x) for rows t < lens[b]*len_mul (else 0), written as hi = 16-bit(y) and
 * lo = 16-bit(y - hi).  act: 0 none, 1 leaky_relu(slope), 2 GELU (erf).  x: fp32 [B*T, ldx]; hi, lo: 16-bit [B*T, ld16].
 * A layer is then three l2s_tapgemm launches into one fp32 output (a_hi w_hi, then a_lo w_hi and a_hi w_lo with L2S_F_ACCUM).
 */
int l2s_split_hi_lo(const float* x, int ldx, void* hi, void* lo, int ld16, int act, float slope, const int32_t* lens,
                    int len_mul, int B, int T, int C, int dtype, void* stream);

/*
 * Fused convolution PAIR of ResBlock1 for the wide vocoder stages (speech-resynthesis/models.py:34-41, one (c1, c2, d) step):
 *   x' = c2(leaky_relu(c1(leaky_relu(x)))) + x,  C in {64, 128, 256}, k odd <= 17, h1 = (k-1)/2 * dil <= 28 (C = 256) or <= 32
 *   (C = 64 / 128: h1 = 29 .. 32 runs on the 192-row kernels of csrc/respair.hip, l2s_respair_variant says which); other shapes
 *   answer L2S_EUNSUPPORTED.  tests/test_vocconv_matrix_gpu.py runs every kernel at these limits.
 * The pair's input and output travel as their LeakyReLU'd 16-bit copies only (x is recovered by the inverse of leaky_relu);
 * the intermediate never leaves LDS.  X: [B*T, C] = leaky_relu(x), rows t >= lens[b]*len_mul zero; W1 / W2: [C][k*C] 16-bit,
 * K = tap*C + c (W1 applied with dilation dil, W2 with dilation 1, both "same" padded); b1 / b2: [C] fp32.
 * last == 0: Y [B*T, C] = leaky_relu(x').   last != 0 (the third pair of a ResBlock): XS [B*T, C] fp32 = x' (+ XS when
 * accumulate: the sum over the stage's ResBlocks, models.py:103-108) and, when Y is given, Y = leaky_relu(XS).
 * last == 2 (the stage's final pair when only Y travels on: `x = xs / num_kernels` feeds leaky_relu + ups, models.py:109,101):
 * XS is read for the sum but NOT written back - Y = leaky_relu(XS + x') is the only output.
 * Rows at or past the clip length are written as zero, in Y and in XS, whatever XS held there before an accumulating launch.
 * lens == NULL: every clip has T rows.
 */
typedef struct l2s_respair_desc {
  const void* X; const void* W1; const void* W2; const float* b1; const float* b2;
  void* Y; float* XS; const int32_t* lens;
  int32_t len_mul, B, T, C, k, dil, last, accumulate, dtype;
  float slope;
} l2s_respair_desc;
int l2s_respair(const l2s_respair_desc* d, void* stream);
/* l2s_respair_variant (host-only, as l2s_attention_variant: nothing is launched, no pointer is dereferenced, pointers count for the
 * null and alignment checks only): RM * 1000 + C of the kernel l2s_respair would run for d, RM = the rows a tile computes -
 * 192064 / 192128: csrc/respair.hip; 512064 / 256128 / 128256: csrc/respair_phase.hip - or the error code of the launch. */
int l2s_respair_variant(const l2s_respair_desc* d);

/*
 * The LAST conv pairs of a stage's n <= 3 ResBlocks in one launch (speech-resynthesis/models.py:103-109 over :34-41):
 *   Y [B*T, C] = leaky_relu( sum_j ( c2_j(leaky_relu(c1_j(leaky_relu(x_j)))) + x_j ) ),  C in {64, 128, 256}
 * where X[j] = leaky_relu(x_j) is the input of ResBlock j's last (c1, c2, d) pair - what l2s_respair(last = 0) of its previous pair
 * wrote.  Same operand layouts and limits as l2s_respair (k odd <= 17, (k-1)/2 * dil <= 28).  The stage's fp32 sum is kept in
 * accumulators across the ResBlocks and never written: use it where only leaky_relu of the sum travels on (`x = xs / num_kernels`
 * feeds leaky_relu + ups, models.py:109,101 - every stage but the last); results equal n l2s_respair(last != 0) launches up to the
 * order of the fp32 additions.  Rows at or past the clip length are written as zero.
 */
typedef struct l2s_respair_final_desc {
  const void* X[3]; const void* W1[3]; const void* W2[3]; const float* b1[3]; const float* b2[3];
  int32_t k[3], dil[3];
  void* Y; const int32_t* lens;
  int32_t n, len_mul, B, T, C, dtype;
  float slope;
} l2s_respair_final_desc;
int l2s_respair_final(const l2s_respair_final_desc* d, void* stream);

/*
 * Fused BasicBlock of the lip frontend's 64-channel stage (avhubert/resnet.py:43-74 with :15-24 conv3x3, layer1 of ResNet-18;
 * eval BatchNorm folded into weight + bias):  y = prelu(conv2(prelu(conv1(x) + b1, s1)) + b2 + x, s2), both convolutions 3x3,
 * stride 1, padding 1, C -> C channels.  One block keeps one image in LDS: HBM sees x once and y once.
 * x, y: [n_images*H*W, C] 16-bit channels-last; w1, w2: [C][9*C] 16-bit, K index = (ky*3 + kx)*C + cin; b*, s*: fp32[C] (bias,
 * PReLU slope).  Supported: C = 64, (H+2)*(W+2) <= 576, W <= 29 (22 x 22 on the path: csrc/basicblock.hip), and C = 128 with H = W = 11
 * (layer2's second block: csrc/basicblock_phase.hip, two images per 256-row tile); anything else returns L2S_EUNSUPPORTED.
 */
int l2s_basicblock_fused(const void* x, const void* w1, const float* b1, const float* s1, const void* w2, const float* b2,
                         const float* s2, void* y, int n_images, int H, int W, int C, int dtype, void* stream);
/*
 * n_blocks (<= 4) BasicBlocks of that stage back to back on the LDS-resident image (avhubert/resnet.py:101-118 `_make_layer`,
 * layer1 = two blocks): the layer's input is read once, its output written once, the activations in between never leave the
 * CU.  Results are bit-identical to n_blocks l2s_basicblock_fused calls (the hand-over is the same 16-bit rounding).
 * w, bias, slope: HOST arrays of 2*n_blocks device pointers in the order conv1, conv2 of block 0, conv1, conv2 of block 1, ...
 */
int l2s_basiclayer_fused(const void* x, const void* const* w, const float* const* bias, const float* const* slope, int n_blocks,
                         void* y, int n_images, int H, int W, int C, int dtype, void* stream);
/* l2s_basicblock_variant (host-only, as l2s_respair_variant: nothing is launched, there is no pointer to dereference): which kernel
 * l2s_basicblock_fused (n_blocks = 1) / l2s_basiclayer_fused run for these arguments under this process's L2S_BASICBLOCK_PHASE, or
 * the error code a launch with valid, 16-byte aligned pointers gives.  The launchers ask the same function. */
#define L2S_BB_PADDED64 576064  /* csrc/basicblock.hip: 576 padded positions per image, C = 64 */
#define L2S_BB_PHASE64 512064   /* csrc/basicblock_phase.hip, CH = 64: 22 x 22, one image per 512-row tile */
#define L2S_BB_PHASE128 256128  /* csrc/basicblock_phase.hip, CH = 128: 11 x 11, two images per 256-row tile */
int l2s_basicblock_variant(int n_images, int H, int W, int C, int n_blocks, int dtype);
/*
 * The rest of ResNet-18's strided 128-channel stage behind its first convolution, in one launch (avhubert/resnet.py:61-74 for a
 * block WITH downsample, :101-118 `_make_layer`, layer2 on the path: 22 x 22 x 64 -> 11 x 11 x 128):
 *   out0 = prelu(conv3x3(t0) + ba + Wd x0[::2, ::2], sa)                  second conv of block 1, residual = the 1x1 stride-2 downsample
 *   y    = prelu(conv3x3(prelu(conv3x3(out0) + b1, s1)) + b2 + out0, s2)  block 2 (= l2s_basicblock_fused, C = 128)
 * x0: the stage input [n_images*(2H)*(2W), 64]; t0: block 1's first conv output [n_images*H*W, 128] (after bn1 + PReLU); both 16-bit
 * channels-last.  wa: [128][9*128 + 64 + 64] 16-bit = the 3x3 weights (K index (ky*3+kx)*128 + cin) | the downsample weights
 * [128][64] | 64 zero columns; ba = the conv's folded bias + the downsample's folded bias; w1, w2: [128][9*128]; b*, s*: fp32[128].
 * The downsample runs as one more K-tile of the same fp32 accumulation (it is not rounded to 16 bits on the way, unlike a separate
 * launch); out0 never leaves the CU.  Supported: H = W = 11 (l2s_basicblock_fused's C = 128 family); else L2S_EUNSUPPORTED.
 */
int l2s_basicstage128_tail_fused(const void* x0, const void* t0, const void* wa, const float* ba, const float* sa, const void* w1,
                                 const float* b1, const float* s1, const void* w2, const float* b2, const float* s2, void* y,
                                 int n_images, int H, int W, int dtype, void* stream);

/*
 * Vocoder tail: leaky_relu(x, 0.01) -> Conv1d(C->1, k7, p3) -> tanh -> *32768 -> int16 truncation.
 * speech-resynthesis/models.py:110-112 ; multi_input_vocoder/inference.py:79-81.
 * x: [B*T, C] fp32 (sum of the three ResBlocks; the /3 is folded into w); w: [k, C] fp32; wav: [B, T] fp32; pcm: [B, T] int16 or NULL.
 * k odd, (256 + k - 1) (C + 1) + k C floats of LDS <= 64 KB (else L2S_EUNSUPPORTED).  Samples at or past the clip length are zero.
 * A saturated sample - tanh returns exactly +-1.0f for a pre-activation beyond about +-9 - has wav * 32768 = +-32768: pcm is
 * -32768 for both signs, what numpy's astype('int16') of the reference gives (+32768 wraps).
 */
int l2s_conv_post_tanh(const float* x, const float* w, float bias, float* wav, int16_t* pcm, const int32_t* lens,
                       int len_mul, int B, int T, int C, int k, void* stream);

/*
 * Fused ResBlock1 (speech-resynthesis/models.py:16-47) for the narrow vocoder stages, C in {16,32}, k in {3,7,11}:
 * six convolutions run out of an LDS-resident time tile; HBM sees one read of xl = leaky_relu(x) and one accumulate of
 * the block output into xs (the sum over the stage's three ResBlocks, models.py:103-108).
 * xl: [B*T, C] 16-bit; w: [6][C][Kpad] 16-bit in the order c1(d0),c2,c1(d1),c2,c1(d2),c2 with K = tap*C + c zero-padded to
 * a multiple of 32; bias: [6][C] fp32; xs: [B*T, C] fp32 (overwritten, or added to when accumulate != 0);
 * xl_out (optional, 8-byte aligned): [B*T, C] 16-bit = leaky_relu(xs after this call).  Rows t >= lens[b]*len_mul are never read
 * from xl and the ResBlock's output is zero there: xs is written as zero when accumulate == 0 and keeps its previous content when
 * accumulate != 0 (0 + xs; a stage's sum starts with an overwriting launch and stays zero there), xl_out is leaky_relu of that.
 * Dilations 1 .. 5 each.  The time tile with its halo of (k-1)/2 * (d0 + d1 + d2 + 3) rows has to fit 160 KB of LDS: that is every
 * set but d0 + d1 + d2 > 11 at C = 32, k = 11, which answers L2S_EUNSUPPORTED (the generator's set is (1, 3, 5)).
 */
int l2s_resblock_fused(const void* xl, const void* w, const float* bias, float* xs, void* xl_out,
                       const int32_t* lens, int len_mul, int B, int T, int C, int k, int d0, int d1, int d2,
                       int accumulate, float slope, int dtype, void* stream);

/*
 * All ResBlocks of one narrow stage in one launch (speech-resynthesis/models.py:103-109, `xs = sum_j resblocks[i*3+j](x)`):
 * each block runs the n_blocks = 3 ResBlocks (resblock_kernel_sizes = [3, 7, 11]) on its time tile back to back, so xl
 * is read from HBM once; at C = 32 the fp32 running sum stays in registers between the ResBlocks, at C = 16 it passes through
 * xs (L2).  Results are those of three l2s_resblock_fused calls (accumulate = 0, 1, 1; xl_out on the last) in the kernel's
 * order, bit for bit: k = 11, 7, 3 at C = 32 (the widest body first: the sum's registers are live through the later ones)
 * and k = 3, 7, 11 at C = 16, i.e. the stage sum is (first + second) + third in fp32.
 * w[j]: [6][C][Kpad_j] 16-bit and bias[j]: [6][C] fp32 as in l2s_resblock_fused (w, bias, ks, dils are HOST arrays: of
 * device pointers, of kernel sizes, and of the n_blocks x 3 dilations); xs: [B*T, C] fp32; xl_out optional.
 * xs_final != 0: xs holds the stage's sum afterwards (conv_post reads it); xs_final == 0 (xl_out required): only
 * leaky_relu(sum) is written and xs is scratch (content afterwards unspecified; ABI 14 - up to ABI 13 it held the partial
 * sum after the second ResBlock).
 * Other stage layouts return L2S_EUNSUPPORTED (the caller launches the ResBlocks one by one); so do, at C = 32, dilation sets
 * whose tile does not fit the LDS: d0 + d1 + d2 > 13 for k = 7 or > 9 for k = 11 (the generator's (1, 3, 5) fits).
 */
int l2s_resstage_fused(const void* xl, const void* const* w, const float* const* bias, const int* ks, const int* dils,
                       int n_blocks, float* xs, void* xl_out, const int32_t* lens, int len_mul, int B, int T, int C,
                       float slope, int xs_final, int dtype, void* stream);

/* frames: uint8 [B,T,Hin,Win] -> centre crop + (x/255-mean)/std, hubert_dataset.py:242-245, utils.py:56-95 -> 16-bit [B,T,crop,crop] */
int l2s_preprocess_frames(const uint8_t* frames, void* y, int B, int T, int Hin, int Win, int crop, float mean,
                          float std, int dtype, void* stream);

/*
 * Log-mel analysis of waveforms, the vocoder's mel conditioning made from audio (create_dataset.py:62-75 extract_mel_spec with
 * config.py:21-27: TacotronSTFT(640, 160, 640, 80, 16000, 0.0, 8000.0).mel_spectrogram; TacotronSTFT itself is third-party -
 * fairseq's examples/.../tacotron2 - and not in the reference tree: an F.conv1d with a dense windowed Fourier basis in fp32,
 * magnitude, a Slaney mel filterbank, log(clamp(., 1e-5))).  One launch, everything fp32 (a k-ordered fma chain per re / im):
 *   wav: [B, S] samples with leading dimension ldw, fp32 in (-1, 1) or (wav_is_i16) int16 PCM taken as value / 32768;
 *   n_samples: int32 [B] clip lengths (clamped to S), NULL = every clip has S samples;
 *   mel: fp32 [B, T_rows, n_mels] time-major with row stride ldm (the .npy layout, and MelCodeGenerator's mel_rows).
 * Each clip is analysed alone: clip b has T_b = 1 + n_b / hop frames, frame t covers samples [t*hop - n_fft/2, t*hop + n_fft/2)
 * reflect-padded against n_b (never S); rows T_b <= t < T_rows are written as zeros, and a clip with n_b <= n_fft/2 (no valid
 * reflect padding) has only zero rows.  Per frame: re/im[k] = sum_n x[n] basis, mag = sqrtf(re^2 + im^2),
 * m[j] = sum_k fb[j][k] mag[k] (k ascending), out = logf(max(m, floor)).  The tables are data, built by the caller:
 *   basis: fp32 [n_fft][n_fft], row n = sample of the frame, the analysis window folded in, 16-byte aligned.  Column c: tile
 *     q = c / 32, lane l = c % 32, bin k = 32 (q / 2) + l; even q holds  w[n] cos(2 pi k n / n_fft), odd q holds
 *     -w[n] sin(2 pi k n / n_fft) - except column 32 (q = 1, l = 0: the imaginary part of bin 0, identically zero), which holds
 *     the real part of bin n_fft/2, w[n] cos(pi n).  Bins 0 and n_fft/2 are the real-only ones: n_fft columns in all, no padding.
 *   fb: fp32 [n_mels][n_fft/2 + 1] dense filterbank; fb_range: int32 [n_mels][2] = [first, past-last) bin of each band's non-zero
 *     weights (bins outside the range are not read; zeros inside it are harmless).
 * Supported: n_fft = 640, hop = 160, n_mels = 80 (any window, filterbank and floor); other sizes return L2S_EUNSUPPORTED.
 * B <= 65535, T_rows <= 2^22.  ldw >= S, ldm >= n_mels.
 */
int l2s_mel_spectrogram(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                        const float* fb, const int32_t* fb_range, float* mel, int ldm, int T_rows, int n_fft, int hop,
                        int n_mels, float floor_, void* stream);

/*
 * The same analysis with the frame placement and the magnitude's epsilon as arguments - what the HiFi-GAN mel_spectrogram of the
 * vocoder's training and validation loss needs (speech-resynthesis/dataset.py:44-67 with configs/lrs3/multi_input.json:
 * n_fft 1024, hop 256, window 1024, 80 bands, 0 Hz .. sr/2; F.pad(reflect, (n_fft - hop) / 2) then torch.stft(center=False),
 * sqrt(re^2 + im^2 + 1e-9), the librosa Slaney filterbank, log(clamp(., 1e-5)); called at multi_input_vocoder/train.py:152,224 and
 * dataset_multi_input.py:275).  The arguments of l2s_mel_spectrogram plus
 *   pad: reflect padding on each side, 0 <= pad <= n_fft/2.  Frame t of clip b covers samples [t*hop - pad, t*hop - pad + n_fft),
 *     reflected against the clip's own n_b; T_b = (n_b + 2 pad - n_fft) / hop + 1 frames when n_b > pad and n_b + 2 pad >= n_fft,
 *     else 0 (no valid reflection, or not one whole frame); rows T_b <= t < T_rows are zeros; every clip is analysed alone;
 *   mag_eps >= 0: mag = sqrtf(fma(im, im, rn(re*re)) + mag_eps): one square rounded, one fused, the sum with mag_eps rounded.
 * wav (int16 or fp32), n_samples, the packed basis [n_fft][n_fft] with its column map (the real part of bin n_fft/2 in column 32),
 * fb / fb_range, the time-major output with ldm, the clamp floor_, logf and the alignment and shape checks are those documented
 * above.  Same kernel template (csrc/melspec.hip): l2s_mel_spectrogram is this entry at (640, 160, pad 320, mag_eps 0).
 * Supported: (n_fft, hop) = (1024, 256) and (640, 160), n_mels = 80; other sizes, a pad outside [0, n_fft/2] or a negative mag_eps
 * return L2S_EUNSUPPORTED.  B <= 65535, T_rows <= 2^22.
 */
int l2s_stft_mel(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                 const float* fb, const int32_t* fb_range, float* mel, int ldm, int T_rows, int n_fft, int hop, int n_mels,
                 int pad, float mag_eps, float floor_, void* stream);

/*
 * Forward (scoring) half of the `multi_target` criterion (multi_target_lip2speech/criterion.py), csrc/criterion.hip.  All three
 * entries write PER-CLIP results that depend on that clip's rows alone (no atomics, fixed reduction order: the same bytes for a
 * clip whatever its batch mates and from run to run); batch totals are the caller's sum over clips in index order.  Terms are
 * evaluated in fp32, sums across lanes / rows / frames are carried in fp64 and rounded to fp32 once.  lens: int32 [B] or NULL.
 *
 * l2s_unit_ce - label-smoothed cross-entropy and accuracy over the unit logits (criterion.py:148-161 get_lprobs_and_target with
 * fairseq's label_smoothed_nll_loss / compute_accuracy, which are not in the reference tree), without writing log-probabilities:
 *   logits: fp32 rows (b, t), row (b*T2 + t) at logits + row*ldl, V <= 4096 classes; target: int32 [B, ldt].
 * A row counts when t < min(T2, ldt) (:151-152), target != pad_idx and t < lens[b]*len_mul (the clip-alone rule: a label
 * past the clip's own frames never scores logits computed from padding).  Per clip over its counted rows:
 *   nll = sum -lprob[target], smooth = sum_t sum_v -lprob[v] (= V*lse - sum_v logit), n_correct = #(argmax == target, first
 *   index on ties), n_tok = #rows.   loss = (1 - eps - eps/(V-1)) nll + eps/(V-1) smooth is the caller's.
 * ignore_prefix must be 0 (:154-160 is not built): anything else returns L2S_EUNSUPPORTED.  A target outside [0, V) is not counted.
 */
int l2s_unit_ce(const float* logits, int ldl, const int32_t* target, int ldt, const int32_t* lens, int len_mul, int B, int T2,
                int V, int pad_idx, int ignore_prefix, float* nll, float* smooth, int32_t* n_correct, int32_t* n_tok,
                void* stream);
/*
 * l2s_mel_l1_sc - the sums behind the masked L1 and spectral-convergence terms (criterion.py:63-89 and :189-201):
 *   pred: fp32 [B, Tm_pred, n_mels] (the conformer's [B*2T, 160] rows viewed 80 wide), targ: fp32 [B, Tm_targ, n_mels] zero-padded,
 *   both dense.  Per clip over rows t < min(lens[b]*len_mul, crop_len, Tm_pred, Tm_targ)  (len_mul = 4; crop_len as at :67):
 *   l1 = sum |p - t|, sq = sum (p - t)^2, tsq = sum t^2, n_rows = the row count.
 * The caller forms  l1 / n_mels [/ n_rows]  and  sqrt(sq) / sqrt(tsq) [* n_rows]  (:78-82, :199-200).
 */
int l2s_mel_l1_sc(const float* pred, int Tm_pred, const float* targ, int Tm_targ, const int32_t* lens, int len_mul, int B,
                  int n_mels, int crop_len, float* l1, float* sq, float* tsq, int32_t* n_rows, void* stream);
/*
 * l2s_ctc_loss - torch.nn.CTCLoss(blank, zero_infinity=True) forward per clip (criterion.py:45,103-112) straight from logits:
 *   logits: fp32 rows (b, t) of L frames per clip, V <= 4096; clip b uses its first min(lens[b]*len_mul, L) frames;
 *   targets: int32 concatenated labels, clip b's are targets[tgt_offs[b] .. + tgt_lens[b]); S_max >= every tgt_lens[b], <= 511.
 *   nll: fp32 [B] = -log p(labels | frames), 0 where that is infinite (no alignment: more labels, counting a blank between
 *   repeats, than frames) and for a clip without frames.  A clip with tgt_lens[b] > S_max or a label outside [0, V) gets NaN.
 * Two launches: every frame's log-sum-exp and the log-probabilities of the blank and the clip's labels go to the compact
 * workspace [B, L, S_max + 1] fp32; one workgroup per clip then runs the alpha recursion over the 2S+1 extended labels.
 * l2s_ctc_loss_workspace gives the bytes needed, 0 for an unsupported size (S_max > 511); such a call returns L2S_EUNSUPPORTED.
 */
size_t l2s_ctc_loss_workspace(int B, int L, int S_max);
int l2s_ctc_loss(const float* logits, int ldl, const int32_t* lens, int len_mul, int B, int L, int V, int blank,
                 const int32_t* targets, const int32_t* tgt_lens, const int32_t* tgt_offs, int S_max, void* workspace,
                 size_t workspace_bytes, float* nll, void* stream);

/*
 * Speech units from audio (extract_speech_units.sh:6-11: HuBERT-base features of transformer layer 6, quantised by a k-means
 * model).  Two entries; the rest of the path runs on l2s_tapgemm, l2s_layernorm and l2s_attention.
 *
 * l2s_wave_stem - layer 0 of fairseq's ConvFeatureExtractionModel in mode="default" (fairseq is not in the reference tree; the
 * script above loads it through hubert_base_ls960.pt), csrc/wavestem.hip:
 *   Conv1d(1 -> C, k = 10, stride 5, no bias), GroupNorm(C groups, C channels, affine, eps), erf GELU.
 *   wav: [B, S] samples with leading dimension ldw, fp32 in (-1, 1) or (wav_is_i16) int16 PCM taken as value / 32768;
 *   n_samples: int32 [B] clip lengths (clamped to S), NULL = every clip has S samples;
 *   w: fp32 [C, 10] taps, gamma / beta: fp32 [C];
 *   out: rows (b, t), row b*T_rows + t at out + row*ldo, C channels each - 16-bit, or fp32 with dtype = L2S_F32: the A operand
 *   of the L2S_MODE_CONV1D tap-GEMM of layer 1.
 * Each clip is normalised alone: clip b has L0 = (n_b - 10) / 5 + 1 frames (0 below 10 samples), the statistics of a channel
 * are taken over those frames only (biased variance), rows L0 <= t < T_rows are written as zeros.  T_rows >= (S - 10) / 5 + 1.
 * The statistics are accumulated in fp64 in a fixed order (no atomics): the same bits for a clip from run to run and whatever
 * its batch mates.  workspace: l2s_wave_stem_workspace bytes of device memory (0 = bad shape).  Supported: C = 512; other
 * widths return L2S_EUNSUPPORTED.  B <= 65535, S < 2^30.
 */
size_t l2s_wave_stem_workspace(int B, int C);
int l2s_wave_stem(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* w,
                  const float* gamma, const float* beta, float eps, void* out, int ldo, int T_rows, int C, void* workspace,
                  size_t workspace_bytes, int dtype, void* stream);
/*
 * l2s_kmeans_assign - nearest-centroid labels (avhubert/clustering/dump_km_label.py:26-52, ApplyKmeans.__call__: the argmin of
 * |x|^2 - 2 x C + |c|^2, here without the row-constant |x|^2), csrc/kmeans.hip.  Everything fp32, products on the f32-input
 * matrix instruction; the [M, K] distances are never written.
 *   x: fp32 rows (b, t), row b*T + t at x + row*ldx, D features; centers: fp32 [K, D]; cnorm: fp32 [K] = |c_k|^2;
 *   ids: int32 [B*T] = argmin_k (cnorm[k] - 2 x . c_k), the lowest index on a tie; -1 for rows t >= lens[b]*len_mul;
 *   best2: NULL or fp32 [B*T, 2] = (smallest, second smallest) of cnorm[k] - 2 x . c_k (zeros for masked rows).
 * Supported: D a multiple of 32 up to 1024, 2 <= K <= 1024; x and centers 16-byte aligned, ldx a multiple of 4.
 */
int l2s_kmeans_assign(const float* x, int ldx, const float* centers, const float* cnorm, const int32_t* lens, int len_mul, int B,
                      int T, int D, int K, int32_t* ids, float* best2, void* stream);

/*
 * Mini-batch k-means fit: what avhubert/clustering/learn_kmeans.py:25-47 (estimator arguments) and :88-121 (fit, score) ask of
 * scikit-learn's MiniBatchKMeans, csrc/kmeans_fit.hip; the host loop is lip2speech_unit_amd/kmeans_fit.py.  Everything fp32 in
 * memory; every sum is taken in a fixed order without floating-point atomics, so results are bit-identical from run to run.
 * Common to the four entries: x is fp32 [N, ldx] (16-byte aligned, ldx a multiple of 4, ldx >= D); a batch or subset of it is named
 * by `rows`, int32 positions into x (repeats are legal; an index outside [0, N) is read as the nearest valid row), or is the first
 * M rows when rows = NULL.  Supported: D a multiple of 32 up to 1024, 2 <= K <= 1024, N < 2^31 with rows.
 *
 * l2s_kmeans_nearest - one mini-batch assignment (the labels and inertia of a step, learn_kmeans.py:116, and of the score, :119):
 *   ids: NULL or int32 [M] = argmin_k |x - c_k|^2, the lowest index on a tie (the distance tile of l2s_kmeans_assign);
 *   dmin: NULL or fp32 [M] = max(0, |x|^2 + cnorm[k] - 2 x . c_k) at that k; inertia: NULL or one double = sum of dmin
 *   (32-row partials, then one finishing block).  workspace: l2s_kmeans_nearest_workspace(M) bytes, needed with inertia.
 *   M < 2^31 - 32.  The [M, K] distances are never written.
 * l2s_kmeans_update - the centre update of a step: for every centre with n > 0 members in the batch (ids[i] = k)
 *   c_k <- (c_k w_k + sum of its rows) / (w_k + n), w_k <- w_k + n; other centres and counts are copied.  Members are summed in
 *   ascending batch position.  centers_out / counts_out may be centers / counts themselves.  cnorm_out: fp32 [K] = |c_k|^2 of the
 *   new centres (summed in fp64).  Labels outside [0, K) belong to no centre.  workspace: l2s_kmeans_update_workspace(M, K)
 *   bytes (0 = unsupported).  M <= 2^24; counts are exact up to 2^24 samples per centre.
 * l2s_kmeans_pp_pot - greedy k-means++: cand int32 [t <= 16] are positions in the subset (0 .. m - 1); closest: fp32 [m] or NULL
 *   (= +inf).  Without closest_out: pot[j] = sum_i min(closest[i], |x_i - x_cand[j]|^2), doubles [t].  With closest_out (fp32 [m],
 *   may be closest itself): one candidate - cand[0] when t = 1 and select = NULL, or cand[argmin select[0..t)] (doubles, the
 *   first of equal ones) - gets closest_out[i] = min(closest[i], |x_i - x_cand|^2); pot (if given) [1] = their sum, chosen (if
 *   given, with select) [1] = that candidate's position.  The squared distance is the direct fp32 sum of (x - c)^2: exact on
 *   small integers.  workspace: l2s_kmeans_pp_workspace(m) bytes.  m < 2^31 - 64.
 * l2s_kmeans_pp_pick - searchsorted(cumsum(closest), thresholds, side = "left") clipped to m - 1, one block, prefix sums in
 *   fp64: threshold j = u[j] * (scale ? *scale : 1) (u, scale: doubles on the device), idx: int32 [t <= 16], total: NULL or one
 *   double = the sum of closest.  m <= 2^24.
 */
size_t l2s_kmeans_nearest_workspace(int M);
int l2s_kmeans_nearest(const float* x, int ldx, int64_t N, const int32_t* rows, int M, const float* centers, const float* cnorm,
                       int D, int K, int32_t* ids, float* dmin, double* inertia, void* workspace, size_t workspace_bytes,
                       void* stream);
size_t l2s_kmeans_update_workspace(int M, int K);
int l2s_kmeans_update(const float* x, int ldx, int64_t N, const int32_t* rows, int M, const int32_t* ids, const float* centers,
                      const float* counts, int D, int K, float* centers_out, float* counts_out, float* cnorm_out, void* workspace,
                      size_t workspace_bytes, void* stream);
size_t l2s_kmeans_pp_workspace(int m);
int l2s_kmeans_pp_pot(const float* x, int ldx, int64_t N, const int32_t* rows, int m, int D, const int32_t* cand, int t,
                      const float* closest, const double* select, double* pot, float* closest_out, int32_t* chosen,
                      void* workspace, size_t workspace_bytes, void* stream);
int l2s_kmeans_pp_pick(const float* closest, int m, const double* u, int t, const double* scale, int32_t* idx, double* total,
                       void* stream);

/*
 * Objective intelligibility of processed speech against its clean original, the numbers the reference publishes for every model
 * (README.md:103-122: STOI / ESTOI), csrc/stoi.hip; the host class is lip2speech_unit_amd/intelligibility.py.  Neither measure
 * is in the reference tree; they are the published algorithms of
 *   STOI:  C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen, "An algorithm for intelligibility prediction of time-frequency
 *          weighted noisy speech", IEEE Trans. Audio, Speech, Language Process. 19(7), 2011;
 *   ESTOI: J. Jensen, C. H. Taal, "An algorithm for predicting the intelligibility of speech masked by modulated noise maskers",
 *          IEEE/ACM Trans. Audio, Speech, Language Process. 24(11), 2016,
 * as restated in DESIGN.md section 17 (its steps 1-6 are cited below).  Four entries, one per observable stage.  Common to them:
 * clips are 16 kHz; n_samples: int32 [B] clip lengths (clamped to [0, S]) or NULL = S; a clip of n samples has
 * len = ceil(5 n / 8) samples at 10 kHz and frames(len) = ceil((len - 256) / 128) analysis frames (0 up to 256 samples).
 * Supported: S <= 419 840 (26 s: 2 048 frames), B <= 65535; more returns L2S_EUNSUPPORTED before anything is launched.  No
 * entry uses an atomic: a clip's results are the same bytes from run to run and whatever its batch mates are.
 *
 * l2s_stoi_resample - step 1 (Taal et al. section II: 10 kHz; the Octave-compatible resampler of the published code), one signal:
 *   wav: [B, S] with leading dimension ldw, fp32 in (-1, 1) or (wav_is_i16) int16 PCM taken as value / 32768;
 *   taps: fp32 [5][117], taps[p][q] = 5 w[p + 5 q] of the 581 normalised Kaiser taps w (0 where p + 5 q > 580);
 *   out: fp32 rows of R >= ceil(5 S / 8) samples, row b at out + b*ldo:  out[m] = sum_q taps[p][q] x[(8 m + 290 - p) / 5 - q],
 *   p = 3 m mod 5, q ascending as one fp32 fma chain, x = 0 outside the clip; zero for m >= len_b.
 * l2s_stoi_frames - step 2 (Taal et al. section II: frames 40 dB below the loudest are dropped), on the resampled CLEAN signal:
 *   x: fp32 rows (ldx >= ceil(5 S / 8)); window: fp32 [256] = hanning(258)[1:-1];
 *   kept: int32 [B, ldk], ldk >= frames(ceil(5 S / 8)): the indices j (ascending) of the frames with
 *   norm_j + 2^-52 > (max_j norm_j + 2^-52) / 100, norm_j = |window * x[128 j .. + 256)| with the squares summed in fp64; -1 past
 *   n_kept[b], the count.
 * l2s_stoi_bands - steps 2-3 (overlap-add of the kept frames; Taal et al. eq. (1): third-octave band magnitudes):
 *   x, y: the resampled clean and processed signals (same ldx); kept / n_kept as above (an index outside the clip's frames is
 *   skipped); basis: fp32 [256][512], 16-byte aligned, row n = sample of a frame with window[n] folded in, column
 *   c -> pass c / 256, wave (c % 256) / 64, part (c % 64) / 32 (0: cos, 1: -sin), lane c % 32, bin 7 + 128 pass + 32 wave + lane
 *   of the 512-point DFT (bins past 218 are not used); band_edges: int32 [16], band i sums bins [edges[i], edges[i+1]) within [7, 219);
 *   bands: fp32 [B, 2, 15, ldf] (0: clean, 1: processed), ldf >= frames - 1: column f < F_b = max(n_kept[b] - 1, 0) holds
 *   sqrt(sum over the band's bins, ascending, of re^2 + im^2) of frame f of the compacted signal, columns F_b <= f < ldf zeros.
 *   The compacted signal and the spectrum exist in LDS and registers only.
 * l2s_stoi_scores - steps 4-6 (Taal et al. eqs. (2)-(6) with N = 30, beta = -15 dB; Jensen & Taal eqs. (4)-(9)):
 *   seg: doubles [B, 2, lds], lds >= max(ldf - 29, 1): workspace; afterwards seg[b][0][s] = the sum over bands of segment s's
 *   clipped correlation, seg[b][1][s] = its ESTOI term, for s < n_segments[b] (the rest is unspecified);
 *   stoi / estoi: fp32 [B] = their means over the clip's segments (STOI also over the 15 bands), n_segments: int32 [B] =
 *   max(F_b - 29, 0); a clip without a segment gets 1e-5 for both, as the published code returns.  Terms are fp32, the sums
 *   over bands, frames and segments fp64 in index order.
 */
int l2s_stoi_resample(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* taps,
                      float* out, int64_t ldo, int R, void* stream);
int l2s_stoi_frames(const float* x, int64_t ldx, const int32_t* n_samples, int B, int S, const float* window, int32_t* kept, int ldk,
                    int32_t* n_kept, void* stream);
int l2s_stoi_bands(const float* x, const float* y, int64_t ldx, const int32_t* n_samples, int B, int S, const int32_t* kept, int ldk,
                   const int32_t* n_kept, const float* window, const float* basis, const int32_t* band_edges, float* bands, int ldf,
                   void* stream);
int l2s_stoi_scores(const float* bands, int ldf, const int32_t* n_kept, int B, double* seg, int lds, float* stoi, float* estoi,
                    int32_t* n_segments, void* stream);

/*
 * Speaker embeddings from audio: what helpers.py:185-198 (_get_speaker_embedding -> sv2s.utils.get_speaker_embedding, the GE2E
 * speaker encoder of Real-Time-Voice-Cloning, none of it in the reference tree) computes for create_dataset.py:94,133 and
 * server.py:115,207 - a float32 (256,) vector per clip.  The algorithm is restated in DESIGN.md section 18; the host class is
 * lip2speech_unit_amd/speaker_encoder.py.  Four entries; the input projections of the LSTM run on l2s_tapgemm (L2S_F32).
 * Everything is fp32 in memory, no entry uses an atomic, and every sum runs in a fixed order: a clip's (a sequence's) result is
 * the same bytes from run to run and whatever its batch (tile) mates are.
 *
 * l2s_wav_gain - the increase-only volume normalisation, csrc/spkemb.hip:
 *   wav: [B, S] with leading dimension ldw, fp32 in (-1, 1) or (wav_is_i16) int16 PCM taken as value / 32768;
 *   n_samples: int32 [B] clip lengths (clamped to [0, S]) or NULL = S;
 *   gain: fp32 [B] = 10^(change / 20) if change = target_dbfs - 10 log10(mean(wav^2)) > 0, else 1; the squares are summed in
 *   fp64.  A clip without samples or of zeros only has no level and gets 1.
 * l2s_stft_mel_power - 40-band power mel, librosa 0.8's melspectrogram(sr 16000, n_fft 400, hop 160, n_mels 40) with center = True,
 *   csrc/spkemb.hip: l2s_stft_mel's span layout (csrc/frame_dft.h) at a frame length that is no multiple of the hop, no sqrt, no log.
 *   frame t = samples [160 t - pad, 160 t - pad + 400) reflected once at either end against n_samples[b], re/im a k-ordered fp32
 *   fma chain, power = re^2 + im^2 (a square may be fused into the sum), band = sum over fb_range[j] in ascending bin order of fb * power.
 *   n_samples: int32 [B] ANALYSIS lengths (NULL = S): they set the frame count (n + 2 pad - 400) / 160 + 1 (0 unless n > pad
 *   and a frame fits) and the reflection, and may exceed S; n_valid: int32 [B] real samples (NULL = n_samples; clamped to
 *   min(n_samples, S)): positions from n_valid on are zeros and are never read - the zero padding of a clip shorter than its last
 *   partial window; scale: fp32 [B] or NULL, multiplied into every sample (after the int16 conversion) - l2s_wav_gain's output.
 *   basis: fp32 [400, 448]: row = sample of the frame, column c -> tile q = c / 32, lane l = c % 32, bin 32 (q / 2) + l; even
 *   tiles hold w cos, odd tiles -w sin (w: periodic Hann), zero columns for bins past 200; fb: fp32 [40, 201];
 *   fb_range: int32 [40, 2] = [first, past-last) non-zero bin of each band; mel: fp32 rows (b, t) at mel + (b*T_rows + t)*ldm;
 *   rows past the clip's frame count are zeros.  Supported: (n_fft, hop, n_mels) = (400, 160, 40), 0 <= pad <= 200, B <= 65535,
 *   S < 2^30; anything else returns L2S_EUNSUPPORTED.
 * l2s_lstm_layer - one LSTM layer's recurrence for S sequences of T steps from zero state, csrc/lstm.hip:
 *   xproj: fp32 [n_rows, ldx >= 1024], the input projection x W_ih^T + b_ih + b_hh with GATE-INTERLEAVED columns: column 4 u + g
 *   holds gate g (torch order i, f, g, o) of hidden unit u; row_off: int32 [S]: sequence s reads row row_off[s] + t at step t
 *   (offsets may overlap and come in any order - overlapping windows are gathered without a copy; a row outside [0, n_rows) is
 *   read as the nearest valid row); w_hh_p: fp32 [256 k][256 u][4 g] = weight_hh[256 g + u][k]; h_seq: NULL or fp32 [S, T, 256];
 *   h_last: NULL or fp32 [S, 256] = h at step T - 1 (at least one of the two).  One workgroup per 16 sequences, no
 *   synchronisation between workgroups; products on v_mfma_f32_16x16x4_f32 in a fixed k order, expf / tanhf and IEEE division in
 *   fp32.  A sequence's result does not depend on S or on the other sequences.  Supported: hidden = 256, any T >= 1, S >= 1,
 *   n_rows >= T; xproj and w_hh_p 16-byte aligned, ldx a multiple of 4.  Other hidden sizes return L2S_EUNSUPPORTED.
 * l2s_spk_embed_head - per clip b, over the windows h_last[first[b] .. first[b] + count[b]) (clamped to n_rows rows):
 *   e = relu(W h + bias), e / (|e| + 1e-5), the mean over the windows in index order, divided by its own L2 norm; norms and the
 *   mean are carried in fp64.  w_t: fp32 [256 k][256 u] = linear.weight[u][k] (transposed); out: fp32 [B, 256].  A clip whose
 *   mean is exactly zero (every ReLU output zero, or count = 0) gets zeros, where 0 / 0 would be NaN.  hidden must be 256.
 */
int l2s_wav_gain(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, float target_dbfs, float* gain,
                 void* stream);
int l2s_stft_mel_power(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, const int32_t* n_valid,
                       const float* scale, int B, int S, const float* basis, const float* fb, const int32_t* fb_range, float* mel,
                       int ldm, int T_rows, int n_fft, int hop, int n_mels, int pad, void* stream);
int l2s_lstm_layer(const float* xproj, int ldx, int64_t n_rows, const int32_t* row_off, const float* w_hh_p, int S, int T, int hidden,
                   float* h_seq, float* h_last, void* stream);
int l2s_spk_embed_head(const float* h_last, int n_rows, const int32_t* first, const int32_t* count, const float* w_t,
                       const float* bias, int B, int hidden, float* out, void* stream);

/*
 * Mouth ROIs from raw frames and 68-point landmarks: what avhubert/preparation/align_mouth.py:33-44 (warp_img / apply_transform:
 * skimage estimate_transform('similarity') + tf.warp), :63-87 (cut_patch) and :130-181 (crop_patch: the forward window of
 * landmarks, the tail rule) compute per frame on the host, and what the reference's server repeats on every request
 * (server.py:268-269, get_mouth_frames).  The algorithm is restated in DESIGN.md section 19; the host class is
 * lip2speech_unit_amd/mouth_roi.py, csrc/mouthroi.hip holds both entries.  All geometry is fp64; neither entry uses an atomic or
 * synchronises with the host, and a frame's bytes do not depend on the other clips of the batch.
 *
 * l2s_mouth_transforms - per clip b = rows [first[b], first[b] + count[b]) (clamped to [0, N)) of landmarks, T = count[b],
 *   margin = min(T, window_margin); for frame t of the clip:
 *   landmarks: fp64 [N, L, 2] (x, y); mean_face: fp64 [L, 2]; stable_ids: int32 [n_stable] (clamped to [0, L); n_stable <= 16);
 *   src = the mean over frames min(t, T - margin) .. + margin - 1 of the stable landmarks (a window looks forward and never leaves
 *   its clip; the last margin - 1 frames reuse the last full window's transform), dst = the mean face at the same ids;
 *   M = Umeyama's similarity src -> dst in its 2-D closed form: A = dst_c^T src_c / n, p = A00 + A11, q = A10 - A01, r = hypot(p, q),
 *   rotation [[p, -q], [q, p]] / r, scale r / (sum of the per-axis variances of src, ddof 0), translation dst_mean - s R src_mean;
 *   (cx, cy) = the mean of frame t's own landmarks [start_idx, stop_idx) through M, clamped in align_mouth.py's order
 *   (cy - crop_h/2 < 0 -> crop_h/2, then x, then cy + crop_h/2 > std_h -> std_h - crop_h/2, then x);
 *   inv: fp64 [N, 6] = the 2 x 3 matrix of M^-1, row-major; origin: int32 [N, 2] = (x0, y0) = (rint(cx) - crop_w/2, rint(cy) - crop_h/2),
 *   rint rounding half to even.  Rows of inv / origin that belong to no clip are not written.  Stable points of zero variance
 *   give NaN in inv (and origin 0): the host class reports them.
 * l2s_mouth_warp - per frame n, the crop_h x crop_w window at origin[n] of tf.warp(frame, inverse_map = inv[n], order 1,
 *   mode 'constant', cval 0), times 255, truncated to uint8; nothing outside the window is computed:
 *   frames: uint8 [N, H, W, C], C = 1 or 3 (any address); the output pixel (x, y) = (x0 + i, y0 + j) samples the source at
 *   (sx, sy) = ((inv0 x + inv1 y) + inv2, (inv3 x + inv4 y) + inv5), bilinearly over the four neighbours of (floor sx, floor sy) as
 *   ((1 - dy) ((1 - dx) tl + dx tr) + dy ((1 - dx) bl + dx br)) of the values u8 / 255.0, a neighbour outside the frame counting as
 *   0; every product and sum is rounded on its own (no fused multiply-add), channels independently;
 *   roi: NULL or uint8 [N, crop_h, crop_w, C]; gray: NULL or uint8 [N, crop_h, crop_w] = cv2's 8-bit BGR2GRAY
 *   (1868 B + 9617 G + 4899 R + 8192) >> 14 of the truncated ROI (C = 1: the ROI itself);
 *   model_in: NULL or fp32 [N, model_crop, model_crop] = ((gray / 255.0f) - mean) / std with fp32 divisions over the centre crop
 *   at offset (crop - model_crop) / 2 - hubert_dataset.py:242-245, bit-identical to numpy.  At least one output is needed; an
 *   output passed as NULL is not written.  roi, gray and model_in must be 4-byte aligned, inv 8-byte aligned.
 *   Supported: C in {1, 3}, H, W <= 32768, crop_h, crop_w <= 4096; anything else returns L2S_EUNSUPPORTED.
 */
int l2s_mouth_transforms(const double* landmarks, int N, int L, const int32_t* first, const int32_t* count, int B,
                         const double* mean_face, const int32_t* stable_ids, int n_stable, int window_margin, int std_h, int std_w,
                         int crop_h, int crop_w, int start_idx, int stop_idx, double* inv, int32_t* origin, void* stream);
int l2s_mouth_warp(const uint8_t* frames, int N, int H, int W, int C, const double* inv, const int32_t* origin, int crop_h, int crop_w,
                   uint8_t* roi, uint8_t* gray, float* model_in, int model_crop, float mean, float std, void* stream);

/*
 * One autoregressive decoder step against a key/value cache: the hot path of the Whisper speech recogniser the reference runs on
 * every synthesis request (server.py:48 `WhisperASR(model='base.en', ...)`, server.py:337-342 `asr.run(pred_audio_path)`), i.e.
 * of openai-whisper's greedy decoding (third-party; the arithmetic is restated in DESIGN.md section 20).  csrc/whisper_decode.hip
 * holds the three entries.  Whatever changes from step to step is read from DEVICE int32 scalars, never passed by value: a step
 * is a fixed launch sequence and can be replayed from a captured graph.  No atomics, every reduction in a fixed order: a clip's
 * bytes do not depend on its batch mates or on the run.
 *
 * l2s_kv_attention - one query per (clip, head) against a cache, heads 64 wide:
 *   q: 16-bit [B, ldq], head h = columns 64 h .. 64 h + 63, ALREADY scaled; k_cache / v_cache: 16-bit dense [B, cache_T, 64 H];
 *   n = the valid length: pos == NULL: n_valid (cross-attention: the encoder's 1500 rows); else p = pos[b * pos_stride]
 *   (pos_stride 0: one position for the batch, 1: per clip) and n = p + 1, clamped to [0, cache_T];
 *   k_new / v_new (both or neither; need pos): 16-bit [B, ld_new]; when 0 <= p < cache_T the rows are first stored at cache row p,
 *   and nothing else of the caches is written;
 *   out[b, 64 h + c] = sum_j softmax_j(q_bh . k_bjh) v_bjhc over j < n: fp32 dot products, fp32 online softmax (v_exp_f32),
 *   keys split over 128 lane groups of a block whose partials are merged in a fixed order, one rounding to 16 bits; n = 0 gives
 *   zeros.  Cache rows at or past n are never read (they may hold anything).
 *   Supported: 64 H <= 1280, cache_T <= 1500, B <= 65535; ldq, ldo, ld_new multiples of 8, pointers 16-byte aligned.
 * l2s_vocab_argmax - the tied output layer with the greedy choice fused in:
 *   x: 16-bit [B, ldx] (d used), emb: 16-bit [V, lde] (the token embedding); logit[b, v] = x_b . emb_v on the 16x16x32 MFMA, fp32
 *   accumulation, k ascending in steps of 32;  suppress / begin_suppress: NULL or uint8 [V], nonzero = the id may not be chosen;
 *   begin_suppress applies only when *step == first_step (step: device int32; needed with begin_suppress);
 *   token[b] = argmax over the allowed ids, the smallest id on a tie (-1 when none is allowed); logprob[b] = that logit's log
 *   softmax over the ALLOWED ids, fp32; logits: NULL or fp32 dense [B, V], the raw logits of every id, suppressed or not.
 *   Two levels: per 64-row tile a (maximum, first index, sum of exp(logit - maximum)) partial per clip, then a finishing block
 *   per clip; no [B, V] tensor unless asked for.  workspace: l2s_vocab_argmax_workspace(V, B) bytes (0 = unsupported).
 *   Supported: V <= 65536 (any value, no multiple of a tile), d a multiple of 64 up to 1280, any B >= 1.
 * l2s_whisper_advance - the bookkeeping of a step, one block; p = *pos:
 *   per clip: t = done[b] ? eot : token[b] (an id outside [0, V) counts as eot); token[b] = t; tokens[b, p] = t (int32
 *   [B, ld_tok]; skipped when p >= ld_tok); while not done: sum_logprob[b] += logprob[b] (the eot's included, as openai-whisper's
 *   sum_logprobs) and lengths[b] += 1 unless t is eot; done[b] |= (t == eot) (uint8);
 *   x_next[b, :d] = tok_emb[t] (16-bit [V, lde]) + pos_emb[p + 1] (fp32 dense [n_ctx, d]), fp32 - the next step's row of the
 *   residual stream; skipped when p + 1 >= n_ctx;  then *pos = p + 1 and *n_active = the number of clips not done.
 *   Supported: d a multiple of 8 up to 1280, V <= 65536, B <= 65535.
 */
/*
 * l2s_whisper_logmel - Whisper's input features as transformers' WhisperFeatureExtractor (and openai-whisper's
 *   log_mel_spectrogram + pad_or_trim) define them, csrc/whisper_logmel.hip:
 *   wav: [B, ldw] int16 (wav_is_i16; x / 32768) or fp32, S <= 480 000 columns used, n_samples[b] (NULL: S) real samples, clamped
 *   to [0, S]; the clip is zero-extended to 480 000 samples; frame t = samples [160 t - 200, 160 t + 200), t = 0 .. 2999 (the
 *   3 001st frame is dropped), positions outside [0, 480 000) reflected once; periodic Hann window of 400, power spectrum
 *   re^2 + im^2 (k-ordered fp32 fma chains on the f32-input MFMA), 80 bands mel[m] = sum_k fb[m, k] P[k], k ascending over
 *   fb_range[m] = [lo, hi); x = log10(max(mel, 1e-10)); x = max(x, clip_max - 8) with clip_max the maximum over the clip's
 *   3000 x 80 values (per 32-frame tile, then over the tiles: no atomics); y = (x + 4) / 4.
 *   basis: fp32 [400, 448] (the table of l2s_stft_mel_power), fb: fp32 [80, 201], fb_range: int32 [80, 2] - data of the caller;
 *   out: 16-bit rows [B * 3000, ld] time-major, ld >= 80 a multiple of 8, columns 80 .. ld - 1 written as zeros (conv1's
 *   tap-GEMM operand); out_f32: NULL or fp32 dense [B * 3000, 80], y before the rounding;
 *   workspace: l2s_whisper_logmel_workspace(B) bytes, 16-byte aligned.  S > 480 000 returns L2S_EUNSUPPORTED (one 30-s window).
 */
size_t l2s_whisper_logmel_workspace(int B);
int l2s_whisper_logmel(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                       const float* fb, const int32_t* fb_range, void* workspace, void* out, int ld, float* out_f32, int dtype,
                       void* stream);
int l2s_kv_attention(const void* q, int ldq, void* k_cache, void* v_cache, int cache_T, const void* k_new, const void* v_new, int ld_new,
                     const int32_t* pos, int pos_stride, int n_valid, int B, int H, void* out, int ldo, int dtype, void* stream);
size_t l2s_vocab_argmax_workspace(int V, int B);
int l2s_vocab_argmax(const void* x, int ldx, const void* emb, int lde, int B, int V, int d, const uint8_t* suppress,
                     const uint8_t* begin_suppress, const int32_t* step, int first_step, void* workspace, int32_t* token, float* logprob,
                     float* logits, int dtype, void* stream);
int l2s_whisper_advance(int32_t* token, const float* logprob, int32_t* tokens, int ld_tok, float* sum_logprob, int32_t* lengths,
                        uint8_t* done, const void* tok_emb, int lde, const float* pos_emb, int n_ctx, float* x_next, int ldx, int32_t* pos,
                        int32_t* n_active, int B, int V, int d, int eot, int dtype, void* stream);

/*
 * One beam-search step of the AV-HuBERT seq2seq lip reader (avhubert/hubert_asr.py:411-507, avhubert/decoder.py:38-243 and
 * fairseq's sequence_generator.py as avhubert/infer_s2s.py drives it; the arithmetic is restated in DESIGN.md section 21).
 * csrc/s2s_decode.hip holds the three entries.  As above, whatever changes from step to step is read from DEVICE memory: p = *step
 * is the position (the index of the newest token of every live slot; 0 = the initial eos), and the double-buffered tables
 * (tokens, anc, scores: leading dimension 2) are read at half p & 1 and written at half (p + 1) & 1.  No floating-point atomics,
 * every reduction in a fixed order, a block reads one clip only: a clip's bytes do not depend on its batch mates or on the run.
 * Row r = b * beam + slot everywhere.  n_live[b] is the number of live slots of clip b, finished[b] != 0 marks an inert clip.
 *
 * l2s_beam_attention - one query per (clip, beam slot, head), heads hd in {64, 128, 192} wide, W = H * hd:
 *   q: 16-bit [B * beam, ldq], head h = columns hd h .. hd h + hd - 1, ALREADY scaled; out: 16-bit [B * beam, ldo].
 *   Self form (k_new, v_new, anc, step given; enc_lens NULL): k_cache / v_cache 16-bit dense [B, beam, T, W] (T = L_max rows per
 *   slot), k_new / v_new 16-bit [B * beam, ld_new]; slot i stores its new rows at (b, i, p) - nothing else of the caches is
 *   written - and attends to keys t = 0 .. p: t < p from row (b, anc[p & 1][b, i, t], t), t = p from the new rows themselves.
 *   anc: int16 [2, B, beam, T], kept by l2s_beam_advance.  The caches are never reordered.
 *   Cross form (enc_lens given; k_new, v_new, anc NULL): k_cache / v_cache 16-bit dense [B, T, W] (T = T_enc), shared by the
 *   clip's slots; keys t < min(max(enc_lens[b], 0), T).  Rows at or past the valid length are never read.
 *   fp32 dot products, fp32 online softmax (v_exp_f32), 8 lane groups of a wave merged in a fixed order, one rounding to 16 bits.
 *   A slot >= n_live[b] (n_live NULL: none), a slot of a finished clip (finished NULL: none) or, in the self form, a position
 *   outside [0, T) writes zeros to out and nothing to the caches.  No valid key gives zeros.
 *   Supported: W <= 1536, beam <= 64, T <= 32767, B <= 65535; ldq, ldo, ld_new multiples of 8, 16-bit pointers 16-byte aligned.
 * l2s_beam_select - the 2 beam best continuations of a clip (sequence_generator.py:319-411 without prefix tokens or constraints):
 *   logits: fp32 [B * beam, ldl], V columns used; scores: fp32 [2, B, beam], the slots' cumulative scores (taken as 0 at p = 0).
 *   Per row, fp32: y = logits * (1 / temperature); lp = (y - max y) - log(sum exp(y - max y)); a NaN lp becomes -inf (a NaN logit
 *   makes its whole row -inf, as torch's log_softmax does); lp[pad] = -inf; lp[unk] -= unk_penalty; p >= max_len[b] leaves only
 *   eos finite; p < min_len makes eos -inf; s = lp + scores[p & 1][b, slot].  Slots considered: slot 0 alone at p = 0, else
 *   slots < n_live[b] (NULL: beam).  Output, K = 2 beam per clip: cand_score fp32 / cand_slot / cand_token int32 [B, K], s
 *   descending, a tie to the smaller flat index slot * V + token.  Radix select over the 64-bit keys (score bits, ~flat index) with
 *   integer LDS histograms.  A finished clip's outputs are left as they are.  n_live[b] is clamped to [1, beam]: a clip that is
 *   not finished always has a live slot (l2s_beam_advance sets n_live[b] = 0 only together with finished[b] = 1).
 *   Supported: beam <= 64, 2 beam + 2 <= V <= 8192; l2s_beam_select_workspace(V, beam) returns 0 for an unsupported size (the
 *   selection itself needs no global workspace).
 * l2s_beam_advance - the bookkeeping of a step (sequence_generator.py:413-557, 605-745), a block per clip that is not finished:
 *   walking the K candidates in order: token == eos: when its rank < beam, its score > -inf and the clip holds < beam hypotheses,
 *   it is finalised as hypothesis number nhyp[b]++ : hyp_tokens[b, n, :] = tokens[p & 1][b, parent, 1 .. p], eos, then pad;
 *   hyp_len = p + 1; hyp_score = score / (p + 1)^lenpen when normalize_scores, else score.  token != eos: the first `beam` such
 *   candidates become slots j = 0, 1, ... of the other half: tokens and anc rows 0 .. p copied from the parent slot,
 *   tokens[.., j, p + 1] = token, anc[.., j, p + 1] = j, scores[.., j] = score, parents[b, j] = parent slot,
 *   x_next[b * beam + j, :d] = embed_scale * emb[token] + pos_table[p + 1] (fp32; emb 16-bit [V, lde], pos_table fp32 dense
 *   [L, d], row t = the position embedding of token index t); n_live[b] = their count.
 *   The clip is finished when nhyp[b] == beam or p >= max_len[b]: then finished[b] = 1, n_live[b] = 0, no new slots are
 *   written and out_tokens / out_len / out_score [B, beam(, L)] receive the nhyp[b] hypotheses by score descending, ties in
 *   finalisation order.  When p + 1 >= L nothing is written.  Last: *step = p + 1, *n_active = the clips not finished.
 *   tokens: int32 [2, B, beam, L]; anc: int16 [2, B, beam, L]; hyp_* are the caller's work buffers.
 *   Supported: beam <= 64, V <= 8192, d a multiple of 8 up to 1536, L <= 32767, B <= 65535.
 */
int l2s_beam_attention(const void* q, int ldq, void* k_cache, void* v_cache, int T, const void* k_new, const void* v_new, int ld_new,
                       const int16_t* anc, const int32_t* step, const int32_t* enc_lens, const int32_t* n_live, const uint8_t* finished,
                       int B, int beam, int H, int hd, void* out, int ldo, int dtype, void* stream);
size_t l2s_beam_select_workspace(int V, int beam);
int l2s_beam_select(const float* logits, int ldl, const float* scores, const int32_t* step, const int32_t* max_len, const int32_t* n_live,
                    const uint8_t* finished, int B, int beam, int V, int pad, int unk, int eos, int min_len, float temperature,
                    float unk_penalty, float* cand_score, int32_t* cand_slot, int32_t* cand_token, void* stream);
int l2s_beam_advance(const float* cand_score, const int32_t* cand_slot, const int32_t* cand_token, int32_t* tokens, int16_t* anc,
                     float* scores, int32_t* n_live, uint8_t* finished, int32_t* parents, int32_t* hyp_tokens, int32_t* hyp_len,
                     float* hyp_score, int32_t* nhyp, int32_t* out_tokens, int32_t* out_len, float* out_score, const int32_t* max_len,
                     const void* emb, int lde, const float* pos_table, float embed_scale, float* x_next, int ldx, int32_t* step,
                     int32_t* n_active, int B, int beam, int L, int V, int d, int eos, int pad, float lenpen, int normalize_scores,
                     int dtype, void* stream);

/*
 * Log filterbank features of 16 kHz waveforms, as rows for AV-HuBERT's audio sub-model (csrc/logfbank.hip): in one launch the
 * python_speech_features.logfbank(wav, samplerate=16000) recipe at that library's defaults followed by the stacker, the alignment
 * to the video's frame count and the F.layer_norm of avhubert/hubert_dataset.py:299-315,370-372, restated in fp32.
 *   wav: int16 or fp32 [B, S] with row stride ldw, samples at INT16 SCALE either way (fp32 input is not rescaled);
 *   n_samples: int32 [B] clip lengths or NULL (all S); lengths above S are taken as S, lengths <= 0 give zero rows.
 * Per clip: y[0] = x[0], y[p] = x[p] - rn(0.97 x[p-1]) over the whole clip; frames of 400 samples every 160, zeros past the clip's
 * end, n_frames = 1 if n <= 400 else 1 + ceil((n - 400) / 160), no window; pspec[k] = fma(im, im, rn(re re)) / 512 of the 512-point
 * DFT, bins 0 .. 255; e[j] = sum_k fb[j][k] pspec[k] (k ascending over fb_range[j]); feat[j] = logf(e[j]), and the constant
 * float(log(2.220446049250313e-16)) for a sum that is exactly 0.  `stack` consecutive frames form one row of 26 stack columns; the frames the last row lacks
 * are 0.0 (padded after the log).  Clip b's rows at or past min(ceil(n_frames / stack), n_rows[b]) - to the end of its T_rows - are
 * written as zeros; n_rows NULL = the audio's own row count.  With normalize != 0 every row is (x - mean) / sqrt(var + 1e-5) with the
 * biased variance, two passes in fp32, the mean taken about the row's first value; an all-zero row stays zero, a constant row becomes zero.  Every clip is analysed alone.
 *   basis: fp32 [400][512], 16-byte aligned, row n = sample of the frame, column c: tile q = c / 32, lane l = c % 32, bin
 *     k = 32 (q / 2) + l; even q holds cos(2 pi k n / 512), odd q -sin(2 pi k n / 512).  Bin 256 has weight 0 in every band and no column.
 *   fb: fp32 [26][257] dense filterbank; fb_range: int32 [26][2] = [first, past-last) bin of each band's non-zero weights.
 *   out: fp32 (out_dtype L2S_F32) or 16-bit (L2S_F16 / L2S_BF16) [B, T_rows, 26 stack] with row stride ldo >= 26 stack; columns
 *     past 26 stack are not written.
 * Supported: stack 1 and 4; other values return L2S_EUNSUPPORTED.  B <= 65535, S < 2^30, T_rows stack <= 2^22.
 */
int l2s_logfbank(const void* wav, int wav_is_i16, int64_t ldw, const int32_t* n_samples, int B, int S, const float* basis,
                 const float* fb, const int32_t* fb_range, const int32_t* n_rows, void* out, int out_dtype, int ldo, int T_rows,
                 int stack, int normalize, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LIP2SPEECH_HIP_H */
