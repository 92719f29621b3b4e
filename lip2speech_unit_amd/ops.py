"""Thin torch-tensor front end over the C ABI (include/lip2speech_hip.h).

torch is used for device memory and the current HIP stream only; every function launches hand-written gfx950 kernels
through liblip2speech_hip.so and raises if the library is missing or rejects the call.  No function here computes.
"""
import ctypes
import os
from typing import Optional

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_LRELU, ACT_NONE, ACT_PRELU, ACT_RELU, ACT_SWISH, ACT_TANH, BF16, F16, F32, F_ACCUM,  # noqa: F401
                   F_DUAL, F_MASK, F_OUT_F32, F_RES_F32, F_RES_POST, F_RES_PRE, MODE_CONV1D, MODE_CONV2D,
                   MODE_LINEAR, GemmDesc, L2SError, check)

# operand / activation storage type of a dtype code (F32 = the fp32 reference-precision mode of stage 1)
_TORCH16 = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}
_DTYPE_NAME = {F16: "f16", BF16: "bf16", F32: "f32"}


class KernelProfiler:
    """Optional per-launch HIP-event timing (events recorded on the stream the kernels are launched on).
    Used by bench.py to find the dominant kernel and its achieved rate; never active on the product path by default."""

    def __init__(self, detail=False):
        self.records = []  # (key, flops, bytes, ev_start, ev_end, shape)
        self.detail = detail  # tap-GEMM keys also carry the problem shape (tools/kernel_table.py --detail)

    def summary(self):
        """Per kernel key: calls, ms, algorithmic flops / bytes, and the same split by problem shape (`shapes`: one kernel
        instantiation serves several GEMM shapes; a roofline of the pooled launches alone would average their intensities)."""
        torch.cuda.synchronize()
        agg = {}
        for key, fl, by, e0, e1, shape in self.records:
            a = agg.setdefault(key, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0, "shapes": {}})
            ms = e0.elapsed_time(e1)
            for t in (a, a["shapes"].setdefault(shape, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})):
                t["calls"] += 1
                t["ms"] += ms
                t["flops"] += fl
                t["bytes"] += by
        return agg


_profiler = None


def set_profiler(p):
    global _profiler
    _profiler = p


def _run(key, call, flops=0.0, nbytes=0.0, shape=None):
    if _profiler is None:
        return check(call(), key)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = call()
    e1.record()
    check(rc, key)
    _profiler.records.append((key, flops, nbytes, e0, e1, shape))


def torch_dtype(dtype: int) -> torch.dtype:
    return _TORCH16[dtype]


def dtype_code(t: torch.dtype) -> int:
    if t == torch.float16:
        return F16
    if t == torch.bfloat16:
        return BF16
    if t == torch.float32:
        return F32
    raise L2SError(f"unsupported operand dtype {t}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L2SError("HIP ops need device tensors (there is no CPU path)")
    return t.data_ptr()


def _req(t: torch.Tensor, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise L2SError(f"{name}: expected a device tensor (there is no CPU path)")
    if dtype is not None and t.dtype != dtype:
        raise L2SError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() >= 2 and t.stride(-1) != 1:
        raise L2SError(f"{name}: innermost dim must be contiguous")
    return t


def _extent(t: torch.Tensor) -> int:
    """Elements addressable from t's first element inside its own view (what a kernel may touch through t.data_ptr())."""
    if t.numel() == 0:
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))


def tapgemm(A, W, C, *, M, N, Cin, ntaps=1, lda=None, ldc=None, bias=None, slope=None, R=None, ldr=None, C2=None,
            ldc2=None, lens=None, mode=MODE_LINEAR, T_out=0, T_in=0, stride=1, dil=1, off=0, Ho=0, Wo=0, Hi=0, Wi=0,
            KW=1, pad=0, out_row_mul=1, out_row_add=0, mask_T=0, mask_mul=1, act=ACT_NONE, flags=0, dtype=F16,
            alpha=1.0, act_slope=0.0, slope2=0.0, groups=1, a_gstride=0, c_gstride=0, w_gstride=0, ktab=None, kflops=None):
    """One tap-GEMM launch. A/W/C/... are torch device tensors (or tensor views whose data_ptr is the origin).
    ktab: int32 [groups, 2 + 2*9] K-block table (include/lip2speech_hip.h, l2s_gemm_desc::ktab); kflops: the FLOPs such a launch
    really does (the profiler's count; default: the dense M x N x K figure)."""
    lib = _lib.load()
    d = GemmDesc()
    d.A, d.W, d.C = _ptr(A), _ptr(W), _ptr(C)
    d.C2, d.bias, d.slope, d.R, d.lens = _ptr(C2), _ptr(bias), _ptr(slope), _ptr(R), _ptr(lens)
    if bias is not None and bias.dtype != torch.float32:
        raise L2SError("bias must be fp32")
    if lens is not None and lens.dtype != torch.int32:
        raise L2SError("lens must be int32")
    d.M, d.N, d.Cin, d.ntaps = M, N, Cin, ntaps
    d.lda = lda if lda is not None else Cin
    d.ldc = ldc if ldc is not None else N * groups
    d.ldc2 = ldc2 if ldc2 is not None else d.ldc
    d.ldr = ldr if ldr is not None else d.ldc
    d.mode = mode
    d.T_out, d.T_in, d.stride, d.dil, d.off = T_out, T_in, stride, dil, off
    d.Ho, d.Wo, d.Hi, d.Wi, d.KW, d.pad = Ho, Wo, Hi, Wi, KW, pad
    d.out_row_mul, d.out_row_add = out_row_mul, out_row_add
    d.mask_T, d.mask_mul = mask_T, mask_mul
    if C.dtype == torch.float32:
        flags |= F_OUT_F32
    if R is not None and R.dtype == torch.float32:
        flags |= F_RES_F32
    d.act, d.flags, d.dtype = act, flags, dtype
    d.alpha, d.act_slope, d.slope2 = alpha, act_slope, slope2
    d.groups, d.a_gstride, d.c_gstride, d.w_gstride = groups, a_gstride, c_gstride, w_gstride
    if ktab is not None:
        if ktab.dtype != torch.int32 or ktab.dim() != 2 or ktab.shape != (groups, 20) or not ktab.is_contiguous():
            raise L2SError("ktab: int32 [groups, 20], contiguous")
        d.ktab = _ptr(ktab)
    if _profiler is None:
        check(lib.l2s_tapgemm(ctypes.byref(d), _stream()), "l2s_tapgemm")
        return
    var = lib.l2s_tapgemm_variant(ctypes.byref(d))
    key = f"tapgemm<{_DTYPE_NAME[dtype]},{var // 1000 % 1000}x{var % 1000},mode{mode}>"   # (fp32: variant 2128128 -> 128x128)
    if _profiler is not None:  # one kernel instantiation per epilogue family: name it like rocprofv3 sees it
        fam = lib.l2s_tapgemm_epilogue_family(ctypes.byref(d))
        if var in (999064, 999128):  # patchconv.hip builds 5 of the 10 families; the others run on a superset
            fam = {0: 2, 1: 3, 2: 2, 3: 3, 6: 6, 7: 7}.get(fam, 9)
        key = key[:-1] + f",e{fam}>"
    if _profiler is not None and _profiler.detail:
        key += f" M{M} N{N} Cin{Cin} taps{ntaps} g{groups} fl{flags:#x} act{act} alpha{alpha:g}"
    ktot = Cin * ntaps
    osz = 4 if dtype == F32 else 2
    esz = 4 if (flags & F_OUT_F32) else osz
    # algorithmic bytes: A once, W once, C written once; + the residual read, the second output, the accumulate read
    mn = float(M) * N * groups
    nbytes = float(osz) * M * ktot * groups / max(ntaps, 1) + float(osz) * N * ktot * groups + esz * mn
    if R is not None:
        nbytes += (4 if (flags & F_RES_F32) else osz) * mn
    if flags & F_DUAL:
        nbytes += osz * mn
    if flags & F_ACCUM:
        nbytes += esz * mn
    _run(key, lambda: lib.l2s_tapgemm(ctypes.byref(d), _stream()), kflops if kflops is not None else 2.0 * M * N * ktot * groups, nbytes,
         shape=f"M{M} N{N * groups} K{ktot}" + (" ktab" if ktab is not None else ""))


def stem_conv3d(x, w, bias, slope, y, B, T, dtype):
    lib = _lib.load()
    _run("l2s_stem_conv3d", lambda: lib.l2s_stem_conv3d(_ptr(x), int(x.dtype == torch.float32), _ptr(w), _ptr(bias), _ptr(slope), _ptr(y), B, T,
                              x.shape[-2], x.shape[-1], dtype, _stream()))


def stem_pool_fused(x, w, bias, slope, y, B, T, dtype):
    lib = _lib.load()
    _run("l2s_stem_pool_fused", lambda: lib.l2s_stem_pool_fused(
        _ptr(x), int(x.dtype == torch.float32), _ptr(w), _ptr(bias), _ptr(slope), _ptr(y), B, T, x.shape[-2], x.shape[-1],
        dtype, _stream()), flops=2.0 * B * T * 44 * 44 * 64 * 245,
        nbytes=B * T * (88 * 88 * (4 if x.dtype == torch.float32 else 2) + 22 * 22 * 64 * 2))


def stem_pool_fused_u8(frames, w, bias, slope, y, B, T, dtype, crop=88, mean=0.421, std=0.165):
    """Fused stem on raw uint8 frames [B,T,Hin,Win]: crop + normalise in the slab fetch (hubert_dataset.py:242-245)."""
    lib = _lib.load()
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError("frames: uint8 [B,T,Hin,Win]")
    Hin, Win = frames.shape[-2], frames.shape[-1]
    _run("l2s_stem_pool_fused", lambda: lib.l2s_stem_pool_fused_u8(
        _ptr(frames), Hin, Win, crop, mean, std, _ptr(w), _ptr(bias), _ptr(slope), _ptr(y), B, T, dtype, _stream()),
        flops=2.0 * B * T * 44 * 44 * 64 * 245, nbytes=B * T * (crop * crop + 22 * 22 * 64 * 2))


def maxpool2d_3x3s2(x, y, N, H, W, C, dtype):
    _run("l2s_maxpool2d_3x3s2", lambda: _lib.load().l2s_maxpool2d_3x3s2(_ptr(x), _ptr(y), N, H, W, C, dtype, _stream()))


def avgpool_hw(x, y, N, HW, C, dtype):
    _run("l2s_avgpool_hw", lambda: _lib.load().l2s_avgpool_hw(_ptr(x), _ptr(y), N, HW, C, dtype, _stream()))


def layernorm(x, gamma, beta, eps, y, *, M, C, ldx=None, ldy=None, y2=None, ldy2=0, zero_prefix=0, lens=None,
              len_mul=1, mask_T=0, dtype=F16):
    ldx = ldx if ldx is not None else C
    ldy = ldy if ldy is not None else C + zero_prefix
    _run("l2s_layernorm", lambda: _lib.load().l2s_layernorm(_ptr(x), int(x.dtype == torch.float32), ldx, _ptr(gamma), _ptr(beta), eps, _ptr(y),
                                    int(y.dtype == torch.float32), ldy, _ptr(y2), ldy2, M, C, zero_prefix,
                                    _ptr(lens), len_mul, mask_T, dtype, _stream()))


def attention(qkv, out, *, B, T, H, ldq=None, ldo=None, pos=None, ldp=0, bias_u=None, bias_v=None, lens=None,
              len_mul=1, dtype=F16):
    ldq = ldq if ldq is not None else 3 * H * 64
    ldo = ldo if ldo is not None else H * 64
    _run("l2s_attention", lambda: _lib.load().l2s_attention(_ptr(qkv), ldq, _ptr(out), ldo, _ptr(pos), ldp, _ptr(bias_u), _ptr(bias_v),
                                    _ptr(lens), len_mul, B, T, H, dtype, _stream()))


def glu_dwconv_swish(x, w, bias, y, *, B, T, C, k, lens=None, len_mul=1, dtype=F16):
    _run("l2s_glu_dwconv_swish", lambda: _lib.load().l2s_glu_dwconv_swish(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), _ptr(lens), len_mul, B, T, C, k,
                                           dtype, _stream()))


def greedy_decode(logits, tokens, lprobs, score, *, B, T2, V, ldl=None, lens=None, len_mul=1, temperature=1.0,
                  lenpen=1.0):
    ldl = ldl if ldl is not None else V
    _run("l2s_greedy_decode", lambda: _lib.load().l2s_greedy_decode(_ptr(logits), ldl, _ptr(lens), len_mul, B, T2, V, temperature, lenpen,
                                        _ptr(tokens), _ptr(lprobs), _ptr(score), _stream()))


def beam_decode(logits, *, B, T2, V, beam, ldl=None, lens=None, len_mul=1, temperature=1.0, lenpen=1.0):
    """n-best decode (the reference's beam search, one wave per clip).  Returns device tensors (tokens int32 [B,beam,T2+1],
    positional scores fp32 [B,beam,T2+1], score fp32 [B,beam], nhyp int32 [B])."""
    lib = _lib.load()
    dev = logits.device
    ldl = ldl if ldl is not None else V
    nbytes = lib.l2s_beam_decode_workspace(B, T2, beam)
    if nbytes == 0:
        raise L2SError("l2s_beam_decode_workspace: bad shape")
    work = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    tokens = torch.empty(B, beam, T2 + 1, device=dev, dtype=torch.int32)
    pos = torch.empty(B, beam, T2 + 1, device=dev, dtype=torch.float32)
    score = torch.empty(B, beam, device=dev, dtype=torch.float32)
    nhyp = torch.empty(B, device=dev, dtype=torch.int32)
    _run("l2s_beam_decode", lambda: lib.l2s_beam_decode(_ptr(_req(logits, torch.float32, "logits")), ldl, _ptr(lens), len_mul, B, T2, V,
                                                          temperature, lenpen, beam, _ptr(work), nbytes, _ptr(tokens), _ptr(pos),
                                                          _ptr(score), _ptr(nhyp), _stream()))
    return tokens, pos, score, nhyp


def ctc_frames(logits, labels, topk_cls, topk_lp, *, B, L, V, K, ldl=None, lens=None, len_mul=1):
    """CTC text head outputs per frame (fp32 softmax of logits [B*L, ldl]): labels int32 [B, L] = framewise argmax, and with
    K > 0 the top-K classes topk_cls int32 / topk_lp fp32 [B, L, K] (log(p + FLT_MIN), p descending)."""
    ldl = ldl if ldl is not None else V
    _run("l2s_ctc_frames", lambda: _lib.load().l2s_ctc_frames(
        _ptr(_req(logits, torch.float32, "logits")), ldl, _ptr(lens), len_mul, B, L, V, K, _ptr(_req(labels, torch.int32, "labels")),
        _ptr(topk_cls), _ptr(topk_lp), _stream()))


def ctc_beam_search(topk_cls, topk_lp, workspace, labels, lengths, scores, *, B, L, K, beam, nbest, lens=None, len_mul=1):
    """CTC prefix beam search (ctcdecode without LM) over ctc_frames' top-K: labels int32 [B, nbest, L], lengths int32
    [B, nbest], scores fp32 [B, nbest] (-log p of the prefix, best first).  workspace: ctc_beam_workspace(B, L, beam) bytes."""
    _run("l2s_ctc_beam_search", lambda: _lib.load().l2s_ctc_beam_search(
        _ptr(_req(topk_cls, torch.int32, "topk_cls")), _ptr(_req(topk_lp, torch.float32, "topk_lp")), _ptr(lens), len_mul, B, L, K,
        beam, nbest, _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(_req(labels, torch.int32, "labels")),
        _ptr(_req(lengths, torch.int32, "lengths")), _ptr(_req(scores, torch.float32, "scores")), _stream()))


def ctc_repeat_labels(x, y, *, B, L, ldx=None, ldy=None, lens=None, len_mul=1):
    """REPEAT_TEXT_LABELS: y[b, t] = the last non-zero label of x[b, :t+1] (0 if none; 0 past lens[b]*len_mul).  int32."""
    _run("l2s_ctc_repeat_labels", lambda: _lib.load().l2s_ctc_repeat_labels(
        _ptr(_req(x, torch.int32, "x")), ldx or x.stride(0), _ptr(lens), len_mul, B, L, _ptr(_req(y, torch.int32, "y")),
        ldy or y.stride(0), _stream()))


def ctc_beam_workspace_bytes(B, L, beam):
    n = _lib.load().l2s_ctc_beam_workspace(B, L, beam)
    if n == 0:
        raise L2SError(f"l2s_ctc_beam_workspace: unsupported size (B={B}, L={L}, beam={beam})")
    return n


def ctc_decode(logits, *, B, L, V, ldl=None, lens=None, len_mul=1, beam=0, K=40, nbest=3):
    """Text decode of the CTC head, all on the device (no host sync: capturable).  Returns {"text": int32 [B, L] framewise
    argmax} and, with beam > 0 (CTC_BS_DECODING=1: beam 30, cutoff_top_n 40, top 3), "text_beams" int32 [B, nbest, L],
    "text_lens" int32 [B, nbest], "text_scores" fp32 [B, nbest]."""
    dev = logits.device
    labels = torch.empty(B, L, device=dev, dtype=torch.int32)
    if beam <= 0:
        ctc_frames(logits, labels, None, None, B=B, L=L, V=V, K=0, ldl=ldl, lens=lens, len_mul=len_mul)
        return {"text": labels}
    K = min(K, V)
    nbest = min(nbest, beam)
    tc = torch.empty(B, L, K, device=dev, dtype=torch.int32)
    tl = torch.empty(B, L, K, device=dev, dtype=torch.float32)
    ctc_frames(logits, labels, tc, tl, B=B, L=L, V=V, K=K, ldl=ldl, lens=lens, len_mul=len_mul)
    work = torch.empty(ctc_beam_workspace_bytes(B, L, beam) // 8, device=dev, dtype=torch.int64)
    beams = torch.empty(B, nbest, L, device=dev, dtype=torch.int32)
    blen = torch.empty(B, nbest, device=dev, dtype=torch.int32)
    bsc = torch.empty(B, nbest, device=dev, dtype=torch.float32)
    ctc_beam_search(tc, tl, work, beams, blen, bsc, B=B, L=L, K=K, beam=beam, nbest=nbest, lens=lens, len_mul=len_mul)
    return {"text": labels, "text_beams": beams, "text_lens": blen, "text_scores": bsc}


def repeat2_cast(x, y, B, T, C, dtype):
    _run("l2s_repeat2_cast", lambda: _lib.load().l2s_repeat2_cast(_ptr(x), _ptr(y), B, T, C, dtype, _stream()))


def splitk_reduce(P, x, *, M, N, S, ldp=None, ldx=None):
    """x[m, n] += sum_{s < S} P[m, s*N + n] (fp32, s ascending): the tail of a split-K residual-stream Linear at small M."""
    _run("l2s_splitk_reduce", lambda: _lib.load().l2s_splitk_reduce(_ptr(P), ldp or S * N, S, _ptr(x), ldx or N, M, N, _stream()))


# Residual-stream Linears at small M (one clip per request: M = 100-500 rows).  A 64 x 64-tile GEMM then fills 32-64 of the 256
# CUs for K / 64 serial K-tiles; cut into S slices of K (one grouped launch, groups = S) it fills them all for K / (64 S), and
# l2s_splitk_reduce folds the fp32 partial products into the stream in a fixed order.
SPLITK_MAX_M = 512
_SPLITK_ON = os.environ.get("L2S_SPLITK", "1") != "0"       # A/B: 0 = the one-launch form at every M


def splitk_slices(M, N, K):
    """K slices for the residual-stream Linear x[M, N] += A[M, K] W^T (0 = one launch as before): the largest power of two <= 8
    that keeps >= 256 columns of K per slice.  M only switches the form on (<= SPLITK_MAX_M rows): the slice count - and with it
    the re-packed weight a layer caches - depends on the layer alone, so whatever batch first takes the split path builds the
    state every later one reads (pipeline.forward_device_u8_streams primes shared state with ONE clip on the caller's stream)."""
    if not _SPLITK_ON or M > SPLITK_MAX_M or K < 1024 or (N & 63):
        return 0
    S = 8
    while S > 1 and (K % (S * 64) or K // S < 256):
        S //= 2
    return S if S > 1 else 0


def splitk_reduce_layernorm(P, x, gamma, beta, eps, y, *, M, C, S, ldp=None, ldx=None, ldy=None, lens=None, len_mul=1, mask_T=0,
                            dtype=F16):
    """splitk_reduce(P, x) and layernorm(x) -> y in one launch (C = 1024 / 512; y may be x itself in fp32)."""
    _run("l2s_splitk_reduce_layernorm", lambda: _lib.load().l2s_splitk_reduce_layernorm(
        _ptr(P), ldp or S * C, S, _ptr(x), ldx or C, _ptr(gamma), _ptr(beta), eps, _ptr(y), int(y.dtype == torch.float32), ldy or C,
        M, C, _ptr(lens), len_mul, mask_T, dtype, _stream()))


def residual_linear(A, W, bias, x, *, M, N, K, dtype, alpha=1.0, cache=None, key=None, ln=None):
    """x (fp32 residual stream, in place) += alpha * (A W^T + bias).  cache / key: where the [S][N][K / S] repack of W and the
    slice-0-only bias of the split-K form are kept (a layer's dict of packed weights).
    ln = (gamma, beta, eps, y): the LayerNorm that follows the update, y = LayerNorm(x) (y may be x) - always applied; in the
    split-K form it rides in the reduction's launch."""
    S = 0 if dtype == F32 else splitk_slices(M, N, K)   # fp32: one tap-GEMM with R = x in place, then l2s_layernorm
    if not S:
        tapgemm(A, W, x, M=M, N=N, Cin=K, bias=bias, alpha=alpha, R=x, ldr=N, flags=F_RES_POST, dtype=dtype)
        if ln is not None:
            layernorm(x, ln[0], ln[1], ln[2], ln[3], M=M, C=N, dtype=dtype)
        return
    ck = (key, S)
    if cache is None or ck not in cache:
        ws = W.view(N, S, K // S).permute(1, 0, 2).contiguous()
        bs = torch.zeros(S * N, device=W.device, dtype=torch.float32)
        if bias is not None:
            bs[:N] = bias
        if cache is not None:
            cache[ck] = (ws, bs)
    else:
        ws, bs = cache[ck]
    P = torch.empty(M, S * N, device=x.device, dtype=torch.float32)
    tapgemm(A, ws, P, M=M, N=N, Cin=K // S, lda=K, ldc=S * N, bias=bs, alpha=alpha, groups=S, a_gstride=K // S, c_gstride=N,
            w_gstride=N * (K // S), dtype=dtype)
    if ln is not None and N in (512, 1024):
        splitk_reduce_layernorm(P, x, ln[0], ln[1], ln[2], ln[3], M=M, C=N, S=S, dtype=dtype)
        return
    splitk_reduce(P, x, M=M, N=N, S=S)
    if ln is not None:
        layernorm(x, ln[0], ln[1], ln[2], ln[3], M=M, C=N, dtype=dtype)


def cast_f32_to_16(x, y, M, C, dtype, ldx=None, ldy=None):
    _run("l2s_cast_f32_to_16", lambda: _lib.load().l2s_cast_f32_to_16(_ptr(x), ldx or C, _ptr(y), ldy or C, M, C, dtype, _stream()))


def cast_16_to_f32(x, y, M, C, dtype, ldx=None, ldy=None):
    _run("l2s_cast_16_to_f32", lambda: _lib.load().l2s_cast_16_to_f32(_ptr(x), ldx or C, _ptr(y), ldy or C, M, C, dtype, _stream()))


def broadcast_rows(v, y, *, B, T, C, ldy, col0=0, ldv=None, lens=None, len_mul=1, dtype=F16):
    _run("l2s_broadcast_rows", lambda: _lib.load().l2s_broadcast_rows(_ptr(v), ldv or C, _ptr(y), ldy, col0, _ptr(lens), len_mul, B, T, C,
                                         int(v.dtype == torch.float32), dtype, _stream()))


def transpose_ct_to_tc(x, y, *, B, C, T, ldy, col0=0, lens=None, len_mul=1, dtype=F16):
    _run("l2s_transpose_ct_to_tc", lambda: _lib.load().l2s_transpose_ct_to_tc(_ptr(x), _ptr(y), ldy, col0, _ptr(lens), len_mul, B, C, T, dtype,
                                             _stream()))


def embedding(code, table, y, *, B, L, C, ldy=None, lens=None, dtype=F16):
    _run("l2s_embedding", lambda: _lib.load().l2s_embedding(_ptr(code), _ptr(table), _ptr(y), ldy or C, _ptr(lens), B, L, C, dtype, _stream()))


def embedding_tokens(tok, table, y, *, B, L, C, token_offset=4, ldt=None, ldy=None, lens=None, len_mul=1, dtype=F16):
    _run("l2s_embedding_tokens", lambda: _lib.load().l2s_embedding_tokens(
        _ptr(tok), ldt or tok.shape[-1], token_offset, _ptr(table), table.shape[0], _ptr(y), ldy or C, _ptr(lens), len_mul, B, L, C,
        dtype, _stream()))


def rows_f32_to_16_masked(x, y, *, B, T, C, ldx=None, ldy=None, col0=0, lens=None, len_mul=1, dtype=F16):
    _run("l2s_rows_f32_to_16_masked", lambda: _lib.load().l2s_rows_f32_to_16_masked(
        _ptr(x), ldx or C, _ptr(y), ldy or C, col0, _ptr(lens), len_mul, B, T, C, dtype, _stream()))


def lens_from_mask(padding_mask, B, T, device):
    """int32 [B] = T - padding_mask.sum(-1) (sequence_generator.py:64-65) on the device, no host sync; None = no padding."""
    import torch
    lens = torch.empty(B, device=device, dtype=torch.int32)
    if padding_mask is not None:
        assert padding_mask.dtype == torch.bool and padding_mask.shape == (B, T) and padding_mask.is_contiguous()
    _run("l2s_lens_from_mask", lambda: _lib.load().l2s_lens_from_mask(_ptr(padding_mask), _ptr(lens), B, T, _stream()))
    return lens


def basicblock_fused(x, w1, b1, s1, w2, b2, s2, y, *, n_images, H, W, C=64, dtype=F16):
    M = float(n_images) * H * W
    _run("l2s_basicblock_fused", lambda: _lib.load().l2s_basicblock_fused(
        _ptr(x), _ptr(w1), _ptr(b1), _ptr(s1), _ptr(w2), _ptr(b2), _ptr(s2), _ptr(y), n_images, H, W, C, dtype, _stream()),
        flops=2.0 * 2 * M * C * C * 9, nbytes=2 * 2 * M * C)


def basicstage128_tail_fused(x0, t0, wa, ba, sa, w1, b1, s1, w2, b2, s2, y, *, n_images, H, W, dtype=F16):
    """The strided 128-channel stage behind its first conv in one launch (csrc/basicblock_phase.hip, TAIL): block 1's second conv
    with the 1x1 stride-2 downsample of the stage input x0 as one more K-tile of the same accumulation, then block 2 on the
    LDS-resident result.  wa: [128][9*128 + 64 + 64] = conv weights | downsample weights | zeros; ba: both folded biases summed."""
    M = float(n_images) * H * W
    _run("l2s_basicstage128_tail_fused", lambda: _lib.load().l2s_basicstage128_tail_fused(
        _ptr(x0), _ptr(t0), _ptr(wa), _ptr(ba), _ptr(sa), _ptr(w1), _ptr(b1), _ptr(s1), _ptr(w2), _ptr(b2), _ptr(s2), _ptr(y),
        n_images, H, W, dtype, _stream()),
        flops=2.0 * M * 128 * (3 * 9 * 128 + 64), nbytes=2 * M * (128 + 64 + 128))


def basiclayer_fused(x, ws, biases, slopes, y, *, n_images, H, W, C=64, dtype=F16):
    """len(ws) / 2 BasicBlocks of the 64-channel stage in one launch (csrc/basicblock.hip): ws / biases / slopes list conv1, conv2
    of block 0, conv1, conv2 of block 1, ..."""
    n = len(ws)
    if n % 2 or len(biases) != n or len(slopes) != n:
        raise L2SError("basiclayer_fused: 2 * n_blocks weights, biases and slopes")
    wp = (ctypes.c_void_p * n)(*[_ptr(_req(w, _TORCH16[dtype], "w")) for w in ws])
    bp = (ctypes.c_void_p * n)(*[_ptr(_req(b_, torch.float32, "bias")) for b_ in biases])
    sp = (ctypes.c_void_p * n)(*[_ptr(_req(s_, torch.float32, "slope")) for s_ in slopes])
    M = float(n_images) * H * W
    _run("l2s_basiclayer_fused", lambda: _lib.load().l2s_basiclayer_fused(
        _ptr(x), wp, bp, sp, n // 2, _ptr(y), n_images, H, W, C, dtype, _stream()),
        flops=2.0 * n * M * C * C * 9, nbytes=2 * 2 * M * C)


def split_hi_lo(x, hi, lo, *, B, T, C, act=0, slope=0.0, ldx=None, ld16=None, lens=None, len_mul=1, dtype=F16):
    _run("l2s_split_hi_lo", lambda: _lib.load().l2s_split_hi_lo(_ptr(x), ldx or C, _ptr(hi), _ptr(lo), ld16 or C, act, float(slope),
                                                                _ptr(lens), len_mul, B, T, C, dtype, _stream()))


def conv_post_tanh(x, w, bias, wav, pcm, *, B, T, C, k, lens=None, len_mul=1):
    _run("l2s_conv_post_tanh", lambda: _lib.load().l2s_conv_post_tanh(_ptr(x), _ptr(w), float(bias), _ptr(wav), _ptr(pcm), _ptr(lens), len_mul, B,
                                         T, C, k, _stream()))


def resblock_fused(xl, w, bias, xs, xl_out, *, B, T, C, k, dil, accumulate, slope, lens=None, len_mul=1, dtype=F16):
    _run(f"l2s_resblock_fused<C{C},k{k}>", lambda: _lib.load().l2s_resblock_fused(
        _ptr(xl), _ptr(w), _ptr(bias), _ptr(xs), _ptr(xl_out), _ptr(lens), len_mul, B, T, C, k, dil[0], dil[1], dil[2],
        int(bool(accumulate)), float(slope), dtype, _stream()),
        flops=2.0 * B * T * C * C * k * 6, nbytes=B * T * C * (2 + 4 + (4 if accumulate else 0) + (2 if xl_out is not None else 0)))


def resstage_fused(xl, ws, biases, xs, xl_out, *, B, T, C, ks, dils, slope, lens=None, len_mul=1, dtype=F16, xs_final=True):
    """The three ResBlocks (k = 3, 7, 11) of a narrow stage in one launch (csrc/resblock.hip): xs = sum_j rb_j(x),
    xl_out = leaky_relu(xs).  ws / biases: per-ResBlock fused layouts of resblock_fused; dils: per-ResBlock dilations.
    xs_final=False: xs is only the running sum's scratch (nobody reads the stage's fp32 sum), its last pass is not written."""
    n = len(ws)
    wp = (ctypes.c_void_p * n)(*[_ptr(_req(w, _TORCH16[dtype], "w")) for w in ws])
    bp = (ctypes.c_void_p * n)(*[_ptr(_req(b_, torch.float32, "bias")) for b_ in biases])
    kk = (ctypes.c_int * n)(*[int(k) for k in ks])
    dd = (ctypes.c_int * (3 * n))(*[int(d) for dl in dils for d in dl])
    if xs.dtype != torch.float32:
        raise L2SError("xs must be fp32")
    _run(f"l2s_resstage_fused<C{C}>", lambda: _lib.load().l2s_resstage_fused(
        _ptr(_req(xl, _TORCH16[dtype], "xl")), wp, bp, kk, dd, n, _ptr(xs), _ptr(xl_out), _ptr(lens), len_mul, B, T, C,
        float(slope), int(bool(xs_final)), dtype, _stream()),
        flops=sum(2.0 * B * T * C * C * k * 6 for k in ks),
        nbytes=B * T * C * (2 + (4 if xs_final else 0) + (2 if xl_out is not None else 0)))


def respair(x_l, w1, b1, w2, b2, *, B, T, C, k, dil, slope, y=None, xs=None, accumulate=False, lens=None, len_mul=1, dtype=F16,
            xs_final=True):
    """One fused conv pair of ResBlock1 (csrc/respair.hip).  y given alone: mid pair, y = leaky_relu(x').  xs given: last
    pair of a ResBlock, xs (+)= x' and (when y is given too) y = leaky_relu(xs).  xs_final=False (with y): xs is read for the
    sum and not written back - nobody reads the stage's fp32 sum."""
    lib = _lib.load()
    d = _lib.RespairDesc()
    d.X, d.W1, d.W2, d.b1, d.b2 = _ptr(_req(x_l, _TORCH16[dtype], "x_l")), _ptr(w1), _ptr(w2), _ptr(_req(b1, torch.float32, "b1")), _ptr(_req(b2, torch.float32, "b2"))
    d.Y, d.XS, d.lens = _ptr(y), _ptr(xs), _ptr(lens)
    if xs is not None and xs.dtype != torch.float32:
        raise L2SError("xs must be fp32")
    if lens is not None and lens.dtype != torch.int32:
        raise L2SError("lens must be int32")
    d.len_mul, d.B, d.T, d.C, d.k, d.dil = len_mul, B, T, C, k, dil
    d.last = 0 if xs is None else (1 if xs_final else 2)
    d.accumulate, d.dtype, d.slope = int(bool(accumulate)), dtype, float(slope)
    kind = "last" if xs is not None else "mid"
    arrays = 2 * 2 + (0 if xs is None else (4 if accumulate else 0) + (4 if xs_final else 0) - (0 if y is not None else 2))
    key = f"l2s_respair<C{C},{kind}>"    # rocprofv3 name: respair_kernel<Elem.., C, KIND> (k is a runtime argument)
    if _profiler is not None and _profiler.detail:
        key += f" k{k} dil{dil}"
    _run(key, lambda: lib.l2s_respair(ctypes.byref(d), _stream()),
         flops=2.0 * B * T * C * C * k * 2, nbytes=float(B) * T * C * arrays + 2.0 * 2 * C * C * k, shape=f"M{B * T} k{k}")


def respair_variant(*, B, T, C, k, dil, slope=0.1, last=0, accumulate=False, lens=True, len_mul=1, dtype=F16):
    """Host-only: RM * 1000 + C of the kernel l2s_respair would run (192064 / 192128: csrc/respair.hip; 512064 / 256128 / 128256:
    csrc/respair_phase.hip), or its negative error code.  Needs no device and no tensors: the operands count as present and aligned."""
    d = _lib.RespairDesc()
    fake = 0x10000
    d.X = d.W1 = d.W2 = d.b1 = d.b2 = fake
    d.Y = fake if last != 1 else None
    d.XS = fake if last else None
    d.lens = fake if lens else None
    d.len_mul, d.B, d.T, d.C, d.k, d.dil = len_mul, B, T, C, k, dil
    d.last, d.accumulate, d.dtype, d.slope = last, int(bool(accumulate)), dtype, float(slope)
    return _lib.load().l2s_respair_variant(ctypes.byref(d))


def respair_final(xs_l, w1s, b1s, w2s, b2s, y, *, B, T, C, ks, dils, slope, lens=None, len_mul=1, dtype=F16):
    """The last conv pairs of a stage's ResBlocks in one launch (csrc/respair_phase.hip: respair_final_kernel):
    y = leaky_relu(sum_j (c2_j(leaky_relu(c1_j(x_l[j]))) + x_j)); the stage's fp32 sum stays in accumulators.  xs_l / w1s / b1s /
    w2s / b2s: per-ResBlock lists (n <= 3) of the operands l2s_respair takes; ks, dils: their kernel sizes and dilations."""
    lib = _lib.load()
    n = len(xs_l)
    if not (1 <= n <= 3 and len(w1s) == len(w2s) == len(b1s) == len(b2s) == len(ks) == len(dils) == n):
        raise L2SError("respair_final: 1..3 ResBlocks, one entry per list each")
    d = _lib.RespairFinalDesc()
    for j in range(n):
        d.X[j], d.W1[j], d.W2[j] = _ptr(_req(xs_l[j], _TORCH16[dtype], "x_l")), _ptr(w1s[j]), _ptr(w2s[j])
        d.b1[j], d.b2[j] = _ptr(_req(b1s[j], torch.float32, "b1")), _ptr(_req(b2s[j], torch.float32, "b2"))
        d.k[j], d.dil[j] = int(ks[j]), int(dils[j])
    if lens is not None and lens.dtype != torch.int32:
        raise L2SError("lens must be int32")
    d.Y, d.lens = _ptr(_req(y, _TORCH16[dtype], "y")), _ptr(lens)
    d.n, d.len_mul, d.B, d.T, d.C, d.dtype, d.slope = n, len_mul, B, T, C, dtype, float(slope)
    _run(f"l2s_respair_final<C{C}>", lambda: lib.l2s_respair_final(ctypes.byref(d), _stream()),
         flops=sum(2.0 * B * T * C * C * k * 2 for k in ks), nbytes=float(B) * T * C * 2 * (n + 1) + sum(2.0 * 2 * C * C * k for k in ks),
         shape=f"M{B * T} n{n}")


def preprocess_frames(frames, y, *, B, T, Hin, Win, crop=88, mean=0.421, std=0.165, dtype=F16):
    _run("l2s_preprocess_frames", lambda: _lib.load().l2s_preprocess_frames(_ptr(frames), _ptr(y), B, T, Hin, Win, crop, mean, std, dtype, _stream()))


def mel_spectrogram(wav, mel, basis, fb, fb_range, *, B, S, T_rows, n_samples=None, ldw=None, ldm=None, n_fft=640, hop=160, n_mels=80,
                    floor=1e-5):
    """Log-mel analysis in one launch (csrc/melspec.hip; audio.TacotronSTFT builds the tables): wav fp32 or int16 [B, S] ->
    mel fp32 [B, T_rows, n_mels], every clip analysed alone against n_samples[b] (int32 device tensor; None = S)."""
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    if n_samples is not None and n_samples.dtype != torch.int32:
        raise L2SError("n_samples must be int32")
    _req(wav, None, "wav"), _req(mel, torch.float32, "mel"), _req(basis, torch.float32, "basis"), _req(fb, torch.float32, "fb")
    _req(fb_range, torch.int32, "fb_range")
    frames = float(B) * T_rows
    _run("l2s_mel_spectrogram", lambda: _lib.load().l2s_mel_spectrogram(
        _ptr(wav), int(wav.dtype == torch.int16), ldw if ldw is not None else S, _ptr(n_samples), B, S, _ptr(basis), _ptr(fb),
        _ptr(fb_range), _ptr(mel), ldm if ldm is not None else n_mels, T_rows, n_fft, hop, n_mels, float(floor), _stream()),
        flops=2.0 * frames * n_fft * n_fft, nbytes=float(B) * S * wav.element_size() + 4.0 * frames * n_mels + 4.0 * n_fft * n_fft)


def stft_mel(wav, mel, basis, fb, fb_range, *, B, S, T_rows, n_fft, hop, pad, mag_eps=0.0, n_samples=None, ldw=None, ldm=None, n_mels=80,
             floor=1e-5):
    """mel_spectrogram with the frame placement (`pad` reflected samples on each side) and the magnitude's epsilon as arguments, at
    (n_fft, hop) = (1024, 256) or (640, 160): the HiFi-GAN analysis of the vocoder's loss (audio.MelSpectrogram builds the tables).
    Clip b has (n_b + 2 pad - n_fft) // hop + 1 rows (0 unless n_b > pad and a whole frame fits); the rest of its T_rows are zeros."""
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    if n_samples is not None and n_samples.dtype != torch.int32:
        raise L2SError("n_samples must be int32")
    _req(wav, None, "wav"), _req(mel, torch.float32, "mel"), _req(basis, torch.float32, "basis"), _req(fb, torch.float32, "fb")
    _req(fb_range, torch.int32, "fb_range")
    ldw = ldw if ldw is not None else S
    ldm = ldm if ldm is not None else n_mels
    if (B - 1) * ldw + S > _extent(wav) or ((B * T_rows - 1) * ldm + n_mels) > _extent(mel):
        raise L2SError("stft_mel: wav smaller than [B, ldw] or mel smaller than [B, T_rows, ldm]")
    if basis.numel() < n_fft * n_fft or fb.numel() < n_mels * (n_fft // 2 + 1) or fb_range.numel() < 2 * n_mels:
        raise L2SError("stft_mel: tables smaller than [n_fft, n_fft], [n_mels, n_fft/2 + 1], [n_mels, 2]")
    if n_samples is not None and n_samples.numel() < B:
        raise L2SError("stft_mel: n_samples shorter than B")
    frames = float(B) * T_rows
    _run("l2s_stft_mel", lambda: _lib.load().l2s_stft_mel(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, _ptr(basis), _ptr(fb), _ptr(fb_range), _ptr(mel), ldm,
        T_rows, n_fft, hop, n_mels, pad, float(mag_eps), float(floor), _stream()),
        flops=2.0 * frames * n_fft * n_fft, nbytes=float(B) * S * wav.element_size() + 4.0 * frames * n_mels + 4.0 * n_fft * n_fft)


def logfbank(wav, out, basis, fb, fb_range, *, B, S, T_rows, stack=4, normalize=True, n_samples=None, n_rows=None, ldw=None, ldo=None):
    """Log filterbank rows for AV-HuBERT's audio sub-model in one launch (csrc/logfbank.hip; audio.LogFbank builds the tables):
    wav int16 or fp32 at int16 scale [B, S] -> out fp32 / f16 / bf16 [B, T_rows, 26 * stack] with row stride ldo, every clip
    analysed alone against n_samples[b] (int32 device tensor; None = S).  Clip b's rows at or past min(its own row count,
    n_rows[b]) are zeros (n_rows: int32 device tensor, the video's frame counts; None = the audio's own)."""
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    for name, t in (("n_samples", n_samples), ("n_rows", n_rows)):
        if t is not None and (_req(t, None, name).dtype != torch.int32 or t.numel() < B):
            raise L2SError(f"logfbank: {name} must be int32 [B]")
    _req(wav, None, "wav"), _req(out, None, "out"), _req(basis, torch.float32, "basis"), _req(fb, torch.float32, "fb")
    _req(fb_range, torch.int32, "fb_range")
    C = 26 * stack
    ldw = ldw if ldw is not None else S
    ldo = ldo if ldo is not None else C
    if B > 0 and T_rows > 0 and ((B - 1) * ldw + S > _extent(wav) or ((B * T_rows - 1) * ldo + C) > _extent(out)):
        raise L2SError("logfbank: wav smaller than [B, ldw] or out smaller than [B, T_rows, ldo]")
    if basis.numel() < 400 * 512 or fb.numel() < 26 * 257 or fb_range.numel() < 2 * 26:
        raise L2SError("logfbank: tables smaller than [400, 512], [26, 257], [26, 2]")
    frames = float(B) * T_rows * stack
    _run("l2s_logfbank", lambda: _lib.load().l2s_logfbank(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, _ptr(basis), _ptr(fb), _ptr(fb_range), _ptr(n_rows),
        _ptr(out), dtype_code(out.dtype), ldo, T_rows, stack, int(bool(normalize)), _stream()),
        flops=2.0 * frames * 400 * 512, nbytes=float(B) * S * wav.element_size() + float(out.element_size()) * B * T_rows * C + 4.0 * 400 * 512)


def unit_ce(logits, target, nll, smooth, n_correct, n_tok, *, B, T2, V, ldl=None, ldt=None, lens=None, len_mul=2, pad_idx=1,
            ignore_prefix=0):
    """Label-smoothed cross-entropy sums and accuracy counts per clip in one pass over fp32 logits [B*T2, ldl] (csrc/criterion.hip):
    target int32 [B, ldt]; outputs nll / smooth fp32 [B], n_correct / n_tok int32 [B].  A row counts when t < min(T2, ldt),
    target != pad_idx and t < lens[b]*len_mul."""
    _req(logits, torch.float32, "logits"), _req(target, torch.int32, "target"), _req(nll, torch.float32, "nll")
    _req(smooth, torch.float32, "smooth"), _req(n_correct, torch.int32, "n_correct"), _req(n_tok, torch.int32, "n_tok")
    if lens is not None:
        _req(lens, torch.int32, "lens")
    ldl = ldl if ldl is not None else V
    ldt = ldt if ldt is not None else target.stride(0)
    if min(nll.numel(), smooth.numel(), n_correct.numel(), n_tok.numel()) < B or (lens is not None and lens.numel() < B):
        raise L2SError("unit_ce: per-clip tensors shorter than B")
    if (B * T2 - 1) * ldl + V > _extent(logits):
        raise L2SError("unit_ce: logits smaller than B*T2 rows of ldl")
    if (B - 1) * ldt + min(T2, ldt) > _extent(target):
        raise L2SError("unit_ce: target smaller than [B, ldt]")
    _run("l2s_unit_ce", lambda: _lib.load().l2s_unit_ce(
        _ptr(logits), ldl, _ptr(target), ldt, _ptr(lens), len_mul, B, T2, V, pad_idx, ignore_prefix, _ptr(nll), _ptr(smooth),
        _ptr(n_correct), _ptr(n_tok), _stream()), nbytes=4.0 * B * T2 * V)


def mel_l1_sc(pred, targ, l1, sq, tsq, n_rows, *, B, Tm_pred, Tm_targ, crop_len, lens=None, len_mul=4, n_mels=80):
    """Masked L1 / spectral-convergence sums per clip (csrc/criterion.hip): pred fp32 [B, Tm_pred, n_mels], targ fp32
    [B, Tm_targ, n_mels], both dense; over rows t < min(lens[b]*len_mul, crop_len, Tm_pred, Tm_targ): l1 = sum|p-t|,
    sq = sum (p-t)^2, tsq = sum t^2 (fp32 [B]) and n_rows int32 [B]."""
    _req(pred, torch.float32, "pred"), _req(targ, torch.float32, "targ")
    for t, n in ((l1, "l1"), (sq, "sq"), (tsq, "tsq")):
        _req(t, torch.float32, n)
    _req(n_rows, torch.int32, "n_rows")
    if lens is not None:
        _req(lens, torch.int32, "lens")
    if not pred.is_contiguous() or not targ.is_contiguous():
        raise L2SError("mel_l1_sc: pred and targ must be dense")
    if pred.numel() < B * Tm_pred * n_mels or targ.numel() < B * Tm_targ * n_mels:
        raise L2SError("mel_l1_sc: pred / targ smaller than [B, Tm, n_mels]")
    if min(l1.numel(), sq.numel(), tsq.numel(), n_rows.numel()) < B or (lens is not None and lens.numel() < B):
        raise L2SError("mel_l1_sc: per-clip tensors shorter than B")
    _run("l2s_mel_l1_sc", lambda: _lib.load().l2s_mel_l1_sc(
        _ptr(pred), Tm_pred, _ptr(targ), Tm_targ, _ptr(lens), len_mul, B, n_mels, crop_len, _ptr(l1), _ptr(sq), _ptr(tsq),
        _ptr(n_rows), _stream()), nbytes=8.0 * B * min(Tm_pred, Tm_targ) * n_mels)


def ctc_loss_workspace_bytes(B, L, S_max):
    n = _lib.load().l2s_ctc_loss_workspace(B, L, S_max)
    if n == 0:
        raise L2SError(f"l2s_ctc_loss_workspace: unsupported size (B={B}, L={L}, S_max={S_max}; at most 511 labels per clip)")
    return n


def ctc_loss(logits, targets, tgt_lens, tgt_offs, workspace, nll, *, B, L, V, S_max, blank=0, ldl=None, lens=None, len_mul=2):
    """torch.nn.CTCLoss(blank, zero_infinity=True) forward per clip from fp32 logits [B*L, ldl] (csrc/criterion.hip): targets
    int32 concatenated, clip b's labels at tgt_offs[b] .. + tgt_lens[b] (int32 [B] each, <= S_max); clip b uses
    min(lens[b]*len_mul, L) frames; nll fp32 [B].  workspace: ctc_loss_workspace_bytes(B, L, S_max) bytes."""
    _req(logits, torch.float32, "logits"), _req(targets, torch.int32, "targets"), _req(tgt_lens, torch.int32, "tgt_lens")
    _req(tgt_offs, torch.int32, "tgt_offs"), _req(nll, torch.float32, "nll")
    if lens is not None:
        _req(lens, torch.int32, "lens")
    ldl = ldl if ldl is not None else V
    if (B * L - 1) * ldl + V > _extent(logits):
        raise L2SError("ctc_loss: logits smaller than B*L rows of ldl")
    if min(tgt_lens.numel(), tgt_offs.numel(), nll.numel()) < B or (lens is not None and lens.numel() < B):
        raise L2SError("ctc_loss: per-clip tensors shorter than B")
    _run("l2s_ctc_loss", lambda: _lib.load().l2s_ctc_loss(
        _ptr(logits), ldl, _ptr(lens), len_mul, B, L, V, blank, _ptr(targets) if targets.numel() else None, _ptr(tgt_lens),
        _ptr(tgt_offs), S_max, _ptr(workspace), workspace.numel() * workspace.element_size(), _ptr(nll), _stream()),
        nbytes=4.0 * B * L * V)


def wave_stem_frames(n):
    """Frames of HuBERT's first conv layer (k = 10, stride 5, no padding) for n samples."""
    return (n - 10) // 5 + 1 if n >= 10 else 0


def wave_stem_workspace_bytes(B, C):
    n = _lib.load().l2s_wave_stem_workspace(B, C)
    if n == 0:
        raise L2SError(f"l2s_wave_stem_workspace: bad shape (B={B}, C={C})")
    return n


def wave_stem(wav, w, gamma, beta, workspace, out, *, B, S, T_rows, C=512, n_samples=None, ldw=None, ldo=None, eps=1e-5, dtype=F16):
    """HuBERT's waveform stem in one call (csrc/wavestem.hip): Conv1d(1 -> C, 10, stride 5), GroupNorm(C, C) over each clip's own
    frames, GELU.  wav fp32 or int16 [B, S]; w fp32 [C, 10]; out [B*T_rows, C] of `dtype` (rows past a clip's frames are
    zeros); workspace: wave_stem_workspace_bytes(B, C) bytes."""
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    if n_samples is not None and n_samples.dtype != torch.int32:
        raise L2SError("n_samples must be int32")
    _req(wav, None, "wav"), _req(w, torch.float32, "w"), _req(gamma, torch.float32, "gamma"), _req(beta, torch.float32, "beta")
    _req(out, _TORCH16[dtype], "out")
    ldw = ldw if ldw is not None else S
    ldo = ldo if ldo is not None else C
    if w.numel() < C * 10 or not w.is_contiguous() or gamma.numel() < C or beta.numel() < C:
        raise L2SError("wave_stem: w [C, 10], gamma / beta [C]")
    if (B - 1) * ldw + S > _extent(wav) or (n_samples is not None and n_samples.numel() < B):
        raise L2SError("wave_stem: wav smaller than [B, S] of ldw / n_samples shorter than B")
    if (B * T_rows - 1) * ldo + C > _extent(out):
        raise L2SError("wave_stem: out smaller than B*T_rows rows of ldo")
    rows = float(B) * T_rows
    _run("l2s_wave_stem", lambda: _lib.load().l2s_wave_stem(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, _ptr(w), _ptr(gamma), _ptr(beta), float(eps), _ptr(out),
        ldo, T_rows, C, _ptr(workspace), workspace.numel() * workspace.element_size(), dtype, _stream()),
        flops=2.0 * rows * C * 10, nbytes=3.0 * B * S * wav.element_size() + rows * C * out.element_size())


def kmeans_assign(x, centers, cnorm, ids, *, B, T, D, K, ldx=None, lens=None, len_mul=1, best2=None):
    """Nearest-centroid labels in one launch (csrc/kmeans.hip): ids int32 [B*T] = argmin_k (cnorm[k] - 2 x . centers[k]) over
    fp32 rows x [B*T, ldx], lowest index on ties, -1 past lens[b]*len_mul; best2 (optional) fp32 [B*T, 2] = the two smallest."""
    _req(x, torch.float32, "x"), _req(centers, torch.float32, "centers"), _req(cnorm, torch.float32, "cnorm")
    _req(ids, torch.int32, "ids")
    if lens is not None:
        _req(lens, torch.int32, "lens")
    if best2 is not None:
        _req(best2, torch.float32, "best2")
    ldx = ldx if ldx is not None else D
    if (B * T - 1) * ldx + D > _extent(x):
        raise L2SError("kmeans_assign: x smaller than B*T rows of ldx")
    if not centers.is_contiguous() or centers.numel() < K * D or cnorm.numel() < K:
        raise L2SError("kmeans_assign: centers [K, D] dense, cnorm [K]")
    if ids.numel() < B * T or not ids.is_contiguous() or (lens is not None and lens.numel() < B):
        raise L2SError("kmeans_assign: ids shorter than B*T / lens shorter than B")
    if best2 is not None and (best2.numel() < 2 * B * T or not best2.is_contiguous()):
        raise L2SError("kmeans_assign: best2 [B*T, 2] dense")
    _run("l2s_kmeans_assign", lambda: _lib.load().l2s_kmeans_assign(
        _ptr(x), ldx, _ptr(centers), _ptr(cnorm), _ptr(lens), len_mul, B, T, D, K, _ptr(ids), _ptr(best2), _stream()),
        flops=2.0 * B * T * K * D, nbytes=4.0 * B * T * D + 4.0 * K * D + 4.0 * B * T)


def _ws_bytes(t):
    return t.numel() * t.element_size()


def _km_batch(name, x, rows, M, D, ldx):
    """Shared checks of the k-means fit entries' batch arguments; returns (ldx, N)."""
    _req(x, torch.float32, "x")
    if x.dim() != 2:
        raise L2SError(f"{name}: x [N, ldx]")
    ldx = ldx if ldx is not None else (x.stride(0) if x.shape[0] > 1 else max(x.shape[1], D))
    N = x.shape[0]
    if x.shape[1] < D or (N - 1) * ldx + D > _extent(x):
        raise L2SError(f"{name}: x smaller than N rows of ldx")
    if rows is not None:
        _req(rows, torch.int32, "rows")
        if rows.numel() < M or not rows.is_contiguous():
            raise L2SError(f"{name}: rows shorter than M")
    elif N < M:
        raise L2SError(f"{name}: x has fewer than M rows")
    return ldx, N


def kmeans_nearest_workspace_bytes(M):
    n = _lib.load().l2s_kmeans_nearest_workspace(M)
    if n == 0:
        raise L2SError(f"l2s_kmeans_nearest_workspace: unsupported size (M={M})")
    return n


def kmeans_update_workspace_bytes(M, K):
    n = _lib.load().l2s_kmeans_update_workspace(M, K)
    if n == 0:
        raise L2SError(f"l2s_kmeans_update_workspace: unsupported size (M={M}, K={K}; M <= 2^24, 2 <= K <= 1024)")
    return n


def kmeans_pp_workspace_bytes(m):
    n = _lib.load().l2s_kmeans_pp_workspace(m)
    if n == 0:
        raise L2SError(f"l2s_kmeans_pp_workspace: unsupported size (m={m})")
    return n


def kmeans_nearest(x, centers, cnorm, *, M, D, K, rows=None, ids=None, dmin=None, inertia=None, workspace=None, ldx=None):
    """One mini-batch assignment (csrc/kmeans_fit.hip): over the batch x[rows] (or x[:M]) ids int32 [M] = the nearest centre
    (lowest index on a tie), dmin fp32 [M] = max(0, |x|^2 + cnorm - 2 x.c) there, inertia float64 [1] = their sum in a fixed
    order.  workspace: kmeans_nearest_workspace_bytes(M) bytes, needed with inertia."""
    ldx, N = _km_batch("kmeans_nearest", x, rows, M, D, ldx)
    _req(centers, torch.float32, "centers"), _req(cnorm, torch.float32, "cnorm")
    if not centers.is_contiguous() or centers.numel() < K * D or cnorm.numel() < K:
        raise L2SError("kmeans_nearest: centers [K, D] dense, cnorm [K]")
    for t, dt, nm, n in ((ids, torch.int32, "ids", M), (dmin, torch.float32, "dmin", M), (inertia, torch.float64, "inertia", 1)):
        if t is not None:
            _req(t, dt, nm)
            if t.numel() < n or not t.is_contiguous():
                raise L2SError(f"kmeans_nearest: {nm} shorter than {n}")
    if workspace is not None:
        _req(workspace, None, "workspace")
    _run("l2s_kmeans_nearest", lambda: _lib.load().l2s_kmeans_nearest(
        _ptr(x), ldx, N, _ptr(rows), M, _ptr(centers), _ptr(cnorm), D, K, _ptr(ids), _ptr(dmin), _ptr(inertia), _ptr(workspace),
        _ws_bytes(workspace) if workspace is not None else 0, _stream()),
        flops=2.0 * M * K * D, nbytes=4.0 * M * D + 4.0 * K * D + 8.0 * M)


def kmeans_update(x, ids, centers, counts, centers_out, counts_out, cnorm_out, workspace, *, M, D, K, rows=None, ldx=None):
    """The centre update of a mini-batch step (csrc/kmeans_fit.hip): c <- (c w + sum of the batch rows labelled k) / (w + n),
    w <- w + n for every centre with members, the others copied; cnorm_out = |c|^2 of the result.  centers_out / counts_out may
    be centers / counts.  workspace: kmeans_update_workspace_bytes(M, K) bytes."""
    ldx, N = _km_batch("kmeans_update", x, rows, M, D, ldx)
    _req(ids, torch.int32, "ids"), _req(workspace, None, "workspace")
    for t, nm, n in ((centers, "centers", K * D), (counts, "counts", K), (centers_out, "centers_out", K * D), (counts_out, "counts_out", K),
                     (cnorm_out, "cnorm_out", K)):
        _req(t, torch.float32, nm)
        if t.numel() < n or not t.is_contiguous():
            raise L2SError(f"kmeans_update: {nm} dense with {n} elements")
    if ids.numel() < M or not ids.is_contiguous():
        raise L2SError("kmeans_update: ids shorter than M")
    _run("l2s_kmeans_update", lambda: _lib.load().l2s_kmeans_update(
        _ptr(x), ldx, N, _ptr(rows), M, _ptr(ids), _ptr(centers), _ptr(counts), D, K, _ptr(centers_out), _ptr(counts_out),
        _ptr(cnorm_out), _ptr(workspace), _ws_bytes(workspace), _stream()), flops=1.0 * M * D, nbytes=4.0 * M * D + 8.0 * K * D + 8.0 * M)


def kmeans_pp_pot(x, cand, workspace, *, m, D, t, rows=None, closest=None, select=None, pot=None, closest_out=None, chosen=None,
                  ldx=None):
    """k-means++ potentials (csrc/kmeans_fit.hip): cand int32 [t <= 16] positions in the subset x[rows] (or x[:m]).  Without
    closest_out: pot float64 [t] = sum_i min(closest[i], |x_i - x_cand|^2) (closest = None: +inf).  With closest_out: the new
    closest of cand[0] (t = 1) or of cand[argmin select] - then chosen int32 [1] = its position - and pot [1] = its sum.
    workspace: kmeans_pp_workspace_bytes(m) bytes."""
    ldx, N = _km_batch("kmeans_pp_pot", x, rows, m, D, ldx)
    _req(cand, torch.int32, "cand"), _req(workspace, None, "workspace")
    n_pot = 1 if closest_out is not None else t
    for a, dt, nm, n in ((closest, torch.float32, "closest", m), (select, torch.float64, "select", t), (pot, torch.float64, "pot", n_pot),
                         (closest_out, torch.float32, "closest_out", m), (chosen, torch.int32, "chosen", 1)):
        if a is not None:
            _req(a, dt, nm)
            if a.numel() < n or not a.is_contiguous():
                raise L2SError(f"kmeans_pp_pot: {nm} shorter than {n}")
    if cand.numel() < t or not cand.is_contiguous():
        raise L2SError("kmeans_pp_pot: cand shorter than t")
    _run("l2s_kmeans_pp_pot", lambda: _lib.load().l2s_kmeans_pp_pot(
        _ptr(x), ldx, N, _ptr(rows), m, D, _ptr(cand), t, _ptr(closest), _ptr(select), _ptr(pot), _ptr(closest_out), _ptr(chosen),
        _ptr(workspace), _ws_bytes(workspace), _stream()), flops=3.0 * m * D * n_pot, nbytes=4.0 * m * D + 8.0 * m)


def kmeans_pp_pick(closest, u, idx, *, m, t, scale=None, total=None):
    """searchsorted(cumsum(closest[:m]) in float64, u * scale, side="left") clipped to m - 1 (csrc/kmeans_fit.hip): u float64 [t <= 16]
    and scale float64 [1] (None: 1) on the device, idx int32 [t], total float64 [1] = the sum of closest."""
    _req(closest, torch.float32, "closest"), _req(u, torch.float64, "u"), _req(idx, torch.int32, "idx")
    for a, nm in ((scale, "scale"), (total, "total")):
        if a is not None:
            _req(a, torch.float64, nm)
            if a.numel() < 1:
                raise L2SError(f"kmeans_pp_pick: {nm} is empty")
    if closest.numel() < m or not closest.is_contiguous() or u.numel() < t or idx.numel() < t:
        raise L2SError("kmeans_pp_pick: closest shorter than m / u, idx shorter than t")
    _run("l2s_kmeans_pp_pick", lambda: _lib.load().l2s_kmeans_pp_pick(
        _ptr(closest), m, _ptr(u) if t else None, t, _ptr(scale), _ptr(idx), _ptr(total), _stream()), nbytes=4.0 * m * (1 + t))


STOI_MAX_SAMPLES = 419840   # csrc/stoi.hip: the longest 16 kHz clip (2 048 analysis frames at 10 kHz); longer is L2S_EUNSUPPORTED


def stoi_len10k(n):
    """Samples at 10 kHz of n samples at 16 kHz: ceil(5 n / 8)."""
    return (5 * n + 7) // 8


def stoi_frames_of(n10k):
    """Analysis frames (256 samples, hop 128, starts i < len - 256) of a 10 kHz signal."""
    return (n10k - 257) // 128 + 1 if n10k > 256 else 0


def _stoi_common(name, n_samples, B, S):
    if n_samples is not None:
        _req(n_samples, torch.int32, "n_samples")
        if n_samples.numel() < B:
            raise L2SError(f"{name}: n_samples shorter than B")


def stoi_resample(wav, taps, out, *, B, S, R, n_samples=None, ldw=None, ldo=None):
    """STOI step 1 (csrc/stoi.hip): wav fp32 or int16 [B, S] at 16 kHz -> out fp32 rows of R >= ceil(5 S / 8) samples at 10 kHz
    (row stride ldo), the 581-tap Kaiser polyphase FIR with taps fp32 [5, 117]; zeros past each clip's own ceil(5 n_b / 8)."""
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    _req(wav, None, "wav"), _req(taps, torch.float32, "taps"), _req(out, torch.float32, "out")
    _stoi_common("stoi_resample", n_samples, B, S)
    ldw = ldw if ldw is not None else S
    ldo = ldo if ldo is not None else R
    if (B - 1) * ldw + S > _extent(wav) or (B - 1) * ldo + R > _extent(out) or taps.numel() < 5 * 117 or not taps.is_contiguous():
        raise L2SError("stoi_resample: wav smaller than [B, S] of ldw, out smaller than [B, R] of ldo, or taps not [5, 117]")
    _run("l2s_stoi_resample", lambda: _lib.load().l2s_stoi_resample(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, _ptr(taps), _ptr(out), ldo, R, _stream()),
        flops=2.0 * 117 * B * R, nbytes=float(B) * S * wav.element_size() + 4.0 * B * R)


def stoi_frames(x, window, kept, n_kept, *, B, S, n_samples=None, ldx=None, ldk=None):
    """STOI step 2 (csrc/stoi.hip): the frames of the resampled clean signal x (fp32 rows, stride ldx) within 40 dB of the loudest:
    kept int32 [B, ldk] ascending indices, -1 past n_kept int32 [B]."""
    _req(x, torch.float32, "x"), _req(window, torch.float32, "window"), _req(kept, torch.int32, "kept"), _req(n_kept, torch.int32, "n_kept")
    _stoi_common("stoi_frames", n_samples, B, S)
    ldx = ldx if ldx is not None else x.stride(0)
    ldk = ldk if ldk is not None else kept.stride(0)
    if (B - 1) * ldx + stoi_len10k(S) > _extent(x) or (B - 1) * ldk + ldk > _extent(kept) or n_kept.numel() < B or window.numel() < 256:
        raise L2SError("stoi_frames: x smaller than [B, ceil(5 S / 8)] of ldx, kept smaller than [B, ldk], n_kept shorter than B or window < 256")
    _run("l2s_stoi_frames", lambda: _lib.load().l2s_stoi_frames(
        _ptr(x), ldx, _ptr(n_samples), B, S, _ptr(window), _ptr(kept), ldk, _ptr(n_kept), _stream()), nbytes=4.0 * B * stoi_len10k(S))


def stoi_bands(x, y, kept, n_kept, window, basis, band_edges, bands, *, B, S, ldf, n_samples=None, ldx=None, ldk=None):
    """STOI steps 2-3 (csrc/stoi.hip): third-octave band magnitudes bands fp32 [B, 2, 15, ldf] of the kept frames of the resampled
    clean (x) and processed (y) signals, overlap-added in LDS; basis fp32 [256, 512], band_edges int32 [16]."""
    for t, n in ((x, "x"), (y, "y"), (window, "window"), (basis, "basis"), (bands, "bands")):
        _req(t, torch.float32, n)
    _req(kept, torch.int32, "kept"), _req(n_kept, torch.int32, "n_kept"), _req(band_edges, torch.int32, "band_edges")
    _stoi_common("stoi_bands", n_samples, B, S)
    ldx = ldx if ldx is not None else x.stride(0)
    ldk = ldk if ldk is not None else kept.stride(0)
    if x.stride(0) != y.stride(0) and B > 1:
        raise L2SError("stoi_bands: x and y need the same row stride")
    if (B - 1) * ldx + stoi_len10k(S) > min(_extent(x), _extent(y)) or (B - 1) * ldk + ldk > _extent(kept) or n_kept.numel() < B:
        raise L2SError("stoi_bands: x / y smaller than [B, ceil(5 S / 8)] of ldx, kept smaller than [B, ldk] or n_kept shorter than B")
    if window.numel() < 256 or basis.numel() < 256 * 512 or not basis.is_contiguous() or band_edges.numel() < 16:
        raise L2SError("stoi_bands: tables smaller than [256], [256, 512], [16]")
    if not bands.is_contiguous() or bands.numel() < B * 2 * 15 * ldf:
        raise L2SError("stoi_bands: bands must be dense [B, 2, 15, ldf]")
    _run("l2s_stoi_bands", lambda: _lib.load().l2s_stoi_bands(
        _ptr(x), _ptr(y), ldx, _ptr(n_samples), B, S, _ptr(kept), ldk, _ptr(n_kept), _ptr(window), _ptr(basis), _ptr(band_edges),
        _ptr(bands), ldf, _stream()), flops=2.0 * 2 * B * ldf * 256 * 512, nbytes=8.0 * B * stoi_len10k(S) + 4.0 * 256 * 512)


def stoi_scores(bands, n_kept, seg, stoi, estoi, n_segments, *, B, ldf, lds=None):
    """STOI steps 4-6 (csrc/stoi.hip): per-clip stoi / estoi fp32 [B] and n_segments int32 [B] from bands fp32 [B, 2, 15, ldf];
    seg float64 [B, 2, lds] is the workspace that ends holding every segment's two terms."""
    _req(bands, torch.float32, "bands"), _req(n_kept, torch.int32, "n_kept"), _req(seg, torch.float64, "seg")
    _req(stoi, torch.float32, "stoi"), _req(estoi, torch.float32, "estoi"), _req(n_segments, torch.int32, "n_segments")
    lds = lds if lds is not None else seg.shape[-1]
    if not bands.is_contiguous() or bands.numel() < B * 2 * 15 * ldf or not seg.is_contiguous() or seg.numel() < B * 2 * lds:
        raise L2SError("stoi_scores: bands must be dense [B, 2, 15, ldf] and seg dense [B, 2, lds]")
    if min(n_kept.numel(), stoi.numel(), estoi.numel(), n_segments.numel()) < B:
        raise L2SError("stoi_scores: per-clip tensors shorter than B")
    _run("l2s_stoi_scores", lambda: _lib.load().l2s_stoi_scores(
        _ptr(bands), ldf, _ptr(n_kept), B, _ptr(seg), lds, _ptr(stoi), _ptr(estoi), _ptr(n_segments), _stream()),
        nbytes=4.0 * B * 2 * 15 * ldf)


def _wav_common(name, wav, n_samples, B, S, ldw):
    if wav.dtype not in (torch.float32, torch.int16):
        raise L2SError(f"wav: expected float32 or int16, got {wav.dtype}")
    _req(wav, None, "wav")
    if n_samples is not None:
        _req(n_samples, torch.int32, "n_samples")
        if n_samples.numel() < B:
            raise L2SError(f"{name}: n_samples shorter than B")
    if (B - 1) * ldw + S > _extent(wav):
        raise L2SError(f"{name}: wav smaller than [B, S] of ldw")


def wav_gain(wav, gain, *, B, S, n_samples=None, ldw=None, target_dbfs=-30.0):
    """Per-clip volume factor of the speaker encoder (csrc/spkemb.hip): gain fp32 [B] = 10^(change/20) where
    change = target_dbfs - 10 log10(mean(wav^2)) > 0, else 1 (increase only); wav fp32 or int16 [B, S], n_samples int32 [B]."""
    ldw = ldw if ldw is not None else S
    _wav_common("wav_gain", wav, n_samples, B, S, ldw)
    _req(gain, torch.float32, "gain")
    if gain.numel() < B:
        raise L2SError("wav_gain: gain shorter than B")
    _run("l2s_wav_gain", lambda: _lib.load().l2s_wav_gain(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, float(target_dbfs), _ptr(gain), _stream()),
        nbytes=float(B) * S * wav.element_size())


def stft_mel_power(wav, mel, basis, fb, fb_range, *, B, S, T_rows, n_samples=None, n_valid=None, scale=None, ldw=None, ldm=None,
                   n_fft=400, hop=160, n_mels=40, pad=200):
    """40-band power mel of 400-sample frames (csrc/spkemb.hip; speaker_encoder.PowerMel builds the tables): wav fp32 or int16
    [B, S] -> mel fp32 [B, T_rows, n_mels], linear power.  n_samples: int32 [B] analysis lengths (frame count and reflection; may
    exceed S), n_valid: int32 [B] real samples (zeros from there on, never read), scale: fp32 [B] per-clip factor."""
    ldw = ldw if ldw is not None else S
    ldm = ldm if ldm is not None else n_mels
    _wav_common("stft_mel_power", wav, n_samples, B, S, ldw)
    _req(mel, torch.float32, "mel"), _req(basis, torch.float32, "basis"), _req(fb, torch.float32, "fb"), _req(fb_range, torch.int32, "fb_range")
    if n_valid is not None:
        _req(n_valid, torch.int32, "n_valid")
    if scale is not None:
        _req(scale, torch.float32, "scale")
    if any(t is not None and t.numel() < B for t in (n_valid, scale)):
        raise L2SError("stft_mel_power: n_valid / scale shorter than B")
    if ((B * T_rows - 1) * ldm + n_mels) > _extent(mel):
        raise L2SError("stft_mel_power: mel smaller than [B, T_rows, ldm]")
    if basis.numel() < n_fft * 448 or not basis.is_contiguous() or fb.numel() < n_mels * (n_fft // 2 + 1) or fb_range.numel() < 2 * n_mels:
        raise L2SError("stft_mel_power: tables smaller than [n_fft, 448], [n_mels, n_fft/2 + 1], [n_mels, 2]")
    frames = float(B) * T_rows
    _run("l2s_stft_mel_power", lambda: _lib.load().l2s_stft_mel_power(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), _ptr(n_valid), _ptr(scale), B, S, _ptr(basis), _ptr(fb),
        _ptr(fb_range), _ptr(mel), ldm, T_rows, n_fft, hop, n_mels, pad, _stream()),
        flops=2.0 * frames * n_fft * 448, nbytes=float(B) * S * wav.element_size() + 4.0 * frames * n_mels + 4.0 * n_fft * 448)


def lstm_layer(xproj, row_off, w_hh_p, *, S, T, n_rows=None, ldx=None, hidden=256, h_seq=None, h_last=None):
    """One LSTM layer's recurrence (csrc/lstm.hip): xproj fp32 [n_rows, ldx] = x W_ih^T + b with gate-interleaved columns 4 u + g,
    row_off int32 [S] (sequence s reads rows row_off[s] + t), w_hh_p fp32 [256, 256, 4] (speaker_encoder.pack_lstm_layer);
    h_seq fp32 [S, T, 256] and / or h_last fp32 [S, 256]."""
    _req(xproj, torch.float32, "xproj"), _req(row_off, torch.int32, "row_off"), _req(w_hh_p, torch.float32, "w_hh_p")
    if xproj.dim() != 2:
        raise L2SError("lstm_layer: xproj must be [n_rows, ldx]")
    n_rows = n_rows if n_rows is not None else xproj.shape[0]
    ldx = ldx if ldx is not None else xproj.stride(0)
    if (n_rows - 1) * ldx + 4 * hidden > _extent(xproj) or row_off.numel() < S or not row_off.is_contiguous():
        raise L2SError("lstm_layer: xproj smaller than [n_rows, 4 hidden] of ldx or row_off shorter than S")
    if not w_hh_p.is_contiguous() or w_hh_p.numel() < 4 * hidden * hidden:
        raise L2SError("lstm_layer: w_hh_p must be dense [hidden, hidden, 4]")
    if h_seq is None and h_last is None:
        raise L2SError("lstm_layer: h_seq or h_last is needed")
    if h_seq is not None:
        _req(h_seq, torch.float32, "h_seq")
        if not h_seq.is_contiguous() or h_seq.numel() < S * T * hidden:
            raise L2SError("lstm_layer: h_seq must be dense [S, T, hidden]")
    if h_last is not None:
        _req(h_last, torch.float32, "h_last")
        if not h_last.is_contiguous() or h_last.numel() < S * hidden:
            raise L2SError("lstm_layer: h_last must be dense [S, hidden]")
    _run("l2s_lstm_layer", lambda: _lib.load().l2s_lstm_layer(
        _ptr(xproj), ldx, n_rows, _ptr(row_off), _ptr(w_hh_p), S, T, hidden, _ptr(h_seq), _ptr(h_last), _stream()),
        flops=2.0 * S * T * hidden * 4 * hidden, nbytes=4.0 * S * T * (4 * hidden + (hidden if h_seq is not None else 0)),
        shape=f"S{S} T{T}")


def spk_embed_head(h_last, first, count, w_t, bias, out, *, B, n_rows=None, hidden=256):
    """The speaker encoder's head (csrc/spkemb.hip): per clip b over h_last rows [first[b], first[b] + count[b]): relu(W h + bias),
    / (norm + 1e-5), mean in index order, / norm -> out fp32 [B, 256].  w_t fp32 [256, 256] = linear.weight transposed."""
    for t, n in ((h_last, "h_last"), (w_t, "w_t"), (bias, "bias"), (out, "out")):
        _req(t, torch.float32, n)
    _req(first, torch.int32, "first"), _req(count, torch.int32, "count")
    n_rows = n_rows if n_rows is not None else h_last.shape[0]
    if not h_last.is_contiguous() or h_last.numel() < n_rows * hidden or not w_t.is_contiguous() or w_t.numel() < hidden * hidden:
        raise L2SError("spk_embed_head: h_last must be dense [n_rows, hidden] and w_t dense [hidden, hidden]")
    if bias.numel() < hidden or min(first.numel(), count.numel()) < B or not out.is_contiguous() or out.numel() < B * hidden:
        raise L2SError("spk_embed_head: bias [hidden], first / count [B], out dense [B, hidden]")
    _run("l2s_spk_embed_head", lambda: _lib.load().l2s_spk_embed_head(
        _ptr(h_last), n_rows, _ptr(first), _ptr(count), _ptr(w_t), _ptr(bias), B, hidden, _ptr(out), _stream()),
        flops=2.0 * n_rows * hidden * hidden, nbytes=4.0 * (n_rows + B + hidden) * hidden)


def mouth_transforms(landmarks, first, count, mean_face, stable_ids, inv, origin, *, B, window_margin=12, std_h=256, std_w=256,
                     crop_h=96, crop_w=96, start_idx=48, stop_idx=68):
    """Per-frame similarity transforms of the mouth cropper (csrc/mouthroi.hip): landmarks fp64 [N, L, 2], clip b = rows
    [first[b], first[b] + count[b]) (int32 [B]), mean_face fp64 [L, 2], stable_ids int32 [n_stable] -> inv fp64 [N, 6] (the 2 x 3
    inverse map) and origin int32 [N, 2] (x0, y0 of the crop window in the std_h x std_w aligned image)."""
    _req(landmarks, torch.float64, "landmarks"), _req(mean_face, torch.float64, "mean_face"), _req(inv, torch.float64, "inv")
    for t, n in ((first, "first"), (count, "count"), (stable_ids, "stable_ids"), (origin, "origin")):
        _req(t, torch.int32, n)
    if landmarks.dim() != 3 or landmarks.shape[2] != 2 or not landmarks.is_contiguous():
        raise L2SError("mouth_transforms: landmarks must be dense [N, L, 2]")
    N, L = landmarks.shape[0], landmarks.shape[1]
    if not mean_face.is_contiguous() or tuple(mean_face.shape) != (L, 2):
        raise L2SError("mouth_transforms: mean_face must be dense [L, 2]")
    if min(first.numel(), count.numel()) < B or not inv.is_contiguous() or inv.numel() < 6 * N or not origin.is_contiguous() or origin.numel() < 2 * N:
        raise L2SError("mouth_transforms: first / count [B], inv dense [N, 6], origin dense [N, 2]")
    _run("l2s_mouth_transforms", lambda: _lib.load().l2s_mouth_transforms(
        _ptr(landmarks), N, L, _ptr(first), _ptr(count), B, _ptr(mean_face), _ptr(stable_ids), stable_ids.numel(), window_margin,
        std_h, std_w, crop_h, crop_w, start_idx, stop_idx, _ptr(inv), _ptr(origin), _stream()),
        nbytes=16.0 * N * L + 56.0 * N)


def mouth_warp(frames, inv, origin, *, crop_h=96, crop_w=96, roi=None, gray=None, model_in=None, model_crop=88, mean=0.421, std=0.165):
    """The crop window of every frame's aligned image (csrc/mouthroi.hip): frames uint8 [N, H, W, C] (C 1 or 3) or [N, H, W], inv
    fp64 [N, 6], origin int32 [N, 2] -> roi uint8 [N, crop_h, crop_w, C], gray uint8 [N, crop_h, crop_w] and / or model_in fp32
    [N, model_crop, model_crop]; an output left None is not written."""
    _req(frames, torch.uint8, "frames"), _req(inv, torch.float64, "inv"), _req(origin, torch.int32, "origin")
    if frames.dim() not in (3, 4) or not frames.is_contiguous():
        raise L2SError("mouth_warp: frames must be dense [N, H, W, C] or [N, H, W]")
    N, H, W = frames.shape[:3]
    C = frames.shape[3] if frames.dim() == 4 else 1
    if not inv.is_contiguous() or inv.numel() < 6 * N or not origin.is_contiguous() or origin.numel() < 2 * N:
        raise L2SError("mouth_warp: inv dense [N, 6], origin dense [N, 2]")
    if roi is None and gray is None and model_in is None:
        raise L2SError("mouth_warp: roi, gray or model_in is needed")
    for t, dt, n, need in ((roi, torch.uint8, "roi", N * crop_h * crop_w * C), (gray, torch.uint8, "gray", N * crop_h * crop_w),
                           (model_in, torch.float32, "model_in", N * model_crop * model_crop)):
        if t is not None:
            _req(t, dt, n)
            if not t.is_contiguous() or t.numel() < need:
                raise L2SError(f"mouth_warp: {n} must be dense with at least {need} elements")
    out_bytes = sum(t.numel() * t.element_size() for t in (roi, gray, model_in) if t is not None)
    _run("l2s_mouth_warp", lambda: _lib.load().l2s_mouth_warp(
        _ptr(frames), N, H, W, C, _ptr(inv), _ptr(origin), crop_h, crop_w, _ptr(roi), _ptr(gray), _ptr(model_in), model_crop,
        float(mean), float(std), _stream()),
        flops=14.0 * N * crop_h * crop_w * C, nbytes=float(out_bytes) + 4.0 * N * crop_h * crop_w * C, shape=f"N{N} {H}x{W}x{C}")


def _req16(t, dtype, name):
    _req(t, _TORCH16[dtype] if dtype in (F16, BF16) else None, name)
    if dtype not in (F16, BF16):
        raise L2SError(f"{name}: the decoder-step kernels take F16 or BF16 operands")


WHISPER_SAMPLES, WHISPER_FRAMES, WHISPER_MELS = 480000, 3000, 80


def whisper_logmel_workspace(B):
    """Bytes of device workspace whisper_logmel needs (0 = unsupported B)."""
    return int(_lib.load().l2s_whisper_logmel_workspace(B))


def whisper_logmel(wav, workspace, out, basis, fb, fb_range, *, B, S, n_samples=None, ldw=None, ld=None, out_f32=None, dtype=F16):
    """Whisper's log-mel input features (csrc/whisper_logmel.hip): wav fp32 or int16 [B, S <= 480 000] (zero-extended to 30 s),
    n_samples int32 [B] real samples -> out 16-bit rows [B * 3000, ld] (80 bands, zeros in the columns past them) and, when given,
    out_f32 fp32 [B * 3000, 80], the values before the rounding.  basis [400, 448] / fb [80, 201] / fb_range [80, 2]: whisper.LogMel's
    tables.  workspace: whisper_logmel_workspace(B) bytes."""
    ldw = ldw if ldw is not None else S
    _wav_common("whisper_logmel", wav, n_samples, B, S, ldw)
    _req16(out, dtype, "out")
    ld = ld if ld is not None else out.stride(0)
    _req(basis, torch.float32, "basis"), _req(fb, torch.float32, "fb"), _req(fb_range, torch.int32, "fb_range")
    if basis.numel() < 400 * 448 or not basis.is_contiguous() or fb.numel() < 80 * 201 or not fb.is_contiguous() or fb_range.numel() < 160:
        raise L2SError("whisper_logmel: tables smaller than [400, 448], [80, 201], [80, 2]")
    if S > WHISPER_SAMPLES:
        raise L2SError(f"whisper_logmel: a clip has at most {WHISPER_SAMPLES} samples (one 30-s window), got {S}")
    if _extent(out) < (B * WHISPER_FRAMES - 1) * ld + ld:
        raise L2SError("whisper_logmel: out smaller than [B * 3000, ld]")
    if out_f32 is not None:
        _req(out_f32, torch.float32, "out_f32")
        if not out_f32.is_contiguous() or out_f32.numel() < B * WHISPER_FRAMES * WHISPER_MELS:
            raise L2SError("whisper_logmel: out_f32 must be dense fp32 [B * 3000, 80]")
    need = whisper_logmel_workspace(B)
    if need == 0 or workspace.numel() * workspace.element_size() < need:
        raise L2SError(f"whisper_logmel: workspace needs {need} bytes (0 = unsupported B)")
    frames = float(B) * WHISPER_FRAMES
    _run("l2s_whisper_logmel", lambda: _lib.load().l2s_whisper_logmel(
        _ptr(wav), int(wav.dtype == torch.int16), ldw, _ptr(n_samples), B, S, _ptr(basis), _ptr(fb), _ptr(fb_range), _ptr(workspace),
        _ptr(out), ld, _ptr(out_f32), dtype, _stream()),
        flops=2.0 * frames * 400 * 448, nbytes=float(B) * S * wav.element_size() + frames * (8.0 * 80 + 2.0 * ld))


def kv_attention(q, k_cache, v_cache, out, *, B, H, pos=None, pos_stride=0, n_valid=0, k_new=None, v_new=None, ldq=None, ld_new=None,
                 ldo=None, dtype=F16):
    """One query per (clip, head) against a key/value cache (csrc/whisper_decode.hip): q 16-bit [B, 64 H] (already scaled),
    k_cache / v_cache 16-bit dense [B, cache_T, 64 H] -> out 16-bit [B, 64 H].  The valid length is pos[b * pos_stride] + 1 (pos:
    device int32; pos_stride 0 = one position for the batch) or, without pos, n_valid.  k_new / v_new [B, 64 H] are stored at
    cache row pos first (self-attention); rows at or past the valid length are never read."""
    for t, n in ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache"), (out, "out")):
        _req16(t, dtype, n)
    W = 64 * H
    if k_cache.dim() != 3 or k_cache.shape != v_cache.shape or k_cache.shape[0] < B or k_cache.shape[2] != W \
            or not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise L2SError("kv_attention: k_cache / v_cache must be dense [B, cache_T, 64 H]")
    cache_T = k_cache.shape[1]
    if (k_new is None) != (v_new is None):
        raise L2SError("kv_attention: k_new and v_new come together")
    ldq = ldq if ldq is not None else q.stride(0)
    ldo = ldo if ldo is not None else out.stride(0)
    if k_new is not None:
        _req16(k_new, dtype, "k_new"), _req16(v_new, dtype, "v_new")
        ld_new = ld_new if ld_new is not None else k_new.stride(0)
        if v_new.stride(0) != k_new.stride(0) or _extent(k_new) < (B - 1) * ld_new + W or _extent(v_new) < (B - 1) * ld_new + W:
            raise L2SError("kv_attention: k_new / v_new must be [B, 64 H] with one row stride")
    if pos is not None:
        _req(pos, torch.int32, "pos")
        if pos_stride not in (0, 1) or pos.numel() < 1 + (B - 1) * pos_stride:
            raise L2SError("kv_attention: pos is one int32 (pos_stride 0) or [B] (pos_stride 1)")
    if _extent(q) < (B - 1) * ldq + W or _extent(out) < (B - 1) * ldo + W:
        raise L2SError("kv_attention: q / out smaller than [B, 64 H]")
    _run("l2s_kv_attention", lambda: _lib.load().l2s_kv_attention(
        _ptr(q), ldq, _ptr(k_cache), _ptr(v_cache), cache_T, _ptr(k_new), _ptr(v_new), ld_new or 0, _ptr(pos), pos_stride, n_valid,
        B, H, _ptr(out), ldo, dtype, _stream()),
        flops=4.0 * B * W * cache_T, nbytes=4.0 * B * W * cache_T, shape=f"B{B} H{H} T{cache_T}")


def vocab_argmax_workspace(V, B):
    """Bytes of device workspace vocab_argmax needs (0 = unsupported size)."""
    return int(_lib.load().l2s_vocab_argmax_workspace(V, B))


def vocab_argmax(x, emb, workspace, token, logprob, *, B, V, d, suppress=None, begin_suppress=None, step=None, first_step=0,
                 logits=None, ldx=None, lde=None, dtype=F16):
    """The tied output layer with the greedy choice fused in (csrc/whisper_decode.hip): x 16-bit [B, d], emb 16-bit [V, d] ->
    token int32 [B] (argmax of x . emb^T over the ids neither uint8 mask forbids, ties to the smaller id), logprob fp32 [B] (its
    log softmax over the allowed ids) and, when given, logits fp32 dense [B, V].  begin_suppress counts only when the device int32
    step equals first_step.  workspace: vocab_argmax_workspace(V, B) bytes."""
    _req16(x, dtype, "x"), _req16(emb, dtype, "emb")
    _req(token, torch.int32, "token"), _req(logprob, torch.float32, "logprob")
    ldx = ldx if ldx is not None else x.stride(0)
    lde = lde if lde is not None else emb.stride(0)
    if _extent(x) < (B - 1) * ldx + d or _extent(emb) < (V - 1) * lde + d or token.numel() < B or logprob.numel() < B:
        raise L2SError("vocab_argmax: x [B, d], emb [V, d], token [B], logprob [B]")
    for m, n in ((suppress, "suppress"), (begin_suppress, "begin_suppress")):
        if m is not None:
            _req(m, torch.uint8, n)
            if m.numel() < V or not m.is_contiguous():
                raise L2SError(f"vocab_argmax: {n} must be dense uint8 [V]")
    if step is not None:
        _req(step, torch.int32, "step")
    if logits is not None:
        _req(logits, torch.float32, "logits")
        if not logits.is_contiguous() or logits.numel() < B * V:
            raise L2SError("vocab_argmax: logits must be dense fp32 [B, V]")
    need = vocab_argmax_workspace(V, B)
    if need == 0 or workspace.numel() * workspace.element_size() < need:
        raise L2SError(f"vocab_argmax: workspace needs {need} bytes (0 = unsupported V, B)")
    _run("l2s_vocab_argmax", lambda: _lib.load().l2s_vocab_argmax(
        _ptr(x), ldx, _ptr(emb), lde, B, V, d, _ptr(suppress), _ptr(begin_suppress), _ptr(step), first_step, _ptr(workspace),
        _ptr(token), _ptr(logprob), _ptr(logits), dtype, _stream()),
        flops=2.0 * B * V * d, nbytes=2.0 * V * d + 2.0 * B * d, shape=f"B{B} V{V} d{d}")


def whisper_advance(token, logprob, tokens, sum_logprob, lengths, done, tok_emb, pos_emb, x_next, pos, n_active, *, B, V, d, eot,
                    lde=None, ldx=None, dtype=F16):
    """The bookkeeping of one decoder step (csrc/whisper_decode.hip), p = the device int32 pos: token int32 [B] (resolved in place:
    eot once done), tokens int32 [B, max_steps] gets column p, sum_logprob fp32 [B] and lengths int32 [B] grow while a clip is not
    done, done uint8 [B] is set on eot, x_next fp32 [B, d] = tok_emb[token] + pos_emb[p + 1]; then pos += 1 and n_active int32 [1]
    = the clips not done."""
    _req16(tok_emb, dtype, "tok_emb")
    for t, dt, n, cnt in ((token, torch.int32, "token", B), (logprob, torch.float32, "logprob", B), (sum_logprob, torch.float32, "sum_logprob", B),
                          (lengths, torch.int32, "lengths", B), (done, torch.uint8, "done", B), (pos, torch.int32, "pos", 1),
                          (n_active, torch.int32, "n_active", 1)):
        _req(t, dt, n)
        if not t.is_contiguous() or t.numel() < cnt:
            raise L2SError(f"whisper_advance: {n} must be dense with at least {cnt} elements")
    _req(tokens, torch.int32, "tokens"), _req(pos_emb, torch.float32, "pos_emb"), _req(x_next, torch.float32, "x_next")
    if tokens.dim() != 2 or not tokens.is_contiguous() or tokens.shape[0] < B:
        raise L2SError("whisper_advance: tokens must be dense int32 [B, max_steps]")
    ld_tok = tokens.shape[1]
    lde = lde if lde is not None else tok_emb.stride(0)
    ldx = ldx if ldx is not None else x_next.stride(0)
    if pos_emb.dim() != 2 or pos_emb.shape[1] != d or not pos_emb.is_contiguous():
        raise L2SError("whisper_advance: pos_emb must be dense fp32 [n_ctx, d]")
    if _extent(tok_emb) < (V - 1) * lde + d or _extent(x_next) < (B - 1) * ldx + d:
        raise L2SError("whisper_advance: tok_emb [V, d], x_next [B, d]")
    _run("l2s_whisper_advance", lambda: _lib.load().l2s_whisper_advance(
        _ptr(token), _ptr(logprob), _ptr(tokens), ld_tok, _ptr(sum_logprob), _ptr(lengths), _ptr(done), _ptr(tok_emb), lde,
        _ptr(pos_emb), pos_emb.shape[0], _ptr(x_next), ldx, _ptr(pos), _ptr(n_active), B, V, d, eot, dtype, _stream()),
        nbytes=10.0 * B * d)


def _dense(t, dtype, name, count):
    _req(t, dtype, name)
    if not t.is_contiguous() or t.numel() < count:
        raise L2SError(f"{name}: must be dense {dtype} with at least {count} elements")


def beam_attention(q, k_cache, v_cache, out, *, B, beam, H, hd, k_new=None, v_new=None, anc=None, step=None, enc_lens=None,
                   n_live=None, finished=None, ldq=None, ld_new=None, ldo=None, dtype=F16):
    """One query per (clip, beam slot, head) (csrc/s2s_decode.hip): q / out 16-bit [B * beam, H hd], q already scaled.
    Self form (k_new, v_new, anc int16 [2, B, beam, L], step int32 [1]): caches 16-bit dense [B, beam, L, H hd]; slot i stores its
    new rows at (b, i, p) and reads position t < p from row (b, anc[p & 1][b, i, t], t).  Cross form (enc_lens int32 [B]): caches
    dense [B, T_enc, H hd] shared by a clip's slots, keys t < enc_lens[b].  Slots >= n_live[b] and slots of a finished clip get zeros."""
    for t, n in ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache"), (out, "out")):
        _req16(t, dtype, n)
    W = H * hd
    self_form = k_new is not None
    if (k_new is None) != (v_new is None):
        raise L2SError("beam_attention: k_new and v_new come together")
    if self_form:
        if anc is None or step is None or enc_lens is not None:
            raise L2SError("beam_attention: the self form takes anc and step, and no enc_lens")
        if k_cache.dim() != 4 or k_cache.shape != v_cache.shape or k_cache.shape[0] < B or k_cache.shape[1] != beam or k_cache.shape[3] != W \
                or not k_cache.is_contiguous() or not v_cache.is_contiguous():
            raise L2SError("beam_attention: self caches must be dense [B, beam, L, H hd]")
        T = k_cache.shape[2]
        _dense(anc, torch.int16, "anc", 2 * B * beam * T)
        if anc.dim() != 4 or tuple(anc.shape) != (2, B, beam, T):
            raise L2SError("beam_attention: anc must be int16 [2, B, beam, L] with the caches' B and L")
        _dense(step, torch.int32, "step", 1)
        _req16(k_new, dtype, "k_new"), _req16(v_new, dtype, "v_new")
        ld_new = ld_new if ld_new is not None else k_new.stride(0)
        need = (B * beam - 1) * ld_new + W
        if v_new.stride(0) != k_new.stride(0) or _extent(k_new) < need or _extent(v_new) < need:
            raise L2SError("beam_attention: k_new / v_new must be [B * beam, H hd] with one row stride")
    else:
        if enc_lens is None or anc is not None:
            raise L2SError("beam_attention: the cross form takes enc_lens and no anc")
        if k_cache.dim() != 3 or k_cache.shape != v_cache.shape or k_cache.shape[0] < B or k_cache.shape[2] != W \
                or not k_cache.is_contiguous() or not v_cache.is_contiguous():
            raise L2SError("beam_attention: cross caches must be dense [B, T_enc, H hd]")
        T = k_cache.shape[1]
        _dense(enc_lens, torch.int32, "enc_lens", B)
    if n_live is not None:
        _dense(n_live, torch.int32, "n_live", B)
    if finished is not None:
        _dense(finished, torch.uint8, "finished", B)
    ldq = ldq if ldq is not None else q.stride(0)
    ldo = ldo if ldo is not None else out.stride(0)
    if _extent(q) < (B * beam - 1) * ldq + W or _extent(out) < (B * beam - 1) * ldo + W:
        raise L2SError("beam_attention: q / out smaller than [B * beam, H hd]")
    _run("l2s_beam_attention", lambda: _lib.load().l2s_beam_attention(
        _ptr(q), ldq, _ptr(k_cache), _ptr(v_cache), T, _ptr(k_new), _ptr(v_new), ld_new or 0, _ptr(anc), _ptr(step), _ptr(enc_lens),
        _ptr(n_live), _ptr(finished), B, beam, H, hd, _ptr(out), ldo, dtype, _stream()),
        flops=4.0 * B * beam * W * T, nbytes=4.0 * B * (beam if self_form else 1) * W * T, shape=f"B{B} beam{beam} H{H} hd{hd} T{T}")


def beam_select_workspace(V, beam):
    """Nonzero when beam_select serves (V, beam): beam <= 64 and 2 beam + 2 <= V <= 8192 (the selection needs no global workspace)."""
    return int(_lib.load().l2s_beam_select_workspace(V, beam))


def beam_select(logits, scores, step, max_len, cand_score, cand_slot, cand_token, *, B, beam, V, pad, unk, eos, min_len=1,
                temperature=1.0, unk_penalty=0.0, n_live=None, finished=None, ldl=None):
    """The 2 beam best continuations of every clip (csrc/s2s_decode.hip): logits fp32 [B * beam, ldl] (V used), scores fp32
    [2, B, beam] (half step & 1 is current) -> cand_score fp32 / cand_slot / cand_token int32 [B, 2 beam], score descending, a tie
    to the smaller slot * V + token.  log_softmax(logits / temperature), NaN -> -inf, pad -inf, unk penalty, step >= max_len[b]
    leaves eos only, step < min_len forbids eos; at step 0 only slot 0 counts, later the slots < n_live[b]."""
    _req(logits, torch.float32, "logits")
    ldl = ldl if ldl is not None else logits.stride(0)
    if _extent(logits) < (B * beam - 1) * ldl + V:
        raise L2SError("beam_select: logits smaller than [B * beam, V]")
    if beam_select_workspace(V, beam) == 0:
        raise L2SError(f"beam_select: unsupported size (beam {beam} <= 64, 2 beam + 2 <= V {V} <= 8192)")
    K = 2 * beam
    _dense(scores, torch.float32, "scores", 2 * B * beam), _dense(step, torch.int32, "step", 1), _dense(max_len, torch.int32, "max_len", B)
    _dense(cand_score, torch.float32, "cand_score", B * K), _dense(cand_slot, torch.int32, "cand_slot", B * K)
    _dense(cand_token, torch.int32, "cand_token", B * K)
    if n_live is not None:
        _dense(n_live, torch.int32, "n_live", B)
    if finished is not None:
        _dense(finished, torch.uint8, "finished", B)
    _run("l2s_beam_select", lambda: _lib.load().l2s_beam_select(
        _ptr(logits), ldl, _ptr(scores), _ptr(step), _ptr(max_len), _ptr(n_live), _ptr(finished), B, beam, V, pad, unk, eos, min_len,
        float(temperature), float(unk_penalty), _ptr(cand_score), _ptr(cand_slot), _ptr(cand_token), _stream()),
        nbytes=4.0 * B * beam * V * 5, shape=f"B{B} beam{beam} V{V}")


def beam_advance(cand_score, cand_slot, cand_token, tokens, anc, scores, n_live, finished, parents, hyp_tokens, hyp_len, hyp_score,
                 nhyp, out_tokens, out_len, out_score, max_len, emb, pos_table, x_next, step, n_active, *, B, beam, V, d, eos, pad,
                 embed_scale=1.0, lenpen=1.0, normalize_scores=True, lde=None, ldx=None, dtype=F16):
    """The bookkeeping of a beam step (csrc/s2s_decode.hip), p = the device int32 step: eos candidates among the first `beam` are
    finalised into hyp_* (score / (p + 1)^lenpen when normalize_scores), the first `beam` other candidates become the slots of the
    other half of tokens int32 / anc int16 [2, B, beam, L] / scores fp32 [2, B, beam] (parents int32 [B, beam]), x_next fp32
    [B * beam, d] = embed_scale * emb[token] + pos_table[p + 1]; a clip finishes with `beam` hypotheses or at p >= max_len[b] and
    then gets out_tokens / out_len / out_score sorted by score; last step += 1 and n_active = the clips not finished."""
    _req16(emb, dtype, "emb")
    if tokens.dim() != 4 or tokens.shape[0] != 2 or tokens.shape[1] != B or tokens.shape[2] != beam:
        raise L2SError("beam_advance: tokens must be int32 [2, B, beam, L]")
    L, K = tokens.shape[3], 2 * beam
    _dense(tokens, torch.int32, "tokens", 2 * B * beam * L), _dense(anc, torch.int16, "anc", 2 * B * beam * L)
    if tuple(anc.shape) != tuple(tokens.shape):
        raise L2SError("beam_advance: anc must have tokens' shape")
    for t, dt, n, cnt in ((cand_score, torch.float32, "cand_score", B * K), (cand_slot, torch.int32, "cand_slot", B * K),
                          (cand_token, torch.int32, "cand_token", B * K), (scores, torch.float32, "scores", 2 * B * beam),
                          (n_live, torch.int32, "n_live", B), (finished, torch.uint8, "finished", B),
                          (parents, torch.int32, "parents", B * beam), (hyp_tokens, torch.int32, "hyp_tokens", B * beam * L),
                          (hyp_len, torch.int32, "hyp_len", B * beam), (hyp_score, torch.float32, "hyp_score", B * beam),
                          (nhyp, torch.int32, "nhyp", B), (out_tokens, torch.int32, "out_tokens", B * beam * L),
                          (out_len, torch.int32, "out_len", B * beam), (out_score, torch.float32, "out_score", B * beam),
                          (max_len, torch.int32, "max_len", B), (step, torch.int32, "step", 1), (n_active, torch.int32, "n_active", 1)):
        _dense(t, dt, n, cnt)
    _req(pos_table, torch.float32, "pos_table"), _req(x_next, torch.float32, "x_next")
    if pos_table.dim() != 2 or pos_table.shape[0] < L or pos_table.shape[1] != d or not pos_table.is_contiguous():
        raise L2SError("beam_advance: pos_table must be dense fp32 [>= L, d]")
    lde = lde if lde is not None else emb.stride(0)
    ldx = ldx if ldx is not None else x_next.stride(0)
    if _extent(emb) < (V - 1) * lde + d or _extent(x_next) < (B * beam - 1) * ldx + d:
        raise L2SError("beam_advance: emb [V, d], x_next [B * beam, d]")
    _run("l2s_beam_advance", lambda: _lib.load().l2s_beam_advance(
        _ptr(cand_score), _ptr(cand_slot), _ptr(cand_token), _ptr(tokens), _ptr(anc), _ptr(scores), _ptr(n_live), _ptr(finished),
        _ptr(parents), _ptr(hyp_tokens), _ptr(hyp_len), _ptr(hyp_score), _ptr(nhyp), _ptr(out_tokens), _ptr(out_len), _ptr(out_score),
        _ptr(max_len), _ptr(emb), lde, _ptr(pos_table), float(embed_scale), _ptr(x_next), ldx, _ptr(step), _ptr(n_active), B, beam, L, V,
        d, eos, pad, float(lenpen), int(bool(normalize_scores)), dtype, _stream()),
        nbytes=12.0 * B * beam * L + 6.0 * B * beam * d)


# ---- torch.library registration ("PyTorch-ROCm custom ops", SURVEY 8b last row) --------------------------------------------------
# Every launcher above is ALSO a dispatcher-visible operator `torch.ops.lip2speech.<name>` (schema below, CUDA = HIP kernel only: a
# CPU tensor finds no kernel and raises; a fake / meta implementation gives shapes to torch.compile and fake-tensor tracing), and
# the module-level names are rebound to route through the dispatcher - host code keeps calling `ops.tapgemm(...)` and ends in the
# same ctypes call.  The operators mutate their output arguments in place (`Tensor(a!)`) and return nothing, exactly as the C ABI
# does; nothing is computed here.  ALIASES are the operator names SURVEY 8(b) lists, bound to the entry that implements them.
_TG = ("(Tensor A, Tensor W, Tensor(a!) C, *, int M, int N, int Cin, int ntaps=1, int? lda=None, int? ldc=None, Tensor? bias=None, "
       "Tensor? slope=None, Tensor? R=None, int? ldr=None, Tensor(b!)? C2=None, int? ldc2=None, Tensor? lens=None, int mode=0, "
       "int T_out=0, int T_in=0, int stride=1, int dil=1, int off=0, int Ho=0, int Wo=0, int Hi=0, int Wi=0, int KW=1, int pad=0, "
       "int out_row_mul=1, int out_row_add=0, int mask_T=0, int mask_mul=1, int act=0, int flags=0, int dtype=0, float alpha=1.0, "
       "float act_slope=0.0, float slope2=0.0, int groups=1, int a_gstride=0, int c_gstride=0, int w_gstride=0, Tensor? ktab=None, "
       "float? kflops=None) -> ()")
_ATT = ("(Tensor qkv, Tensor(a!) out, *, int B, int T, int H, int? ldq=None, int? ldo=None, Tensor? pos=None, int ldp=0, "
        "Tensor? bias_u=None, Tensor? bias_v=None, Tensor? lens=None, int len_mul=1, int dtype=0) -> ()")
_STEM = "(Tensor x, Tensor w, Tensor bias, Tensor? slope, Tensor(a!) y, int B, int T, int dtype) -> ()"
_RP = ("(Tensor x_l, Tensor w1, Tensor b1, Tensor w2, Tensor b2, *, int B, int T, int C, int k, int dil, float slope, "
       "Tensor(a!)? y=None, Tensor(b!)? xs=None, bool accumulate=False, Tensor? lens=None, int len_mul=1, int dtype=0, "
       "bool xs_final=True) -> ()")
_CPT = ("(Tensor x, Tensor w, float bias, Tensor(a!) wav, Tensor(b!)? pcm, *, int B, int T, int C, int k, Tensor? lens=None, "
        "int len_mul=1) -> ()")
_GLU = ("(Tensor x, Tensor w, Tensor bias, Tensor(a!) y, *, int B, int T, int C, int k, Tensor? lens=None, int len_mul=1, "
        "int dtype=0) -> ()")
_LN = ("(Tensor x, Tensor gamma, Tensor beta, float eps, Tensor(a!) y, *, int M, int C, int? ldx=None, int? ldy=None, "
       "Tensor(b!)? y2=None, int ldy2=0, int zero_prefix=0, Tensor? lens=None, int len_mul=1, int mask_T=0, int dtype=0) -> ()")
_GD = ("(Tensor logits, Tensor(a!) tokens, Tensor(b!) lprobs, Tensor(c!) score, *, int B, int T2, int V, int? ldl=None, "
       "Tensor? lens=None, int len_mul=1, float temperature=1.0, float lenpen=1.0) -> ()")
_BL = "(Tensor x, Tensor[] ws, Tensor[] biases, Tensor[] slopes, Tensor(a!) y, *, int n_images, int H, int W, int C=64, int dtype=0) -> ()"
_SCHEMAS = {
    "tapgemm": _TG,
    "stem_conv3d": _STEM,
    "stem_pool_fused": _STEM,
    "stem_pool_fused_u8": "(Tensor frames, Tensor w, Tensor bias, Tensor? slope, Tensor(a!) y, int B, int T, int dtype, int crop=88, "
                          "float mean=0.421, float std=0.165) -> ()",
    "maxpool2d_3x3s2": "(Tensor x, Tensor(a!) y, int N, int H, int W, int C, int dtype) -> ()",
    "avgpool_hw": "(Tensor x, Tensor(a!) y, int N, int HW, int C, int dtype) -> ()",
    "layernorm": _LN,
    "attention": _ATT,
    "glu_dwconv_swish": _GLU,
    "greedy_decode": _GD,
    "beam_decode": "(Tensor logits, *, int B, int T2, int V, int beam, int? ldl=None, Tensor? lens=None, int len_mul=1, "
                   "float temperature=1.0, float lenpen=1.0) -> (Tensor, Tensor, Tensor, Tensor)",
    "repeat2_cast": "(Tensor x, Tensor(a!) y, int B, int T, int C, int dtype) -> ()",
    "ctc_frames": "(Tensor logits, Tensor(a!) labels, Tensor(b!)? topk_cls, Tensor(c!)? topk_lp, *, int B, int L, int V, int K, "
                  "int? ldl=None, Tensor? lens=None, int len_mul=1) -> ()",
    "ctc_repeat_labels": "(Tensor x, Tensor(a!) y, *, int B, int L, int? ldx=None, int? ldy=None, Tensor? lens=None, "
                         "int len_mul=1) -> ()",
    "ctc_beam_search": "(Tensor topk_cls, Tensor topk_lp, Tensor(a!) workspace, Tensor(b!) labels, Tensor(c!) lengths, "
                       "Tensor(d!) scores, *, int B, int L, int K, int beam, int nbest, Tensor? lens=None, int len_mul=1) -> ()",
    "splitk_reduce": "(Tensor P, Tensor(a!) x, *, int M, int N, int S, int? ldp=None, int? ldx=None) -> ()",
    "splitk_reduce_layernorm": "(Tensor P, Tensor(a!) x, Tensor gamma, Tensor beta, float eps, Tensor(b!) y, *, int M, int C, int S, "
                               "int? ldp=None, int? ldx=None, int? ldy=None, Tensor? lens=None, int len_mul=1, int mask_T=0, int dtype=0) -> ()",
    "cast_f32_to_16": "(Tensor x, Tensor(a!) y, int M, int C, int dtype, int? ldx=None, int? ldy=None) -> ()",
    "cast_16_to_f32": "(Tensor x, Tensor(a!) y, int M, int C, int dtype, int? ldx=None, int? ldy=None) -> ()",
    "broadcast_rows": "(Tensor v, Tensor(a!) y, *, int B, int T, int C, int ldy, int col0=0, int? ldv=None, Tensor? lens=None, "
                      "int len_mul=1, int dtype=0) -> ()",
    "transpose_ct_to_tc": "(Tensor x, Tensor(a!) y, *, int B, int C, int T, int ldy, int col0=0, Tensor? lens=None, int len_mul=1, "
                          "int dtype=0) -> ()",
    "embedding": "(Tensor code, Tensor table, Tensor(a!) y, *, int B, int L, int C, int? ldy=None, Tensor? lens=None, int dtype=0) -> ()",
    "embedding_tokens": "(Tensor tok, Tensor table, Tensor(a!) y, *, int B, int L, int C, int token_offset=4, int? ldt=None, "
                        "int? ldy=None, Tensor? lens=None, int len_mul=1, int dtype=0) -> ()",
    "rows_f32_to_16_masked": "(Tensor x, Tensor(a!) y, *, int B, int T, int C, int? ldx=None, int? ldy=None, int col0=0, "
                             "Tensor? lens=None, int len_mul=1, int dtype=0) -> ()",
    "lens_from_mask": "(Tensor? padding_mask, int B, int T, Device device) -> Tensor",
    "basicblock_fused": "(Tensor x, Tensor w1, Tensor b1, Tensor s1, Tensor w2, Tensor b2, Tensor s2, Tensor(a!) y, *, int n_images, "
                        "int H, int W, int C=64, int dtype=0) -> ()",
    "basiclayer_fused": _BL,
    "basicstage128_tail_fused": "(Tensor x0, Tensor t0, Tensor wa, Tensor ba, Tensor sa, Tensor w1, Tensor b1, Tensor s1, Tensor w2, "
                                "Tensor b2, Tensor s2, Tensor(a!) y, *, int n_images, int H, int W, int dtype=0) -> ()",
    "split_hi_lo": "(Tensor x, Tensor(a!) hi, Tensor(b!) lo, *, int B, int T, int C, int act=0, float slope=0.0, int? ldx=None, "
                   "int? ld16=None, Tensor? lens=None, int len_mul=1, int dtype=0) -> ()",
    "conv_post_tanh": _CPT,
    "resblock_fused": "(Tensor xl, Tensor w, Tensor bias, Tensor(a!) xs, Tensor(b!)? xl_out, *, int B, int T, int C, int k, int[] dil, "
                      "bool accumulate, float slope, Tensor? lens=None, int len_mul=1, int dtype=0) -> ()",
    "resstage_fused": "(Tensor xl, Tensor[] ws, Tensor[] biases, Tensor(a!) xs, Tensor(b!)? xl_out, *, int B, int T, int C, int[] ks, "
                      "int[] dils, float slope, Tensor? lens=None, int len_mul=1, int dtype=0, bool xs_final=True) -> ()",
    "respair": _RP,
    "respair_final": "(Tensor[] xs_l, Tensor[] w1s, Tensor[] b1s, Tensor[] w2s, Tensor[] b2s, Tensor(a!) y, *, int B, int T, int C, int[] ks, "
                     "int[] dils, float slope, Tensor? lens=None, int len_mul=1, int dtype=0) -> ()",
    "preprocess_frames": "(Tensor frames, Tensor(a!) y, *, int B, int T, int Hin, int Win, int crop=88, float mean=0.421, "
                         "float std=0.165, int dtype=0) -> ()",
    "mel_spectrogram": "(Tensor wav, Tensor(a!) mel, Tensor basis, Tensor fb, Tensor fb_range, *, int B, int S, int T_rows, "
                       "Tensor? n_samples=None, int? ldw=None, int? ldm=None, int n_fft=640, int hop=160, int n_mels=80, "
                       "float floor=1e-05) -> ()",
    "stft_mel": "(Tensor wav, Tensor(a!) mel, Tensor basis, Tensor fb, Tensor fb_range, *, int B, int S, int T_rows, int n_fft, int hop, "
                "int pad, float mag_eps=0.0, Tensor? n_samples=None, int? ldw=None, int? ldm=None, int n_mels=80, "
                "float floor=1e-05) -> ()",
    "unit_ce": "(Tensor logits, Tensor target, Tensor(a!) nll, Tensor(b!) smooth, Tensor(c!) n_correct, Tensor(d!) n_tok, *, int B, "
               "int T2, int V, int? ldl=None, int? ldt=None, Tensor? lens=None, int len_mul=2, int pad_idx=1, "
               "int ignore_prefix=0) -> ()",
    "mel_l1_sc": "(Tensor pred, Tensor targ, Tensor(a!) l1, Tensor(b!) sq, Tensor(c!) tsq, Tensor(d!) n_rows, *, int B, int Tm_pred, "
                 "int Tm_targ, int crop_len, Tensor? lens=None, int len_mul=4, int n_mels=80) -> ()",
    "ctc_loss": "(Tensor logits, Tensor targets, Tensor tgt_lens, Tensor tgt_offs, Tensor(a!) workspace, Tensor(b!) nll, *, int B, "
                "int L, int V, int S_max, int blank=0, int? ldl=None, Tensor? lens=None, int len_mul=2) -> ()",
    "wave_stem": "(Tensor wav, Tensor w, Tensor gamma, Tensor beta, Tensor(a!) workspace, Tensor(b!) out, *, int B, int S, int T_rows, "
                 "int C=512, Tensor? n_samples=None, int? ldw=None, int? ldo=None, float eps=1e-05, int dtype=0) -> ()",
    "kmeans_assign": "(Tensor x, Tensor centers, Tensor cnorm, Tensor(a!) ids, *, int B, int T, int D, int K, int? ldx=None, "
                     "Tensor? lens=None, int len_mul=1, Tensor(b!)? best2=None) -> ()",
    "kmeans_nearest": "(Tensor x, Tensor centers, Tensor cnorm, *, int M, int D, int K, Tensor? rows=None, Tensor(a!)? ids=None, "
                      "Tensor(b!)? dmin=None, Tensor(c!)? inertia=None, Tensor(d!)? workspace=None, int? ldx=None) -> ()",
    "kmeans_update": "(Tensor x, Tensor ids, Tensor centers, Tensor counts, Tensor(a!) centers_out, Tensor(b!) counts_out, "
                     "Tensor(c!) cnorm_out, Tensor(d!) workspace, *, int M, int D, int K, Tensor? rows=None, int? ldx=None) -> ()",
    "kmeans_pp_pot": "(Tensor x, Tensor cand, Tensor(a!) workspace, *, int m, int D, int t, Tensor? rows=None, Tensor? closest=None, "
                     "Tensor? select=None, Tensor(b!)? pot=None, Tensor(c!)? closest_out=None, Tensor(d!)? chosen=None, "
                     "int? ldx=None) -> ()",
    "kmeans_pp_pick": "(Tensor closest, Tensor u, Tensor(a!) idx, *, int m, int t, Tensor? scale=None, Tensor(b!)? total=None) -> ()",
    "stoi_resample": "(Tensor wav, Tensor taps, Tensor(a!) out, *, int B, int S, int R, Tensor? n_samples=None, int? ldw=None, "
                     "int? ldo=None) -> ()",
    "stoi_frames": "(Tensor x, Tensor window, Tensor(a!) kept, Tensor(b!) n_kept, *, int B, int S, Tensor? n_samples=None, int? ldx=None, "
                   "int? ldk=None) -> ()",
    "stoi_bands": "(Tensor x, Tensor y, Tensor kept, Tensor n_kept, Tensor window, Tensor basis, Tensor band_edges, Tensor(a!) bands, *, "
                  "int B, int S, int ldf, Tensor? n_samples=None, int? ldx=None, int? ldk=None) -> ()",
    "stoi_scores": "(Tensor bands, Tensor n_kept, Tensor(a!) seg, Tensor(b!) stoi, Tensor(c!) estoi, Tensor(d!) n_segments, *, int B, "
                   "int ldf, int? lds=None) -> ()",
    "wav_gain": "(Tensor wav, Tensor(a!) gain, *, int B, int S, Tensor? n_samples=None, int? ldw=None, float target_dbfs=-30.0) -> ()",
    "stft_mel_power": "(Tensor wav, Tensor(a!) mel, Tensor basis, Tensor fb, Tensor fb_range, *, int B, int S, int T_rows, "
                      "Tensor? n_samples=None, Tensor? n_valid=None, Tensor? scale=None, int? ldw=None, int? ldm=None, int n_fft=400, "
                      "int hop=160, int n_mels=40, int pad=200) -> ()",
    "lstm_layer": "(Tensor xproj, Tensor row_off, Tensor w_hh_p, *, int S, int T, int? n_rows=None, int? ldx=None, int hidden=256, "
                  "Tensor(a!)? h_seq=None, Tensor(b!)? h_last=None) -> ()",
    "spk_embed_head": "(Tensor h_last, Tensor first, Tensor count, Tensor w_t, Tensor bias, Tensor(a!) out, *, int B, "
                      "int? n_rows=None, int hidden=256) -> ()",
    "mouth_transforms": "(Tensor landmarks, Tensor first, Tensor count, Tensor mean_face, Tensor stable_ids, Tensor(a!) inv, "
                        "Tensor(b!) origin, *, int B, int window_margin=12, int std_h=256, int std_w=256, int crop_h=96, int crop_w=96, "
                        "int start_idx=48, int stop_idx=68) -> ()",
    "mouth_warp": "(Tensor frames, Tensor inv, Tensor origin, *, int crop_h=96, int crop_w=96, Tensor(a!)? roi=None, "
                  "Tensor(b!)? gray=None, Tensor(c!)? model_in=None, int model_crop=88, float mean=0.421, float std=0.165) -> ()",
    "whisper_logmel": "(Tensor wav, Tensor(a!) workspace, Tensor(b!) out, Tensor basis, Tensor fb, Tensor fb_range, *, int B, int S, "
                      "Tensor? n_samples=None, int? ldw=None, int? ld=None, Tensor(c!)? out_f32=None, int dtype=0) -> ()",
    "kv_attention": "(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor(c!) out, *, int B, int H, Tensor? pos=None, "
                    "int pos_stride=0, int n_valid=0, Tensor? k_new=None, Tensor? v_new=None, int? ldq=None, int? ld_new=None, "
                    "int? ldo=None, int dtype=0) -> ()",
    "vocab_argmax": "(Tensor x, Tensor emb, Tensor(a!) workspace, Tensor(b!) token, Tensor(c!) logprob, *, int B, int V, int d, "
                    "Tensor? suppress=None, Tensor? begin_suppress=None, Tensor? step=None, int first_step=0, "
                    "Tensor(d!)? logits=None, int? ldx=None, int? lde=None, int dtype=0) -> ()",
    "whisper_advance": "(Tensor(a!) token, Tensor logprob, Tensor(b!) tokens, Tensor(c!) sum_logprob, Tensor(d!) lengths, "
                       "Tensor(e!) done, Tensor tok_emb, Tensor pos_emb, Tensor(f!) x_next, Tensor(g!) pos, Tensor(h!) n_active, *, "
                       "int B, int V, int d, int eot, int? lde=None, int? ldx=None, int dtype=0) -> ()",
    "beam_attention": "(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor(c!) out, *, int B, int beam, int H, int hd, "
                      "Tensor? k_new=None, Tensor? v_new=None, Tensor? anc=None, Tensor? step=None, Tensor? enc_lens=None, "
                      "Tensor? n_live=None, Tensor? finished=None, int? ldq=None, int? ld_new=None, int? ldo=None, int dtype=0) -> ()",
    "beam_select": "(Tensor logits, Tensor scores, Tensor step, Tensor max_len, Tensor(a!) cand_score, Tensor(b!) cand_slot, "
                   "Tensor(c!) cand_token, *, int B, int beam, int V, int pad, int unk, int eos, int min_len=1, float temperature=1.0, "
                   "float unk_penalty=0.0, Tensor? n_live=None, Tensor? finished=None, int? ldl=None) -> ()",
    "beam_advance": "(Tensor cand_score, Tensor cand_slot, Tensor cand_token, Tensor(a!) tokens, Tensor(b!) anc, Tensor(c!) scores, "
                    "Tensor(d!) n_live, Tensor(e!) finished, Tensor(f!) parents, Tensor(g!) hyp_tokens, Tensor(h!) hyp_len, "
                    "Tensor(i!) hyp_score, Tensor(j!) nhyp, Tensor(k!) out_tokens, Tensor(l!) out_len, Tensor(m!) out_score, "
                    "Tensor max_len, Tensor emb, Tensor pos_table, Tensor(n!) x_next, Tensor(o!) step, Tensor(p!) n_active, *, int B, "
                    "int beam, int V, int d, int eos, int pad, float embed_scale=1.0, float lenpen=1.0, bool normalize_scores=True, "
                    "int? lde=None, int? ldx=None, int dtype=0) -> ()",
    "logfbank": "(Tensor wav, Tensor(a!) out, Tensor basis, Tensor fb, Tensor fb_range, *, int B, int S, int T_rows, int stack=4, "
                "bool normalize=True, Tensor? n_samples=None, Tensor? n_rows=None, int? ldw=None, int? ldo=None) -> ()",
}
# C-ABI entry each operator launches (tests/test_torchlib_cpu.py: every device entry of include/lip2speech_hip.h has a twin)
ENTRY_OF = {n: "l2s_" + n for n in _SCHEMAS}
ENTRY_OF.update({"maxpool2d_3x3s2": "l2s_maxpool2d_3x3s2", "avgpool_hw": "l2s_avgpool_hw"})
# host-side queries of the ABI (no launch, nothing for the dispatcher to see)
HOST_QUERIES = ("l2s_abi_version", "l2s_build_info", "l2s_tapgemm_variant", "l2s_tapgemm_epilogue_family", "l2s_attention_variant", "l2s_layernorm_variant", "l2s_respair_variant",
                "l2s_glu_dwconv_tile", "l2s_basicblock_variant", "l2s_stem_pool_frames", "l2s_beam_decode_workspace",
                "l2s_ctc_beam_workspace", "l2s_ctc_loss_workspace", "l2s_wave_stem_workspace", "l2s_kmeans_nearest_workspace",
                "l2s_kmeans_update_workspace", "l2s_kmeans_pp_workspace", "l2s_vocab_argmax_workspace", "l2s_whisper_logmel_workspace",
                "l2s_beam_select_workspace")
# SURVEY 8(b)'s operator names -> the entry that implements them (`mel_head` is a composition of linear_epilogue launches,
# conformer.py::Conformer.forward_rows; it has no kernel of its own)
ALIASES = {"frontend3d_stem": "stem_pool_fused", "resnet_trunk": "basiclayer_fused", "linear_epilogue": "tapgemm",
           "posconv_gelu": "tapgemm", "convtranspose1d": "tapgemm", "mel_head": "tapgemm", "mhsa_padmask": "attention",
           "relpos_mhsa": "attention", "conformer_conv_module": "glu_dwconv_swish", "greedy_unit_decode": "greedy_decode",
           "resblock1": "respair", "tanh_to_int16": "conv_post_tanh"}

_TORCH_LIB = torch.library.Library("lip2speech", "DEF")


def _fake_none(*a, **k):
    return None


def _fake_beam_decode(logits, *, B, T2, V, beam, ldl=None, lens=None, len_mul=1, temperature=1.0, lenpen=1.0):
    return (logits.new_empty((B, beam, T2 + 1), dtype=torch.int32), logits.new_empty((B, beam, T2 + 1), dtype=torch.float32),
            logits.new_empty((B, beam), dtype=torch.float32), logits.new_empty((B,), dtype=torch.int32))


def _fake_lens_from_mask(padding_mask, B, T, device):
    return torch.empty(B, device=device, dtype=torch.int32)


def _resstage_fused_flat(xl, ws, biases, xs, xl_out, *, B, T, C, ks, dils, slope, lens=None, len_mul=1, dtype=F16, xs_final=True):
    return _IMPL["resstage_fused"](xl, ws, biases, xs, xl_out, B=B, T=T, C=C, ks=ks, dils=[dils[i:i + 3] for i in range(0, len(dils), 3)],
                                   slope=slope, lens=lens, len_mul=len_mul, dtype=dtype, xs_final=xs_final)


_IMPL = {}


def _register_torch_ops():
    g = globals()
    for name, schema in _SCHEMAS.items():
        _IMPL[name] = g[name]
    for name, schema in _SCHEMAS.items():
        impl = _resstage_fused_flat if name == "resstage_fused" else _IMPL[name]
        fake = {"beam_decode": _fake_beam_decode, "lens_from_mask": _fake_lens_from_mask}.get(name, _fake_none)
        for op in [name] + [a for a, base in ALIASES.items() if base == name]:
            _TORCH_LIB.define(op + schema)
            # lens_from_mask may be called with no tensor at all (padding_mask = None): it cannot dispatch on a device key
            _TORCH_LIB.impl(op, impl, "CompositeExplicitAutograd" if name == "lens_from_mask" else "CUDA")
            torch.library.register_fake("lip2speech::" + op)(fake)

    def router(name):
        op = getattr(torch.ops.lip2speech, name)

        def call(*a, **k):
            try:
                return op(*a, **k)
            except NotImplementedError as e:    # the dispatcher found no kernel: the operators exist for the HIP device only
                raise L2SError(f"lip2speech::{name}: HIP ops need device tensors (there is no CPU path)") from e
        call.__name__ = name
        call.__doc__ = _IMPL[name].__doc__
        return call
    for name in _SCHEMAS:
        if name == "resstage_fused":
            op = torch.ops.lip2speech.resstage_fused

            def resstage_fused(xl, ws, biases, xs, xl_out, *, B, T, C, ks, dils, slope, lens=None, len_mul=1, dtype=F16, xs_final=True):
                try:
                    return op(xl, list(ws), list(biases), xs, xl_out, B=B, T=T, C=C, ks=[int(k) for k in ks],
                              dils=[int(d) for dl in dils for d in dl], slope=slope, lens=lens, len_mul=len_mul, dtype=dtype,
                              xs_final=xs_final)
                except NotImplementedError as e:
                    raise L2SError("lip2speech::resstage_fused: HIP ops need device tensors (there is no CPU path)") from e
            resstage_fused.__doc__ = _IMPL[name].__doc__
            g[name] = resstage_fused
        else:
            g[name] = router(name)


_register_torch_ops()
