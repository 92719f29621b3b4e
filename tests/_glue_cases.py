"""Case generator of the unit decoders' and the layout / cast kernels' matrix (tools/check_glue_kernels.py, tests/test_glue_matrix_*.py):
every kernel of csrc/misc.hip and csrc/decode.hip, rows_f32_kernel of csrc/f32_kernels.hip, ctc_frames_kernel and ctc_repeat_kernel of
csrc/ctc.hip, every instantiation.

Pure Python: no torch, no GPU, no library.  A case is a dict with `op`, `name`, `dt` ("f16" | "bf16" | "f32" for the kernels that take a
dtype, "-" for the others), the arguments of the launch, `expect` (the error code of a launch that must be refused and must write
nothing, 0 otherwise) and `inst`, the kernel instantiation the case claims to run on.  grid_for (csrc/misc.hip), the routing of the f32
dtype to l2s_f32_rows and the LDS size of conv_post_kernel are restated here; tests/test_glue_matrix_cpu.py proves the coverage.
These kernels read no environment switches: the parts (one child process each) split the work by run time only.
"""

DTYPES = ("f16", "bf16")
EINVAL, ESHAPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4      # include/lip2speech_hip.h
GUARD = 3                                  # guard rows in front of and behind every buffer
CANARY32, CANARY16 = 0x5A5A5A5A, 0x5A5A    # int32 / int16 and 16-bit float bit patterns; floating point buffers of 32 bits carry NaN
GRID_CAP, GRID_BLOCK = 8192, 256
CAP_ITEMS = GRID_CAP * GRID_BLOCK          # 2 097 152 work items: one more and the grid-stride loop takes a second trip
DELTA = 2.0 ** -6                          # coded beams: the runner-up of coded step i sits delta 2^i below the best unit
TOL_ABS = {"convpost": 2e-5, "greedy": 1e-4, "beam": 1e-4}   # criterion (a), the tolerances of tests/test_kernels_gpu.py
SKIP_CAP = 0.25                            # random beams: the share of ranks that may be too close to compare

PARTS = ("casts", "rows", "lookups", "split", "reduce-post", "greedy", "beam", "ctc")

# worst |fp32 - fp64| / (2^-24 A) of the operation evaluated in torch fp32 on the CPU against the fp64 reference over the cases of this
# file (`tools/check_glue_kernels.py --cpu-f32`); the kernels get 8 times that, floored at 8 (tests/_frontend_cases.py::F_of).
CPU_F32_WORST = {"beam-pos": 1.175, "beam-score": 0.545, "convpost": 1.246, "ctc-lp": 1.623, "greedy-lprob": 1.566, "greedy-score": 2.340,
                 "split-gelu": 1.949}
# random beams: G = 16 x the largest deviation of the fp32 oracle's hypothesis scores from the fp64 restatement on that case
# (`--cpu-f32` prints it); a rank closer than G to a neighbour is not compared
BEAM_G = {"beam/random-V204-beam5-L30": 4.491e-06, "beam/random-V204-beam50-L30": 5.768e-07, "beam/random-V204-beam64-L30": 3.478e-06,
          "beam/random-V256-beam64-L24": 1.848e-05, "beam/random-V68-beam64-L30": 2.283e-06, "beam/random-V5-beam1-L30": 5.903e-06,
          "beam/random-V204-beam2-L30-mul2": 3.019e-06}


def F_of(kind):
    return max(8.0, 8.0 * CPU_F32_WORST[kind])


def cdiv(a, b):
    return (a + b - 1) // b


def grid_for(total, block=GRID_BLOCK):
    return max(1, min(GRID_CAP, cdiv(total, block)))


def takes_stride_loop(total):
    return total > CAP_ITEMS


def convpost_smem(C, k):
    """bytes of LDS l2s_conv_post_tanh asks for (CP_TILE = 256); more than 64 KB is refused"""
    return ((256 + k - 1) * (C + 1) + k * C) * 4


def lens_of(B, T, len_mul):
    """The ragged clip lengths of a masked case: 0, a value past T (the clamp), about half of T, T exactly, ... (before len_mul)"""
    base = [0, T // len_mul + 2, max(1, (T // 2) // len_mul), cdiv(T, len_mul), 1]
    return [base[b % 5] for b in range(B)]


# ---- the kernel a case runs on, and its grid-stride work items ---------------------------------------------------------------------------
CAPPED = ("repeat2_cast_kernel", "cast_to16_kernel", "cast_to32_kernel", "broadcast_rows_kernel", "embedding_kernel", "embedding_tokens_kernel",
          "rows_to16_masked_kernel", "split_hi_lo_kernel", "splitk_reduce_kernel", "rows_f32_kernel")
F32_ROUTED = ("repeat2", "cast16", "cast32", "bcast", "rows16")        # entry points whose f32 dtype goes to l2s_f32_rows
F32_REFUSED = ("transpose", "embedding", "embtok", "split")            # DISPATCH_ET: L2S_EINVAL


def inst_of(c):
    op, dt = c["op"], c["dt"]
    if dt == "f32" and op in F32_ROUTED:
        return ("rows_f32_kernel", "f32", op == "bcast")
    return {"repeat2": ("repeat2_cast_kernel", dt, None), "cast16": ("cast_to16_kernel", dt, None), "cast32": ("cast_to32_kernel", dt, None),
            "bcast": ("broadcast_rows_kernel", dt, c.get("v32")), "transpose": ("transpose_ct_kernel", dt, None),
            "embedding": ("embedding_kernel", dt, None), "embtok": ("embedding_tokens_kernel", dt, None),
            "rows16": ("rows_to16_masked_kernel", dt, None), "lensmask": ("lens_from_mask_kernel", "-", None),
            "split": ("split_hi_lo_kernel", dt, c.get("act")), "splitk": ("splitk_reduce_kernel", "-", None),
            "convpost": ("conv_post16_kernel" if (c.get("C"), c.get("k")) == (16, 7) and not c.get("xoff") else "conv_post_kernel", "-", None),
            "greedy": ("greedy_decode_kernel+decode_score_kernel", "-", None), "beam": ("beam_decode_kernel", "-", None),
            "ctcframes": ("ctc_frames_kernel", "-", None), "ctcrepeat": ("ctc_repeat_kernel", "-", None)}[op]


def instantiations():
    out = [("lens_from_mask_kernel", "-", None), ("splitk_reduce_kernel", "-", None), ("conv_post_kernel", "-", None), ("conv_post16_kernel", "-", None),
           ("rows_f32_kernel", "f32", False), ("rows_f32_kernel", "f32", True), ("greedy_decode_kernel+decode_score_kernel", "-", None),
           ("beam_decode_kernel", "-", None), ("ctc_frames_kernel", "-", None), ("ctc_repeat_kernel", "-", None)]
    for dt in DTYPES:
        out += [(k, dt, None) for k in ("repeat2_cast_kernel", "cast_to16_kernel", "cast_to32_kernel", "transpose_ct_kernel", "embedding_kernel",
                                        "embedding_tokens_kernel", "rows_to16_masked_kernel")]
        out += [("broadcast_rows_kernel", dt, v32) for v32 in (True, False)] + [("split_hi_lo_kernel", dt, act) for act in (0, 1, 2)]
    return out


def items_of(c):
    """The grid-stride work items of a launch on a capped kernel."""
    op, f32 = c["op"], c["dt"] == "f32"
    if op == "repeat2":
        return c["B"] * c["T"] * (c["C"] if f32 else c["C"] // 4)
    if op in ("cast16", "cast32"):
        return c["M"] * c["C"]
    if op == "bcast":
        return c["B"] * c["T"] * c["C"]
    if op in ("rows16", "split"):
        return c["B"] * c["T"] * (c["C"] if f32 else c["C"] // 4)
    if op in ("embedding", "embtok"):
        return c["B"] * c["L"] * (c["C"] // 8)
    if op == "splitk":
        return c["M"] * (c["N"] // 4)
    raise ValueError(op)


def one_row_less(c):
    """items_of the same launch with one row (of the slowest dimension the kernel's alignment rules leave free) less"""
    d = dict(c)
    for k in ("T", "M", "L"):
        if k in d:
            d[k] -= 1
            return items_of(d) if d[k] > 0 else 0
    raise ValueError(c["op"])


def K(op, name, dt, expect=0, **kw):
    c = dict(op=op, name=f"{op}/{name}", dt=dt, expect=expect, **kw)
    c["inst"] = inst_of(c)
    return c


# ---- casts ------------------------------------------------------------------------------------------------------------------------------
CAST_SHAPES = ((1, 1, 0, 0), (3, 7, 0, 0), (37, 80, 4, 11), (2049, 1024, 0, 0))     # M, C, ldx - C, ldy - C


def cast_cases():
    out = []
    for dt in DTYPES:
        out.append(K("cast32", "all-patterns-64x1024", dt, M=64, C=1024, ldx=1032, ldy=1028, data="patterns"))
        out.append(K("cast32", "3x7", dt, M=3, C=7, ldx=9, ldy=7, data="patterns"))
        out.append(K("cast32", "cap-2049x1024", dt, M=2049, C=1024, ldx=1024, ldy=1024, data="patterns"))
        for M, C, px, py in CAST_SHAPES:
            out.append(K("cast16", f"coded-{M}x{C}" + ("-cap" if M == 2049 else ""), dt, M=M, C=C, ldx=C + px, ldy=C + py, data="coded"))
    out.append(K("cast16", "f32-copy-37x80", "f32", M=37, C=80, ldx=84, ldy=91, data="coded"))
    out.append(K("cast16", "f32-copy-cap-2049x1024", "f32", M=2049, C=1024, ldx=1024, ldy=1024, data="coded"))
    out.append(K("cast32", "f32-copy-3x7", "f32", M=3, C=7, ldx=9, ldy=8, data="patterns"))
    return out


# ---- row kernels ------------------------------------------------------------------------------------------------------------------------
def row_cases():
    out = []
    for dt in DTYPES + ("f32",):
        for C in (4, 12, 512):
            for B, T in ((1, 1), (3, 13)):
                out.append(K("repeat2", f"C{C}-B{B}-T{T}", dt, B=B, T=T, C=C))
        if dt != "f32":
            out.append(K("repeat2", "cap-rows8193-C1024", dt, B=1, T=8193, C=1024))
        out.append(K("repeat2", "refused-C6", dt, EALIGN, B=3, T=13, C=6))
        i = 0
        for C in (4, 80):
            for col0 in (0, 4, 128):
                for len_mul in (1, 4):
                    lens = "none" if i % 3 == 2 else "mixed"
                    out.append(K("rows16", f"C{C}-col{col0}-mul{len_mul}-lens-{lens}", dt, B=5, T=(13, 1, 16)[i % 3], C=C, ldx=C + 4, ldy=col0 + C + 8,
                                 col0=col0, len_mul=len_mul, lens=lens))
                    i += 1
        if dt != "f32":
            out.append(K("rows16", "cap-B3-T2731-C1024", dt, B=3, T=2731, C=1024, ldx=1024, ldy=1024, col0=0, len_mul=1, lens="mixed"))
        out.append(K("rows16", "refused-col2", dt, EALIGN, B=2, T=5, C=4, ldx=8, ldy=16, col0=2, len_mul=1, lens="mixed"))
        out.append(K("rows16", "refused-ldx-odd", dt, EALIGN, B=2, T=5, C=4, ldx=9, ldy=16, col0=0, len_mul=1, lens="mixed"))
        out.append(K("rows16", "refused-mul0", dt, ESHAPE, B=2, T=5, C=4, ldx=8, ldy=16, col0=0, len_mul=0, lens="mixed"))
        for v32 in ((True,) if dt == "f32" else (True, False)):
            i = 0
            for C in (1, 7, 128):
                for col0 in (3, 0, 4):
                    for T in (1, 33):
                        lens = "none" if i % 4 == 3 else "mixed"
                        out.append(K("bcast", f"{'v32' if v32 else 'v16'}-C{C}-col{col0}-T{T}-lens-{lens}", dt, B=4, T=T, C=C, ldv=C + 3, ldy=col0 + C + 5,
                                     col0=col0, len_mul=1 + i % 2, lens=lens, v32=v32))
                        i += 1
        if dt == "f32":
            out.append(K("bcast", "refused-f32-with-v16", dt, EINVAL, B=2, T=3, C=7, ldv=8, ldy=8, col0=0, len_mul=1, lens="mixed", v32=False))
        else:
            out.append(K("bcast", "v16-cap-B2-T1025-C1024", dt, B=2, T=1025, C=1024, ldv=1024, ldy=1024, col0=0, len_mul=1, lens="mixed", v32=False))
    return out


# ---- look-ups, the transpose, lens_from_mask --------------------------------------------------------------------------------------------
TRANSPOSE_CT = ((80, 13), (32, 32), (33, 31), (1, 1), (31, 65))
LENSMASK_T = (1, 63, 64, 65, 200)


def lookup_cases():
    out = []
    for dt in DTYPES + ("f32",):
        refused = EINVAL if dt == "f32" else 0
        for i, (C, T) in enumerate(TRANSPOSE_CT):
            if refused and i:
                continue
            for col0 in (0, 5):
                lens = "none" if (i + col0) % 3 == 2 else "mixed"
                out.append(K("transpose", f"C{C}-T{T}-col{col0}-lens-{lens}" + ("-refused-f32" if refused else ""), dt, refused, B=3, C=C, T=T,
                             col0=col0, ldy=col0 + C + 3, len_mul=1 + i % 2, lens=lens))
        if refused:
            out.append(K("embedding", "refused-f32", dt, EINVAL, B=2, L=5, C=8, ldy=16, n=7, lens="mixed"))
            out.append(K("embtok", "refused-f32", dt, EINVAL, B=2, L=5, C=8, ldy=16, ldt=6, n=7, off=4, len_mul=1, lens="mixed"))
            continue
        for C in (8, 128):
            for lens in ("mixed", "none"):
                out.append(K("embedding", f"C{C}-lens-{lens}", dt, B=5, L=11, C=C, ldy=C + 8, n=204, lens=lens))
                for off in (0, 4):
                    for len_mul in (1, 2):
                        out.append(K("embtok", f"C{C}-off{off}-mul{len_mul}-lens-{lens}", dt, B=5, L=11, C=C, ldy=C + 8, ldt=14, n=23, off=off,
                                     len_mul=len_mul, lens=lens))
        out.append(K("embedding", "cap-B5-L3277-C1024", dt, B=5, L=3277, C=1024, ldy=1024, n=64, lens="mixed"))
        out.append(K("embtok", "cap-B5-L3277-C1024", dt, B=5, L=3277, C=1024, ldy=1024, ldt=3280, n=64, off=4, len_mul=1, lens="mixed"))
        out.append(K("embedding", "refused-C12", dt, EALIGN, B=2, L=5, C=12, ldy=16, n=7, lens="mixed"))
        out.append(K("embtok", "refused-ldt-below-L", dt, ESHAPE, B=2, L=5, C=8, ldy=16, ldt=4, n=7, off=4, len_mul=1, lens="mixed"))
    for T in LENSMASK_T:
        out.append(K("lensmask", f"T{T}", "-", B=5, T=T, mask=True))
    out.append(K("lensmask", "T65-no-mask", "-", B=5, T=65, mask=False))
    return out


# ---- split_hi_lo ------------------------------------------------------------------------------------------------------------------------
SLOPE = 0.1


def split_cases():
    out = []
    for dt in DTYPES:
        i = 0
        for act in (0, 1, 2):
            for C in (4, 64):
                for len_mul in (1, 4):
                    lens = "none" if i % 3 == 2 else "mixed"
                    out.append(K("split", f"act{act}-C{C}-mul{len_mul}-lens-{lens}", dt, act=act, B=5, T=(13, 16, 29)[i % 3], C=C, ldx=C + 4, ld16=C + 8,
                                 len_mul=len_mul, lens=lens))
                    i += 1
            out.append(K("split", f"act{act}-cap-B3-T2731-C1024" if act == 0 else f"act{act}-B3-T27-C1024", dt, act=act, B=3, T=2731 if act == 0 else 27,
                         C=1024, ldx=1024, ld16=1024, len_mul=1, lens="mixed"))
        out.append(K("split", "refused-act3", dt, ESHAPE, act=3, B=2, T=5, C=4, ldx=8, ld16=8, len_mul=1, lens="mixed"))
        out.append(K("split", "refused-C6", dt, EALIGN, act=0, B=2, T=5, C=6, ldx=8, ld16=8, len_mul=1, lens="mixed"))
    out.append(K("split", "refused-f32", "f32", EINVAL, act=0, B=2, T=5, C=4, ldx=8, ld16=8, len_mul=1, lens="mixed"))
    return out


# ---- splitk_reduce and conv_post_tanh ---------------------------------------------------------------------------------------------------
CONVPOST_SHAPES = ((16, 7, 0), (16, 7, 1), (16, 5, 0), (32, 7, 0), (1, 1, 0), (59, 7, 0))     # C, k, x offset in floats
CONVPOST_T = (1, 3, 255, 256, 257, 700)


def reduce_post_cases():
    out = []
    for S in (1, 2, 8):
        for N in (4, 64, 1024):
            for M in (1, 37):
                out.append(K("splitk", f"S{S}-N{N}-M{M}", "-", S=S, N=N, M=M, ldp=S * N + 4, ldx=N + 8, data="randn"))
    out.append(K("splitk", "order-S8-N64-M37", "-", S=8, N=64, M=37, ldp=8 * 64 + 4, ldx=72, data="order"))
    out.append(K("splitk", "cap-S2-N1024-M8193", "-", S=2, N=1024, M=8193, ldp=2048, ldx=1024, data="randn"))
    for C, k, xoff in CONVPOST_SHAPES:
        for i, T in enumerate(CONVPOST_T):
            lens = "none" if (i + C) % 3 == 2 else "mixed"
            out.append(K("convpost", f"C{C}-k{k}{'-offset' if xoff else ''}-T{T}-lens-{lens}", "-", B=5, T=T, C=C, k=k, xoff=xoff, len_mul=1 + i % 2, lens=lens,
                         pcm=True, data="randn"))
    for xoff in (0, 1):
        out.append(K("convpost", f"C16-k7{'-offset' if xoff else ''}-T257-no-pcm", "-", B=5, T=257, C=16, k=7, xoff=xoff, len_mul=1, lens="mixed", pcm=False,
                     data="randn"))
        out.append(K("convpost", f"C16-k7{'-offset' if xoff else ''}-T300-saturated", "-", B=4, T=300, C=16, k=7, xoff=xoff, len_mul=1, lens="none", pcm=True,
                     data="saturated"))
    out.append(K("convpost", "refused-C60-k7", "-", EUNSUPPORTED, B=2, T=5, C=60, k=7, xoff=0, len_mul=1, lens="mixed", pcm=True, data="randn"))
    out.append(K("convpost", "refused-k4", "-", ESHAPE, B=2, T=5, C=16, k=4, xoff=0, len_mul=1, lens="mixed", pcm=True, data="randn"))
    return out


# ---- decoders -----------------------------------------------------------------------------------------------------------------------------
GREEDY_V = (5, 63, 64, 65, 204, 256, 257, 1004)
GREEDY_T2 = (1, 2, 3, 4, 62, 63, 64, 65, 130)
TEMPS, LENPENS = (0.5, 1.0, 1.3), (0.0, 1.0, 1.7)
GREEDY_LENS = ("none", "full", "zero-first", "clamp", "mul2")       # see greedy_lens


def greedy_lens(mode, B, T2):
    """(lens or None, len_mul, the effective L per clip)"""
    if mode == "none":
        return None, 1, [T2] * B
    if mode == "mul0":                                    # refused
        return [1] * B, 0, [0] * B
    if mode == "mul2":
        lens = [cdiv(T2, 2), T2 // 2, max(0, T2 // 2 - 1), T2][:B]          # the last clamps: 2 T2 > T2
        return lens, 2, [min(2 * n, T2) for n in lens]
    lens = {"full": [T2, T2 - 1, T2, max(T2 - 2, 0)], "zero-first": [0, T2, T2 // 2, T2 - 1], "clamp": [T2 + 3, T2, 2 * T2, T2 // 3]}[mode][:B]
    return lens, 1, [min(n, T2) for n in lens]


def greedy_cases():
    out = []
    i = 0
    for V in GREEDY_V:
        for T2 in GREEDY_T2:
            mode = GREEDY_LENS[i % 5]
            out.append(K("greedy", f"V{V}-T{T2}-{mode}-temp{TEMPS[i % 3]}-lenpen{LENPENS[(i // 3) % 3]}-ldl+{3 * (i % 2)}", "-", B=4, V=V, T2=T2, ldl=V + 3 * (i % 2),
                         temp=TEMPS[i % 3], lenpen=LENPENS[(i // 3) % 3], lens=mode))
            i += 7                                        # 7 is coprime to 2, 3, 5, 9: every value of every parameter meets every V
    base = dict(B=2, V=204, T2=6, ldl=204, temp=1.0, lenpen=1.0, lens="full")
    out.append(K("greedy", "refused-V4", "-", ESHAPE, **{**base, "V": 4, "ldl": 4}))
    out.append(K("greedy", "refused-ldl-below-V", "-", ESHAPE, **{**base, "ldl": 203}))
    out.append(K("greedy", "refused-temperature-0", "-", EINVAL, **{**base, "temp": 0.0}))
    out.append(K("greedy", "refused-len_mul-0", "-", EINVAL, **{**base, "lens": "mul0"}))
    return out


BEAM_L = (0, 1, 2, 63, 64, 65, 130)


def n_coded(L):
    return min(7, L)


def beam_cases():
    """Ls: the clips' lengths; T2 = max(max(Ls), 1); lens = Ls ("lens": "none" when every L is T2)."""
    out = []

    def add(name, data, V, beam, Ls, temp=1.0, lenpen=1.0, ldl=0, len_mul=1, lens="lens", expect=0, **kw):
        T2 = max(max(Ls), 1)
        out.append(K("beam", name, "-", expect, data=data, V=V, beam=beam, Ls=list(Ls), T2=T2, B=len(Ls), temp=temp, lenpen=lenpen, ldl=V + ldl,
                     len_mul=len_mul, lens=lens, **kw))

    # coded clips: every rank is checked
    add("coded-V204-beam64-L130-65-64", "coded", 204, 64, (130, 65, 64))
    add("coded-V204-beam64-L130-temp0.9", "coded", 204, 64, (130, 63), temp=0.9, lenpen=1.7, ldl=3)
    add("coded-V204-beam64-L130-temp2-no-lens", "coded", 204, 64, (130, 130), temp=2.0, lenpen=0.0, lens="none")
    add("coded-V256-beam64-L65-130", "coded", 256, 64, (65, 130, 8), ldl=3)
    add("coded-V256-beam50-L64-62-130-mul2", "coded", 256, 50, (64, 62, 130), temp=1.3, len_mul=2)
    add("coded-V68-beam64-L64-63", "coded", 68, 64, (64, 63, 7), temp=0.5)
    add("coded-V204-beam5-L130-clamp", "coded", 204, 5, (65, 3, 130), lens="clamp")
    add("coded-V204-beam2-L1-2-0", "coded", 204, 2, (1, 2, 0, 2))
    add("coded-V5-beam1-L0-1-2-65", "coded", 5, 1, (0, 1, 2, 65), lenpen=1.7)
    add("coded-V204-beam1-L130", "coded", 204, 1, (130, 64))
    # random clips (randn 2.5): a rank is compared where the fp64 score separates it from both neighbours by more than G
    add("random-V204-beam5-L30", "random", 204, 5, (30, 24, 30, 17))
    add("random-V204-beam50-L30", "random", 204, 50, (30, 29), temp=1.3, lenpen=1.7, ldl=3)
    add("random-V204-beam64-L30", "random", 204, 64, (30, 30), lens="none")
    add("random-V256-beam64-L24", "random", 256, 64, (24, 12), temp=0.5, lenpen=0.0)
    add("random-V68-beam64-L30", "random", 68, 64, (30, 16))
    add("random-V5-beam1-L30", "random", 5, 1, (30, 2, 1, 0))
    add("random-V204-beam2-L30-mul2", "random", 204, 2, (30, 16, 2), len_mul=2)
    # refusals
    add("refused-V257", "random", 257, 5, (6, 6), expect=EUNSUPPORTED)
    add("refused-beam65", "random", 204, 65, (6, 6), expect=EUNSUPPORTED)
    add("refused-beam-V-3", "random", 67, 64, (6, 6), expect=EUNSUPPORTED)
    add("refused-beam-V-3-small", "random", 12, 9, (6, 6), expect=EUNSUPPORTED)
    add("refused-workspace-one-byte-short", "random", 204, 5, (6, 6), expect=ESHAPE, ws_short=1)
    add("refused-workspace-misaligned-by-2", "random", 204, 5, (6, 6), expect=ESHAPE, ws_off=2)
    return out


CTC_V = (2, 63, 64, 65, 4095, 4096)
CTCREPEAT_L = (1, 63, 64, 65, 129, 200)


def ctc_cases():
    out = []
    for i, V in enumerate(CTC_V):
        for K_ in (0, 1, min(V, 64)):
            lens = ("mixed", "none", "mixed")[(i + K_) % 3]
            out.append(K("ctcframes", f"V{V}-K{K_}-lens-{lens}", "-", B=3, L=5, V=V, K=K_, ldl=V + 3, len_mul=1 + i % 2, lens=lens))
    out.append(K("ctcframes", "refused-V4097", "-", EUNSUPPORTED, B=2, L=5, V=4097, K=1, ldl=4097, len_mul=1, lens="mixed"))
    out.append(K("ctcframes", "refused-K65", "-", EUNSUPPORTED, B=2, L=5, V=4096, K=65, ldl=4096, len_mul=1, lens="mixed"))
    out.append(K("ctcframes", "refused-K-above-V", "-", ESHAPE, B=2, L=5, V=2, K=3, ldl=2, len_mul=1, lens="mixed"))
    for i, L in enumerate(CTCREPEAT_L):
        for mode in ("none", "mixed", "mul2"):
            inplace = (i + len(mode)) % 2 == 0
            out.append(K("ctcrepeat", f"L{L}-lens-{mode}" + ("-in-place" if inplace else ""), "-", B=6, L=L, ldx=L + 3, ldy=L + 3 if inplace else L + 5,
                         len_mul=2 if mode == "mul2" else 1, lens="none" if mode == "none" else "mixed", inplace=inplace))
    return out


_CASES = {"casts": cast_cases, "rows": row_cases, "lookups": lookup_cases, "split": split_cases, "reduce-post": reduce_post_cases,
          "greedy": greedy_cases, "beam": beam_cases, "ctc": ctc_cases}


def cases_of(part):
    return _CASES[part]()


def all_cases():
    return [(p, c) for p in PARTS for c in cases_of(p)]
