"""Case generator of the vocoder-convolution matrix (tools/check_vocoder_convs.py, tests/test_vocconv_matrix_*.py): l2s_respair,
l2s_respair_final, l2s_resblock_fused, l2s_resstage_fused and l2s_conv_post_tanh, every instantiation of their kernels.

Pure Python: no torch, no GPU, no library.  A case is a dict with `op` ("pair" | "final" | "resblock" | "resstage" | "post"),
`name`, `dt` ("f16" | "bf16"; "f32" for `post`), the shapes and arguments of the launch, its data set (`data`) and `inst`, the
kernel instantiation the case claims to run on under the environment of its child process (ENVS): the launchers read their
switches once per process.  For `pair` the third field of `inst` is the code l2s_respair_variant answers (RM * 1000 + C); for the
others it is the kernel's name and template arguments, read off dispatch_rb / launch_rs (csrc/resblock.hip), l2s_respair_final
(csrc/respair_phase.hip) and the branch of l2s_conv_post_tanh (csrc/misc.hip).  `expect` is the error code of a launch that must be
refused (and must write nothing), 0 otherwise.  The selection rule of l2s_respair, the LDS sizes of csrc/resblock.hip and the tile
walk of csrc/phase_stream.h are restated here; tests/test_vocconv_matrix_cpu.py holds them to the library and to the issue's
figures, the GPU child holds every `pair` case to the instantiation it claims.
"""

DTYPES = ("f16", "bf16")
EUNSUPPORTED = -4                          # include/lip2speech_hip.h
GUARD = 3                                  # guard rows in front of and behind every output buffer

# ---- the child processes: name -> switches -------------------------------------------------------------------------------------------
SWITCHES = ("L2S_RESPAIR_PHASE", "L2S_RESPAIR_XCD", "L2S_RESPAIR_SLOTS")
ENVS = {
    # the default selection, in three children so that each takes a few seconds: the pairs and conv_post; respair_final; the
    # ResBlock and stage kernels
    "default": {},
    "default-final": {},
    "default-narrow": {},
    "pair192": {"L2S_RESPAIR_PHASE": "0"},
    "walk": {"L2S_RESPAIR_SLOTS": "8"},
    "walk-plain": {"L2S_RESPAIR_SLOTS": "8", "L2S_RESPAIR_XCD": "0"},
    "walk192": {"L2S_RESPAIR_SLOTS": "8", "L2S_RESPAIR_PHASE": "0"},
    "walk192-plain": {"L2S_RESPAIR_SLOTS": "8", "L2S_RESPAIR_PHASE": "0", "L2S_RESPAIR_XCD": "0"},
}

# ---- criterion (b): |got - ref| <= FU u max(|ref|, smallest normal) [16-bit output] + F 2^-24 A --------------------------------------
FU = 1.5                                   # the project's margin over the half-ulp bound (tests/_seq_cases.py)
# worst |fp32 - fp64| / (2^-24 A) of the operation evaluated in torch fp32 on the CPU, with the kernels' 16-bit intermediate
# roundings, against the mirrored fp64 reference, over the cases of this file (`tools/check_vocoder_convs.py --cpu-f32`,
# profiles/vocoder_conv_matrix.md has the case behind each figure); the kernels get 8 times that, floored at 8.
# What these figures measure is the one-ulp flip of a 16-bit intermediate: where the fp32 and the fp64 evaluation round t1 (or a
# ResBlock's XL hand-over) to different neighbours the result moves by 2 u of ONE term of A.  That is 2^14 u times the term's share
# of A in units of 2^-24 A, so the figure grows with u (bf16: 8 times f16) and falls with the number of terms K = C k.  One figure
# per operation over both types and every width would hand the f16 kernels bf16's flips and the workload's wide convolutions
# (K = 192 .. 2816) those of K = 64: the figures are therefore kept per type and, for the pairs, per width class (fkind) - each
# is at most the operation-wide figure, never above it, as tests/_seq_cases.py keeps "ln-offset" apart from "ln".
WIDE_K = 768
CPU_F32_WORST = {("pair-narrow", "f16"): 2357.760, ("pair-narrow", "bf16"): 6741.364, ("pair-wide", "f16"): 515.737,
                 ("pair-wide", "bf16"): 1461.525, ("final-narrow", "f16"): 591.165, ("final-narrow", "bf16"): 2542.359,
                 ("final-wide", "f16"): 177.175, ("final-wide", "bf16"): 578.424, ("resblock", "f16"): 10451.162,
                 ("resblock", "bf16"): 102426.152, ("resstage", "f16"): 4269.180, ("resstage", "bf16"): 20008.121, ("post", "f32"): 1.721}


def fkind(c):
    """The class of a case's figure: the pairs by K = C k of their narrowest convolution."""
    if c["op"] == "pair":
        return "pair-wide" if c["C"] * c["k"] >= WIDE_K else "pair-narrow"
    if c["op"] == "final":
        return "final-wide" if c["C"] * min(c["ks"]) >= WIDE_K else "final-narrow"
    return c["op"]


def F_of(kind, dt):
    return max(8.0, 8.0 * CPU_F32_WORST[(kind, dt)])


def cdiv(a, b):
    return (a + b - 1) // b


# ---- l2s_respair: the selection rule, restated (csrc/respair.hip: respair_select) ----------------------------------------------------
RM_PHASE = {64: 512, 128: 256, 256: 128}   # csrc/respair_phase.hip: XGeo<C>::RM
RM_192 = 192                               # csrc/respair.hip: RM
PHASE_H1, R192_H1, PAIR_H2 = 28, 32, 8     # the halos the two kernel families admit


def phase_supports(C, h1, h2):
    return C in RM_PHASE and h1 <= PHASE_H1 and h2 <= PAIR_H2 and RM_PHASE[C] - 2 * h2 >= 16


def respair_variant(C, k, dil, env):
    """RM * 1000 + C of the kernel l2s_respair runs for a valid 16-bit launch, or the error code."""
    if C not in RM_PHASE:
        return EUNSUPPORTED
    h2 = (k - 1) // 2
    h1 = h2 * dil
    mask = int(env.get("L2S_RESPAIR_PHASE", "3"))
    if C == 256 or ((mask & (1 if C == 128 else 2)) and phase_supports(C, h1, h2)):
        return RM_PHASE[C] * 1000 + C if phase_supports(C, h1, h2) else EUNSUPPORTED
    return RM_192 * 1000 + C if (h1 <= R192_H1 and h2 <= PAIR_H2) else EUNSUPPORTED


def respair_grid(ntiles, slots, env):
    """csrc/respair.hip: l2s_respair_grid."""
    n = int(env.get("L2S_RESPAIR_SLOTS", "0"))
    cap = (n & ~7) if n >= 8 else 0
    grid = min((ntiles + 7) & ~7, slots)
    return min(grid, cap) if cap else grid


def tile_walk(ntiles, grid, xcd_order):
    """csrc/phase_stream.h: TileWalk - the tiles of every block, in the order it walks them."""
    out = []
    per, gx = (ntiles + 7) >> 3, (grid + 7) >> 3
    for blk in range(grid):
        if not xcd_order:
            out.append(list(range(blk, ntiles, grid)))
        else:
            xcd, bx = blk & 7, blk >> 3
            lo, hi = xcd * per, min(xcd * per + per, ntiles)
            out.append(list(range(lo + bx, hi, gx)))
    return out


# ---- csrc/resblock.hip: tiles and LDS, restated --------------------------------------------------------------------------------------
def rb_tt(C, k):
    """RBCfg<C, K>::TT."""
    return (368 if k == 7 else 384) if (C == 32 and k != 11) else 512


def rb_halo(k, dils):
    return (k - 1) // 2 * (sum(dils) + 3)


def rb_smem(C, k, dils, stage):
    """rb_smem<C, K, RBCfg | RSCfg>(TT, H) in bytes."""
    H = rb_halo(k, dils)
    gp = 2 if (C == 16 and k != 11) else 1
    if stage:
        TT, RS, lead, wb2 = 512, (16 if C == 16 else 48), cdiv(H, 32) * 32, k != 11
    else:
        TT, RS, lead = rb_tt(C, k), (16 if C == 16 else (48 if k == 11 else 32)), H
        wb2 = not (C == 32 and k != 3) and not (C == 16 and k == 11)
    rows = cdiv(TT + lead + H, 16 * gp) * 16 * gp
    kpad = cdiv(k * C, 32) * 32
    cprp = ((kpad // 8 + 1) // 4) * 4 + 2
    return 2 * (rows + 64) * RS * 2 + (2 if wb2 else 1) * C * cprp * 16


def rb_launches(C, k, dils):
    return rb_smem(C, k, dils, False) <= 160 * 1024


def rs_launches(C, table):
    return max(rb_smem(C, k, d, True) for k, d in zip((3, 7, 11), table)) <= 160 * 1024


def post_smem(C, k):
    return ((256 + k - 1) * (C + 1) + k * C) * 4


# every instantiation the matrix must reach (some child, some case): (op, dt, code)
def instantiations():
    out = []
    for dt in DTYPES:
        out += [("pair", dt, (RM_192 * 1000 + C, kind)) for C in (64, 128) for kind in (0, 1)]
        out += [("pair", dt, (RM_PHASE[C] * 1000 + C, kind)) for C in (256, 128, 64) for kind in (0, 1)]
        out += [("final", dt, ("respair_final_kernel", C)) for C in (256, 128, 64)]
        out += [("resblock", dt, ("resblock_kernel", C, k)) for C in (16, 32) for k in (3, 7, 11)]
        out += [("resstage", dt, ("resstage_kernel", C)) for C in (16, 32)]
    out += [("post", "f32", ("conv_post16_kernel",)), ("post", "f32", ("conv_post_kernel",))]
    return out


def lims(c):
    """Valid rows per clip: lens * len_mul clamped to T."""
    if c["lens"] is None:
        return [c["T"]] * c["B"]
    return [min(n * c["len_mul"], c["T"]) for n in c["lens"]]


def draw(cand, T, i, B=3):
    """B lengths drawn in turn from the candidates that fit in T."""
    fit = []
    for n in cand:
        if 0 <= n <= T and n not in fit:
            fit.append(n)
    return [fit[(3 * i + j) % len(fit)] for j in range(B)]


# ---- conv pairs ----------------------------------------------------------------------------------------------------------------------
KINDS = ("mid", "last", "acc", "last2")    # mid pair; last with overwrite; last with accumulate and Y; last = 2
GEOS = ((1, 1), (3, 1), (5, 3), (7, 3), (7, 4), (9, 3), (11, 1), (11, 5), (3, 28), (9, 7), (13, 2), (17, 1))
SWEEP_GEOS = ((3, 1), (11, 5))
FALLBACK_GEOS = ((9, 8), (11, 6), (3, 29))            # h1 = 32, 30, 29: past the phase kernels' 28, inside respair.hip's 32
REJECT_GEO = (3, 33)


def _pair(name, dt, C, k, dil, T, lens, kind, rm, *, B=3, len_mul=1, slope=0.1, data="randn", expect=0):
    return dict(op="pair", name=name, dt=dt, C=C, k=k, dil=dil, B=B, T=T, lens=lens, len_mul=len_mul, kind=kind, slope=slope,
                data=data, expect=expect, rm=rm, S=rm - (k - 1) if rm else 0)


def pair_cases_of_kernel(dt, C, rm, geos=GEOS, full=True):
    """The cases of one (C, kernel): rm is the kernel's rows per tile."""
    out, tag = [], f"C{C}-rm{rm}"
    for k, dil in geos:
        S = rm - (k - 1)
        for kind in KINDS:
            out.append(_pair(f"{tag}/k{k}d{dil}-{kind}", dt, C, k, dil, S + 1, [S + 1, S, S - 1], kind, rm))
    if not full:
        return out
    i = 0
    for k, dil in SWEEP_GEOS:
        h2 = (k - 1) // 2
        h1, S = h2 * dil, rm - 2 * h2
        for T in sorted({1, h1, S - 1, S, S + 1, 2 * S, 2 * S + 1}):
            lens = draw((T, T - 1, 1, 0, S, S + 1, S - 1, h2, h1 + 1), T, i)
            i += 1
            for kind in ("mid", "acc"):
                out.append(_pair(f"{tag}/k{k}d{dil}-T{T}-{kind}", dt, C, k, dil, T, lens, kind, rm))
    S5 = rm - 4                                           # k = 5: S is a multiple of 4
    for kind in ("mid", "acc"):
        out.append(_pair(f"{tag}/no-lens-{kind}", dt, C, 7, 3, rm - 6 + 1, None, kind, rm))
        # len_mul = 4: the boundary on S, inside the first tile, and clamped to T in the second
        out.append(_pair(f"{tag}/len-mul4-{kind}", dt, C, 5, 3, S5 + 12, [S5 // 4, S5 // 4 - 5, S5 // 4 + 10], kind, rm, len_mul=4))
        out.append(_pair(f"{tag}/slope1-{kind}", dt, C, 3, 1, rm - 1, [rm - 1, rm - 2, rm - 3], kind, rm, slope=1.0))
        out.append(_pair(f"{tag}/slope0.01-negative-{kind}", dt, C, 3, 1, rm - 1, [rm - 1, rm - 2, rm - 3], kind, rm, slope=0.01, data="negative"))
        out.append(_pair(f"{tag}/negative-{kind}", dt, C, 7, 3, rm - 5, [rm - 5, rm - 6, rm - 7], kind, rm, data="negative"))
    for k, dil in SWEEP_GEOS:
        S = rm - (k - 1)
        for kind in ("mid", "last", "acc"):
            out.append(_pair(f"{tag}/k{k}d{dil}-tapcode-{kind}", dt, C, k, dil, 2 * S + 1, [2 * S + 1, S + 3, S - 1], kind, rm, data="tapcode"))
    return out


def pair_walk_cases(dt, C, rm):
    """A block walks three tiles and more: 19 tiles (19 clips of one tile; full, ragged and empty clips) and 21 (3 clips of 7)."""
    out, tag = [], f"C{C}-rm{rm}"
    for k, dil in ((11, 5), (3, 1)):
        S = rm - (k - 1)
        lens19 = [(S, S - 1, 0, S // 2, 1, k)[b % 6] for b in range(19)]
        for kind in ("mid", "acc"):
            out.append(_pair(f"{tag}/walk19-k{k}d{dil}-{kind}", dt, C, k, dil, S, lens19, kind, rm, B=19))
            out.append(_pair(f"{tag}/walk21-k{k}d{dil}-{kind}", dt, C, k, dil, 6 * S + 3, [6 * S + 3, 3 * S + 1, 0], kind, rm))
    return out


def pair_cases(env_name):
    env, out = ENVS[env_name], []
    if env_name in ("default-final", "default-narrow"):
        return out
    for dt in DTYPES:
        if env_name == "default":
            for C in (256, 128, 64):
                out += pair_cases_of_kernel(dt, C, RM_PHASE[C])
            for C in (128, 64):
                # halos only respair.hip holds: the default path falls back to its 192-row kernels
                out += pair_cases_of_kernel(dt, C, RM_192, geos=FALLBACK_GEOS, full=False)
            for k, dil in FALLBACK_GEOS:
                out.append(_pair(f"C256/reject-k{k}d{dil}", dt, 256, k, dil, 100, [100, 99, 0], "mid", 0, expect=EUNSUPPORTED))
            for C in (256, 128, 64):
                for kind in ("mid", "acc"):
                    out.append(_pair(f"C{C}/reject-k3d33-{kind}", dt, C, 3, 33, 100, [100, 99, 0], kind, 0, expect=EUNSUPPORTED))
        elif env_name == "pair192":
            for C in (128, 64):
                out += pair_cases_of_kernel(dt, C, RM_192)
        elif env_name in ("walk", "walk-plain"):
            for C in (256, 128, 64):
                out += pair_walk_cases(dt, C, RM_PHASE[C])
        else:
            for C in (128, 64):
                out += pair_walk_cases(dt, C, RM_192)
    for c in out:
        v = respair_variant(c["C"], c["k"], c["dil"], env)
        c["inst"] = ("pair", c["dt"], (v, 0 if c["kind"] == "mid" else 1))
        assert (v < 0) == (c["expect"] != 0) and (v < 0 or v // 1000 == c["rm"]), (env_name, c["name"], v)
    return out


# ---- the last pairs of a stage in one launch ----------------------------------------------------------------------------------------
FINAL_SETS = (((11,), (5,)), ((3, 7), (5, 3)), ((3, 7, 11), (5, 3, 1)), ((11, 7, 3), (1, 3, 5)), ((1, 17, 5), (4, 1, 3)),
              ((3, 7, 11), (28, 9, 5)))                # the last one reaches h1 = 28, 27, 25
FINAL_SWEEP = (((3, 7, 11), (5, 3, 1)), ((1, 17, 5), (4, 1, 3)))


def _final(name, dt, C, ks, dils, T, lens, *, B=3, len_mul=1, data="randn"):
    rm = RM_PHASE[C]
    return dict(op="final", name=name, dt=dt, C=C, ks=ks, dils=dils, B=B, T=T, lens=lens, len_mul=len_mul, slope=0.1, data=data,
                expect=0, rm=rm, S=rm - (max(ks) - 1), inst=("final", dt, ("respair_final_kernel", C)))


def final_cases(env_name):
    out = []
    for dt in DTYPES:
        for C in (256, 128, 64):
            rm = RM_PHASE[C]
            if env_name == "default":
                i = 0
                for ks, dils in FINAL_SETS:
                    S = rm - (max(ks) - 1)
                    tag = f"C{C}/ks{'-'.join(map(str, ks))}-d{'-'.join(map(str, dils))}"
                    Ts = sorted({1, S - 1, S, S + 1, 2 * S + 1}) if (ks, dils) in FINAL_SWEEP else [S + 1]
                    for T in Ts:
                        out.append(_final(f"{tag}-T{T}", dt, C, ks, dils, T, draw((T, T - 1, 0, S, 1, S - 1), T, i)))
                        i += 1
                S = rm - 10
                out.append(_final(f"C{C}/no-lens", dt, C, (3, 7, 11), (5, 3, 1), S + 1, None))
                S4 = rm - 4
                out.append(_final(f"C{C}/len-mul4", dt, C, (3, 5), (5, 3), S4 + 12, [S4 // 4, S4 // 4 - 5, S4 // 4 + 10], len_mul=4))
                out.append(_final(f"C{C}/negative", dt, C, (3, 7, 11), (5, 3, 1), S + 1, [S + 1, S, 0], data="negative"))
            elif env_name == "walk":
                for ks, dils in (((3, 7, 11), (5, 3, 1)), ((3,), (1,))):
                    S = rm - (max(ks) - 1)
                    lens19 = [(S, S - 1, 0, S // 2, 1, 11)[b % 6] for b in range(19)]
                    tag = f"C{C}/ks{'-'.join(map(str, ks))}"
                    out.append(_final(f"{tag}-walk19", dt, C, ks, dils, S, lens19, B=19))
                    out.append(_final(f"{tag}-walk21", dt, C, ks, dils, 6 * S + 3, [6 * S + 3, 3 * S + 1, 0]))
    return out


# ---- ResBlocks of the narrow stages --------------------------------------------------------------------------------------------------
RB_DILS = ((1, 3, 5), (1, 1, 1), (5, 5, 5), (2, 4, 1), (5, 1, 3))
RB_SWEEP = ((1, 3, 5), (5, 5, 5))


def _rb(name, dt, C, k, dils, T, lens, i, *, len_mul=1, data="randn", slope=0.1):
    # accumulate and xl_out rotate so that every instantiation sees all four combinations; xl_out sits at an address that is 8- but
    # not 16-byte aligned (the launcher admits that)
    return dict(op="resblock", name=name, dt=dt, C=C, k=k, dils=dils, B=3, T=T, lens=lens, len_mul=len_mul, slope=slope, data=data,
                accumulate=bool(i & 1), xl_out=bool(i & 2), xl_off=4, expect=0 if rb_launches(C, k, dils) else EUNSUPPORTED,
                inst=("resblock", dt, ("resblock_kernel", C, k)))


def resblock_cases():
    out = []
    for dt in DTYPES:
        for C in (16, 32):
            for k in (3, 7, 11):
                TT, i, tag = rb_tt(C, k), 0, f"C{C}-k{k}"
                for dils in RB_DILS:
                    H = rb_halo(k, dils)
                    Ts = sorted({1, H, TT - 1, TT, TT + 1, 2 * TT + 1}) if dils in RB_SWEEP else [TT + 1]
                    for T in Ts:
                        lens = draw((T, T - 1, 0, TT, H, 1, TT - 1), T, i)
                        out.append(_rb(f"{tag}/d{''.join(map(str, dils))}-T{T}", dt, C, k, dils, T, lens, i))
                        i += 1
                for j in range(4):                        # every (accumulate, xl_out) combination at one shape, plainly
                    out.append(_rb(f"{tag}/combo{j}", dt, C, k, (1, 3, 5), TT + 1, [TT + 1, TT, 0], j))
                out.append(_rb(f"{tag}/no-lens", dt, C, k, (1, 3, 5), TT + 1, None, 3))
                out.append(_rb(f"{tag}/len-mul4", dt, C, k, (2, 4, 1), TT + 12, [TT // 4, TT // 4 - 5, TT // 4 + 10], 2, len_mul=4))
                out.append(_rb(f"{tag}/negative-slope0.01", dt, C, k, (1, 3, 5), TT + 1, [TT + 1, TT, 7], 1, data="negative", slope=0.01))
                out.append(_rb(f"{tag}/tapcode", dt, C, k, (1, 3, 5), TT + 40, [TT + 40, TT + 3, TT - 1], 2, data="tapcode"))
    return out


# rows: the dilations of the ResBlocks k = 3, 7, 11.  The second table is the widest one the C = 32 kernel's 160 KB of LDS hold (k = 7:
# H = 48 rows, k = 11: H = 60); the third and the fourth launch at C = 16 only and are refused at C = 32 (rs_launches)
RS_TABLES = (((1, 3, 5), (1, 3, 5), (1, 3, 5)), ((5, 5, 5), (5, 5, 3), (1, 3, 5)), ((1, 3, 5), (5, 5, 5), (1, 1, 1)),
             ((5, 5, 5), (5, 5, 5), (5, 5, 5)), ((1, 1, 1), (1, 1, 1), (1, 1, 1)))
RS_T = (1, 511, 512, 513, 1025)


def _rs(name, dt, C, table, T, lens, i, *, len_mul=1, data="randn"):
    xs_final, xl_out = ((True, True), (True, False), (False, True))[i % 3]
    return dict(op="resstage", name=name, dt=dt, C=C, table=table, B=3, T=T, lens=lens, len_mul=len_mul, slope=0.1, data=data,
                xs_final=xs_final, xl_out=xl_out, xl_off=4, expect=0 if rs_launches(C, table) else EUNSUPPORTED,
                inst=("resstage", dt, ("resstage_kernel", C)))


def resstage_cases():
    out = []
    for dt in DTYPES:
        for C in (16, 32):
            i = 0
            for table in RS_TABLES:
                tag = f"C{C}/" + "-".join("".join(map(str, d)) for d in table)
                for T in (RS_T if table in RS_TABLES[:2] else (513,)):
                    out.append(_rs(f"{tag}-T{T}", dt, C, table, T, draw((T, T - 1, 0, 512, 1, 511), T, i), i))
                    i += 1
            for j in range(3):
                out.append(_rs(f"C{C}/combo{j}", dt, C, RS_TABLES[1], 513, [513, 512, 0], j))
            out.append(_rs(f"C{C}/no-lens", dt, C, RS_TABLES[0], 513, None, 0))
            out.append(_rs(f"C{C}/len-mul4", dt, C, RS_TABLES[1], 524, [128, 123, 138], 2, len_mul=4))
            out.append(_rs(f"C{C}/negative", dt, C, RS_TABLES[0], 513, [513, 512, 7], 0, data="negative"))
    return out


# ---- conv_post ----------------------------------------------------------------------------------------------------------------------
POST_SHAPES = ((16, 7, 0), (16, 7, 2), (32, 7, 0), (16, 5, 0), (16, 1, 0), (8, 3, 0), (64, 7, 0))    # (C, k, x offset in floats)
POST_T = (1, 255, 256, 257, 513)


def _post(name, C, k, off, T, lens, *, len_mul=1, pcm=True, data="randn"):
    kern = "conv_post16_kernel" if (C == 16 and k == 7 and (4 * off) % 16 == 0) else "conv_post_kernel"
    return dict(op="post", name=name, dt="f32", C=C, k=k, x_off=off, B=3, T=T, lens=lens, len_mul=len_mul, pcm=pcm, data=data,
                expect=0 if post_smem(C, k) <= 64 * 1024 else EUNSUPPORTED, inst=("post", "f32", (kern,)))


def post_cases():
    out, i = [], 0
    for C, k, off in POST_SHAPES:
        tag = f"C{C}-k{k}" + ("-off8" if off else "")
        for T in POST_T:
            out.append(_post(f"{tag}/T{T}", C, k, off, T, draw((T, T - 1, 0, 256, 1, 255, 257), T, i)))
            i += 1
        out.append(_post(f"{tag}/len-mul4", C, k, off, 268, [64, 59, 74], len_mul=4))
        out.append(_post(f"{tag}/no-pcm-no-lens", C, k, off, 257, None, pcm=False))
        out.append(_post(f"{tag}/saturate", C, k, off, 257, [257, 256, 100], data="saturate"))
    return out


# ---- parts of a child ----------------------------------------------------------------------------------------------------------------
def cases_of(env_name):
    if env_name == "default":
        return pair_cases(env_name) + post_cases()
    if env_name == "default-final":
        return final_cases("default")
    if env_name == "default-narrow":
        return resblock_cases() + resstage_cases()
    if env_name == "walk":
        return pair_cases(env_name) + final_cases(env_name)
    return pair_cases(env_name)
