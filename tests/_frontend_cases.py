"""Case generator of the lip front end's kernel matrix (tools/check_frontend_kernels.py, tests/test_frontend_matrix_*.py): the fused
BasicBlocks (csrc/basicblock.hip, csrc/basicblock_phase.hip incl. the TAIL variant), the stem kernels, the pools and
preprocess_frames (csrc/frontend.hip), every instantiation.

Pure Python: no torch, no GPU, no library.  A case is a dict with `op` ("bb" | "tail" | "stem" | "stem2" | "maxpool" | "avgpool" |
"preproc"), `name`, `dt` ("f16" | "bf16"; the pools and preprocess also "f32"), the arguments of the launch, its data set (`data`)
and `inst`, the kernel instantiation the case claims to run on under the environment of its child (ENVS): the launchers read their
switches once per process.  For `bb` the third field of `inst` is the code l2s_basicblock_variant answers; a stem case also carries
`ft`, the frames per block l2s_stem_pool_frames answers in that child.  `expect` is the error code of a launch that must be refused
(and must write nothing), 0 otherwise.  The admission rule of bb_launch_checked (csrc/basicblock.hip), the ft rule of
stem_pool_dispatch and grid_for (csrc/frontend.hip) and the persistent blocks' tile walk are restated here;
tests/test_frontend_matrix_cpu.py holds them to the library's queries, the GPU children hold every case to what it claims.
"""

DTYPES = ("f16", "bf16")
EINVAL, ESHAPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4      # include/lip2speech_hip.h
GUARD = 3                                  # guard rows in front of and behind every output window
PADDED64, PHASE64, PHASE128 = 576064, 512064, 256128       # l2s_basicblock_variant
POOL = 7                                   # distinct images of a walk case: image i = pool[i % 7]

# ---- the child processes: name -> switches -------------------------------------------------------------------------------------------
SWITCHES = ("L2S_BASICBLOCK_PHASE", "L2S_STEM_FT")
# the parts of the matrix and their switches; a part that would take a child more than a few seconds is run once per type
PARTS = {
    "default": {},                         # the phase kernels and TAIL at small N, the padded kernel at maps other than 22 x 22
    "default-grid64": {},                  # phase CH = 64 around the 256-block grid (255, 256, 257 tiles)
    "default-grid128": {},                 # phase CH = 128 around it (511, 512, 513 images)
    "default-gridtail": {},                # TAIL around it
    "default-walk": {},                    # three tiles in one block
    "padded64": {"L2S_BASICBLOCK_PHASE": "0"},
    "stem": {},
    "stem-ft25": {"L2S_STEM_FT": "25"},
    "stem-ft1": {"L2S_STEM_FT": "1"},
    "stem-ft3": {"L2S_STEM_FT": "3"},
    "pools": {},
}
PER_TYPE = ("default-grid64", "default-grid128", "default-gridtail", "default-walk", "stem", "stem-ft25", "stem-ft1", "stem-ft3")
STEM_ENVS = ("stem", "stem-ft25", "stem-ft1", "stem-ft3")
ENVS = {}                                  # child -> switches
for _p, _sw in PARTS.items():
    for _name in ([f"{_p}-{_dt}" for _dt in DTYPES] if _p in PER_TYPE else [_p]):
        ENVS[_name] = _sw


def part_of(env):
    """(part, type or None) of a child."""
    for dt in DTYPES:
        if env.endswith("-" + dt) and env[: -len(dt) - 1] in PER_TYPE:
            return env[: -len(dt) - 1], dt
    return env, None


# ---- criterion (b): |got - ref| <= FU u max(|ref|, smallest normal) + F 2^-24 A -------------------------------------------------------
FU = 1.5
# worst |fp32 - fp64| / (2^-24 A) of the operation evaluated in torch fp32 on the CPU with the kernels' 16-bit intermediate roundings
# against the mirrored fp64 reference, over the cases of this file (`tools/check_frontend_kernels.py --cpu-f32`;
# profiles/frontend_matrix.md has the case behind each figure).  Kept per kernel class and type; the kernels get 8 times that,
# floored at 8 (tests/_vocconv_cases.py::F_of).
CPU_F32_WORST = {("bb64", "f16"): 500.143, ("bb64", "bf16"): 2324.122, ("bb64-layer", "f16"): 4885.322, ("bb64-layer", "bf16"): 30607.022,
                 ("bb128", "f16"): 446.590, ("bb128", "bf16"): 1537.107, ("tail", "f16"): 3002.826, ("tail", "bf16"): 18297.607,
                 ("stem-mono", "f16"): 977.173, ("stem-mono", "bf16"): 6564.392, ("stem-act", "f16"): 0.581, ("stem-act", "bf16"): 0.207,
                 ("stem-swish", "f16"): 0.324, ("stem-swish", "bf16"): 0.114, ("avgpool", "f16"): 0.0, ("avgpool", "bf16"): 0.0,
                 ("avgpool", "f32"): 6.294, ("preproc", "f16"): 0.0, ("preproc", "bf16"): 0.0, ("preproc", "f32"): 0.758}


def fkind(c):
    """The class of a case's figure."""
    if c["op"] == "bb":                                   # a launch of several blocks adds the flips of its 16-bit hand-overs, which reach the
        return ("bb64" if c["nb"] == 1 else "bb64-layer") if c["C"] == 64 else "bb128"    # result unweighted, as its residual
    if c["op"] in ("stem", "stem2"):
        return "stem-mono" if c["slopes"] in ("positive", "zero-and-one") else ("stem-swish" if c["slopes"] == "swish" else "stem-act")
    return c["op"]


def F_of(kind, dt):
    return max(8.0, 8.0 * CPU_F32_WORST[(kind, dt)])


def cdiv(a, b):
    return (a + b - 1) // b


# ---- csrc/basicblock.hip: bb_select, restated ------------------------------------------------------------------------------------------
BB_NP, BB_HALO, BB_MAXNB, BB_GRID = 576, 32, 4, 256


def phase_supports(C, H, W):
    return (C == 128 and H == 11 and W == 11) or (C == 64 and H == 22 and W == 22)


def basicblock_variant(N, H, W, C, nb, env, dtype_ok=True):
    """The code l2s_basicblock_variant answers for a 16-bit launch, or the error code."""
    if N <= 0 or H <= 0 or W <= 0 or nb <= 0:
        return ESHAPE
    phase64 = not env.get("L2S_BASICBLOCK_PHASE", "1").startswith("0")
    if C == 128 or (C == 64 and phase64 and phase_supports(C, H, W) and nb <= BB_MAXNB):
        if (C == 128 and nb != 1) or not phase_supports(C, H, W):
            return EUNSUPPORTED
        if N * H * W * C >= 2 ** 31:
            return EUNSUPPORTED
        if not dtype_ok:
            return EINVAL
        return PHASE128 if C == 128 else PHASE64
    if C != 64 or nb > BB_MAXNB:
        return EUNSUPPORTED
    if (H + 2) * (W + 2) > BB_NP or W + 3 > BB_HALO:
        return EUNSUPPORTED
    if N * H * W * 64 >= 2 ** 40:
        return EUNSUPPORTED
    return PADDED64 if dtype_ok else EINVAL


def images_per_tile(code):
    return 2 if code in (PHASE128, "tail") else 1


def tiles_per_block(ntiles):
    """Persistent blocks: grid = min(ntiles, 256), block b walks tiles b, b + grid, ...: the tiles of every block."""
    grid = min(ntiles, BB_GRID)
    return [list(range(b, ntiles, grid)) for b in range(grid)]


# ---- csrc/frontend.hip: stem_pool_frames and grid_for, restated ----------------------------------------------------------------------
GRID_CAP, GRID_BLOCK = 8192, 256


def stem_ft(B, T, env):
    ft = int(env.get("L2S_STEM_FT", "0"))
    return ft if ft > 0 else (25 if 6 * ((T + 24) // 25) * B >= 2048 else 10)


def grid_for(total, block=GRID_BLOCK):
    return max(1, min(GRID_CAP, cdiv(total, block)))


def takes_stride_loop(total):
    return total > GRID_CAP * GRID_BLOCK


# every instantiation the matrix must reach (some child, some case): (op, dt, code)
XKS = ("x16", "f32", "u8")


def instantiations():
    out = []
    for dt in DTYPES:
        out += [("bb", dt, code) for code in (PADDED64, PHASE64, PHASE128)]
        out += [("tail", dt, "tail")]
        out += [("stem", dt, ("stem_pool_kernel", xk, swish)) for xk in XKS for swish in (False, True)]
        out += [("stem2", dt, ("stem_kernel", xk, swish)) for xk in XKS[:2] for swish in (False, True)]
    for dt in DTYPES + ("f32",):
        out += [("maxpool", dt, "maxpool_kernel"), ("avgpool", dt, "avgpool_kernel"), ("preproc", dt, "preprocess_kernel")]
    return out


# ---- BasicBlocks ---------------------------------------------------------------------------------------------------------------------
BB_DATA = ("randn", "negative", "mixed-slope", "coded")
PADDED_MAPS = ((16, 29), (94, 4), (4, 29), (1, 1), (1, 29), (3, 5), (10, 10), (21, 21), (13, 22), (22, 13))
PADDED_REFUSED = ((17, 29), (5, 30), (23, 22), (95, 4))
LAYER_MAPS = ((22, 13), (5, 7))


def _bb(env, name, dt, N, H, W, C, nb, data, *, walk=False, expect=None):
    v = basicblock_variant(N, H, W, C, nb, PARTS[env])
    c = dict(op="bb", name=name, dt=dt, N=N, H=H, W=W, C=C, nb=nb, data=data, walk=walk, expect=min(v, 0), inst=("bb", dt, v))
    assert expect is None or c["expect"] == expect, (env, name, v)
    return c


def bb_cases(env):
    out = []
    for dt in DTYPES:
        if env == "default":
            i = 0
            for H, W in PADDED_MAPS:
                for N in (1, 2, 5):
                    out.append(_bb(env, f"padded/{H}x{W}-N{N}-{BB_DATA[i % 3]}", dt, N, H, W, 64, 1, BB_DATA[i % 3], expect=0))
                    i += 1
                out.append(_bb(env, f"padded/{H}x{W}-N2-coded", dt, 2, H, W, 64, 1, "coded", expect=0))
            for H, W in PADDED_REFUSED:
                out.append(_bb(env, f"padded/refused-{H}x{W}", dt, 2, H, W, 64, 1, "randn", expect=EUNSUPPORTED))
            for H, W in LAYER_MAPS:
                for nb in (2, 3, 4):
                    for data in ("randn", "mixed-slope", "coded"):
                        out.append(_bb(env, f"padded/{H}x{W}-nb{nb}-{data}", dt, 3, H, W, 64, nb, data, expect=0))
            out.append(_bb(env, "padded/refused-nb5", dt, 3, 22, 13, 64, 5, "randn", expect=EUNSUPPORTED))
            out.append(_bb(env, "phase64/refused-nb5", dt, 3, 22, 22, 64, 5, "randn", expect=EUNSUPPORTED))
            for N in (1, 2, 3):
                for nb in (1, 2, 3, 4):
                    out.append(_bb(env, f"phase64/N{N}-nb{nb}-{BB_DATA[i % 3]}", dt, N, 22, 22, 64, nb, BB_DATA[i % 3], expect=0))
                    i += 1
            for nb in (1, 2, 3, 4):
                out.append(_bb(env, f"phase64/N2-nb{nb}-coded", dt, 2, 22, 22, 64, nb, "coded", expect=0))
            for N in (1, 2, 3, 4, 5):
                for data in BB_DATA:
                    out.append(_bb(env, f"phase128/N{N}-{data}", dt, N, 11, 11, 128, 1, data, expect=0))
            out.append(_bb(env, "phase128/refused-nb2", dt, 2, 11, 11, 128, 2, "randn", expect=EUNSUPPORTED))
            out.append(_bb(env, "phase128/refused-10x10", dt, 2, 10, 10, 128, 1, "randn", expect=EUNSUPPORTED))
        elif env == "default-grid64":
            for N, nb, data in ((255, 1, "randn"), (256, 2, "negative"), (257, 1, "mixed-slope")):
                out.append(_bb(env, f"phase64/N{N}-nb{nb}-{data}", dt, N, 22, 22, 64, nb, data, expect=0))
        elif env == "default-grid128":
            for N, data in ((511, "randn"), (512, "negative"), (513, "mixed-slope")):
                out.append(_bb(env, f"phase128/N{N}-{data}", dt, N, 11, 11, 128, 1, data, expect=0))
        elif env == "default-walk":
            for N, nb, data in ((257, 1, "randn"), (513, 1, "randn"), (513, 2, "mixed-slope"), (513, 1, "coded"), (513, 3, "coded")):
                out.append(_bb(env, f"padded/walk-5x7-N{N}-nb{nb}-{data}", dt, N, 5, 7, 64, nb, data, walk=True, expect=0))
            for nb, data in ((1, "randn"), (2, "randn"), (1, "coded"), (2, "coded"), (1, "negative")):
                out.append(_bb(env, f"phase64/walk-N513-nb{nb}-{data}", dt, 513, 22, 22, 64, nb, data, walk=True, expect=0))
            for data in ("randn", "coded", "mixed-slope"):
                out.append(_bb(env, f"phase128/walk-N1025-{data}", dt, 1025, 11, 11, 128, 1, data, walk=True, expect=0))
        elif env == "padded64":
            for N in (1, 2, 5):
                for data in BB_DATA:
                    out.append(_bb(env, f"padded/22x22-N{N}-{data}", dt, N, 22, 22, 64, 1, data, expect=0))
            for nb in (2, 4):
                for data in ("randn", "coded"):
                    out.append(_bb(env, f"padded/22x22-nb{nb}-{data}", dt, 3, 22, 22, 64, nb, data, expect=0))
            out.append(_bb(env, "padded/walk-22x22-N513-randn", dt, 513, 22, 22, 64, 1, "randn", walk=True, expect=0))
    return out


def _tail(name, dt, N, data, *, walk=False, H=11, W=11, misalign=None):
    expect = EALIGN if misalign else (0 if phase_supports(128, H, W) else EUNSUPPORTED)
    return dict(op="tail", name=name, dt=dt, N=N, H=H, W=W, C=128, nb=1, data=data, walk=walk, misalign=misalign, expect=expect,
                inst=("tail", dt, "tail"))


def tail_cases(env):
    out = []
    for dt in DTYPES:
        if env == "default":
            for N in (1, 2, 3, 4, 5):
                for data in BB_DATA:
                    out.append(_tail(f"tail/N{N}-{data}", dt, N, data))
            out.append(_tail("tail/refused-10x10", dt, 2, "randn", H=10, W=10))
            for which in ("x0", "t0", "wa", "y", "b2"):
                out.append(_tail(f"tail/misaligned-{which}", dt, 2, "randn", misalign=which))
        elif env == "default-gridtail":
            for N, data in ((511, "randn"), (512, "negative"), (513, "mixed-slope")):
                out.append(_tail(f"tail/N{N}-{data}", dt, N, data))
        elif env == "default-walk":
            for data in ("randn", "coded", "negative"):
                out.append(_tail(f"tail/walk-N1025-{data}", dt, 1025, data, walk=True))
    return out


# ---- stem ----------------------------------------------------------------------------------------------------------------------------
STEM_T = (1, 2, 3, 4, 5, 9, 10, 11, 20, 21, 26)
STEM_SLOPES = ("positive", "mixed", "zero-and-one", "swish")
U8_HW = ((96, 96), (88, 88), (97, 120), (89, 91))


def _stem(name, dt, B, T, xk, slopes, data, env, *, hw=(96, 96), wset=0, pool=0):
    Hin, Win = hw if xk == "u8" else (88, 88)
    return dict(op="stem", name=name, dt=dt, B=B, T=T, xk=xk, Hin=Hin, Win=Win, slopes=slopes, data=data, wset=wset, pool=pool,
                expect=0, ft=stem_ft(B, T, PARTS[env]), inst=("stem", dt, ("stem_pool_kernel", xk, slopes == "swish")))


def stem_cases(env):
    """The same cases in every stem child: only `ft` differs."""
    out = []
    for dt in DTYPES:
        for i, T in enumerate(STEM_T):
            xk, sl, hw = XKS[i % 3], STEM_SLOPES[i % 4], U8_HW[i % 4]
            out.append(_stem(f"T{T}-{xk}-{sl}", dt, 2 + i % 2, T, xk, sl, "randn", env, hw=hw))
        j = 0
        for xk in XKS:                                    # every input kind with every activation, across a 10-frame chunk boundary
            for sl in STEM_SLOPES:
                out.append(_stem(f"T11-cross-{xk}-{sl}", dt, 2, 11, xk, sl, "randn", env, hw=U8_HW[j % 4]))
                j += 1
        for hw in U8_HW:
            out.append(_stem(f"T3-u8-{hw[0]}x{hw[1]}", dt, 2, 3, "u8", "mixed", "randn", env, hw=hw))
        for i, sl in enumerate(("positive", "mixed", "swish", "zero-and-one")):
            out.append(_stem(f"T5-negbias-{sl}", dt, 3, 5, XKS[i % 3], sl, "negbias", env, hw=(89, 91)))
        for s in range(4):                                # tap-coded: weight set s, slopes without Swish (not exact)
            out.append(_stem(f"T26-coded-set{s}", dt, 2, 26, XKS[s % 3], STEM_SLOPES[s % 3], "coded", env, wset=s, hw=(97, 120)))
        for B in (342, 341):                              # the launcher's own ft = 25 and the last B below it: clips from a pool of 3
            out.append(_stem(f"B{B}-T1-u8-pool3", dt, B, 1, "u8", "positive" if B == 342 else "mixed", "randn", env, hw=(96, 96), pool=3))
    return out


def stem2_cases():
    """l2s_stem_conv3d in 16 bits against fp64, then l2s_maxpool2d_3x3s2 of it against the fused kernel (2 ulp)."""
    out = []
    for dt in DTYPES:
        for T, xk, sl in ((1, "x16", "positive"), (5, "f32", "swish"), (11, "f32", "mixed"), (11, "x16", "swish"), (5, "x16", "mixed"),
                          (1, "f32", "zero-and-one")):
            out.append(dict(op="stem2", name=f"conv3d-T{T}-{xk}-{sl}", dt=dt, B=2, T=T, xk=xk, Hin=88, Win=88, slopes=sl, data="lowbias",
                            wset=0, pool=0, expect=0, inst=("stem2", dt, ("stem_kernel", xk, sl == "swish"))))
    return out


# ---- pools and preprocess --------------------------------------------------------------------------------------------------------------
MAXPOOL_SHAPES = ((44, 44, 64), (43, 44, 64), (1, 1, 8), (2, 3, 8), (5, 4, 72))
AVGPOOL_SHAPES = ((9, 512), (1, 512), (121, 128), (484, 8))


def pool_cases():
    out = []
    for dt in DTYPES + ("f32",):
        for i, (H, W, C) in enumerate(MAXPOOL_SHAPES):
            for data in ("randn", "negative"):
                out.append(dict(op="maxpool", name=f"maxpool/{H}x{W}x{C}-{data}", dt=dt, N=3, H=H, W=W, C=C, data=data, expect=0,
                                inst=("maxpool", dt, "maxpool_kernel")))
        out.append(dict(op="maxpool", name="maxpool/stride-loop-N542", dt=dt, N=542, H=44, W=44, C=64, data="negative", expect=0,
                        inst=("maxpool", dt, "maxpool_kernel")))
        out.append(dict(op="maxpool", name="maxpool/refused-C12", dt=dt, N=2, H=5, W=4, C=12, data="randn", expect=EALIGN,
                        inst=("maxpool", dt, "maxpool_kernel")))
        for HW, C in AVGPOOL_SHAPES:
            out.append(dict(op="avgpool", name=f"avgpool/{HW}x{C}", dt=dt, N=5, HW=HW, C=C, data="randn", expect=0,
                            inst=("avgpool", dt, "avgpool_kernel")))
        out.append(dict(op="avgpool", name="avgpool/stride-loop-N32769", dt=dt, N=32769, HW=1, C=512, data="randn", expect=0,
                        inst=("avgpool", dt, "avgpool_kernel")))
        for Hin, Win in U8_HW:
            out.append(dict(op="preproc", name=f"preproc/{Hin}x{Win}-crop88", dt=dt, B=2, T=3, Hin=Hin, Win=Win, crop=88, expect=0,
                            inst=("preproc", dt, "preprocess_kernel")))
        out.append(dict(op="preproc", name="preproc/97x120-crop61", dt=dt, B=2, T=3, Hin=97, Win=120, crop=61, expect=0,
                        inst=("preproc", dt, "preprocess_kernel")))
        out.append(dict(op="preproc", name="preproc/stride-loop-271-frames", dt=dt, B=1, T=271, Hin=89, Win=91, crop=88, expect=0,
                        inst=("preproc", dt, "preprocess_kernel")))
    return out


def items_of(c):
    """The grid-stride items of a pool / preprocess launch (csrc/frontend.hip)."""
    if c["op"] == "maxpool":
        return c["N"] * ((c["H"] - 1) // 2 + 1) * ((c["W"] - 1) // 2 + 1) * (c["C"] // 8)
    if c["op"] == "avgpool":
        return c["N"] * (c["C"] // 8)
    return c["B"] * c["T"] * c["crop"] * c["crop"]


# ---- the cases of a child -------------------------------------------------------------------------------------------------------------
def cases_of(env):
    part, dt = part_of(env)
    if part in STEM_ENVS:
        out = stem_cases(part) + (stem2_cases() if part == "stem" else [])
    elif part == "pools":
        out = pool_cases()
    else:
        out = bb_cases(part) + tail_cases(part)
    return [c for c in out if dt is None or c["dt"] == dt]
