"""Case generator of the tap-GEMM instantiation matrix (tools/check_tapgemm_matrix.py, tests/test_tapgemm_matrix_*.py).

Pure Python: no torch, no GPU, no library.  A case is a dict

    name, dt ("f16" | "bf16"), mode (0 LINEAR, 1 CONV1D, 2 CONV2D), uni (uniform-tap path of the conv modes),
    family (the epilogue family of csrc/tapgemm_tiles.h::pick_epilogue the case claims), geom, epi

`geom` describes the operands and the oracle op, `epi` the epilogue; `descriptors(case)` turns both into the integer fields of
l2s_gemm_desc (one dict per launch: a ConvTranspose1d case is one launch per output phase).  Shapes are functions of the forced
block tile (BM, BN), so that every tile sees interior full wave tiles and ragged edge tiles in one launch.

The parts of PART_ENV are the same for the two specialised kernels (phase-staggered 256 x 256, LDS patch): their cases also carry
`kernel` and `inst`, and the child process of a part runs under the switches PART_ENV names.
"""

# ---- constants of include/lip2speech_hip.h (tests/test_tapgemm_matrix_cpu.py checks them against the binding) -------------------
ACT_NONE, ACT_RELU, ACT_GELU, ACT_SWISH, ACT_PRELU, ACT_LRELU, ACT_TANH = range(7)
F_RES_PRE, F_RES_POST, F_ACCUM, F_DUAL, F_MASK, F_OUT_F32, F_RES_F32 = (1 << i for i in range(7))
MODE_LINEAR, MODE_CONV1D, MODE_CONV2D = range(3)
DTYPES = ("f16", "bf16")
LIN_ACTS = (ACT_NONE, ACT_RELU, ACT_PRELU, ACT_LRELU)        # held to the element-wise bound; the others to max-error only

# tile code -> (BM, BN, waves, ring stages): csrc/tapgemm_kernel.h::launch_mode_uni
TILES = {256128: (256, 128, 8, 3), 256064: (256, 64, 8, 3), 128128: (128, 128, 4, 2), 128064: (128, 64, 4, 3),
         64064: (64, 64, 4, 3), 128032: (128, 32, 4, 3), 128016: (128, 16, 4, 2)}
BK = 64
NCLIPS = 5                      # clips of the row mask: lens = T, 0, 1, T - 1, T
ALPHA, ACT_SLOPE, SLOPE2 = 0.5, 0.1, 0.2


def cdiv(a, b):
    return (a + b - 1) // b


def pick_epilogue(flags, act):
    """csrc/tapgemm_tiles.h::pick_epilogue, restated."""
    lin = act in LIN_ACTS
    if flags & ~F_MASK == 0:
        m = 1 if flags & F_MASK else 0
        if act == ACT_NONE:
            return 0 + m
        if lin:
            return 2 + m
        if act == ACT_GELU:
            return 4 + m
        return 9
    if flags & ~(F_RES_PRE | F_RES_POST) == 0 and lin:
        return 6
    if flags & ~(F_RES_PRE | F_RES_POST | F_DUAL | F_MASK) == 0 and lin:
        return 7
    if flags & ~(F_RES_PRE | F_RES_POST | F_OUT_F32 | F_RES_F32) == 0 and flags & F_OUT_F32 and lin:
        return 8
    return 9


# ---- persistent schedule of csrc/tapgemm_kernel.h, restated ---------------------------------------------------------------------
def blocks_per_cu(tile):
    BM, BN, waves, stages = TILES[tile]
    return min((160 * 1024) // (stages * (BM + BN) * BK * 2), 32 // waves)


def schedule(tile, M, N, groups=1):
    """(ntiles, chunk, slots, max my_n over the blocks) of launch_tile / tapgemm_kernel for this problem."""
    BM, BN = TILES[tile][:2]
    ntiles = cdiv(M, BM) * cdiv(N, BN) * groups
    chunk = cdiv(ntiles, 8)
    slots = min(chunk, 32 * blocks_per_cu(tile))
    worst = 0
    for x in range(8):
        lo = x * chunk
        hi = min(lo + chunk, ntiles)
        for slot in range(slots):
            if lo + slot < hi:
                worst = max(worst, (hi - lo - slot + slots - 1) // slots)
    return ntiles, chunk, slots, worst


# ---- epilogues ------------------------------------------------------------------------------------------------------------------
def epi(name, family, act=ACT_NONE, res=None, when=None, out32=False, dual=False, mask=False, accum=False, inplace=False,
        ldr_delta=0):
    """res: None | "16" | "32" (type of R); when: "pre" | "post" (side of the activation R is added on)."""
    flags = 0
    if res:
        flags |= F_RES_PRE if when == "pre" else F_RES_POST
        if res == "32":
            flags |= F_RES_F32
    flags |= (F_ACCUM if accum else 0) | (F_DUAL if dual else 0) | (F_MASK if mask else 0) | (F_OUT_F32 if out32 else 0)
    e = dict(name=name, family=family, act=act, res=res, when=when, out32=out32, dual=dual, mask=mask, accum=accum,
             inplace=inplace, ldr_delta=ldr_delta, flags=flags, alpha=ALPHA)
    assert pick_epilogue(flags, act) == family, (name, family, pick_epilogue(flags, act))
    return e


def family_epilogues():
    """At least one epilogue per family 0-9; every one carries a bias and alpha = 0.5."""
    E = [epi("none", 0), epi("none+mask", 1, mask=True)]
    for nm, a in (("relu", ACT_RELU), ("prelu", ACT_PRELU), ("lrelu", ACT_LRELU)):
        E += [epi(nm, 2, act=a), epi(nm + "+mask", 3, act=a, mask=True)]
    E += [epi("gelu", 4, act=ACT_GELU), epi("gelu+mask", 5, act=ACT_GELU, mask=True)]
    E += [epi("res16pre+relu", 6, act=ACT_RELU, res="16", when="pre"),
          epi("lrelu+res16post", 6, act=ACT_LRELU, res="16", when="post")]
    E += [epi("dual", 7, dual=True), epi("res16post+dual+mask", 7, res="16", when="post", dual=True, mask=True)]
    E += [epi("f32out+relu", 8, act=ACT_RELU, out32=True),
          epi("f32out+res32pre+prelu", 8, act=ACT_PRELU, res="32", when="pre", out32=True),
          epi("f32out+res16post", 8, res="16", when="post", out32=True),
          epi("stream32", 8, res="32", when="post", out32=True),
          epi("stream32-inplace", 8, res="32", when="post", out32=True, inplace=True),
          epi("stream32-ldr", 8, res="32", when="post", out32=True, ldr_delta=4)]   # ldr != ldc: epilogue_impl
    E += [epi("swish", 9, act=ACT_SWISH), epi("tanh", 9, act=ACT_TANH),
          epi("gelu+res32post+f32out", 9, act=ACT_GELU, res="32", when="post", out32=True),
          epi("accum16", 9, accum=True),
          epi("accum32+dual+mask", 9, accum=True, out32=True, dual=True, mask=True),
          epi("mask+f32out", 9, mask=True, out32=True)]
    return E


def _by_name(names):
    table = {e["name"]: e for e in family_epilogues()}
    return [table[n] for n in names]


# ---- geometries -----------------------------------------------------------------------------------------------------------------
def _geom(kind, mode, M, N, Cin, ntaps, **kw):
    g = dict(kind=kind, mode=mode, M=M, N=N, Cin=Cin, ntaps=ntaps, groups=1, a_gstride=0, c_gstride=0, lda_pad=0, ldc_pad=0,
             ldc2_pad=0, c2_skew=False)
    g.update(kw)
    G = g["groups"]
    g["a_cols"] = g["a_gstride"] * (G - 1) + Cin       # columns of A that hold data
    g["c_cols"] = g["c_gstride"] * (G - 1) + N         # columns of C the launch writes
    g["lda"] = g["a_cols"] + g["lda_pad"]
    g["ldc"] = g["c_cols"] + g["ldc_pad"]
    g["ldc2"] = g["c_cols"] + g["ldc2_pad"]
    g["uni"] = mode != MODE_LINEAR and Cin % BK == 0
    g["mask_T"] = cdiv(M * g.get("out_row_mul", 1), NCLIPS)
    return g


def g_linear(M, N, K, **kw):
    return _geom("linear", MODE_LINEAR, M, N, K, 1, **kw)


def g_conv1d(M, N, Cin, k, dil, **kw):
    """NCLIPS clips of T = ceil(M / NCLIPS) frames, 'same' padding; the launch computes the first M rows."""
    B = kw.pop("B", NCLIPS)
    T = cdiv(M, B)
    return _geom("conv1d", MODE_CONV1D, M, N, Cin, k, k=k, dil=dil, off=-((k - 1) * dil // 2), B=B, T=T, **kw)


def g_conv2d(M, N, Cin, H, stride, W=None, **kw):
    """3 x 3, padding 1, on H x H maps (H x W where W is given); the launch computes the first M rows of the (image, y, x) space."""
    Ho = (H + 2 - 3) // stride + 1
    if W is None:
        return _geom("conv2d", MODE_CONV2D, M, N, Cin, 9, H=H, Ho=Ho, stride=stride, nimg=cdiv(M, Ho * Ho), **kw)
    Wo = (W + 2 - 3) // stride + 1
    return _geom("conv2d", MODE_CONV2D, M, N, Cin, 9, H=H, Ho=Ho, Wi=W, Wo=Wo, stride=stride, nimg=cdiv(M, Ho * Wo), **kw)


def g_convt(B, L, N, Cin, k=8, s=4, **kw):
    """ConvTranspose1d(k, stride s, padding (k - s) / 2) as s CONV1D phases (packing.convtranspose_phases)."""
    p = (k - s) // 2
    phases = []
    for r in range(s):
        k0 = (r + p) % s
        phases.append(dict(r=r, off=(r + p - k0) // s, ntaps=len(range(k0, k, s))))
    return _geom("convt", MODE_CONV1D, B * L, N, Cin, phases[0]["ntaps"], B=B, T=L, k=k, s=s, p=p, phases=phases,
                 out_row_mul=s, **kw)


def base_geometries(BM, BN):
    """The five (mode, tap path) geometries of the family cases at M = 2 BM + 37, N = 2 BN + 20."""
    M, N = 2 * BM + 37, 2 * BN + 20
    return [("linear", g_linear(M, N, 72)),                       # nk = 2 with a K tail
            ("conv1d-uni", g_conv1d(M, N, 64, 3, 1)),
            ("conv1d-lane", g_conv1d(M, N, 24, 5, 3)),            # Ktot = 120: K tail
            ("conv2d-uni", g_conv2d(M, N, 64, 7, 1)),
            ("conv2d-lane", g_conv2d(M, N, 40, 13, 2))]           # stride 2 on an odd map, Ktot = 360: K tail


def addressing_geometries(BM, BN):
    """(name, geometry, epilogue names) of the addressing cases, on LINEAR and CONV1D."""
    M, N = 2 * BM + 37, 2 * BN + 20
    out = []

    def both(name, names, lin_kw, conv_kw=None, M=M, N=N, K=72, Cin=24, B=NCLIPS):
        conv_kw = lin_kw if conv_kw is None else conv_kw
        out.append((name + "/linear", g_linear(M, N, K, **lin_kw), names))
        out.append((name + "/conv1d", g_conv1d(M, N, Cin, 3, 2, B=B, **conv_kw), names))

    # lda > Cin, ldc > N with ldc % 8 == 4 (N % 8 == 4): no row of C but the first is 16-byte aligned
    both("lda+ldc", ["none", "lrelu+res16post", "f32out+res16post", "accum16"], dict(lda_pad=16, ldc_pad=8))
    # ldc2 != ldc, and C2 itself only 8-byte aligned
    both("ldc2", ["dual", "res16post+dual+mask", "accum32+dual+mask"], dict(ldc_pad=4, ldc2_pad=8, c2_skew=True))
    # grouped: whole 16-byte groups per group, then groups whose columns start at 24-byte offsets
    grp_epi = ["none", "prelu+mask", "lrelu+res16post", "dual", "f32out+res32pre+prelu", "stream32", "accum16"]
    both("groups3-n16", grp_epi, dict(groups=3, a_gstride=16, c_gstride=16), N=16, K=16, Cin=16)
    both("groups3-n12", grp_epi, dict(groups=3, a_gstride=16, c_gstride=12), N=12, K=16, Cin=16)
    for n in (4, 12, 16):
        both(f"N{n}", ["none", "relu+mask", "dual", "f32out+relu", "accum16"], {}, N=n)
    # N % 8 == 0 at full width: the wave-uniform 16-byte store path across several wave tiles
    both("N8", ["none", "lrelu+mask", "lrelu+res16post", "res16post+dual+mask", "accum16"], {}, N=N + 4)
    for m in (1, 7):
        both(f"M{m}", ["none", "gelu", "res16pre+relu", "stream32", "mask+f32out"], {}, M=m, B=1)
    # ConvTranspose1d k = 8, s = 4: negative dilation, out_row_mul = 4; 16-bit C and the fp32 residual stream
    L = cdiv(M, 3)
    for cin in (64, 24):
        out.append((f"convt-c{cin}/conv1d", g_convt(3, L, N, cin), ["none", "res16post+dual+mask", "stream32", "stream32-inplace"]))
    return out


def family_cases(tile):
    BM, BN = TILES[tile][:2]
    cases = []
    for dt in DTYPES:
        for gname, g in base_geometries(BM, BN):
            for e in family_epilogues():
                cases.append(dict(name=f"{gname}/{e['name']}", dt=dt, mode=g["mode"], uni=g["uni"], family=e["family"],
                                  geom=g, epi=e))
        for gname, g, names in addressing_geometries(BM, BN):
            for e in _by_name(names):
                cases.append(dict(name=f"{gname}/{e['name']}", dt=dt, mode=g["mode"], uni=g["uni"], family=e["family"],
                                  geom=g, epi=e))
    return cases


def schedule_shape(tile):
    """Smallest (tilesM, tilesN) with more than 2 * 8 * 32 * BPC tiles, a tile count that is no multiple of 8 and the aspect
    closest to square in elements; M and N are ragged."""
    BM, BN = TILES[tile][:2]
    need = 2 * 8 * 32 * blocks_per_cu(tile)
    n = need + 1
    while True:
        if n % 8:
            pairs = [(tm, n // tm) for tm in range(3, n // 3 + 1) if n % tm == 0]
            pairs = [(tm, tn) for tm, tn in pairs if tm * BM >= tn * BN and tm * BM <= 8 * tn * BN]
            if pairs:
                tm, tn = min(pairs, key=lambda q: q[0] * BM / (q[1] * BN))
                return (tm - 1) * BM + 37, tn * BN - 4, tm, tn
        n += 1


def schedule_cases(tile):
    """LINEAR, families 0 and 8, some block walking at least three output tiles, at nk = 1, nk = 2 and with a K tail."""
    M, N, tm, tn = schedule_shape(tile)
    ntiles, chunk, slots, my_n = schedule(tile, M, N)
    assert ntiles == tm * tn and ntiles % 8 and ntiles > 2 * 8 * 32 * blocks_per_cu(tile) and M % TILES[tile][0]
    assert my_n >= 3, (tile, ntiles, chunk, slots, my_n)
    cases = []
    for dt in DTYPES:
        for K in (64, 128, 200):
            g = g_linear(M, N, K)
            for e in _by_name(["none", "stream32"]):
                cases.append(dict(name=f"walk-K{K}/{e['name']}", dt=dt, mode=g["mode"], uni=False, family=e["family"], geom=g,
                                  epi=e))
    return cases


BAND_TILE, BAND = 128064, 3


def band_cases():
    """Tile 128 x 64 under L2S_BAND=3 with tilesM = 7, tilesN = 3: the last band of tile_coords is one tile tall."""
    BM, BN = TILES[BAND_TILE][:2]
    M, N = 6 * BM + 37, 2 * BN + 20
    assert cdiv(M, BM) == 7 and cdiv(N, BN) == 3 and cdiv(M, BM) % BAND
    cases = []
    for dt in DTYPES:
        for gname, g in (("linear", g_linear(M, N, 200)), ("conv1d-lane", g_conv1d(M, N, 24, 5, 3))):
            for e in _by_name(["none", "lrelu+mask", "stream32"]):
                cases.append(dict(name=f"band/{gname}/{e['name']}", dt=dt, mode=g["mode"], uni=g["uni"], family=e["family"],
                                  geom=g, epi=e))
    return cases


# ---- the two specialised kernels: phase-staggered 256 x 256 (csrc/phasegemm_kernel.h) and LDS patch (csrc/patchconv.hip) ------------
# A case of these parts also carries `kernel` (what l2s_tapgemm_variant must answer) and `inst`, the instantiation it claims:
# (dt, mode, EPI) of phasegemm_kernel, (dt, mode, CH, EPI) of patchconv64_kernel.
PHASE, PATCH64, PATCH128 = 256256, 999064, 999128
EPI_G16A, EPI_G16B, EPI_S32, EPI_ALL, EPI_X32 = 6, 7, 8, 9, 10
PHASE_EPIS = (0, 1, 2, 3, 4, 5, EPI_G16A, EPI_G16B, EPI_S32, EPI_X32)      # launch_phase_mode
PATCH_EPIS = (2, 3, EPI_G16A, EPI_G16B, EPI_ALL)                           # launch_patch_epi
PHASE_SLOTS, PATCH_SLOTS = 2, 4                                            # the slot caps of the walk parts
# every switch a part's child process depends on: those named here are set to these values, the others are unset
SWITCHES = ("L2S_FORCE_TILE", "L2S_BAND", "L2S_PHASEGEMM", "L2S_PHASEGEMM_RES", "L2S_PHASE_SLOTS", "L2S_NO_PATCHCONV",
            "L2S_PATCH128", "L2S_PATCH_SLOTS", "L2S_PATCH_MIN_M")
_PH, _PA = dict(L2S_PHASEGEMM="2"), dict(L2S_PATCH_MIN_M="1", L2S_PHASEGEMM="0")
PART_ENV = {"phase-families": _PH, "phase-walk": dict(_PH, L2S_PHASE_SLOTS=str(PHASE_SLOTS)), "phase-natural": _PH,
            "patch-families": _PA, "patch-walk": dict(_PA, L2S_PATCH_SLOTS=str(PATCH_SLOTS)), "patch-natural": _PA}
PART_KERNELS = {"phase-families": (PHASE,), "phase-walk": (PHASE,), "phase-natural": (PHASE,),
                "patch-families": (PATCH64, PATCH128), "patch-walk": (PATCH64, PATCH128), "patch-natural": (PATCH64,)}


def is_x32(flags, act):
    """csrc/tapgemm_tiles.h::is_x32, restated."""
    need, may = F_RES_POST | F_OUT_F32, F_ACCUM | F_DUAL | F_MASK
    return act == ACT_NONE and flags & need == need and flags & ~(need | may) == 0


def x32_epilogues():
    """The ResBlock-sum update of the phase kernel: fp32 out + 16-bit residual after no activation; pick_epilogue family 9."""
    kw = dict(res="16", when="post", out32=True)
    E = [epi("x32+mask", 9, mask=True, **kw), epi("x32+accum", 9, accum=True, **kw),
         epi("x32+accum+dual+mask", 9, accum=True, dual=True, mask=True, **kw), epi("x32+dual", 9, dual=True, **kw)]
    assert all(is_x32(e["flags"], e["act"]) for e in E)
    return E


def _named(names):
    table = {e["name"]: e for e in family_epilogues() + x32_epilogues()}
    return [table[n] for n in names]


def phase_epi(e, N=0):
    """EPI of the phasegemm_kernel instantiation launch_phase_mode picks, None where l2s_phasegemm_eligible declines: family 9
    but for X32, and families 0-6 (whole 8-channel groups stored from the MFMA layout) at N % 8 != 0."""
    if e["family"] <= EPI_G16A:
        return e["family"] if N % 8 == 0 else None
    if e["family"] < EPI_ALL:
        return e["family"]
    return EPI_X32 if is_x32(e["flags"], e["act"]) else None


def patch_epi(e):
    return {0: 2, 1: 3, 2: 2, 3: 3, EPI_G16A: EPI_G16A, EPI_G16B: EPI_G16B}.get(e["family"], EPI_ALL)


def phase_band(M, N, Cin, ntaps):
    """launch_phase's band height (the operand-footprint minimum over b = 1 .. tilesM, first minimum wins), restated."""
    tilesM, tilesN = cdiv(M, 256), cdiv(N, 256)
    chunk = cdiv(tilesM * tilesN, 8)
    ap, wp = 256.0 * Cin * 2.0, 256.0 * Cin * ntaps * 2.0
    band, best = 1, 1e300
    for b in range(1, tilesM + 1):
        wn = min(cdiv(chunk, b), tilesN)
        an = b * cdiv(chunk, b * tilesN)
        fp = ap * min(an, tilesM) + wp * wn
        if fp < best:
            best, band = fp, b
    return band


def phase_schedule(M, N, slots_cap=32):
    """(ntiles, chunk, slots, my_n of every block [xcd][slot]) of launch_phase / phasegemm_kernel."""
    ntiles = cdiv(M, 256) * cdiv(N, 256)
    chunk = cdiv(ntiles, 8)
    slots = min(chunk, slots_cap)
    my_n = []
    for x in range(8):
        lo = x * chunk
        hi = min(lo + chunk, ntiles)
        my_n.append([(hi - lo - s + slots - 1) // slots if lo + s < hi else 0 for s in range(slots)])
    return ntiles, chunk, slots, my_n


def patch_schedule(g, ch, slots_cap=None):
    """(ntiles, grid, tiles of every block) of launch_patch / patchconv64_kernel; a CONV1D tile is (clip, first frame), a CONV2D
    tile the first padded-flattened position."""
    if g["mode"] == MODE_CONV1D:
        per_clip = cdiv(g["T"], 256)
        ntiles = (g["M"] // g["T"]) * per_clip
        tile = lambda L: (L // per_clip, (L % per_clip) * 256)
    else:
        H, W = g["H"], g.get("Wi", g["H"])
        ntiles = cdiv((g["M"] // (H * W)) * (H + 2) * (W + 2), 256)
        tile = lambda L: L * 256
    resident = 512 if ch == 64 else 256
    grid = min(ntiles, slots_cap if slots_cap and 1 <= slots_cap < resident else resident)
    return ntiles, grid, [[tile(L) for L in range(b, ntiles, grid)] for b in range(grid)]


def patch_eligible(d):
    """l2s_patchconv_eligible without its measured-speed row threshold: the conditions that are about correctness."""
    if not ((d["Cin"], d["N"]) in ((64, 64), (128, 128)) and d["groups"] == 1):
        return False
    if d["mode"] == MODE_CONV1D:
        if d["stride"] != 1 or d["T_out"] != d["T_in"] or d["ntaps"] < 2 or d["M"] % d["T_out"]:
            return False
        a, b = d["off"], (d["ntaps"] - 1) * d["dil"] + d["off"]
        return max(a, b) - min(a, b) <= 64 and min(a, b) <= 0 <= max(a, b)
    if d["mode"] == MODE_CONV2D:
        if d["stride"] != 1 or d["KW"] != 3 or d["ntaps"] != 9 or d["pad"] != 1 or d["Ho"] != d["Hi"] or d["Wo"] != d["Wi"]:
            return False
        if d["M"] % (d["Hi"] * d["Wi"]) or 4 * (d["Hi"] + 2) * (d["Wi"] + 2) > 5 * d["Hi"] * d["Wi"]:
            return False
        return 2 * (d["Wi"] + 3) <= 64
    return False


def _case(name, dt, g, e, kernel, ch=None):
    ep = phase_epi(e, g["N"]) if kernel == PHASE else patch_epi(e)
    assert ep is not None, (name, e["name"])
    inst = (dt, g["mode"], ep) if kernel == PHASE else (dt, g["mode"], ch, ep)
    return dict(name=f"{name}/{e['name']}", dt=dt, mode=g["mode"], uni=g["uni"], family=e["family"], geom=g, epi=e,
                kernel=kernel, inst=inst)


def _phase_conv_geoms(M, N4, N8, B):
    """The conv-mode geometries of the phase parts at N4 (N % 8 == 4: families 7, 8 and X32) and at N8 (N % 8 == 0: every family)."""
    out = []
    for n in dict.fromkeys((N4, N8)):
        sfx = f"-n{n}"
        out += [("conv1d-k3" + sfx, g_conv1d(M, n, 64, 3, 1)), ("conv1d-c128-k5d3" + sfx, g_conv1d(M, n, 128, 5, 3)),
                ("conv2d-7x7" + sfx, g_conv2d(M, n, 64, 7, 1)), ("conv2d-13x13s2" + sfx, g_conv2d(M, n, 64, 13, 2)),
                ("convt-k8s4" + sfx, g_convt(B, M // B, n, 64, 8, 4)), ("convt-k11s5" + sfx, g_convt(B, M // B, n, 64, 11, 5))]
    return out


def phase_family_cases():
    """Every (type, mode, EPI) of phasegemm_kernel on 3 x 3 ragged tiles: nk = 1 and odd nk, N % 8 == 4 in the conv modes, both
    ConvTranspose1d phase shapes (negative dilation, out_row_mul), and the leading-dimension cases."""
    M, N = 2 * 256 + 37, 2 * 256 + 20                   # conv modes: N % 8 == 4
    ML, NL = M + 3, N + 4                               # LINEAR: whole 8-row / 8-column staging groups
    geoms = [("linear-K64", g_linear(ML, NL, 64)), ("linear-K192", g_linear(ML, NL, 192))]
    geoms += _phase_conv_geoms(M, N, NL, 3)
    assert M % 3 == 0 and (ML, NL) == (552, 536) and (M, N) == (549, 532)
    epis = [e for e in family_epilogues() if phase_epi(e) is not None] + x32_epilogues()
    addr = []
    for gname, mk in (("linear", lambda **kw: g_linear(ML, NL, 192, **kw)), ("conv1d", lambda **kw: g_conv1d(M, NL, 64, 3, 1, **kw)),
                      ("conv1d-n532", lambda **kw: g_conv1d(M, N, 64, 3, 1, **kw))):
        n = N if gname == "conv1d-n532" else NL
        pad4 = 4 if n % 8 == 0 else 8                   # ldc % 8 == 4: no row of C but the first is 16-byte aligned
        addr.append((f"lda+ldc/{gname}", mk(lda_pad=16, ldc_pad=pad4),
                     ["none", "gelu+mask", "lrelu+res16post", "f32out+res16post", "x32+accum"]))
        addr.append((f"ldc2/{gname}", mk(ldc_pad=pad4 + 4, ldc2_pad=pad4 + 8, c2_skew=True),      # ldc2 % 8 == 4, C2 8-byte aligned
                     ["dual", "res16post+dual+mask", "x32+accum+dual+mask"]))
        addr.append((f"ldr/{gname}", mk(lda_pad=8, ldc_pad=pad4), ["stream32-ldr", "stream32-inplace"]))
    cases = []
    for dt in DTYPES:
        for gname, g in geoms:
            cases += [_case(gname, dt, g, e, PHASE) for e in epis if phase_epi(e, g["N"]) is not None]
        for gname, g, names in addr:
            assert (g["ldc2"] % 8 == 4 and g["ldc2"] != g["ldc"]) if g["c2_skew"] else g["ldc"] % 8 == 4
            cases += [_case(gname, dt, g, e, PHASE) for e in _named(names) if phase_epi(e, g["N"]) is not None]
    return cases


def phase_declined_cases():
    """The conv-mode launches with N % 8 == 4 and a family 0-6 epilogue: l2s_phasegemm_eligible must decline them even when forced
    (epilogue_direct16 would leave their last four columns unwritten); the generic tiles serve them."""
    M, N = 2 * 256 + 37, 2 * 256 + 20
    return [dict(name=f"{gname}/{e['name']}", dt=dt, mode=g["mode"], uni=g["uni"], family=e["family"], geom=g, epi=e)
            for dt in DTYPES for gname, g in _phase_conv_geoms(M, N, N, 3) for e in family_epilogues() if e["family"] <= EPI_G16A]


WALK_EPIS = ["none", "lrelu+mask", "gelu+mask", "lrelu+res16post", "res16post+dual+mask", "stream32", "x32+accum+dual+mask"]


def phase_walk_cases():
    """7 x 7 tiles under L2S_PHASE_SLOTS=2: slot 0 of XCDs 0-6 walks four tiles, slot 1 three, XCD 7 has none.  The quarter stream,
    the K-tile parity (odd nk), the accumulators and the conv modes' tap cursor all cross tile boundaries."""
    ML, NL, M, N = 6 * 256 + 40, 7 * 256 - 8, 6 * 256 + 37, 7 * 256 - 4
    assert (ML, NL, M, N) == (1576, 1784, 1573, 1788) and M == 11 * 143
    geoms = [(f"linear-K{K}", g_linear(ML, NL, K)) for K in (64, 128, 192)]
    for n in (N, NL):                                   # N % 8 == 4: families 7, 8 and X32; N % 8 == 0: 0, 3, 5 and 6
        geoms += [(f"conv1d-k3-n{n}", g_conv1d(M, n, 64, 3, 1)), (f"conv2d-7x7-n{n}", g_conv2d(M, n, 64, 7, 1)),
                  (f"convt-k8s4-n{n}", g_convt(11, 143, n, 64, 8, 4))]
    return [_case("walk/" + gname, dt, g, e, PHASE) for dt in DTYPES for gname, g in geoms for e in _named(WALK_EPIS)
            if phase_epi(e, g["N"]) is not None and (g["mode"] == MODE_LINEAR or (g["N"] == N) == (e["family"] > EPI_G16A))]


def phase_natural_cases():
    """19 x 14 = 266 tiles on the real grid of 8 x 32 blocks: chunk 34, so slots 0 and 1 of XCDs 0-6 walk two tiles."""
    M, N = 18 * 256 + 40, 14 * 256 - 8
    assert (M, N) == (4648, 3576)
    return [_case(f"natural/linear-K{K}", dt, g_linear(M, N, K), e, PHASE) for dt in DTYPES for K in (64, 192)
            for e in _named(["none", "stream32"])]


def _patch_conv1d(ch, T, k, dil, B=NCLIPS, **kw):
    return g_conv1d(B * T, ch, ch, k, dil, B=B, **kw)


def _patch_conv2d(ch, H, W, nimg, **kw):
    return g_conv2d(nimg * H * W, ch, ch, H, 1, W=W, **kw)


def patch_family_cases(ch):
    """Every (type, mode, EPI) of patchconv64_kernel<CH> on whole clips / whole images, one to three tiles per clip."""
    geoms = [("conv1d-k3-T549", _patch_conv1d(ch, 549, 3, 1)),          # three tiles per clip, the last one 37 rows
             ("conv1d-k11d5-T549", _patch_conv1d(ch, 549, 11, 5)),
             ("conv1d-k9d8-T300", _patch_conv1d(ch, 300, 9, 8)),        # tap span 64 = the halo limit
             ("conv1d-k2-T256", _patch_conv1d(ch, 256, 2, 1)),          # ntaps == 2 (offsets 0, +1), T_out == one tile exactly
             ("conv1d-k7d3-T100", _patch_conv1d(ch, 100, 7, 3)),        # T_out < 256
             ("conv1d-k3-T7", _patch_conv1d(ch, 7, 3, 1)),
             ("convt-k8s4", g_convt(NCLIPS, 300, ch, ch, 8, 4)),        # dil -1, out_row_mul 4
             ("conv2d-18x18", _patch_conv2d(ch, 18, 18, 3)),
             ("conv2d-16x29", _patch_conv2d(ch, 16, 29, 3)),            # Wi = 29: the widest map the halo admits
             ("conv2d-40x12", _patch_conv2d(ch, 40, 12, 3))]
    pads = [("lda+ldc/conv1d", _patch_conv1d(ch, 549, 3, 1, lda_pad=16, ldc_pad=12)),
            ("lda+ldc/conv2d", _patch_conv2d(ch, 16, 29, 3, lda_pad=16, ldc_pad=12))]
    pad_epis = _named(["none", "lrelu+mask", "lrelu+res16post", "res16post+dual+mask", "f32out+res16post", "accum16"])
    kernel = 999000 + ch
    cases = []
    for dt in DTYPES:
        for gname, g in geoms:
            cases += [_case(gname, dt, g, e, kernel, ch) for e in family_epilogues()]
        for gname, g in pads:
            assert g["ldc"] % 8 == 4
            cases += [_case(gname, dt, g, e, kernel, ch) for e in pad_epis]
    return cases


PATCH_WALK_EPIS = ["relu", "prelu+mask", "res16pre+relu", "res16post+dual+mask",      # paired: next patch issued in the epilogue
                   "gelu+mask", "stream32", "accum32+dual+mask"]                       # catch-all: barrier, then the next patch


def patch_walk_cases(ch):
    """15 tiles under L2S_PATCH_SLOTS=4: blocks walk 4 / 4 / 4 / 3 tiles, consecutive tiles of a block lie in different clips."""
    geoms = [("conv1d-k3-T700", _patch_conv1d(ch, 700, 3, 1)), ("conv2d-18x18", _patch_conv2d(ch, 18, 18, 9))]
    return [_case("walk/" + gname, dt, g, e, 999000 + ch, ch) for dt in DTYPES for gname, g in geoms
            for e in _named(PATCH_WALK_EPIS)]


def patch_natural_cases():
    """More tiles than the 512 resident blocks of the 64-channel kernel: blocks 0-9 / 0-5 take a second tile."""
    geoms = [("conv1d-k11d5-T14600", _patch_conv1d(64, 14600, 11, 5, B=9), "res16post+dual+mask"),
             ("conv2d-22x22", _patch_conv2d(64, 22, 22, 230), "res16pre+relu")]
    return [_case("natural/" + gname, dt, g, _named([en])[0], PATCH64, 64) for dt in DTYPES for gname, g, en in geoms]


def special_cases(part, kernel):
    if part == "phase-families":
        return phase_family_cases()
    if part == "phase-walk":
        return phase_walk_cases()
    if part == "phase-natural":
        return phase_natural_cases()
    ch = kernel - 999000
    if part == "patch-families":
        return patch_family_cases(ch)
    if part == "patch-walk":
        return patch_walk_cases(ch)
    if part == "patch-natural":
        return patch_natural_cases()
    raise ValueError(part)


def cases_of(part, tile):
    if part in PART_ENV:
        assert tile in PART_KERNELS[part], (part, tile)
        return special_cases(part, tile)
    if part == "families":
        return family_cases(tile)
    if part == "schedule":
        return schedule_cases(tile)
    if part == "band":
        assert tile == BAND_TILE
        return band_cases()
    raise ValueError(part)


# ---- descriptors ----------------------------------------------------------------------------------------------------------------
def descriptors(case):
    """Integer / float fields of l2s_gemm_desc for every launch of the case (pointers excluded)."""
    g, e = case["geom"], case["epi"]
    d = dict(M=g["M"], N=g["N"], Cin=g["Cin"], ntaps=g["ntaps"], lda=g["lda"], ldc=g["ldc"], ldc2=g["ldc2"],
             ldr=g["ldc"] + e["ldr_delta"], mode=g["mode"], act=e["act"], flags=e["flags"], dtype=DTYPES.index(case["dt"]),
             alpha=e["alpha"], act_slope=ACT_SLOPE if e["act"] == ACT_LRELU else 0.0, slope2=SLOPE2 if e["dual"] else 0.0,
             groups=g["groups"], a_gstride=g["a_gstride"], c_gstride=g["c_gstride"], w_gstride=g["N"] * g["Cin"] * g["ntaps"],
             out_row_mul=g.get("out_row_mul", 1), out_row_add=0)
    if e["mask"]:
        d.update(mask_T=g["mask_T"], mask_mul=1)
    if g["kind"] == "conv1d":
        d.update(T_out=g["T"], T_in=g["T"], stride=1, dil=g["dil"], off=g["off"])
    elif g["kind"] == "conv2d":
        d.update(Ho=g["Ho"], Wo=g.get("Wo", g["Ho"]), Hi=g["H"], Wi=g.get("Wi", g["H"]), KW=3, pad=1, stride=g["stride"])
    elif g["kind"] == "convt":
        return [dict(d, T_out=g["T"], T_in=g["T"], stride=1, dil=-1, off=ph["off"], ntaps=ph["ntaps"], out_row_add=ph["r"],
                     w_gstride=0) for ph in g["phases"]]
    return [d]


def mask_lens(case):
    T = case["geom"]["mask_T"]
    return [T, 0, 1, T - 1, T]


def alignment_ok(d):
    """The descriptor rules of l2s_tapgemm (csrc/tapgemm.hip) that do not involve pointers."""
    if d["M"] <= 0 or d["N"] <= 0 or d["Cin"] <= 0 or d["ntaps"] <= 0:
        return False
    if d["Cin"] & 7 or d["lda"] & 7 or d["N"] & 3 or d["ldc"] & 3 or d["a_gstride"] & 7 or d["c_gstride"] & 3 or d["w_gstride"] & 7:
        return False
    if d["flags"] & (F_RES_PRE | F_RES_POST) and d["ldr"] & 3:
        return False
    if d["flags"] & F_DUAL and d["ldc2"] & 3:
        return False
    if d["flags"] & F_MASK and (d.get("mask_T", 0) <= 0 or d.get("mask_mul", 0) <= 0):
        return False
    if d["mode"] == MODE_CONV1D and (d.get("T_out", 0) <= 0 or d.get("T_in", 0) <= 0):
        return False
    if d["mode"] == MODE_CONV2D and min(d.get(k, 0) for k in ("Ho", "Wo", "Hi", "Wi", "KW")) <= 0:
        return False
    if d["mode"] != MODE_LINEAR and d["Cin"] * d["ntaps"] > 1 << 15:
        return False
    return d["M"] * d["out_row_mul"] + d["out_row_add"] < 1 << 31
