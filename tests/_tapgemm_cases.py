"""Case generator of the tap-GEMM instantiation matrix (tools/check_tapgemm_matrix.py, tests/test_tapgemm_matrix_*.py).

Pure Python: no torch, no GPU, no library.  A case is a dict

    name, dt ("f16" | "bf16"), mode (0 LINEAR, 1 CONV1D, 2 CONV2D), uni (uniform-tap path of the conv modes),
    family (the epilogue family of csrc/tapgemm_tiles.h::pick_epilogue the case claims), geom, epi

`geom` describes the operands and the oracle op, `epi` the epilogue; `descriptors(case)` turns both into the integer fields of
l2s_gemm_desc (one dict per launch: a ConvTranspose1d case is one launch per output phase).  Shapes are functions of the forced
block tile (BM, BN), so that every tile sees interior full wave tiles and ragged edge tiles in one launch.
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


def g_conv2d(M, N, Cin, H, stride, **kw):
    """3 x 3, padding 1, on H x H maps; the launch computes the first M rows of the (image, y, x) space."""
    Ho = (H + 2 - 3) // stride + 1
    return _geom("conv2d", MODE_CONV2D, M, N, Cin, 9, H=H, Ho=Ho, stride=stride, nimg=cdiv(M, Ho * Ho), **kw)


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


def cases_of(part, tile):
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
        d.update(Ho=g["Ho"], Wo=g["Ho"], Hi=g["H"], Wi=g["H"], KW=3, pad=1, stride=g["stride"])
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
