"""Case generator of the sequence-kernel matrix (tools/check_seq_kernels.py, tests/test_seq_matrix_*.py): l2s_attention,
l2s_layernorm, l2s_splitk_reduce_layernorm and l2s_glu_dwconv_swish, every instantiation of their kernels.

Pure Python: no torch, no GPU, no library.  A case is a dict with `op` ("attn" | "ln" | "skln" | "glu"), `name`, `dt`
("f16" | "bf16"), the shapes and leading dimensions of the launch, and `inst`, the kernel instantiation the case claims to run on
under the environment of its child process (ENVS): the launchers read their switches once per process.  The three selection
rules of the launchers are restated here (attention_variant, layernorm_variant, glu_tile); tests/test_seq_matrix_cpu.py holds
the restatement to the library's host-only queries, the GPU child holds every case to the instantiation it claims.
"""

DTYPES = ("f16", "bf16")
D = 64                                     # head dimension
# include/lip2speech_hip.h (tests/test_seq_matrix_cpu.py checks them against the binding)
SEQ_VARIANT_F32, LN_GENERIC, ATTN_RESIDENT = 2000, 10, 1000
EALIGN = -3

# ---- the child processes: name -> (switches, parts run under them) ----------------------------------------------------------------
SWITCHES = ("L2S_ATTN_RESIDENT", "L2S_ATTN_RESIDENT_PLAIN", "L2S_ATTN_QB", "L2S_LN_ROWS")
ENVS = {
    "default": {},
    "ln-rows-off": {"L2S_LN_ROWS": "0"},
    "resident-off": {"L2S_ATTN_RESIDENT": "0"},
    "resident-plain": {"L2S_ATTN_RESIDENT_PLAIN": "1"},
    # a forced query-block size counts on the tiled kernels only: the resident one is switched off to reach them at T <= 208
    "qb64": {"L2S_ATTN_QB": "64", "L2S_ATTN_RESIDENT": "0"},
    "qb128": {"L2S_ATTN_QB": "128", "L2S_ATTN_RESIDENT": "0"},
}

# ---- criterion (b): |got - ref| <= FU u |ref| [16-bit output] + FU u A [attention] + F 2^-24 A ------------------------------------
FU = 1.5                                   # the project's margin over the half-ulp bound (tools/check_tapgemm_matrix.py)
# worst |fp32 - fp64| / (2^-24 A) of the operation evaluated in torch fp32 on the CPU over the cases of this file
# (`tools/check_seq_kernels.py --cpu-f32`, profiles/seq_kernels_matrix.md); the kernels get 8 times that, floored at 8.
# "ln-offset" is the one data set x = 100 + 0.01 randn: the statistics of a row whose mean is 10^4 times its spread lose that
# factor in ANY fp32 evaluation, so it carries its own figure and leaves the others as they are.
# "ln" / "skln" are large as well: A = |gamma| |x - mean| rstd + |beta| vanishes where x = mean and beta = 0, the rounding of the
# mean (2^-24 of mean|x|, times rstd |gamma|) does not.  "ln2" / "skln2" are the same figures on A2 = |gamma| (|x| + mean|x|) rstd
# + |beta|, criterion (c) of the driver: the bound that still tells round-to-nearest from truncation in a LayerNorm output.
CPU_F32_WORST = {"attn": 77.144, "ln": 1261.831, "ln-offset": 5493154.656, "skln": 313.717, "glu": 4.918,
                 "ln2": 18.135, "skln2": 3.126}


def F_of(kind):
    return max(8.0, 8.0 * CPU_F32_WORST[kind])


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the selection rules, restated -------------------------------------------------------------------------------------------------
RES_MAX_T = 208                            # csrc/attention.hip:241


def res_layout_bytes(T, relpos):
    """csrc/attention.hip:245-258 (ResLayout)."""
    tp16, tp32 = (T + 15) & ~15, (T + 31) & ~31
    prows = 2 * T + 47 if relpos else 0
    return tp16 * 128 + tp32 * 128 + prows * 128 + (2 * D * 4 if relpos else 0) + ((tp16 >> 4) * 48 * 16 * 4 if relpos else 0)


def attention_variant(T, H, pos, env):
    """csrc/attention.hip:533-555 (attention_select) for a 16-bit launch with valid arguments."""
    resident_on = int(env.get("L2S_ATTN_RESIDENT", "1"))
    plain_on = int(env.get("L2S_ATTN_RESIDENT_PLAIN", "0"))
    force_qb = int(env.get("L2S_ATTN_QB", "0"))
    rel = 1 if pos else 0
    if resident_on and (pos or plain_on) and T <= RES_MAX_T and H <= 256 and res_layout_bytes(T, pos) <= 160 * 1024:
        return ATTN_RESIDENT + rel
    big = force_qb == 128 if force_qb else (cdiv(T, 64) % 2 == 0 or T >= 512)
    return (128 if big else 64) + rel


def layernorm_variant(C, xf, yf, y2, zp, ldy, y_align16, env):
    """csrc/norm.hip:259-272 (layernorm_select) for a 16-bit-mode launch with valid arguments."""
    rows_on = int(env.get("L2S_LN_ROWS", "1"))
    if rows_on and xf and not y2 and zp == 0 and C in (512, 1024) and (yf or (y_align16 and ldy % 8 == 0)):
        return C + (1 if yf else 0)
    return LN_GENERIC + (2 if xf else 0) + (1 if yf else 0)


def glu_tile(T):
    """csrc/conformer_conv.hip:69-79 (glu_dwconv_select)."""
    r128, r100 = cdiv(T, 128) * 128, cdiv(T, 100) * 100
    return 100 if r100 + cdiv(T, 100) * 10 < r128 + cdiv(T, 128) * 10 else 128


# every instantiation the matrix must reach (some child, some case): (op, dt, code)
def instantiations():
    out = []
    for dt in DTYPES:
        out += [("attn", dt, v) for v in (64, 65, 128, 129, ATTN_RESIDENT, ATTN_RESIDENT + 1)]
        out += [("ln", dt, LN_GENERIC + i) for i in range(4)] + [("ln", dt, v) for v in (512, 513, 1024, 1025)]
        out += [("skln", dt, C + yf) for C in (512, 1024) for yf in (0, 1)]      # splitk_reduce_ln_kernel<ET, C / 256, yf>
        out += [("glu", dt, t) for t in (100, 128)]
    return out


# ---- attention ---------------------------------------------------------------------------------------------------------------------
ATTN_GUARD = 2                             # guard rows in front of and behind every buffer
POS_NL, POS_LI = 3, 1                      # the position table is the column window li of an nl-layer table (conformer.py)
REL_RESIDENT_T = (1, 15, 16, 17, 33, 64, 65, 129, 193, 207, 208)
REL_TILED_T = (209, 257, 320, 513)
PLAIN_T = (1, 37, 63, 64, 65, 128, 129, 192, 257, 512)
QB_T = (1, 65, 130, 513)
HEADS = (1, 2, 8)


def attn_lens(T, i, B=3):
    """B lengths drawn in turn from {T, 1, 64, 65, 128, T - 1, 0} (those that fit in T)."""
    cand = []
    for n in (T, 1, 64, 65, 128, T - 1, 0):
        if 0 <= n <= T and n not in cand:
            cand.append(n)
    return [cand[(3 * i + j) % len(cand)] for j in range(B)]


def _attn(name, dt, T, H, pos, lens, B=3, len_mul=1, data="randn"):
    return dict(op="attn", name=name, dt=dt, B=B, T=T, H=H, pos=pos, lens=lens, len_mul=len_mul, data=data,
                ldq=3 * H * D + 8, ldo=H * D + 4, ldp=POS_NL * H * D)


def klens(c):
    """Valid keys per clip: lens * len_mul clamped to T (the kernels' klen)."""
    if c["lens"] is None:
        return [c["T"]] * c["B"]
    return [min(n * c["len_mul"], c["T"]) for n in c["lens"]]


def _attn_grid(dt, Ts, pos, tag):
    out, i = [], 0
    for T in Ts:
        for H in HEADS:
            out.append(_attn(f"{tag}/T{T}-H{H}", dt, T, H, pos, attn_lens(T, i)))
            i += 1
    return out


def _attn_special(dt, pos):
    tag = "rel" if pos else "plain"
    out = [_attn(f"{tag}/no-lens-T65", dt, 65, 2, pos, None),
           # len_mul = 2: clip 0 clamps (2 x 60 > 100), clip 1 does not, clip 2 lands on T
           _attn(f"{tag}/len-mul2-T100", dt, 100, 2, pos, [60, 30, 50], len_mul=2),
           # online-softmax rescale: scores reach +-60, the dominant key in the last key tile for half the rows, the first for the rest
           _attn(f"{tag}/rescale-T130", dt, 130, 2, pos, [130, 130, 129], data="rescale")]
    return out


def _attn_slots(dt):
    # the resident kernel's persistent blocks: 256 / H slots; H = 128, B = 5: 2 slots, slot 0 takes clips 0, 2, 4; H = 256: one slot
    return [_attn("rel/slots-H128-B5-T33", dt, 33, 128, True, [33, 0, 17, 32, 1], B=5),
            _attn("rel/slots-H256-B3-T17", dt, 17, 256, True, [17, 16, 0], B=3)]


def attention_cases(env_name):
    out = []
    for dt in DTYPES:
        if env_name == "default":
            out += _attn_grid(dt, REL_RESIDENT_T + REL_TILED_T, True, "rel") + _attn_grid(dt, PLAIN_T, False, "plain")
            out += _attn_special(dt, True) + _attn_special(dt, False) + _attn_slots(dt)
        elif env_name == "resident-off":
            out += _attn_grid(dt, REL_RESIDENT_T, True, "rel") + _attn_special(dt, True)
        elif env_name == "resident-plain":
            out += _attn_grid(dt, [T for T in PLAIN_T if T <= RES_MAX_T], False, "plain") + _attn_special(dt, False)
        elif env_name in ("qb64", "qb128"):
            out += _attn_grid(dt, QB_T, True, "rel") + _attn_grid(dt, QB_T, False, "plain")
    for c in out:
        c["inst"] = ("attn", c["dt"], attention_variant(c["T"], c["H"], c["pos"], ENVS[env_name]))
    return out


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_GUARD = 2
ROWS_M = (1, 2, 3, 7, 8, 9, 15, 16, 17, 33)
GENERIC_C = (4, 252, 256, 260, 768, 2048)
ZPS = (0, 4, 1024)
LN_MASKS = {33: (11, 2, [3, 0, 7]), 17: (6, 2, [1, 0, 3]), 9: (4, 2, [1, 0, 2])}    # M -> (mask_T, len_mul, lens)


def _ln(name, dt, M, C, *, xf=True, yf=False, ldx=None, ldy=None, y_off=0, y2=False, zp=0, eps=1e-5, inplace=False, data="randn",
        zero_row=False, mask=None, skip_a=False):
    W = C + zp
    return dict(op="ln", name=name, dt=dt, M=M, C=C, xf=xf, yf=yf, ldx=ldx if ldx is not None else C + 4,
                ldy=ldy if ldy is not None else W + 4, y_off=y_off, y2=y2, ldy2=W + 8 if y2 else 0, zp=zp, eps=eps, inplace=inplace,
                data=data, zero_row=zero_row, mask=mask, skip_a=skip_a)


def layernorm_cases(env_name):
    out = []
    for dt in DTYPES:
        # the rows kernel's shapes: every M around its 8- / 16-row blocks, fp32 in place, fp32 elsewhere, 16-bit
        for C in (512, 1024):
            eps = 1e-12 if C == 512 else 1e-5
            for M in ROWS_M:
                mask = LN_MASKS.get(M)
                kw = dict(eps=eps, mask=mask, zero_row=eps == 1e-12 and M in (3, 16))
                out.append(_ln(f"rows/C{C}-M{M}-f32-inplace", dt, M, C, yf=True, ldy=C + 4, inplace=True, **kw))
                out.append(_ln(f"rows/C{C}-M{M}-f32", dt, M, C, yf=True, ldy=C + 4, **kw))
                out.append(_ln(f"rows/C{C}-M{M}-16", dt, M, C, yf=False, ldy=C + 8, **kw))
            # x = 100 + 0.01 randn.  The fp32-output cases are held to (b) and (c) only (`skip_a`): the fp32 tolerance of criterion
            # (a), 2e-5 max|ref| + 1e-5, is out of reach of ANY fp32 LayerNorm on such a row - the mean of 512 values near 100 carries
            # about 2^-24 x 100 = 6e-6, that is 6e-4 of the spread 0.01 and of every output (profiles/seq_kernels_matrix.md has the
            # kernels' figures against it)
            out.append(_ln(f"rows/C{C}-M9-f32-offset", dt, 9, C, yf=True, ldy=C + 4, data="offset", eps=eps, skip_a=True))
            out.append(_ln(f"rows/C{C}-M9-16-offset", dt, 9, C, yf=False, ldy=C + 8, data="offset", eps=eps))
            # the two fallbacks to the generic kernel: ldy % 8 == 4, and a y that is 8- but not 16-byte aligned
            out.append(_ln(f"fallback/C{C}-ldy", dt, 9, C, yf=False, ldy=C + 4, eps=eps, mask=LN_MASKS[9]))
            out.append(_ln(f"fallback/C{C}-yoff", dt, 9, C, yf=False, ldy=C + 8, y_off=4, eps=eps))
        # the generic kernel: every (x, y) type pair at every width, zero prefix, second output, both eps
        for ci, C in enumerate(GENERIC_C):
            for xi, xf in enumerate((True, False)):
                for yi, yf in enumerate((True, False)):
                    for zi, zp in enumerate(ZPS):
                        M = (1, 5, 9)[(ci + xi + yi + zi) % 3]
                        eps = (1e-5, 1e-12)[(ci + zi) % 2]
                        out.append(_ln(f"generic/C{C}-x{32 if xf else 16}-y{32 if yf else 16}-zp{zp}", dt, M, C, xf=xf, yf=yf,
                                       y2=(ci + xi + 2 * yi + zi) % 2 == 0, zp=zp, eps=eps, zero_row=eps == 1e-12 and M == 5,
                                       mask=LN_MASKS[9] if M == 9 else None))
        out.append(_ln("generic/C768-x32-y16-offset", dt, 9, 768, xf=True, yf=False, data="offset"))
    for c in out:
        y_align16 = (c["y_off"] * 2) % 16 == 0          # 16-bit y: guard rows and leading dimensions keep the base 16-byte aligned
        c["inst"] = ("ln", c["dt"], layernorm_variant(c["C"], c["xf"], c["yf"], c["y2"], c["zp"], c["ldy"], y_align16, ENVS[env_name]))
    return out


def ln_keep(c):
    """Rows the mask keeps (None: no mask)."""
    if c["mask"] is None:
        return None
    mask_T, len_mul, lens = c["mask"]
    return [(r % mask_T) < lens[r // mask_T] * len_mul for r in range(c["M"])]


def splitk_ln_cases():
    out = []
    for dt in DTYPES:
        for C in (512, 1024):
            for M in (1, 5, 9):
                for S in (1, 3):
                    for yf in (False, True):
                        out.append(dict(op="skln", name=f"skln/C{C}-M{M}-S{S}-{'f32-inplace' if yf else '16'}", dt=dt, M=M, C=C, S=S,
                                        yf=yf, inplace=yf, ldp=S * C + 4, ldx=C + 4, ldy=C + 4 if yf else C + 8,
                                        eps=1e-12 if C == 512 else 1e-5, mask=(3, 2, [1, 0, 2]) if M == 9 else None,
                                        inst=("skln", dt, C + (1 if yf else 0))))
    return out


# ---- GLU / depthwise conv / swish --------------------------------------------------------------------------------------------------
GLU_GUARD = 2
GLU_T128 = (101, 128, 250)
GLU_T100 = (1, 31, 99, 100, 200, 257)
GLU_C = (64, 128, 512)
GLU_K = (1, 3, 15, 31)


def glu_len_candidates(T):
    """Lengths at every tile edge +- 1, {0, 1, 15, 16}, tile + 7 (the next tile holds 7 valid rows and the previous tile's halo
    crosses the limit), T - 1 and T; those that fit in T."""
    tile = glu_tile(T)
    cand = [T]
    for e in range(tile, T + 1, tile):
        cand += [e - 1, e, e + 1]
    cand += [0, 1, 15, 16, tile + 7, T - 1]
    out = []
    for n in cand:
        if 0 <= n <= T and n not in out:
            out.append(n)
    return out


def glu_cases():
    out = []
    for dt in DTYPES:
        for ti, T in enumerate(GLU_T128 + GLU_T100):
            cand = glu_len_candidates(T)
            for ki, k in enumerate(GLU_K):
                C = GLU_C[(ti + ki) % 3]
                lens = [cand[(3 * ki + j) % len(cand)] for j in range(3)]
                out.append(dict(op="glu", name=f"glu/T{T}-C{C}-k{k}", dt=dt, B=3, T=T, C=C, k=k, lens=lens, len_mul=1))
        # len_mul = 2: a clamp (2 x lens > T), a tile edge, an empty clip
        out.append(dict(op="glu", name="glu/T250-len-mul2", dt=dt, B=3, T=250, C=128, k=31, lens=[130, 64, 0], len_mul=2))
        out.append(dict(op="glu", name="glu/T200-len-mul2", dt=dt, B=3, T=200, C=128, k=31, lens=[101, 50, 57], len_mul=2))
        out.append(dict(op="glu", name="glu/T128-no-lens", dt=dt, B=3, T=128, C=64, k=31, lens=None, len_mul=1))
    for c in out:
        c["inst"] = ("glu", c["dt"], glu_tile(c["T"]))
    return out


def glu_lims(c):
    if c["lens"] is None:
        return [c["T"]] * c["B"]
    return [min(n * c["len_mul"], c["T"]) for n in c["lens"]]


# ---- parts of a child ----------------------------------------------------------------------------------------------------------------
def cases_of(env_name):
    if env_name == "default":
        return attention_cases(env_name) + layernorm_cases(env_name) + splitk_ln_cases() + glu_cases()
    if env_name == "ln-rows-off":
        return layernorm_cases(env_name)
    return attention_cases(env_name)
