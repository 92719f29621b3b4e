"""The step matrix as data: the autoregressive decoding kernels of csrc/whisper_decode.hip (l2s_kv_attention, l2s_vocab_argmax,
l2s_whisper_advance), csrc/s2s_decode.hip (l2s_beam_attention, l2s_beam_select, l2s_beam_advance) with their closed loop, and
l2s_ctc_beam_search of csrc/ctc.hip.  A case is a
dict: `name` part/descriptive-name, `op` (the entry), shapes, leading dimensions, `dt`, `expect` (the return code) and `hits` (what it
is there for).  PARTS maps a part to its cases; the parts split the work by run time only.  tools/check_step_kernels.py runs a part;
tests/test_step_matrix_cpu.py proves the coverage.  No device, no torch."""
from collections import OrderedDict

GUARD = 3
CANARY16, CANARY32 = 0x5A5A, 0x5A5A5A5A
OK, EINVAL, ESHAPE, EALIGN, EUNSUPPORTED = 0, -1, -2, -3, -4
DTS = ("f16", "bf16")
PADS = (8, 16, 24)               # ldq = W + 8, ldo = W + 16, ld_new = W + 24
ATTN_F = 4.0                     # |gpu - f64| <= ATTN_F max |round16(ref) - ref| (tests/test_whisper_kernels_gpu.py, tests/test_lipread_kernels_gpu.py)
# l2s_ctc_beam_search cases: seeds 0, 1, .. tried in order, the first at which every frame of every clip is decisive
CT_SEED = {'ctc/beam2-K64-L50-len_mul2': 1, 'ctc/beam30-K40-L50': 15, 'ctc/beam64-K64-L2-nbest64': 5, 'ctc/noblank-beam30-K40': 6, 'ctc/blankfirst-beam30-K40': 7,
           'ctc/ties-beam30-K6': 4,
           'ctc/revival-beam3-V5': 490}       # revival: the first decisive seed at which a pruned prefix does come back
DECISIVE = 2.0                   # every gap that decides an id or a candidate exceeds DECISIVE x the value bound, or the tie is bit-exact


def _chunks(xs, n):
    xs = list(xs)
    out = []
    for i in range(0, len(xs), n):
        c = xs[i:i + n]
        out.append(c + c[:1] * (n - len(c)))
    return out


# ---- l2s_kv_attention ---------------------------------------------------------------------------------------------------------------------------
def kv(name, hits, H, B, T, dt, form="self", append=True, pos=None, stride=1, n_valid=0, pads=PADS, value="rand", expect=OK, **kw):
    return dict(name=name, op="kv", hits=hits, H=H, B=B, T=T, dt=dt, form=form, append=append, pos=pos, stride=stride, n_valid=n_valid,
                pads=pads, value=value, expect=expect, **kw)


KV_VALID = (0, 1, 7, 8, 9, 127, 128, 129, 255, 256, 257)


def kv_cases():
    out = []
    hs = (1, 2, 20)
    n = 0
    for T in (1, 8, 257, 448):
        valid = sorted({v for v in KV_VALID if v <= T} | {T - 1, T})
        for ci, ch in enumerate(_chunks(valid, 5)):
            for append in (True, False):
                H = hs[n % 3]
                n += 1
                for dt in DTS:
                    out.append(kv(f"kvattn/self-T{T}-valid-{'-'.join(map(str, ch))}-H{H}-{'app' if append else 'ro'}-{dt}",
                                  "valid lengths at the 8 / 128 / 256 key edges, per-clip positions mixed in one launch", H, 5, T, dt,
                                  append=append, pos=[v - 1 for v in ch]))
    for dt in DTS:
        out += [
            kv(f"kvattn/self-p-at-and-past-T-{dt}", "p = cache_T and cache_T + 5: no append, all rows attended; p = -1: zeros", 2, 5, 8, dt,
               pos=[8, 13, -1, 7, 3]),
            kv(f"kvattn/self-p-at-and-past-T257-{dt}", "p >= cache_T at a cache of three loads", 1, 5, 257, dt, pos=[257, 262, -1, 256, 128]),
            kv(f"kvattn/self-stride0-p128-{dt}", "pos_stride 0: one position for every clip", 2, 5, 257, dt, pos=[128], stride=0),
            kv(f"kvattn/self-stride0-pT-{dt}", "pos_stride 0 at p = cache_T", 1, 5, 8, dt, pos=[8], stride=0),
            kv(f"kvattn/self-stride0-pminus1-{dt}", "pos_stride 0 at p = -1: zeros, nothing appended", 1, 5, 8, dt, pos=[-1], stride=0),
            kv(f"kvattn/self-B1-H20-p255-{dt}", "one clip, 20 heads", 20, 1, 448, dt, pos=[255]),
            kv(f"kvattn/self-B1-H1-T1-{dt}", "the smallest launch", 1, 1, 1, dt, pos=[0]),
            kv(f"kvattn/self-B70-{dt}", "70 clips in one launch", 1, 70, 8, dt, pos=[(3 * b) % 10 - 1 for b in range(70)]),
            kv(f"kvattn/self-tight-ld-{dt}", "every leading dimension at its minimum", 2, 5, 257, dt, pos=[0, 127, 128, 255, 256], pads=(0, 0, 0)),
            kv(f"kvattn/value-dominant-first-group-{dt}", "key 0 leads by >= 30", 2, 5, 448, dt, pos=[300] * 5, value="dom:0"),
            kv(f"kvattn/value-dominant-wave15-last-group-{dt}", "key 127 leads by >= 30", 2, 5, 448, dt, pos=[300] * 5, value="dom:127"),
            kv(f"kvattn/value-dominant-second-half-{dt}", "key 200 (second load of a double iteration) leads by >= 30", 2, 5, 448, dt,
               pos=[300] * 5, value="dom:200"),
            kv(f"kvattn/value-dominant-appended-row-{dt}", "the appended key leads by >= 30", 2, 5, 448, dt, pos=[300] * 5, value="dom:new"),
            kv(f"kvattn/value-all-scores-equal-{dt}", "every score equal: the mean of the value rows", 2, 5, 448, dt, pos=[0, 8, 129, 300, 447],
               value="equal"),
            kv(f"kvattn/value-scores-pm60-{dt}", "scores of exactly +60 and -60: the online-softmax rescale", 2, 5, 448, dt,
               pos=[1, 9, 129, 300, 447], value="pm60"),
        ]
        for nv in (0, 1, 128, 129, 1001, 1500):
            out.append(kv(f"kvattn/cross-n{nv}-{dt}", "cross form at cache_T = 1500", 2, 1 if nv in (1001, 1500) else 5, 1500, dt, form="cross",
                          append=False, n_valid=nv))
    return out


def kv_refusals():
    base = dict(H=2, B=2, T=8, dt="f16", pos=[3, 4])
    r = lambda name, expect, **kw: kv("refusals/kv-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    return [r("null-q", EINVAL, null="q"), r("null-kc", EINVAL, null="kc"), r("null-vc", EINVAL, null="vc"), r("null-out", EINVAL, null="out"),
            r("k_new-without-v_new", EINVAL, null="v_new"), r("v_new-without-k_new", EINVAL, null="k_new"),
            r("k_new-without-pos", EINVAL, null="pos"), r("pos_stride-2", EINVAL, stride=2),
            r("B-0", ESHAPE, B_arg=0), r("H-0", ESHAPE, H_arg=0), r("cache_T-0", ESHAPE, T_arg=0),
            r("ldq-below-W", ESHAPE, ld_arg=dict(q=120)), r("ldo-below-W", ESHAPE, ld_arg=dict(out=120)),
            r("ld_new-below-W", ESHAPE, ld_arg=dict(new=120)),
            r("n_valid-above-T", ESHAPE, form="cross", append=False, n_valid=9), r("n_valid-negative", ESHAPE, form="cross", append=False, n_valid=-1),
            r("dtype-f32", EUNSUPPORTED, dtype_arg=2), r("H-21", EUNSUPPORTED, H_arg=21, ld_arg=dict(q=1344, out=1344, new=1344)),
            r("cache_T-1501", EUNSUPPORTED, T_arg=1501),
            r("misaligned-q", EALIGN, off=dict(q=2)), r("misaligned-cache", EALIGN, off=dict(kc=8)), r("misaligned-out", EALIGN, off=dict(out=4)),
            r("misaligned-k_new", EALIGN, off=dict(k_new=2)), r("misaligned-pos", EALIGN, off=dict(pos=2)),
            r("ldq-and-7", EALIGN, ld_arg=dict(q=132)), r("ldo-and-7", EALIGN, ld_arg=dict(out=129)), r("ld_new-and-7", EALIGN, ld_arg=dict(new=134))]


# ---- l2s_beam_attention -------------------------------------------------------------------------------------------------------------------------
def ba(name, hits, hd, H, beam, B, T, dt, form="self", p=0, anc="rand", n_live=None, finished=None, enc_lens=None, pads=PADS, expect=OK, **kw):
    return dict(name=name, op="ba", hits=hits, hd=hd, H=H, beam=beam, B=B, T=T, dt=dt, form=form, p=p, anc=anc, n_live=n_live,
                finished=finished, enc_lens=enc_lens, pads=pads, expect=expect, **kw)


BA_P = (0, 1, 7, 8, 15, 16, 17, 31, 32, 33)
BA_BEAMS = (1, 3, 4, 5, 8, 64)
BA_ANC = ("identity", "one", "perm", "clamp", "rand")


def ba_cases():
    out = []
    n = 0
    for T in (18, 40):
        for p in sorted({q for q in BA_P if q < T} | {T - 1}):
            hd = (64, 128, 192)[n % 3]
            beam = BA_BEAMS[n % 5]                    # 64 has cases of its own
            H = (1, 2)[(n // 3) % 2]
            anc = BA_ANC[(n // 2) % 5]
            n += 1
            for dt in DTS:
                out.append(ba(f"battn/self-T{T}-p{p}-hd{hd}-H{H}-beam{beam}-{anc}-{dt}", "positions at the 8 / 16 key edges; the other half of "
                              "the ancestor buffer holds different parents", hd, H, beam, 3, T, dt, p=p, anc=anc))
    for dt in DTS:
        out += [
            ba(f"battn/self-p-T-{dt}", "p = T: zero rows, the caches unchanged", 64, 2, 5, 3, 18, dt, p=18),
            ba(f"battn/self-p-minus1-{dt}", "p = -1: zero rows, the caches unchanged", 128, 1, 4, 3, 18, dt, p=-1),
            ba(f"battn/self-beam64-p17-{dt}", "64 slots: 16 blocks of four", 64, 1, 64, 1, 18, dt, p=17, anc="perm"),
            ba(f"battn/self-beam64-p32-clamp-{dt}", "64 slots with entries -3 and beam + 2", 64, 2, 64, 3, 40, dt, p=32, anc="clamp"),
            ba(f"battn/self-W1536-p16-{dt}", "H = 8 at hd = 192: W = 1536", 192, 8, 3, 1, 18, dt, p=16),
            ba(f"battn/self-W1536-beam8-p33-{dt}", "W = 1536 with two blocks of slots", 192, 8, 8, 3, 40, dt, p=33, anc="one"),
            ba(f"battn/self-B70-{dt}", "70 clips", 64, 1, 3, 70, 18, dt, p=9, n_live=[b % 5 for b in range(70)], finished=[int(b % 7 == 3) for b in range(70)]),
            ba(f"battn/self-B1-beam1-{dt}", "the smallest launch", 64, 1, 1, 1, 18, dt, p=0, anc="identity"),
            ba(f"battn/self-n_live-0-1-beam-{dt}", "n_live 0, 1, beam", 64, 2, 5, 3, 18, dt, p=8, n_live=[0, 1, 5]),
            ba(f"battn/self-n_live-beam-1-beam+3-{dt}", "n_live beam - 1 and beam + 3, a finished clip between live ones", 128, 2, 4, 3, 18, dt, p=15,
               n_live=[3, 4, 7], finished=[0, 1, 0]),
            ba(f"battn/self-n_live-null-finished-{dt}", "n_live NULL, finished given", 64, 2, 8, 3, 40, dt, p=31, finished=[0, 1, 0]),
            ba(f"battn/self-n_live-finished-null-{dt}", "both NULL (the sweep above) against n_live given, finished NULL", 64, 2, 3, 3, 18, dt, p=7,
               n_live=[2, 3, 1]),
            ba(f"battn/self-tight-ld-{dt}", "every leading dimension at its minimum", 128, 2, 5, 3, 40, dt, p=33, pads=(0, 0, 0)),
            ba(f"battn/self-odd-p-other-half-{dt}", "p odd: half 1 is current, half 0 holds other parents", 64, 2, 4, 3, 18, dt, p=15, anc="perm"),
            ba(f"battn/self-even-p-other-half-{dt}", "p even: half 0 is current, half 1 holds other parents", 64, 2, 4, 3, 18, dt, p=16, anc="perm"),
            ba(f"battn/cross-T16-{dt}", "enc_lens -2, 0, 1, 15, 16, 17, T + 9 in one launch", 64, 2, 3, 7, 16, dt, form="cross",
               enc_lens=[-2, 0, 1, 15, 16, 17, 25]),
            ba(f"battn/cross-T200-{dt}", "enc_lens across the 16-key iterations of a longer cache", 128, 1, 5, 8, 200, dt, form="cross",
               enc_lens=[-2, 0, 1, 15, 16, 17, 200, 209], n_live=[5, 5, 4, 5, 1, 8, 5, 0], finished=[0, 0, 0, 1, 0, 0, 0, 0]),
            ba(f"battn/cross-W1536-{dt}", "cross form at W = 1536", 192, 8, 4, 1, 16, dt, form="cross", enc_lens=[16]),
            ba(f"battn/cross-beam64-hd192-{dt}", "cross form, 64 slots, three chunks per head", 192, 1, 64, 3, 16, dt, form="cross", enc_lens=[15, 16, 1]),
            ba(f"battn/cross-beam1-B70-{dt}", "70 clips, one slot", 64, 1, 1, 70, 16, dt, form="cross", enc_lens=[(5 * b) % 20 - 2 for b in range(70)]),
            ba(f"battn/cross-beam8-hd128-H2-tight-{dt}", "two full blocks of slots, tight leading dimensions", 128, 2, 8, 3, 200, dt, form="cross",
               enc_lens=[200, 17, 33], pads=(0, 0, 0)),
        ]
    return out


def ba_refusals():
    base = dict(hd=64, H=2, beam=3, B=2, T=18, dt="f16", p=4)
    cross = dict(form="cross", enc_lens=[5, 6])
    r = lambda name, expect, **kw: ba("refusals/ba-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    return [r("null-q", EINVAL, null="q"), r("null-kc", EINVAL, null="kc"), r("null-vc", EINVAL, null="vc"), r("null-out", EINVAL, null="out"),
            r("k_new-without-v_new", EINVAL, null="v_new"), r("self-without-anc", EINVAL, null="anc"), r("self-without-step", EINVAL, null="step"),
            r("self-with-enc_lens", EINVAL, extra="enc_lens"), r("cross-without-enc_lens", EINVAL, **cross, null="enc_lens"),
            r("cross-with-anc", EINVAL, **cross, extra="anc"),
            r("B-0", ESHAPE, B_arg=0), r("beam-0", ESHAPE, beam_arg=0), r("H-0", ESHAPE, H_arg=0), r("T-0", ESHAPE, T_arg=0),
            r("hd-32", EUNSUPPORTED, hd_arg=32), r("hd-256", EUNSUPPORTED, hd_arg=256),
            r("ldq-below-W", ESHAPE, ld_arg=dict(q=120)), r("ldo-below-W", ESHAPE, ld_arg=dict(out=120)), r("ld_new-below-W", ESHAPE, ld_arg=dict(new=120)),
            r("dtype-f32", EUNSUPPORTED, dtype_arg=2), r("W-1600", EUNSUPPORTED, H_arg=25, ld_arg=dict(q=1600, out=1600, new=1600)),
            r("beam-65", EUNSUPPORTED, beam_arg=65), r("T-32768", EUNSUPPORTED, T_arg=32768),
            r("misaligned-q", EALIGN, off=dict(q=2)), r("misaligned-cache", EALIGN, off=dict(vc=8)), r("misaligned-out", EALIGN, off=dict(out=4)),
            r("misaligned-anc", EALIGN, off=dict(anc=1)), r("misaligned-step", EALIGN, off=dict(step=2)),
            r("misaligned-enc_lens", EALIGN, **cross, off=dict(enc_lens=2)), r("misaligned-n_live", EALIGN, n_live=[3, 3], off=dict(n_live=2)),
            r("ldq-and-7", EALIGN, ld_arg=dict(q=132)), r("ldo-and-7", EALIGN, ld_arg=dict(out=129)), r("ld_new-and-7", EALIGN, ld_arg=dict(new=134))]


# ---- l2s_vocab_argmax ---------------------------------------------------------------------------------------------------------------------------
def va(name, hits, V, d, B, dt, plant, mask="none", step=None, first=3, ldpad=(8, 16), expect=OK, **kw):
    """plant: [(top id, id of an exact copy or None), ...]; clip b's input is base vector b % len(plant), whose planted row is plant[b % n]"""
    return dict(name=name, op="va", hits=hits, V=V, d=d, B=B, dt=dt, plant=plant, mask=mask, step=step, first=first, ldpad=ldpad, expect=expect, **kw)


def va_cases():
    out = []
    big = 65536
    last = (big - 1) // 64
    for dt in DTS:
        out += [
            va(f"vocab/V1-d64-B1-{dt}", "one id; d = 64 is the tail loop alone", 1, 64, 1, dt, [(0, None)]),
            va(f"vocab/V15-d128-B15-{dt}", "V below a wave's rows; B <= 16 from below", 15, 128, 15, dt, [(0, None), (14, None), (7, None)]),
            va(f"vocab/V16-d256-B16-{dt}", "V = one wave; B = 16: one B operand; d = one 256 block", 16, 256, 16, dt, [(15, None), (0, None)]),
            va(f"vocab/V17-d320-B17-{dt}", "B = 17: two B operands; d = 256 + one tail step", 17, 320, 17, dt, [(16, None), (0, 16 - 8), (3, None)]),
            va(f"vocab/V63-d1280-B32-{dt}", "B = 32; d = 1280", 63, 1280, 32, dt, [(62, None), (0, None), (33, 49)]),
            va(f"vocab/V64-d128-B33-{dt}", "V = one tile; B = 33: four B operands", 64, 128, 33, dt, [(63, None), (0, None), (16, 32), (47, None)]),
            va(f"vocab/V65-d64-B64-{dt}", "V = a tile and one row; B = 64 fills grid.y = 1", 65, 64, 64, dt, [(64, None), (0, 64), (31, None)]),
            va(f"vocab/V333-d128-B65-{dt}", "B = 65: grid.y = 2", 333, 128, 65, dt, [(332, None), (0, None), (100, 164), (5, 6)]),
            va(f"vocab/V333-d320-B130-{dt}", "B = 130: grid.y = 3", 333, 320, 130, dt, [(1, None), (320, 332), (200, None)]),
            va(f"vocab/V333-waves-and-fq-{dt}", "the maximum in each wave of a tile and each fq group of a wave", 333, 64, 16, dt,
               [(64 + 16 * w + 4 * f + (w + f) % 4, None) for w in range(4) for f in range(4)]),
            va(f"vocab/V333-ties-lane-lanes-waves-tiles-{dt}", "exact ties inside a lane's four rows, across lanes, waves and tiles: the lowest id",
               333, 128, 4, dt, [(8, 9), (20, 27), (70, 118), (130, 322)]),
            va(f"vocab/V16385-d64-tiles-0-255-256-last-{dt}", "the finish kernel's second round: maxima in tiles 0, 255, 256 and the last", 16385, 64, 4, dt,
               [(3, None), (255 * 64 + 5, None), (256 * 64, None), (16384, None)]),
            va(f"vocab/V65536-d64-tiles-{dt}", "the largest vocabulary: maxima in tiles 0, 255, 256 and the last (row V - 1)", big, 64, 4, dt,
               [(0, None), (255 * 64 + 63, None), (256 * 64 + 1, None), (big - 1, None)]),
            va(f"vocab/V65536-d64-ties-t-and-t+256-{dt}", "exact ties across tiles t and t + 256 (one thread of the finish kernel) and t, t + 257", big, 64, 3, dt,
               [(5 * 64 + 2, (5 + 256) * 64 + 2), (700 * 64, (700 + 257) * 64 + 9), (64 * last + 1, None)]),
            va(f"vocab/V333-suppress-top-{dt}", "suppress on the maximum: the copy, or the runner-up, wins", 333, 128, 17, dt, [(40, 41), (100, None), (300, 10)],
               mask="top"),
            va(f"vocab/V333-suppress-all-{dt}", "every id suppressed: -1 and -inf", 333, 128, 3, dt, [(40, None)], mask="all"),
            va(f"vocab/V333-begin-at-first-{dt}", "begin_suppress at *step == first_step", 333, 128, 5, dt, [(40, 41), (100, None)], mask="begin", step=3),
            va(f"vocab/V333-begin-not-first-{dt}", "begin_suppress at *step != first_step: no effect", 333, 128, 5, dt, [(40, 41), (100, None)], mask="begin", step=4),
            va(f"vocab/V333-suppress-and-begin-{dt}", "both masks: the maximum by suppress, its copy by begin_suppress", 333, 128, 5, dt, [(40, 41), (100, 200)],
               mask="both", step=3),
            va(f"vocab/V64-tight-ld-{dt}", "ldx = lde = d", 64, 128, 3, dt, [(5, None)], ldpad=(0, 0)),
        ]
    return out


def va_refusals():
    base = dict(V=64, d=64, B=2, dt="f16", plant=[(5, None)])
    r = lambda name, expect, **kw: va("refusals/va-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    return [r("null-x", EINVAL, null="x"), r("null-emb", EINVAL, null="emb"), r("null-work", EINVAL, null="work"), r("null-token", EINVAL, null="token"),
            r("null-logprob", EINVAL, null="logprob"), r("begin-without-step", EINVAL, mask="begin", step=None),
            r("B-0", ESHAPE, B_arg=0), r("V-0", ESHAPE, V_arg=0), r("d-0", ESHAPE, d_arg=0), r("ldx-below-d", ESHAPE, ld_arg=dict(x=56)),
            r("lde-below-d", ESHAPE, ld_arg=dict(emb=56)), r("dtype-f32", EUNSUPPORTED, dtype_arg=2), r("V-65537", EUNSUPPORTED, V_arg=65537),
            r("d-and-63", EUNSUPPORTED, d_arg=32), r("d-1344", EUNSUPPORTED, d_arg=1344, ld_arg=dict(x=1344, emb=1344)),
            r("ldx-and-7", EALIGN, ld_arg=dict(x=68)), r("lde-and-7", EALIGN, ld_arg=dict(emb=70)), r("misaligned-x", EALIGN, off=dict(x=2)),
            r("misaligned-emb", EALIGN, off=dict(emb=8)), r("misaligned-work", EALIGN, off=dict(work=2)), r("misaligned-token", EALIGN, off=dict(token=2)),
            r("misaligned-logprob", EALIGN, off=dict(logprob=1)), r("misaligned-logits", EALIGN, off=dict(logits=2)),
            r("misaligned-step", EALIGN, mask="begin", step=3, off=dict(step=2))]


# ---- l2s_whisper_advance ------------------------------------------------------------------------------------------------------------------------
def wa(name, hits, B, d, dt, pos, ld_tok=5, n_ctx=9, V=50, eot=7, ldpad=(4, 8), live="mixed", expect=OK, **kw):
    return dict(name=name, op="wa", hits=hits, B=B, d=d, dt=dt, pos=pos, ld_tok=ld_tok, n_ctx=n_ctx, V=V, eot=eot, ldpad=ldpad, live=live,
                expect=expect, **kw)


def wa_cases():
    out = []
    for dt in DTS:
        for pos, (B, d) in zip((-1, 0, 4, 5, 7, 8), ((1, 8), (255, 384), (256, 8), (257, 8), (300, 1280), (5, 384))):
            out.append(wa(f"wadv/pos{pos}-B{B}-d{d}-{dt}", "*pos at -1, 0, ld_tok - 1, ld_tok, n_ctx - 2, n_ctx - 1: the no-write rules of tokens "
                          "and x_next; tokens -1 and V and done clips resolve to eot", B, d, dt, pos))
        out += [wa(f"wadv/only-clip-256-live-{dt}", "n_active across the 256-thread boundary", 300, 8, dt, 2, live="only256"),
                wa(f"wadv/all-done-{dt}", "every clip done before: nothing moves but pos", 257, 8, dt, 1, live="none"),
                wa(f"wadv/tight-ld-{dt}", "ldx = lde = d", 5, 384, dt, 3, ldpad=(0, 0))]
    return out


def wa_refusals():
    base = dict(B=3, d=8, dt="f16", pos=1)
    r = lambda name, expect, **kw: wa("refusals/wa-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    names = ("token", "logprob", "tokens", "sum_logprob", "lengths", "done", "emb", "pos_emb", "x", "pos", "n_active")
    return [r("null-" + n, EINVAL, null=n) for n in names] + [
        r("B-0", ESHAPE, B_arg=0), r("V-0", ESHAPE, V_arg=0), r("d-0", ESHAPE, d_arg=0), r("ld_tok-0", ESHAPE, ld_tok_arg=0), r("n_ctx-0", ESHAPE, n_ctx_arg=0),
        r("eot-negative", EINVAL, eot_arg=-1), r("eot-V", EINVAL, eot_arg=50), r("lde-below-d", ESHAPE, ld_arg=dict(emb=0)), r("ldx-below-d", ESHAPE, ld_arg=dict(x=4)),
        r("dtype-f32", EUNSUPPORTED, dtype_arg=2), r("d-and-7", EUNSUPPORTED, d_arg=4), r("d-1288", EUNSUPPORTED, d_arg=1288, ld_arg=dict(x=1288, emb=1288)),
        r("V-65537", EUNSUPPORTED, V_arg=65537), r("lde-and-7", EALIGN, ld_arg=dict(emb=12)), r("ldx-and-3", EALIGN, ld_arg=dict(x=10)),
        r("misaligned-emb", EALIGN, off=dict(emb=8)), r("misaligned-pos_emb", EALIGN, off=dict(pos_emb=8)), r("misaligned-x", EALIGN, off=dict(x=8)),
        r("misaligned-token", EALIGN, off=dict(token=2)), r("misaligned-pos", EALIGN, off=dict(pos=2))]


# ---- l2s_beam_select ----------------------------------------------------------------------------------------------------------------------------
def bs(name, hits, beam, V, step, kind="crafted", ldpad=0, n_live="beam", null_live=False, min_len=2, pad=1, unk=3, B=3, expect=OK, **kw):
    return dict(name=name, op="bs", hits=hits, beam=beam, V=V, step=step, kind=kind, ldpad=ldpad, n_live=n_live, null_live=null_live,
                min_len=min_len, pad=pad, unk=unk, B=B, expect=expect, **kw)


BS_SHAPES = ((1, 4), (2, 6), (5, 36), (50, 1004), (64, 130), (64, 8192))


def bs_cases():
    out = []
    for beam, V in BS_SHAPES:
        for step, what in ((0, "step 0: slot 0 alone"), (1, "below min_len: no eos"), (3, "free"), (5, ">= max_len of clip 1: eos alone is finite")):
            pad = 0 if step in (0, 3) else 5
            out.append(bs(f"select/beam{beam}-V{V}-step{step}-ld+{pad}", what + "; a NaN logit and a NaN row; a finished clip", beam, V, step, ldpad=pad,
                          n_live="mixed"))
    out += [
        bs("select/n_live-minus1-0-1", "n_live -1, 0 and 1 are one live slot", 5, 36, 3, n_live=[-1, 0, 1], ldpad=4),
        bs("select/n_live-beam-beam+5", "n_live beam and beam + 5 are beam live slots", 5, 36, 3, n_live=[5, 10, 4]),
        bs("select/n_live-null", "n_live NULL: beam live slots", 5, 36, 3, null_live=True, ldpad=4),
        bs("select/finished-null", "finished NULL: every clip is selected", 5, 36, 3, null_fin=True),
        bs("select/pad-unk-off", "pad = unk = -1: no pad rule, no unk penalty", 5, 36, 3, pad=-1, unk=-1, ldpad=4),
        bs("select/pad-unk-off-V1004", "rules off at a larger vocabulary", 50, 1004, 4, pad=-1, unk=-1),
        bs("select/tie-top-byte-bucket", "the K best fill one top-byte bucket exactly: the radix select ends after its first pass", 2, 6, 0, kind="topbyte", min_len=0),
        bs("select/tie-index-bytes-V36", "identical rows with equal cumulative scores: decided in the index bytes", 5, 36, 3, kind="tierows", ldpad=4),
        bs("select/tie-index-bytes-V8192", "the same at V = 8192", 64, 8192, 3, kind="tierows", B=1),
        bs("select/tie-index-bytes-beam2", "two identical rows", 2, 36, 2, kind="tierows"),
    ]
    return out


def bs_refusals():
    base = dict(beam=2, V=8, step=2)
    r = lambda name, expect, **kw: bs("refusals/bs-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    return [r("null-" + n, EINVAL, null=n) for n in ("logits", "scores", "step", "max_len", "cand_score", "cand_slot", "cand_token")] + [
        r("B-0", ESHAPE, B_arg=0), r("beam-0", ESHAPE, beam_arg=0), r("V-0", ESHAPE, V_arg=0), r("ldl-below-V", ESHAPE, ldl_arg=7),
        r("temperature-0", EINVAL, temp_arg=0.0), r("temperature-nan", EINVAL, temp_arg=float("nan")), r("eos-negative", EINVAL, eos_arg=-1), r("eos-V", EINVAL, eos_arg=8),
        r("V-below-2beam+2", EUNSUPPORTED, V_arg=5, eos_arg=2), r("beam-65", EUNSUPPORTED, beam_arg=65), r("V-8193", EUNSUPPORTED, V_arg=8193, ldl_arg=8200),
        r("misaligned-logits", EALIGN, off=dict(logits=2)), r("misaligned-scores", EALIGN, off=dict(scores=2)), r("misaligned-step", EALIGN, off=dict(step=2)),
        r("misaligned-max_len", EALIGN, off=dict(max_len=1)), r("misaligned-n_live", EALIGN, off=dict(n_live=2)), r("misaligned-cand_score", EALIGN, off=dict(cand_score=2)),
        r("misaligned-cand_slot", EALIGN, off=dict(cand_slot=2)), r("misaligned-cand_token", EALIGN, off=dict(cand_token=2))]


# ---- l2s_beam_advance ---------------------------------------------------------------------------------------------------------------------------
def bd(name, hits, beam, L, d, B, dt, script, lenpen=1.0, normalize=1, max_len=None, ldpad=(8, 4), V=300, expect=OK, **kw):
    return dict(name=name, op="bd", hits=hits, beam=beam, L=L, d=d, B=B, dt=dt, script=script, lenpen=lenpen, normalize=normalize,
                max_len=max_len, ldpad=ldpad, V=V, expect=expect, **kw)


BD_SCRIPTS = ("eos-first", "eos-late", "eos-neginf", "nhyp-mid", "maxlen", "equal", "outlen", "clamp", "noroom", "inert")


def bd_cases():
    out = []
    n = 0
    for script in BD_SCRIPTS:
        beam = (2, 3, 64, 1)[n % 4] if script not in ("eos-late", "nhyp-mid", "equal", "outlen") else (3, 64, 2)[n % 3]
        L = 3 if script == "noroom" else (40, 8)[n % 2]
        d = (8, 512, 1536)[n % 3]
        lenpen, normalize = ((0.0, 1), (1.0, 1), (2.0, 1), (1.0, 0), (2.0, 0), (0.0, 0))[n % 6]
        n += 1
        for dt in DTS:
            out.append(bd(f"badv/{script}-beam{beam}-L{L}-d{d}-lp{lenpen:g}-n{normalize}-{dt}", "scripted candidates: " + script, beam, L, d, 3, dt, script,
                          lenpen=lenpen, normalize=normalize))
    for dt in DTS:
        out += [bd(f"badv/L2-{dt}", "L = 2: one step fits, the second has no room", 2, 2, 8, 3, dt, "noroom"),
                bd(f"badv/B70-{dt}", "70 clips", 3, 8, 8, 70, dt, "eos-first"),
                bd(f"badv/B1-beam1-{dt}", "one clip, one slot", 1, 8, 8, 1, dt, "eos-first"),
                bd(f"badv/tight-ld-{dt}", "lde = ldx = d", 3, 8, 512, 3, dt, "nhyp-mid", ldpad=(0, 0))]
    return out


def bd_refusals():
    base = dict(beam=2, L=8, d=8, B=2, dt="f16", script="eos-first")
    r = lambda name, expect, **kw: bd("refusals/bd-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    names = ("cand_score", "cand_slot", "cand_token", "tokens", "anc", "scores", "n_live", "finished", "parents", "hyp_tokens", "hyp_len", "hyp_score", "nhyp",
             "out_tokens", "out_len", "out_score", "max_len", "emb", "pos_table", "x", "step", "n_active")
    return [r("null-" + n, EINVAL, null=n) for n in names] + [
        r("B-0", ESHAPE, B_arg=0), r("beam-0", ESHAPE, beam_arg=0), r("L-1", ESHAPE, L_arg=1), r("V-0", ESHAPE, V_arg=0), r("d-0", ESHAPE, d_arg=0),
        r("eos-negative", ESHAPE, eos_arg=-1), r("eos-V", ESHAPE, eos_arg=300), r("lde-below-d", ESHAPE, ld_arg=dict(emb=0)), r("ldx-below-d", ESHAPE, ld_arg=dict(x=4)),
        r("dtype-f32", EUNSUPPORTED, dtype_arg=2), r("beam-65", EUNSUPPORTED, beam_arg=65), r("V-8193", EUNSUPPORTED, V_arg=8193), r("d-and-7", EUNSUPPORTED, d_arg=4),
        r("d-1544", EUNSUPPORTED, d_arg=1544, ld_arg=dict(emb=1544, x=1544)), r("L-32768", EUNSUPPORTED, L_arg=32768),
        r("lde-and-7", EALIGN, ld_arg=dict(emb=12)), r("misaligned-emb", EALIGN, off=dict(emb=8)), r("misaligned-pos_table", EALIGN, off=dict(pos_table=2)),
        r("misaligned-x", EALIGN, off=dict(x=2)), r("misaligned-tokens", EALIGN, off=dict(tokens=2)), r("misaligned-anc", EALIGN, off=dict(anc=1)),
        r("misaligned-scores", EALIGN, off=dict(scores=2)), r("misaligned-step", EALIGN, off=dict(step=2)), r("misaligned-n_active", EALIGN, off=dict(n_active=2))]


# ---- l2s_ctc_beam_search ------------------------------------------------------------------------------------------------------------------------
CTC_TOL = 1e-4                   # |score err| <= CTC_TOL max(1, |score|): the tolerance of the beam tests in tests/test_text_gpu.py


def ct(name, hits, beam, K, nbest, L, lens, kind="geo", len_mul=1, seed=0, V=None, expect=OK, **kw):
    """lens: one entry per clip (None: the launch gets lens = NULL and every clip has L frames; then `B` clips)"""
    B = kw.pop("B", len(lens) if lens is not None else 2)
    return dict(name=name, op="ct", hits=hits, beam=beam, K=K, nbest=nbest, L=L, lens=lens, kind=kind, len_mul=len_mul, seed=CT_SEED.get(name, seed),
                V=V if V is not None else K + 3, B=B, expect=expect, **kw)


CT_KINDS = ("geo", "noblank", "blankfirst", "repeat", "revival", "ties")


def ct_cases():
    # seeds: 0, 1, .. tried in order, the first at which every frame of every clip is decisive (tests/test_step_matrix_cpu.py asserts it)
    return [
        ct("ctc/beam1-K1-L1", "beam 1, K 1, one frame; lens 0, 1, L + 3", 1, 1, 1, 1, [0, 1, 4]),
        ct("ctc/beam1-K40-L50", "beam 1 is a greedy prefix walk", 1, 40, 1, 50, [50, 1, 53]),
        ct("ctc/beam2-K2-L2-nbest2", "beam 2, K 2, L 2, nbest = beam; a beam that does not exist: length 0, score FLT_MAX", 2, 2, 2, 2, [2, 1, 0, 5]),
        ct("ctc/beam2-K64-L50-len_mul2", "K 64; len_mul 2 with lens 25, 26, 1, 0 and a negative length", 2, 64, 2, 50, [25, 26, 1, 0, -3], len_mul=2),
        ct("ctc/beam30-K40-L50", "the production sizes, nbest 1", 30, 40, 1, 50, [50, 7, 53]),
        ct("ctc/beam30-K40-L50-nbest30", "the production sizes, nbest = beam", 30, 40, 30, 50, [50, 2]),
        ct("ctc/beam64-K64-L2-nbest64", "the largest beam and K, every beam returned", 64, 64, 64, 2, [2, 1, 0]),
        ct("ctc/beam64-K1-L50", "K 1: one class per frame", 64, 1, 64, 50, [50, 50]),
        ct("ctc/beam2-K2-L50-lens-null", "lens NULL: every clip has L frames", 2, 2, 2, 50, None),
        ct("ctc/noblank-beam2-K2", "blank absent from every frame's top-K", 2, 2, 2, 50, [50, 9], kind="noblank"),
        ct("ctc/noblank-beam30-K40", "blank absent from every frame's top-K at the production sizes", 30, 40, 30, 50, [50, 4], kind="noblank"),
        ct("ctc/noblank-beam1-K1", "blank absent, beam 1, K 1: the one class repeats or changes", 1, 1, 1, 50, [50, 2], kind="noblank"),
        ct("ctc/blankfirst-beam2-K40", "blank ranked first in every frame", 2, 40, 2, 50, [50, 11], kind="blankfirst"),
        ct("ctc/blankfirst-beam30-K40", "blank ranked first in every frame at the production sizes", 30, 40, 1, 50, [50, 2], kind="blankfirst"),
        ct("ctc/repeat-beam2-K2", "one class leads every frame: the c == last and merge paths", 2, 2, 2, 50, [50, 3], kind="repeat"),
        ct("ctc/repeat-beam3-K40", "one class leads every frame, K 40", 3, 40, 3, 50, [50, 12], kind="repeat"),
        ct("ctc/revival-beam3-V5", "a pruned prefix comes back and merges (inputs as tests/test_text_cpu.py REVIVAL)", 3, 5, 3, 12, [12, 12], kind="revival", V=5),
        ct("ctc/ties-beam2-K3", "bit-identical log-probabilities: the ch-then-slot order decides", 2, 3, 2, 9, [9, 4], kind="ties", V=4),
        ct("ctc/ties-beam30-K6", "bit-identical log-probabilities under a wide beam", 30, 6, 30, 2, [2, 1], kind="ties", V=7),
    ]


def ct_refusals():
    base = dict(beam=2, K=2, nbest=2, L=4, lens=[4, 2])
    r = lambda name, expect, **kw: ct("refusals/ct-" + name, "refused by its code", **{**base, **kw}, expect=expect)
    return [r("null-" + n, EINVAL, null=n) for n in ("topk_cls", "topk_lp", "work", "labels", "lengths", "scores")] + [
        r("B-0", ESHAPE, B_arg=0), r("L-0", ESHAPE, L_arg=0), r("K-0", ESHAPE, K_arg=0), r("beam-0", ESHAPE, beam_arg=0), r("nbest-0", ESHAPE, nbest_arg=0),
        r("nbest-above-beam", ESHAPE, nbest_arg=3), r("K-65", EUNSUPPORTED, K_arg=65), r("beam-65", EUNSUPPORTED, beam_arg=65, nbest_arg=65),
        r("len_mul-0", EINVAL, len_mul=0), r("len_mul-negative", EINVAL, len_mul=-1), r("beam-times-L-2pow19", EUNSUPPORTED, beam_arg=64, L_arg=8192),
        r("workspace-8-short", ESHAPE, ws_short=8), r("misaligned-workspace", ESHAPE, off=dict(work=4))]


# ---- the closed loop ----------------------------------------------------------------------------------------------------------------------------
def loop_cases():
    return [dict(name=f"loop/beam{beam}-hd{hd}-{dt}", op="loop", hits="beam_attention (self) -> logits table -> beam_select -> beam_advance on device state, "
                 "12 steps: the p & 1 halves, an ancestor table the kernels wrote, one clip finishing early", beam=beam, hd=hd, H=2, L=20, steps=12, B=3,
                 max_len=[15, 4, 9], dt=dt, V=36, seed=seed, expect=OK)
            for beam, hd, seed in ((3, 64, 0), (8, 128, 9)) for dt in DTS]     # seeds 0, 1, .. tried in order: the first whose every step is decisive


PARTS = OrderedDict([
    ("kvattn", kv_cases()),
    ("battn", ba_cases()),
    ("vocab", va_cases()),
    ("select", bs_cases()),
    ("wadv", wa_cases()),
    ("badv", bd_cases()),
    ("loop", loop_cases()),
    ("ctc", ct_cases()),
    ("refusals", kv_refusals() + ba_refusals() + va_refusals() + wa_refusals() + bs_refusals() + bd_refusals() + ct_refusals()),
])


def cases_of(part):
    return PARTS[part]


def all_cases():
    return [(p, c) for p, cs in PARTS.items() for c in cs]
