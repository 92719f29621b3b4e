"""Case generator of the waveform analysis kernels' matrix (tools/check_wave_kernels.py, tests/test_wave_matrix_*.py): l2s_stft_mel and
l2s_mel_spectrogram (csrc/melspec.hip), l2s_stft_mel_power and l2s_wav_gain (csrc/spkemb.hip), l2s_whisper_logmel
(csrc/whisper_logmel.hip), l2s_wave_stem (csrc/wavestem.hip) and the four stages of csrc/stoi.hip.

Pure Python: no torch, no GPU, no library.  A case is a dict with `op`, `name` (stable, in every failure message), `expect` (the code of
a launch that must be refused and must write nothing, 0 otherwise) and the arguments of the launch.  Clip lengths come from the frame
rule of each entry (first_n, stem_n, resample_n, stoi_n below), restated here from the kernels; tests/test_wave_matrix_cpu.py proves the
coverage.  Waveforms are described, not stored: `kinds` names what each clip holds (tools/check_wave_kernels.py::wave_data), always as
int16-representable values, so that `intype` "both" can feed the same samples as int16 PCM and as fp32 and demand the same bytes.
`ns` are the raw n_samples handed to the launch (None: a NULL pointer); they may be negative or lie past S.
These kernels read no environment switches: the parts (one child process each) split the work by run time only.
"""
from collections import OrderedDict

EINVAL, ESHAPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4      # include/lip2speech_hip.h
GUARD = 3                                  # guard rows in front of and behind every buffer
CANARY32, CANARY16 = 0x5A5A5A5A, 0x5A5A    # int32 / int16 and 16-bit float bit patterns; fp32 and fp64 buffers carry NaN
MARGIN_DB = 0.01                           # kept lists: no frame of the fp64 reference within this of the 40 dB threshold (but the exact tie)
TOL_BANDS = 4.0e-6                         # tests/test_stoi_gpu.py

# frames (outputs) per block of every tiled kernel
FT = {640: 64, 1024: 32, 400: 32}          # melspec.hip Tile640 / Tile1024, spkemb.hip / whisper_logmel.hip FrameSpan<400, 160, 32>
STEM_FT, STEM_STAT_STRIDE = 64, 256        # wavestem.hip: frames per block; frames per trip of the statistics loop
RS_OUT = 256                               # stoi.hip: resampled samples per block
FR_PER_THREAD, FR_THREADS = 2, 1024        # stoi.hip: the kept-frame scan, a wave's share is 128 frames
BT_F = 32                                  # stoi.hip: band frames per block
SC_SEG = 32                                # stoi.hip: segments per block
WHISPER_S, WHISPER_T = 480000, 3000
STOI_MAX_S, STOI_MAX_FRAMES = 419840, 2048

# worst (second fp32 evaluation order on the CPU: the dense k-ordered basis product) / (e32 of the FFT evaluation), over the cases of
# this file: `tools/check_wave_kernels.py --cpu-f32`.  F = max(4, 4 x that); kinds without a second order keep 4.
# A clip riding on a DC offset ("dc") costs the dense chain more than the FFT; it is a kind of its own so that its F does not loosen the others.
CPU_F32_WORST = {"logmel1024": 3.190, "logmel1024-dc": 7.156, "logmel640": 3.956, "logmel640-dc": 9.098, "power": 6.398, "power-dc": 3.062,
                 "whisper": 2.298}
KINDS = ("logmel640", "logmel640-dc", "logmel1024", "logmel1024-dc", "power", "power-dc", "whisper", "whisper16", "stem", "stem16", "gain", "resample",
         "bands", "scores")


def F_of(kind):
    return max(4.0, 4.0 * CPU_F32_WORST.get(kind.replace("16", ""), 1.0))


def cdiv(a, b):
    return (a + b - 1) // b


# ---- frame rules, restated from the kernels ---------------------------------------------------------------------------------------------------
def reflect_frames(n, pad, K, hop):
    """frame_dft.h: none unless the reflection is valid (n > pad) and one whole frame fits"""
    return (n + 2 * pad - K) // hop + 1 if (n > pad and n + 2 * pad >= K) else 0


def first_n(T, pad, K, hop):
    """the smallest n with at least T >= 1 frames (exactly T unless the reflection rule alone already gives more)"""
    return max(pad + 1, K - 2 * pad + (T - 1) * hop)


def clip_n(n, S):
    """what the kernels make of a raw n_samples"""
    return max(0, min(S if n is None else n, S))


def stem_frames(n):
    return (n - 10) // 5 + 1 if n >= 10 else 0


def stem_n(L0):
    return 10 + 5 * (L0 - 1) if L0 > 0 else 9


def len10k(n):
    return (5 * n + 7) // 8


def resample_n(R):
    """the smallest n with len10k(n) == R"""
    n = (8 * R) // 5 - 2
    while len10k(n) < R:
        n += 1
    assert len10k(n) == R
    return n


def stoi_frames_of(length):
    return (length - 256 - 1) // 128 + 1 if length > 256 else 0


def stoi_n(frames):
    """the smallest n (16 kHz) whose resampled clip has `frames` analysis frames"""
    return resample_n(257 + 128 * (frames - 1)) if frames > 0 else resample_n(256)


def K(op, name, expect=0, **kw):
    return dict(op=op, name=f"{op}/{name}", expect=expect, **kw)


# ---- l2s_stft_mel / l2s_mel_spectrogram ---------------------------------------------------------------------------------------------------------
MEL_PADS = {640: (320, 240, 1, 319, 0), 1024: (384, 512, 0, 383)}
MEL_HOP = {640: 160, 1024: 256}
MEL_TB = {640: (63, 64, 65, 129), 1024: (31, 32, 33, 65)}


def mel_case(name, Kf, pad, ns, kinds, T_rows=None, S=None, ldw=0, ldm=80, mag_eps=0.0, floor=1e-5, fb="prod", intype="both", twin=False, op="mel",
             expect=0, **kw):
    hop = MEL_HOP.get(Kf, Kf // 4)
    real = [n for n in (ns or []) if n is not None]
    S = S if S is not None else max(real + [1]) + 7
    frames = [reflect_frames(clip_n(n, S), pad, Kf, hop) for n in (ns if ns is not None else [S] * len(kinds))]
    T_rows = T_rows if T_rows is not None else max(frames + [1])
    return K(op, name, expect, K=Kf, hop=hop, pad=pad, ns=ns, kinds=list(kinds), T_rows=T_rows, S=S, ldw=S + ldw, ldm=ldm, mag_eps=mag_eps, floor=floor,
             fb=fb, intype=intype, twin=twin, **kw)


def mel_cases(Kf):
    out = []
    hop, ft = MEL_HOP[Kf], FT[Kf]
    for i, pad in enumerate(MEL_PADS[Kf]):
        n1 = first_n(1, pad, Kf, hop)
        tb = MEL_TB[Kf]
        ragged = [first_n(tb[0], pad, Kf, hop), first_n(tb[1], pad, Kf, hop) + hop - 1, first_n(tb[2], pad, Kf, hop), first_n(tb[3], pad, Kf, hop)]
        eps, floor = (0.0, 1e-9)[i % 2], (1e-5, 1e-10)[(i // 2) % 2]
        twin = Kf == 640 and pad == 320
        if twin:
            eps = 0.0
        # the last n without a frame, the first with one, n = pad and n = pad + 1 (the minimum valid reflection)
        out.append(mel_case(f"K{Kf}-pad{pad}-frame-rule", Kf, pad, [n1 - 1, n1, pad, pad + 1], ["noise"] * 4, ldw=3 * (i % 2), ldm=(80, 83)[i % 2],
                            mag_eps=eps, floor=floor, twin=twin))
        # T_b one frame before, on and past a tile edge and two tiles on; T_rows at, a tile past and below the clips' frames
        tmax = tb[3]
        for j, T_rows in enumerate((tmax, tmax + ft, 1, ft, ft + 1)):
            out.append(mel_case(f"K{Kf}-pad{pad}-tiles-Trows{T_rows}", Kf, pad, ragged, ["noise"] * 4, T_rows=T_rows, ldw=3 * ((i + j) % 2),
                                ldm=(80, 83)[(i + j + 1) % 2], mag_eps=eps, floor=floor, twin=twin and j < 2))
        # one-hot clips: a wrong reflection convention moves whole frames
        n5 = first_n(5, pad, Kf, hop) + 3
        hot = sorted({0, pad, n5 - 1 - pad, n5 - 1})
        out.append(mel_case(f"K{Kf}-pad{pad}-one-hot", Kf, pad, [n5] * len(hot), [f"onehot:{p}" for p in hot], ldw=3, ldm=83, mag_eps=eps, floor=1e-10,
                            twin=twin))
        # inputs: zeros, a +-0.05 signal on a 0.5 offset, int16 at -32768 / 32767
        out.append(mel_case(f"K{Kf}-pad{pad}-inputs", Kf, pad, [first_n(3, pad, Kf, hop), first_n(ft, pad, Kf, hop), first_n(ft + 2, pad, Kf, hop)],
                            ["zeros", "dc", "extreme"], mag_eps=(1e-9, 0.0)[i % 2], floor=floor))
    pad = MEL_PADS[Kf][0]
    n65 = first_n(FT[Kf] + 1, pad, Kf, hop)
    out.append(mel_case(f"K{Kf}-pad{pad}-ns-null", Kf, pad, None, ["noise"] * 2, S=n65, ldw=3, ldm=83, twin=Kf == 640))
    out.append(mel_case(f"K{Kf}-pad{pad}-ns-past-S-zero-negative", Kf, pad, [n65 + 5, 0, -3, n65], ["noise"] * 4, S=n65, twin=Kf == 640))
    for p in (MEL_PADS[Kf][0], 0):
        out.append(mel_case(f"K{Kf}-pad{p}-edge-filterbank", Kf, p, [first_n(2, p, Kf, hop), first_n(FT[Kf] + 1, p, Kf, hop)], ["noise", "extreme"], fb="edge",
                            ldw=3, ldm=83, mag_eps=1e-9))
    n1 = first_n(1, pad, Kf, hop)
    out.append(mel_case(f"K{Kf}-pad{pad}-B70-shortest", Kf, pad, [n1 - (b % 3 == 2) for b in range(70)], ["noise"] * 70, S=n1, intype=("i16", "f32")[Kf == 1024]))
    return out


def melspec_twin(c):
    """the l2s_mel_spectrogram case of a 640 / pad 320 / mag_eps 0 l2s_stft_mel case: the same arguments, the same bytes"""
    assert c["twin"] and (c["K"], c["pad"], c["mag_eps"]) == (640, 320, 0.0)
    d = dict(c, op="melspec", name=c["name"].replace("mel/", "melspec/"), twin=False)
    return d


# ---- l2s_stft_mel_power ----------------------------------------------------------------------------------------------------------------------------
POWER_PADS = (200, 120, 0, 199)
POWER_TB = (31, 32, 33, 65)


def power_case(name, pad, ns, kinds, nv=None, scale=None, T_rows=None, S=None, ldw=0, ldm=40, intype="both", expect=0, **kw):
    real = [n for n in (ns or [])]
    S = S if S is not None else max(real + [1]) + 7
    frames = [reflect_frames(S if n is None else n, pad, 400, 160) for n in (ns if ns is not None else [None] * len(kinds))]
    T_rows = T_rows if T_rows is not None else max(frames + [1])
    return K("power", name, expect, pad=pad, ns=ns, nv=nv, scale=scale, kinds=list(kinds), T_rows=T_rows, S=S, ldw=S + ldw, ldm=ldm, intype=intype, **kw)


def power_cases():
    out = []
    for i, pad in enumerate(POWER_PADS):
        n1 = first_n(1, pad, 400, 160)
        ragged = [first_n(POWER_TB[0], pad, 400, 160), first_n(POWER_TB[1], pad, 400, 160) + 159, first_n(POWER_TB[2], pad, 400, 160),
                  first_n(POWER_TB[3], pad, 400, 160)]
        out.append(power_case(f"pad{pad}-frame-rule", pad, [n1 - 1, n1, pad, pad + 1], ["noise"] * 4, ldw=3 * (i % 2), ldm=(40, 43)[i % 2],
                              scale=None if i % 2 else [1.0, 3.25, 0.5, 2.0]))
        for j, T_rows in enumerate((65, 97, 1, 32, 33)):
            out.append(power_case(f"pad{pad}-tiles-Trows{T_rows}", pad, ragged, ["noise"] * 4, T_rows=T_rows, ldw=3 * ((i + j) % 2), ldm=(40, 43)[(i + j + 1) % 2],
                                  scale=[1.0, 1.0, 3.25, 0.5] if (i + j) % 2 else None))
        n5 = first_n(5, pad, 400, 160) + 3
        hot = sorted({0, pad, n5 - 1 - pad, n5 - 1})
        out.append(power_case(f"pad{pad}-one-hot", pad, [n5] * len(hot), [f"onehot:{p}" for p in hot], ldw=3, ldm=43))
        out.append(power_case(f"pad{pad}-inputs", pad, [first_n(3, pad, 400, 160), first_n(32, pad, 400, 160), first_n(34, pad, 400, 160)],
                              ["zeros", "dc", "extreme"]))
        # the analysis length past the buffer: n_valid NULL (the buffer), = n_samples (clamped to it), below it, and 0; the frames
        # behind the real samples are made of zeros only
        S = first_n(33, pad, 400, 160)
        na = S + 160 * 7 + 5
        out.append(power_case(f"pad{pad}-analysis-past-S-valid-null", pad, [na, na - 160, S, S + 1], ["noise"] * 4, S=S, ldw=3, ldm=43))
        out.append(power_case(f"pad{pad}-analysis-past-S-valid-mixed", pad, [na, na, na, S + 1], ["noise"] * 4, nv=[na, S - 901, 0, S + 1], S=S,
                              scale=[2.0, 1.0, 1.0, 0.25]))
    out.append(power_case("pad200-ns-null", 200, None, ["noise"] * 2, S=first_n(33, 200, 400, 160), ldw=3, ldm=43))
    out.append(power_case("pad200-ns-zero-negative", 200, [0, -3, 801], ["noise"] * 3, nv=[5, 7, -2], S=801))
    n1 = first_n(1, 200, 400, 160)
    out.append(power_case("pad200-B70-shortest", 200, [n1 - (b % 3 == 2) for b in range(70)], ["noise"] * 70, S=n1, intype="i16"))
    return out


# ---- l2s_whisper_logmel -------------------------------------------------------------------------------------------------------------------------------
def whisper_case(name, ns, kinds, S, ld=80, f32out=True, dt="f16", ldw=0, intype="both", expect=0, **kw):
    return K("whisper", name, expect, ns=ns, kinds=list(kinds), S=S, ldw=S + ldw, ld=ld, f32out=f32out, dt=dt, intype=intype, **kw)


def whisper_cases():
    out = []
    edge = 160 * FT[400] - 200                            # the first sample of frame 32: one tile is frames 0 .. 31
    out.append(whisper_case("n0-1-200-201", [0, 1, 200, 201], ["noise"] * 4, S=208, ld=88, dt="f16", ldw=3))
    out.append(whisper_case("first-tile-edge", [edge, edge + 1], ["noise"] * 2, S=edge + 9, ld=96, dt="bf16", f32out=False))
    out.append(whisper_case("first-tile-edge-f32out", [edge, edge + 1], ["noise"] * 2, S=edge + 9, ld=80, dt="bf16", ldw=3))
    out.append(whisper_case("n-equals-S-480000", None, ["noise"], S=WHISPER_S, ld=88, dt="bf16", intype="i16"))
    out.append(whisper_case("ns-past-S-zero-negative", [4000 + 5, 0, -3], ["noise"] * 3, S=4000, ld=80, dt="f16", f32out=False))
    # the loudest frame in tile 0, in a middle tile and in frame 2999 (the ragged last tile of 24 frames), each clip at its own level,
    # a stretch 60 dB lower, digital silence elsewhere: the clamp 8 below the maximum binds in each clip at its own level
    for dt, ld, f32out in (("f16", 96, True), ("bf16", 80, False)):
        out.append(whisper_case(f"loudest-tile-0-mid-last-{dt}-ld{ld}", None, ["loud:0:20000", "loud:1500:8000", "loud:2999:3200"], S=WHISPER_S, ld=ld, dt=dt,
                                f32out=f32out, intype="f32" if dt == "f16" else "i16"))
    out.append(whisper_case("B70-shortest", [b % 2 for b in range(70)], ["const"] * 70, S=1, ld=80, dt="f16", f32out=False, intype="i16"))
    return out


# ---- l2s_wave_stem and l2s_wav_gain ------------------------------------------------------------------------------------------------------------------
def stem_case(name, ns, kinds, dt, S=None, T_rows=0, ldo=512, ldw=0, eps=1e-5, intype="both", expect=0, **kw):
    S = S if S is not None else max([n for n in ns] + [1]) + 4
    return K("stem", f"{name}-{dt}", expect, ns=ns, kinds=list(kinds), S=S, ldw=S + ldw, ldo=ldo, T_rows=stem_frames(S) + T_rows, dt=dt, eps=eps, C=512,
             intype=intype, **kw)


def stem_gain_cases():
    out = []
    for i, dt in enumerate(("f32", "f16", "bf16")):
        pad, eps = i % 2, (1e-5, 1e-3)[i % 2]
        out.append(stem_case("n9-10-14-15", [9, 10, 14, 15], ["noise"] * 4, dt, ldo=512 + 2 * pad, ldw=3 * pad, eps=eps))
        out.append(stem_case("frames-64-65-257", [stem_n(64), stem_n(65) + 4, stem_n(257), stem_n(1)], ["noise", "noise", "noise", "noise"], dt,
                             T_rows=64 * (1 - pad), ldo=514 - 2 * pad, ldw=3 - 3 * pad, eps=(1e-3, 1e-5)[i % 2]))
        out.append(stem_case("constant-one-frame-dc", [stem_n(64), stem_n(1) + 2, stem_n(66)], ["const", "noise", "dc"], dt, T_rows=64 * pad, ldo=512 + 2 * pad,
                             eps=eps))
        out.append(stem_case("ns-null", None, ["noise"] * 2, dt, S=stem_n(65), ldo=514, ldw=3))
        out.append(stem_case("ns-past-S-zero-negative", [stem_n(3) + 5, 0, -3], ["noise"] * 3, dt, S=stem_n(3)))
    out.append(stem_case("B70-shortest", [10 - (b % 3 == 2) for b in range(70)], ["noise"] * 70, "f16", S=10, intype="i16"))
    # gain: no samples, zeros, above the target, 0.5 dB either side of it, a 30 000-sample clip
    g = dict(S=4000, target=-30.0)
    out.append(K("gain", "n0-zeros-loud", ns=[0, 2000, 3000, -3], kinds=["noise", "zeros", "level:+6", "noise"], ldw=g["S"] + 3, intype="both", **g))
    out.append(K("gain", "half-a-dB-either-side", ns=[4000, 3999], kinds=["level:+0.5", "level:-0.5"], ldw=g["S"], intype="both", **g))
    out.append(K("gain", "ns-null", ns=None, kinds=["level:-20", "level:-3"], ldw=g["S"] + 3, intype="both", **g))
    out.append(K("gain", "n30000", ns=[30000, 29999 + 7], kinds=["level:-12", "level:-25"], S=30000, ldw=30000, target=-30.0, intype="both"))
    out.append(K("gain", "B70-shortest", ns=[b % 4 for b in range(70)], kinds=["level:-12"] * 70, S=3, ldw=4, target=-30.0, intype="i16"))
    return out


# ---- STOI ------------------------------------------------------------------------------------------------------------------------------------------------
def stoi_cases():
    out = []
    # resample: block edges of 256 outputs, R past ceil(5 S / 8), one-hot inputs (the output is a column of the polyphase taps)
    ns = [0, 1, 8, resample_n(255), resample_n(256), resample_n(257), resample_n(513)]
    S = max(ns) + 5
    for i, (R, ldo) in enumerate(((len10k(S), 0), (len10k(S) + 300, 5))):
        out.append(K("resample", f"block-edges-R{'+300' if i else ''}", ns=ns, kinds=["noise"] * len(ns), S=S, ldw=S + 3 * i, R=R, ldo=R + ldo, intype="both"))
    n = resample_n(257) + 2
    out.append(K("resample", "one-hot", ns=[n, n, n], kinds=["onehot:0", f"onehot:{n - 1}", "onehot:200"], S=n, ldw=n + 3, R=len10k(n), ldo=len10k(n) + 3,
                 intype="both"))
    out.append(K("resample", "ns-null", ns=None, kinds=["noise"] * 2, S=resample_n(257), ldw=resample_n(257), R=257, ldo=257, intype="both"))
    out.append(K("resample", "B70-shortest", ns=[b % 2 for b in range(70)], kinds=["noise"] * 70, S=1, ldw=4, R=1, ldo=4, intype="i16"))
    # kept frames, x fed directly: a wave's share of the scan is 128 frames, the block's 2048
    fr = (0, 1, 2, 127, 128, 129)
    S = stoi_n(129) + 3
    out.append(K("frames", "count-0-1-2-127-128-129", ns=[stoi_n(f) for f in fr], kinds=["gaps"] * 6, S=S, ldx=len10k(S) + 5, ldk=stoi_frames_of(len10k(S)) + 3))
    fr = (1023, 1024, 1025)
    S = stoi_n(1025)
    out.append(K("frames", "count-1023-1024-1025", ns=[stoi_n(f) for f in fr], kinds=["gaps"] * 3, S=S, ldx=len10k(S), ldk=stoi_frames_of(len10k(S))))
    out.append(K("frames", "count-2048-zeros-129", ns=[STOI_MAX_S, stoi_n(129)], kinds=["gaps", "zeros"], S=STOI_MAX_S, ldx=len10k(STOI_MAX_S), ldk=2048 + 5))
    out.append(K("frames", "ns-past-S-negative", ns=[stoi_n(40) + 9, -3, stoi_n(40)], kinds=["gaps"] * 3, S=stoi_n(40), ldx=len10k(stoi_n(40)) + 5,
                 ldk=40))
    # the one exact tie: a window of ones, one sample of 99 x 2^-52 (clip 0) / 98 x 2^-52 (clip 1) in an otherwise silent clip.  Clip 0: the
    # silent frames sit exactly ON the threshold, (99 + 1) 2^-52 / 100 = 2^-52, and `>` drops them; clip 1: just above it, all kept.  Every
    # quantity is exact in fp32 and fp64, the reference is the header's rule in rational arithmetic - the 0.01 dB margin cannot apply
    out.append(K("frames", "threshold-tie-exact", ns=[stoi_n(12), stoi_n(12)], kinds=["tie:99", "tie:98"], S=stoi_n(12), ldx=len10k(stoi_n(12)) + 5, ldk=12,
                 window="ones"))
    out.append(K("frames", "B70-shortest", ns=[stoi_n(1) - (b % 3 == 2) for b in range(70)], kinds=["gaps"] * 70, S=stoi_n(1), ldx=len10k(stoi_n(1)), ldk=1))
    # bands: hand-made kept lists
    S = stoi_n(80)
    nf = 80
    nk = (0, 1, 2, 32, 33, 34, 66)
    for i, (ldk, ldf, ldx) in enumerate(((nf, nf - 1, 0), (nf + 3, nf + 20, 5))):
        out.append(K("bands", f"n_kept-0-1-2-32-33-34-66{'-padded' if i else ''}", ns=[S - 13 * b for b in range(len(nk))], n_kept=list(nk), kept="gaps", S=S,
                     ldx=len10k(S) + ldx, ldk=ldk, ldf=ldf))
    out.append(K("bands", "index-outside-the-clip", ns=[S, stoi_n(40), S], n_kept=[34, 34, 10], kept="outside", S=S, ldx=len10k(S) + 5, ldk=nf + 3, ldf=nf - 1))
    out.append(K("bands", "n_kept-above-ldk", ns=[S, stoi_n(40)], n_kept=[nf + 9, 1 << 20], kept="all", S=S, ldx=len10k(S), ldk=nf, ldf=nf + 5))
    out.append(K("bands", "B70-shortest", ns=[stoi_n(2)] * 70, n_kept=[2 - (b % 3 == 2) for b in range(70)], kept="all", S=stoi_n(2), ldx=len10k(stoi_n(2)), ldk=2,
                 ldf=1))
    # scores
    fb = (0, 29, 30, 31, 64)
    for i, (ldf, lds) in enumerate(((64, 35), (64 + 5, 64 + 5 - 29 + 3))):
        out.append(K("scores", f"F-0-29-30-31-64{'-padded' if i else ''}", n_kept=[f + 1 if f else 0 for f in fb], kinds=["rand"] * 5, ldf=ldf, lds=lds))
    out.append(K("scores", "same-negated-zero-band", n_kept=[65, 65, 62, 31], kinds=["same", "neg", "zeroband", "same"], ldf=66, lds=37))
    out.append(K("scores", "n_kept-above-ldf", n_kept=[200, 1 << 20], kinds=["rand", "rand"], ldf=40, lds=11))
    out.append(K("scores", "B70-shortest", n_kept=[31 - (b % 3 == 2) for b in range(70)], kinds=["rand"] * 70, ldf=30, lds=1))
    return out


# ---- refusals: the first value past every documented limit and alignment rule, per launcher in the order of its checks -------------------------------
def refusal_cases():
    out = []

    def mel(name, code, Kf=640, op="mel", **kw):
        pad = kw.pop("pad", Kf // 2 if Kf in (640, 1024) else 0)
        n = first_n(3, min(max(pad, 0), Kf // 2), Kf, max(Kf // 4, 1))
        out.append(mel_case(f"refused-{name}", Kf, pad, [n, n - 1], ["noise"] * 2, S=n, T_rows=4, intype="i16", op=op, expect=code, **kw))

    for op in ("mel", "melspec"):
        for operand in ("wav", "basis", "fb", "fb_range", "mel"):
            mel(f"null-{operand}", EINVAL, op=op, null=operand)
        mel("ldw-below-S", ESHAPE, op=op, ldw=-1)
        mel("ldm-below-n_mels", ESHAPE, op=op, ldm=79)
        mel("n_fft-512", EUNSUPPORTED, Kf=512, op=op)
        mel("hop-161", EUNSUPPORTED, op=op, hop_arg=161)
        mel("n_mels-81", EUNSUPPORTED, op=op, n_mels=81, ldm=83)
        mel("basis-off-by-4-bytes", EALIGN, op=op, off={"basis": 4})
    mel("n_fft-1024", EUNSUPPORTED, Kf=1024, op="melspec")            # l2s_mel_spectrogram serves (640, 160) alone
    for Kf in (640, 1024):
        mel(f"K{Kf}-pad-minus-1", EUNSUPPORTED, Kf=Kf, pad=-1)
        mel(f"K{Kf}-pad-past-half", EUNSUPPORTED, Kf=Kf, pad=Kf // 2 + 1)
        mel(f"K{Kf}-mag_eps-negative", EUNSUPPORTED, Kf=Kf, mag_eps=-1e-9)
        mel(f"K{Kf}-mag_eps-nan", EUNSUPPORTED, Kf=Kf, mag_eps=float("nan"))

    def power(name, code, **kw):
        n = first_n(3, 200, 400, 160)
        out.append(power_case(f"refused-{name}", kw.pop("pad", 200), [n, n - 1], ["noise"] * 2, S=n, T_rows=4, intype="i16", expect=code, **kw))

    for operand in ("wav", "basis", "fb", "fb_range", "mel"):
        power(f"null-{operand}", EINVAL, null=operand)
    power("ldw-below-S", ESHAPE, ldw=-1)
    power("ldm-below-n_mels", ESHAPE, ldm=39)
    power("n_fft-640", EUNSUPPORTED, n_fft=640)
    power("hop-161", EUNSUPPORTED, hop_arg=161)
    power("n_mels-80", EUNSUPPORTED, n_mels=80, ldm=83)
    power("pad-minus-1", EUNSUPPORTED, pad=-1)
    power("pad-201", EUNSUPPORTED, pad=201)

    def whisper(name, code, **kw):
        args = dict(ns=[100, 50], kinds=["noise"] * 2, S=100, ld=80, dt="f16", intype="i16", f32out=True)
        args.update(kw)
        out.append(whisper_case(f"refused-{name}", expect=code, **args))

    for operand in ("wav", "basis", "fb", "fb_range", "work", "out"):
        whisper(f"null-{operand}", EINVAL, null=operand)
    whisper("ldw-below-S", ESHAPE, ldw=-1)
    whisper("ld-72", ESHAPE, ld=72)
    whisper("S-480001", EUNSUPPORTED, S=WHISPER_S + 1, ns=[100, 50])
    whisper("dtype-f32", EUNSUPPORTED, dt="f32")
    whisper("ld-84-no-multiple-of-8", EALIGN, ld=84)
    whisper("work-off-by-4-bytes", EALIGN, off={"work": 4})

    def stem(name, code, **kw):
        args = dict(ns=[30, 12], kinds=["noise"] * 2, dt="f16", S=40, intype="i16")
        args.update(kw)
        out.append(stem_case(f"refused-{name}", expect=code, **args))

    for operand in ("wav", "w", "gamma", "beta", "out", "work"):
        stem(f"null-{operand}", EINVAL, null=operand)
    stem("dtype-3", EINVAL, dtype_arg=3)
    stem("ldw-below-S", ESHAPE, ldw=-1)
    stem("ldo-below-C", ESHAPE, ldo=510)
    stem("T_rows-below-frames-of-S", ESHAPE, T_rows=-1)
    stem("C-256", EUNSUPPORTED, C_arg=256)
    stem("workspace-one-byte-short", ESHAPE, ws_short=1)
    stem("ldo-odd", EALIGN, ldo=513)

    out.append(K("gain", "refused-null-wav", EINVAL, ns=[10], kinds=["noise"], S=16, ldw=16, target=-30.0, intype="i16", null="wav"))
    out.append(K("gain", "refused-null-gain", EINVAL, ns=[10], kinds=["noise"], S=16, ldw=16, target=-30.0, intype="i16", null="gain"))
    out.append(K("gain", "refused-ldw-below-S", ESHAPE, ns=[10], kinds=["noise"], S=16, ldw=15, target=-30.0, intype="i16"))

    def resample(name, code, **kw):
        args = dict(ns=[700, 650], kinds=["noise"] * 2, S=700, ldw=700, R=len10k(700), ldo=len10k(700), intype="i16")
        args.update(kw)
        out.append(K("resample", f"refused-{name}", code, **args))

    for operand in ("wav", "taps", "out"):
        resample(f"null-{operand}", EINVAL, null=operand)
    resample("S-419841", EUNSUPPORTED, S=STOI_MAX_S + 1, ldw=STOI_MAX_S + 1, R=len10k(STOI_MAX_S + 1), ldo=len10k(STOI_MAX_S + 1))
    resample("ldw-below-S", ESHAPE, ldw=699)
    resample("R-below-len10k-S", ESHAPE, R=len10k(700) - 1)
    resample("ldo-below-R", ESHAPE, ldo=len10k(700) - 1)

    def frames(name, code, **kw):
        S = stoi_n(5)
        args = dict(ns=[S, S - 9], kinds=["gaps"] * 2, S=S, ldx=len10k(S), ldk=5)
        args.update(kw)
        out.append(K("frames", f"refused-{name}", code, **args))

    for operand in ("x", "window", "kept", "n_kept"):
        frames(f"null-{operand}", EINVAL, null=operand)
    frames("S-419841", EUNSUPPORTED, S=STOI_MAX_S + 1, ns=[100, 50], ldx=len10k(STOI_MAX_S + 1), ldk=2048)
    frames("ldx-below-len10k-S", ESHAPE, ldx=len10k(stoi_n(5)) - 1)
    frames("ldk-below-the-frame-count", ESHAPE, ldk=4)

    def bands(name, code, **kw):
        S = stoi_n(5)
        args = dict(ns=[S, S - 9], n_kept=[5, 3], kept="all", S=S, ldx=len10k(S), ldk=5, ldf=4)
        args.update(kw)
        out.append(K("bands", f"refused-{name}", code, **args))

    for operand in ("x", "y", "kept", "n_kept", "window", "basis", "band_edges", "bands"):
        bands(f"null-{operand}", EINVAL, null=operand)
    bands("S-419841", EUNSUPPORTED, S=STOI_MAX_S + 1, ns=[100, 50], ldx=len10k(STOI_MAX_S + 1), ldk=2048, ldf=2047)
    bands("ldf-2049", EUNSUPPORTED, ldf=2049)
    bands("ldx-below-len10k-S", ESHAPE, ldx=len10k(stoi_n(5)) - 1)
    bands("ldk-below-the-frame-count", ESHAPE, ldk=4)
    bands("ldf-below-frames-minus-1", ESHAPE, ldf=3)
    bands("basis-off-by-4-bytes", EALIGN, off={"basis": 4})

    def scores(name, code, **kw):
        args = dict(n_kept=[31, 40], kinds=["rand"] * 2, ldf=40, lds=11)
        args.update(kw)
        out.append(K("scores", f"refused-{name}", code, **args))

    for operand in ("bands", "n_kept", "seg", "stoi", "estoi", "n_segments"):
        scores(f"null-{operand}", EINVAL, null=operand)
    scores("ldf-2049", EUNSUPPORTED, ldf=2049, lds=2049 - 29)
    scores("lds-below-ldf-minus-29", ESHAPE, lds=10)
    scores("seg-off-by-4-bytes", EALIGN, off={"seg": 4})
    return out


def mel640_cases():
    base = mel_cases(640)
    return base + [melspec_twin(c) for c in base if c["twin"]]


PARTS = OrderedDict([("mel640", mel640_cases), ("mel1024", lambda: mel_cases(1024)), ("power", power_cases), ("whisper", whisper_cases),
                     ("stem-gain", stem_gain_cases), ("stoi", stoi_cases), ("refusals", refusal_cases)])


def cases_of(part):
    return PARTS[part]()


def all_cases():
    return [(p, c) for p in PARTS for c in cases_of(p)]
