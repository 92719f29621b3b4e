"""l2s_logfbank on the device against the float64 restatement of the audio features (tests/_logfbank_reference.py).  One batch of
nine clips - 1, 399, 400, 401, 561 and 4000 samples, 10 640 and 10 801 samples (65 and 67 frames: across the 64-frame tile) and
digital silence - over three signals (noise of sigma 3000, a 440 Hz tone of amplitude 8000 plus noise of sigma 3, a random walk),
as int16 and as the same values in float.  The gate is the rule of tests/test_mel_gpu.py: the device's largest error against
float64 on a clip is at most 4 x the error of the float32 restatement (dense DFT products, the same arithmetic class) on that
clip; a 16-bit output adds half an ulp of the output type at the value.

MEASURED holds what an MI355X gave (MEASURE lines of this file); no bound is derived from it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import _lib, audio, ops  # noqa: E402
from tests import _logfbank_reference as R  # noqa: E402

CLIPS = [("noise", 1), ("tone", 399), ("walk", 400), ("noise", 401), ("tone", 561), ("walk", 4000), ("noise", 10640), ("tone", 10801),
         ("zero", 2000)]
SILENT = 8
S = max(n for _, n in CLIPS)
# largest |device - float64| over the batch and the float32 restatement's own error on the same clip (for the 16-bit outputs: what is
# left beyond half an ulp); the tightest clip against its 4 x gate is the one-sample clip in raw mode, 1.79e-6 against 2.35e-6
MEASURED = {"raw": (1.658e-5, 1.610e-5), "model_f32": (5.631e-6, 5.869e-6), "model_f16": (7.94e-7, 3.681e-6), "model_bf16": (4.69e-7, 5.869e-6)}


@pytest.fixture(scope="module")
def batch():
    """(int16 [B, S] zero padded, lengths, the clips) - made once and left unchanged."""
    clips = [R.signal(k, n, 100 + i) for i, (k, n) in enumerate(CLIPS)]
    pcm = np.zeros((len(clips), S), dtype=np.int16)
    for i, c in enumerate(clips):
        pcm[i, :len(c)] = c
    return pcm, [len(c) for c in clips], clips


@pytest.fixture(scope="module")
def refs(batch):
    """Per clip: float64 and float32 restatements, raw (stack 1, no norm) and model (stack 4, normalised) - computed once."""
    out = []
    for c in batch[2]:
        out.append({"raw64": R.logfbank(c), "raw32": R.logfbank(c, np.float32).astype(np.float64),
                    "model64": R.audio_rows(c, 4), "model32": R.audio_rows(c, 4, None, True, np.float32).astype(np.float64)})
    return out


def _run(pcm, lens, stack, normalize, dtype=torch.float32, n_rows=None, T_rows=None, as_float=False):
    t = audio.LogFbank(stack, normalize)
    wav = torch.from_numpy(pcm).cuda()
    if as_float:
        wav = wav.float()
    return t.rows(wav, lens, n_rows, T_rows=T_rows, dtype=dtype).float().cpu().numpy().astype(np.float64)


def test_raw_mode_against_float64(batch, refs):
    pcm, lens, _ = batch
    got = _run(pcm, lens, 1, False)
    assert got.shape == (len(lens), R.n_frames(S), 26)
    worst = (0.0, 0.0)
    for b, r in enumerate(refs):
        nf = r["raw64"].shape[0]
        err, own = np.abs(got[b, :nf] - r["raw64"]).max(), np.abs(r["raw32"] - r["raw64"]).max()
        print(f"MEASURE raw clip{b} {CLIPS[b]} frames={nf} err={err:.3e} f32_restatement={own:.3e} gate={4 * own:.3e}")
        worst = max(worst, (err, own))
        assert (got[b, nf:] == 0).all()
        assert err <= 4.0 * own, (b, err, own)
    print(f"MEASURE raw worst {worst[0]:.3e} {worst[1]:.3e}")
    nf = refs[SILENT]["raw64"].shape[0]
    assert (got[SILENT, :nf].astype(np.float32) == np.float32(np.log(2.220446049250313e-16))).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_model_mode_against_float64(batch, refs, dtype):
    pcm, lens, _ = batch
    got = _run(pcm, lens, 4, True, dtype)
    assert got.shape == (len(lens), -(-R.n_frames(S) // 4), 104)
    ulp = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]      # half an ulp, relative to the binade
    worst = (0.0, 0.0)
    for b, r in enumerate(refs):
        ref, nr = r["model64"], r["model64"].shape[0]
        own = np.abs(r["model32"] - ref).max()
        mag = np.maximum(np.maximum(np.abs(ref), np.abs(got[b, :nr])), 2.0 ** -14)
        half = ulp * 2.0 ** np.floor(np.log2(mag))       # half an ulp of the output type at the value
        over = (np.abs(got[b, :nr] - ref) - half).max()
        print(f"MEASURE model_{dtype} clip{b} {CLIPS[b]} rows={nr} err_less_half_ulp={over:.3e} f32_restatement={own:.3e} gate={4 * own:.3e}")
        worst = max(worst, (over, own))
        assert (got[b, nr:] == 0).all()
        assert over <= 4.0 * own, (b, over, own)
        if R.n_frames(lens[b]) % 4:                      # the frames the last row lacks are 0.0 before the norm, not log(eps)
            assert (np.abs(got[b, nr - 1] - ref[-1]) - half[-1]).max() <= 4.0 * own
            st = R.stacker(r["raw64"], 4)
            st[-1, 26 * (R.n_frames(lens[b]) % 4):] = np.log(R.EPS)                          # what padding BEFORE the log would give
            assert np.abs(got[b, nr - 1] - R.layer_norm(st)[-1]).max() > 0.1
    print(f"MEASURE model_{dtype} worst {worst[0]:.3e} {worst[1]:.3e}")


def test_n_rows_pads_and_trims(batch):
    pcm, lens, _ = batch
    own = [audio.logfbank_rows(n, 4) for n in lens]      # 1 1 1 1 1 6 17 17 3
    plain = _run(pcm, lens, 4, True)
    n_rows = [3, 1, 2, 1, 1, 4, 20, 16, 5]               # larger, equal and smaller than the audio's own
    T = 22
    wav = torch.from_numpy(pcm).cuda()
    out = torch.full((len(lens), T, 104), float("nan"), device="cuda")
    audio.LogFbank(4, True).rows(wav, lens, n_rows, out=out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()                        # every element of the buffer is written
    for b, (a, v) in enumerate(zip(own, n_rows)):
        keep = min(a, v)
        assert np.array_equal(got[b, :keep], plain[b, :keep].astype(np.float32)), b        # kept rows: bit-equal to the unaligned run
        assert (got[b, keep:] == 0).all(), b             # padded rows and everything past n_rows[b]
    dev_rows = torch.tensor(n_rows, dtype=torch.int32).cuda()                               # the same from device lengths
    out2 = torch.full_like(out, float("nan"))
    audio.LogFbank(4, True).rows(wav, torch.tensor(lens, dtype=torch.int32).cuda(), dev_rows, out=out2)
    assert torch.equal(out, out2)


def test_invariance_alone_in_batch_int16_float_and_graph(batch):
    pcm, lens, clips = batch
    for stack, norm in ((1, False), (4, True)):
        both = _run(pcm, lens, stack, norm)
        assert np.array_equal(both, _run(pcm, lens, stack, norm, as_float=True))             # int16 and float input: the same bits
        for b, c in enumerate(clips):
            alone = _run(c[None], [len(c)], stack, norm)
            assert np.array_equal(alone[0], both[b, :alone.shape[1]]), (stack, b)           # a clip alone: the same bits
    t = audio.LogFbank(4, True)
    x = torch.from_numpy(pcm).cuda()
    n = torch.tensor(lens, dtype=torch.int32).cuda()
    basis, fb, rng = t.tables(x.device)
    T = audio.logfbank_rows(S, 4)
    eager = torch.from_numpy(_run(pcm, lens, 4, True)).float().cuda()
    out = torch.empty_like(eager)
    kw = dict(B=len(lens), S=S, T_rows=T, stack=4, normalize=True, n_samples=n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.logfbank(x, out, basis, fb, rng, **kw)       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.logfbank(x, out, basis, fb, rng, **kw)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    rev = np.ascontiguousarray(pcm[::-1])                # new audio in the captured buffer, same graph
    x.copy_(torch.from_numpy(rev))
    n.copy_(torch.tensor(lens[::-1], dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), _run(rev, lens[::-1], 4, True))


def test_argument_checks_launch_nothing(batch):
    pcm, lens, _ = batch
    t = audio.LogFbank(4, True)
    x = torch.from_numpy(pcm).cuda()
    basis, fb, rng = t.tables(x.device)
    T = audio.logfbank_rows(S, 4)
    out = torch.full((len(lens), T, 128), 7.0, device="cuda")
    kw = dict(B=len(lens), S=S, T_rows=T)
    with pytest.raises(ops.L2SError, match="L2S_ESHAPE"):
        ops.logfbank(x, out, basis, fb, rng, stack=4, ldo=100, **kw)                         # a leading dimension below 104
    with pytest.raises(ops.L2SError, match="L2S_ESHAPE"):
        ops.logfbank(x, out, basis, fb, rng, stack=4, ldo=128, ldw=S - 1, **kw)
    off = torch.zeros(400 * 512 + 1, device="cuda")[1:]                                      # 4 bytes off a 16-byte boundary
    with pytest.raises(ops.L2SError, match="L2S_EALIGN"):
        ops.logfbank(x, out, off, fb, rng, stack=4, ldo=128, **kw)
    with pytest.raises(ops.L2SError, match="L2S_EUNSUPPORTED"):
        ops.logfbank(x, out, basis, fb, rng, stack=3, ldo=128, **kw)
    lib = _lib.load()
    args = [x.data_ptr(), 1, S, None, len(lens), S, basis.data_ptr(), fb.data_ptr(), rng.data_ptr(), None, out.data_ptr(), ops.F32, 128, T]
    assert lib.l2s_logfbank(*args, 4, 1, None) == 0
    torch.cuda.synchronize()
    assert not (out[:, :, :104] == 7.0).all() and (out[:, :, 104:] == 7.0).all()            # columns past 26 * stack are not written
    out.fill_(7.0)
    for bad, code in (((args[:12] + [100, T]), -2), ((args[:6] + [basis.data_ptr() + 4] + args[7:]), -3), (None, -4), ((args[:6] + [None] + args[7:]), -1)):
        rc = lib.l2s_logfbank(*(bad if bad is not None else args), 3 if bad is None else 4, 1, None)
        assert rc == code, (rc, code)
    torch.cuda.synchronize()
    assert (out == 7.0).all()                            # none of the refused calls launched anything
