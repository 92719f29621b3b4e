"""The two kernels of the speech-unit path on the device, each against float64 (tests/_units_reference.py):
l2s_wave_stem (csrc/wavestem.hip) and l2s_kmeans_assign (csrc/kmeans.hip)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import ops  # noqa: E402
from tests import _units_reference as R  # noqa: E402

SAMPLES = (400, 3207, 8000)          # 79, 640 and 1599 frames: one tile, ten tiles, a partial last tile (64-frame tiles)
DC_CLIP = 1
# fp32 output against float64, max abs error over a clip's [L0, 512] values (normalised values reach +-4.1): measured
# 6.8e-7 / 6.9e-7 (the DC-offset clip) / 8.4e-7 for the three clips; the gate is 4 x the largest.  The same
# factor bounds the DC-offset clip against the zero-mean ones.
F32_MEASURED = 8.4e-7
F32_GATE = 4.0 * F32_MEASURED
# 16-bit outputs: two ulps of the type at the normalised value's scale, ulp(v) = eps * max(1, |v|) (one rounding is half of one)
EPS16 = {ops.F16: 2.0 ** -10, ops.BF16: 2.0 ** -7}


@pytest.fixture(scope="module")
def stem_case():
    sd = R.init_weights(0, layers=0)
    rng = np.random.default_rng(7)
    clips = []
    for b, n in enumerate(SAMPLES):
        t = np.arange(n)
        x = 0.3 * np.sin(2 * np.pi * 220.0 * t / 16000.0) + 0.2 * rng.uniform(-1, 1, n)
        if b == DC_CLIP:
            x = 0.5 + 0.05 * rng.uniform(-1, 1, n)                      # a +-0.05 signal riding on a DC offset of 0.5
        clips.append(np.round(x * 32768.0).astype(np.int16))            # exactly representable in both input types
    ref = [R.wave_stem(sd, R.pcm_to_wave(c)) for c in clips]
    return sd, clips, ref


def _run_stem(sd, clips, dtype, i16):
    B, S = len(clips), max(c.shape[0] for c in clips)
    T = ops.wave_stem_frames(S)
    pcm = np.zeros((B, S), np.int16)
    for b, c in enumerate(clips):
        pcm[b, : c.shape[0]] = c
        pcm[b, c.shape[0]:] = 12345                                     # padding that would show if it were read
    wav = torch.from_numpy(pcm).cuda() if i16 else torch.from_numpy(pcm.astype(np.float32) / 32768.0).cuda()
    w = sd["feature_extractor.conv_layers.0.0.weight"].reshape(512, 10).contiguous().cuda()
    g, b_ = sd["feature_extractor.conv_layers.0.2.weight"].cuda(), sd["feature_extractor.conv_layers.0.2.bias"].cuda()
    work = torch.empty(ops.wave_stem_workspace_bytes(B, 512), device="cuda", dtype=torch.uint8)
    out = torch.full((B * T, 512), float("nan"), device="cuda", dtype=ops.torch_dtype(dtype))
    ns = torch.tensor([c.shape[0] for c in clips], dtype=torch.int32).cuda()
    ops.wave_stem(wav, w, g, b_, work, out, B=B, S=S, T_rows=T, n_samples=ns, dtype=dtype)
    torch.cuda.synchronize()
    return out.view(B, T, 512)


@pytest.mark.parametrize("i16", [False, True], ids=["fp32_in", "int16_in"])
@pytest.mark.parametrize("dtype", [ops.F32, ops.F16, ops.BF16], ids=["f32", "f16", "bf16"])
def test_wave_stem_against_float64(stem_case, dtype, i16):
    sd, clips, ref = stem_case
    out = _run_stem(sd, clips, dtype, i16)
    again = _run_stem(sd, clips, dtype, i16)
    assert torch.equal(out.view(torch.uint8), again.view(torch.uint8)), "two runs differ"
    errs = []
    for b, (c, r) in enumerate(zip(clips, ref)):
        L0 = ops.wave_stem_frames(c.shape[0])
        assert r.shape == (L0, 512)
        got = out[b, :L0].double().cpu()
        assert not bool((out[b, L0:] != 0).any()) and not bool(torch.isnan(out[b]).any()), "rows past L0 must be exactly zero"
        alone = _run_stem(sd, [c], dtype, i16)
        assert torch.equal(alone[0, :L0].view(torch.uint8), out[b, :L0].view(torch.uint8)), f"clip {b}: batched != alone"
        err = (got - r).abs()
        errs.append(err.max().item())
        if dtype != ops.F32:
            tol = 2.0 * EPS16[dtype] * r.abs().clamp(min=1.0)
            worst = (err / tol).max().item()
            print(f"clip {b} ({c.shape[0]} samples): max err / (2 ulp) = {worst:.3f}, max |ref| {r.abs().max().item():.2f}")
            assert worst <= 1.0, (b, worst)
    if dtype == ops.F32:
        print("fp32 output, max abs err per clip:", " ".join(f"{e:.3e}" for e in errs), f"gate {F32_GATE:.2e}")
        assert max(errs) <= F32_GATE, errs
        others = max(e for b, e in enumerate(errs) if b != DC_CLIP)
        assert errs[DC_CLIP] <= 4.0 * others, (errs[DC_CLIP], others)


def _run_kmeans(x, c, lens, T):
    B = len(lens)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    cn = torch.from_numpy(c).double().pow(2).sum(1).float().cuda()
    ids = torch.full((B * T,), -7, device="cuda", dtype=torch.int32)
    best2 = torch.full((B * T, 2), float("nan"), device="cuda")
    ops.kmeans_assign(xd, cd, cn, ids, B=B, T=T, D=x.shape[1], K=c.shape[0], lens=torch.tensor(lens, dtype=torch.int32).cuda(),
                      len_mul=1, best2=best2)
    torch.cuda.synchronize()
    return ids.cpu(), best2.cpu(), cn.cpu()


@pytest.mark.parametrize("D,K", [(768, 200), (32, 2), (1024, 1000), (768, 37)])
def test_kmeans_assign_against_float64(D, K):
    x, c = R.kmeans_case(D, K)                                          # 130 rows: two clips of 65, the second 50 long
    T, lens = 65, [65, 50]
    ids, best2, cn = _run_kmeans(x, c, lens, T)
    valid = torch.cat([torch.arange(T) < n for n in lens])
    assert bool((ids[~valid] == -1).all()) and bool((best2[~valid] == 0).all())
    # the reference sees the same fp32 |c|^2 the kernel is handed
    d = cn.double()[None, :] - 2 * torch.from_numpy(x).double() @ torch.from_numpy(c).double().t()
    two = d.topk(2, dim=1, largest=False)
    ref_ids, _, mask = R.decisive_rows(x, c)
    assert (~mask).double().mean().item() <= 0.01
    m = mask & valid
    assert torch.equal(ids[m].long(), ref_ids[m]), int((ids[m].long() != ref_ids[m]).sum())
    assert bool(((ids[valid] >= 0) & (ids[valid] < K)).all())
    rel = ((best2[valid].double() - two.values[valid]).abs() / two.values[valid].abs()).max().item()
    print(f"D={D} K={K}: {int(m.sum())} decisive rows agree, best2 max rel err {rel:.2e}")
    assert rel <= 1e-4
    ids2, b2, _ = _run_kmeans(x, c, lens, T)
    assert torch.equal(ids, ids2) and torch.equal(b2[valid], best2[valid])
    # without lens and without best2
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    ids3 = torch.empty(2 * T, device="cuda", dtype=torch.int32)
    ops.kmeans_assign(xd, cd, cn.cuda(), ids3, B=2, T=T, D=D, K=K)
    assert torch.equal(ids3.cpu()[valid], ids[valid]) and bool((ids3.cpu() >= 0).all())


def test_kmeans_exact_tie_goes_to_the_lower_index():
    x, c = R.kmeans_case(64, 40)
    c[7], c[38] = c[3], c[3]                                            # three identical centres, in two different waves' tiles
    ids, best2, _ = _run_kmeans(x, c, [65, 65], 65)
    ref = R.kmeans_ids(x, c)                                            # torch argmin: the first minimal index
    near = ref == 3
    assert int(near.sum()) >= 1 and not bool(((ids == 7) | (ids == 38)).any())
    assert torch.equal(ids.long()[near], ref[near]) and bool((best2[near, 0] == best2[near, 1]).all())
    x2, c2 = R.kmeans_case(32, 2)
    c2[1] = c2[0]
    ids, _, _ = _run_kmeans(x2, c2, [65, 65], 65)
    assert bool((ids == 0).all())
