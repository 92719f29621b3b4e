"""Tile edges of the framed-DFT kernels (csrc/frame_dft.h under melspec.hip, stoi.hip and spkemb.hip): in every case the clips of one
batch end one frame before, exactly on and one frame after a tile boundary, and the output reaches a further tile that lies wholly
past every clip.  The input is seeded int16 noise over the whole buffer, so what lies behind a clip is garbage, not zeros.

Each case asserts: a clip's rows are the bytes of its own single-clip launch; rows / columns past the clip are exactly zero; the
values meet the gate of the entry's own test against its float64 restatement - 4 x the distance of the float32 CPU evaluation from
float64, computed here (for the STOI bands also the fixed TOL_BANDS of tests/test_stoi_gpu.py; their restatement has no float32
evaluation, the one used here is _bands_f32 below: the same steps in float32 with torch's FFT)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import audio, intelligibility, ops, speaker_encoder  # noqa: E402
from tests import _hifigan_mel_reference as hr  # noqa: E402
from tests import _mel_reference as mr  # noqa: E402
from tests import _spk_reference as sr  # noqa: E402
from tests import _stoi_reference as st  # noqa: E402
from tests.test_spk_emb_gpu import _band_relative  # noqa: E402
from tests.test_stoi_gpu import TOL_BANDS  # noqa: E402


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, size=shape, dtype=np.int16)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32).cuda()


def _log_mel_case(an, batch, lens, frames, tile, T_rows, f64, f32):
    """an.mel_rows on the batch and on every clip alone; f64 / f32: the restatement and its float32 evaluation of one clip."""
    out = an.mel_rows(torch.from_numpy(batch).cuda(), _i32(lens)).cpu().numpy()
    assert out.shape == (len(lens), T_rows, 80) and T_rows > (max(frames) + tile - 1) // tile * tile
    for i, (n, T) in enumerate(zip(lens, frames)):
        alone = an.mel_rows(torch.from_numpy(batch[i:i + 1, :n].copy()).cuda())[0].cpu().numpy()
        assert alone.shape == (T, 80) and np.array_equal(out[i, :T], alone), n
        assert not out[i, T:].any(), n
        x = batch[i, :n]
        ref = f64(x)
        e32 = float(np.abs(f32(x).astype(np.float64) - ref).max())
        err = float(np.abs(out[i, :T].astype(np.float64) - ref).max())
        print(f"n {n} ({T} frames): max |gpu - f64| {err:.3e}, max |f32 cpu - f64| {e32:.3e}, gate {4 * e32:.3e}")
        assert err <= 4.0 * e32, (n, err, e32)


def test_log_mel_640_160_tile_edges():
    """64 frames per tile: T_b = 63, 64, 65 and 3; 130 rows, so the tile of rows 128 .. 129 is past every clip."""
    _log_mel_case(audio.TacotronSTFT(), _noise((4, 20640), 1), [9927, 10080, 10399, 321], [63, 64, 65, 3], 64, 130, mr.mel_f64, mr.mel_f32)


def test_log_mel_1024_256_tile_edges():
    """32 frames per tile: T_b = 31, 32, 33; 70 rows, so the tile of rows 64 .. 69 is past every clip."""
    as_f32 = lambda p: p.astype(np.float32) / 32768.0  # noqa: E731
    _log_mel_case(audio.MelSpectrogram(), _noise((3, 17920), 2), [7941, 8192, 8703], [31, 32, 33], 32, 70,
                  lambda p: hr.mel_f64(as_f32(p)), lambda p: hr.mel_f32(as_f32(p)))


def test_power_mel_400_160_tile_edges():
    """32 frames per tile: T_b = 31, 32, 33 and 2; clip 1 has 4000 real samples of its 4960 (zeros behind them, not the buffer's
    noise), clip 2 a volume factor; 70 rows.  Band-relative error over the batch <= 4 x the worst float32 CPU evaluation."""
    batch = _noise((4, 11040), 3)
    lens, valid, scale, frames = [4801, 4960, 5279, 201], [4801, 4000, 5279, 201], [1.0, 1.0, 3.25, 1.0], [31, 32, 33, 2]
    pm = speaker_encoder.PowerMel()
    g = torch.tensor(scale).cuda()
    out = pm.mel_rows(torch.from_numpy(batch).cuda(), n_samples=_i32(lens), n_valid=_i32(valid), scale=g, T_rows=70).cpu().numpy()
    assert out.shape == (4, 70, 40)
    errs, worst32 = [], 0.0
    for i, (n, nv, T) in enumerate(zip(lens, valid, frames)):
        alone = pm.mel_rows(torch.from_numpy(batch[i:i + 1].copy()).cuda(), n_samples=_i32([n]), n_valid=_i32([nv]), scale=g[i:i + 1],
                            T_rows=70)[0].cpu().numpy()
        assert np.array_equal(out[i], alone), n
        assert not out[i, T:].any(), n
        x = np.zeros(n)
        x[:nv] = ((batch[i, :nv].astype(np.float32) / 32768.0) * np.float32(scale[i])).astype(np.float64)
        ref = sr.mel_power(x)
        assert ref.shape == (T, 40) and np.array_equal(out[i, :T].any(1), ref.any(1))   # frames of zeros only: exactly zero
        e32 = _band_relative(sr.mel_power(x, torch.float32).astype(np.float64), ref)
        errs.append(_band_relative(out[i, :T].astype(np.float64), ref))
        worst32 = max(worst32, e32)
        print(f"n {n} valid {nv} scale {scale[i]} ({T} frames): band-relative gpu {errs[-1]:.3e}, f32 cpu {e32:.3e}")
    print(f"gate {4 * worst32:.3e}")
    assert max(errs) <= 4.0 * worst32, (errs, worst32)


def _bands_f32(x, kept):
    """[15, len(kept) - 1] band magnitudes of the kept frames of x, every step of st.compact / st.band_matrix in float32."""
    w = st.window().astype(np.float32)
    z = np.zeros((len(kept) - 1) * st.HOP + st.N_FRAME, np.float32)
    for k, j in enumerate(kept):
        z[k * st.HOP:k * st.HOP + st.N_FRAME] += w * x[j * st.HOP:j * st.HOP + st.N_FRAME]
    frames = torch.from_numpy(z).unfold(0, st.N_FRAME, st.HOP)[:len(kept) - 1] * torch.from_numpy(w)
    spec = torch.view_as_real(torch.fft.rfft(frames, st.NFFT, dim=1))
    p = (spec[..., 0] * spec[..., 0] + spec[..., 1] * spec[..., 1]).t()
    e = st.band_edges()
    return torch.sqrt(torch.stack([p[e[i]:e[i + 1]].sum(0) for i in range(st.NUMBAND)])).numpy()


def test_stoi_bands_tile_edges():
    """ops.stoi_bands on hand-made kept lists with gaps: n_kept = 32, 33, 34, so F = 31, 32, 33 frames of 32 per tile; ldf = 70, so
    the tile of columns 64 .. 69 is past every clip.  Entries of `kept` behind n_kept and samples behind a clip are garbage."""
    S, ns, nk = 14747, [14747, 14000, 13000], [32, 33, 34]
    R = ops.stoi_len10k(S)
    assert ops.stoi_frames_of(R) == 71
    x, y = (_noise((3, R), s).astype(np.float32) / 32768.0 for s in (70, 71))
    rng = np.random.default_rng(7)
    kept = np.full((3, 71), 1 << 20, np.int32)
    for b in range(3):
        kept[b, :nk[b]] = np.sort(rng.choice(ops.stoi_frames_of(ops.stoi_len10k(ns[b])), nk[b], replace=False))
    assert all((np.diff(kept[b, :nk[b]]) > 1).any() for b in range(3))
    _, win, basis, edges = intelligibility.STOI().tables("cuda")
    dev = [torch.from_numpy(t).cuda() for t in (x, y, kept)]

    def run(sel):
        bands = torch.full((len(sel), 2, 15, 70), 7.0, device="cuda")
        ops.stoi_bands(dev[0][sel].contiguous(), dev[1][sel].contiguous(), dev[2][sel].contiguous(), _i32([nk[b] for b in sel]), win, basis,
                       edges, bands, B=len(sel), S=S, ldf=70, n_samples=_i32([ns[b] for b in sel]), ldx=R, ldk=71)
        return bands.cpu().numpy()

    out = run([0, 1, 2])
    for b in range(3):
        F = nk[b] - 1
        assert np.array_equal(out[b], run([b])[0]), b
        assert not out[b, :, :, F:].any(), b
        for s, sig in enumerate((x, y)):
            ref = st.band_matrix(st.compact(sig[b].astype(np.float64), kept[b, :nk[b]]))
            assert ref.shape == (15, F)
            rel = lambda d: float((np.abs(d.astype(np.float64) - ref).max(1) / ref.max(1)).max())  # noqa: E731
            err, e32 = rel(out[b, s, :, :F]), rel(_bands_f32(sig[b], kept[b, :nk[b]]))
            print(f"clip {b} signal {s} ({F} frames): band-relative gpu {err:.3e}, f32 cpu {e32:.3e}, gates {4 * e32:.3e} and {TOL_BANDS:.1e}")
            assert err < TOL_BANDS and err <= 4.0 * e32, (b, s, err, e32)
