"""The HiFi-GAN mel analysis of the vocoder's validation loss on the device (l2s_stft_mel at 1024 / 256 through
audio.MelSpectrogram) and the validation protocol around it, against the float64 restatement of tests/_hifigan_mel_reference.py and
the reference-made fixture tests/golden/vocoder_mel_loss.npz.  Gates are stated in float32's own distance from float64 on the same
input (DESIGN.md sections 11, 12 and 16), never in absolute figures picked from a run."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import audio, ops  # noqa: E402
from tests import _hifigan_mel_reference as hr  # noqa: E402
from tests import _mel_reference as mr  # noqa: E402

SLICES = (("whole", None), ("35 frames", (5120, 14080)), ("4 frames", (2048, 3072)), ("1 frame", (4000, 4385)))


@pytest.fixture(scope="module")
def ms():
    return audio.MelSpectrogram()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return mr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return hr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def segments(fx, gold):
    """The six ground-truth segments of the fixture, float32 [8960], cut from the stored audio at the stored start_step."""
    out = []
    for i, clip in enumerate(gold["clips"]):
        pcm = fx[i][1] if i < 5 else fx[[c for c, _, _, _ in fx].index(hr.SHORT_CLIP)][1][: hr.SHORT_SAMPLES]
        x = hr.normalise(pcm)
        x = x if i < 5 else np.hstack([x, x])                             # the short item is doubled once
        s = int(gold["start_step"][i]) * 320
        out.append(x[s: s + hr.SEGMENT].astype(np.float32))
        assert out[-1].shape == (hr.SEGMENT,)
    return out


def _gpu_mel(ms, x):
    """[T, 80] numpy of one clip analysed alone; x: int16 or float32 numpy."""
    return ms.mel_rows(torch.from_numpy(np.ascontiguousarray(x))[None].cuda())[0].cpu().numpy()


def _cell_gate(x):
    """(f64 mel, 4 x max |fp32 torch.stft evaluation - f64|) of one float32 input."""
    ref = hr.mel_f64(x)
    return ref, 4.0 * float(np.abs(hr.mel_f32(x).astype(np.float64) - ref).max())


def test_any_input_against_the_float64_restatement(ms, fx):
    """The five fixture clips (peak-normalised x 0.95, truncated to a multiple of 256) and the synthetic clip, each as a whole, as
    x[5120:14080] (35 frames, a validation segment), x[2048:3072] (4 frames) and x[4000:4385] (one frame, the shortest input with
    a valid reflection): max |gpu - f64| <= 4 x max |fp32 torch.stft evaluation - f64| per input."""
    clips = [(c, hr.normalise(p)) for c, p, _, _ in fx] + [("synthetic", mr.synthetic_clip().astype(np.float64) / 32768.0)]
    for clip, x in clips:
        x = x[: x.shape[0] // 256 * 256].astype(np.float32)
        for tag, sl in SLICES:
            y = x if sl is None else x[sl[0]: sl[1]]
            ref, gate = _cell_gate(y)
            got = _gpu_mel(ms, y)
            assert got.shape == ref.shape == (hr.num_frames(y.shape[0]), 80) and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - ref).max())
            floor = float((ref == np.log(1e-5)).mean())
            print(f"{clip} {tag}: max |gpu - f64| {err:.3e}, gate {gate:.3e} ({err / max(gate / 4, 1e-30):.2f} x the fp32 FFT), "
                  f"{100 * floor:.0f} % of the cells on the floor")
            assert err <= gate, (clip, tag, err, gate)


def test_segments_against_the_reference_fixture(ms, gold, segments):
    """y_mel from the stored audio and y_g_hat_mel from the reference generator's stored y_g_hat, against the mels the reference's
    own mel_spectrogram made: max |gpu - stored| <= 4 x max |f64 restatement - stored| per item."""
    for i, clip in enumerate(gold["clips"]):
        pairs = [("y_mel", segments[i], gold[f"c{i}_y_mel"])]
        if f"c{i}_y_g_hat" in gold:
            pairs.append(("y_g_hat_mel", gold[f"c{i}_y_g_hat"], gold[f"c{i}_y_g_hat_mel"]))
        for tag, x, stored in pairs:
            gate = 4.0 * float(np.abs(hr.mel_f64(x).T - stored).max())
            err = float(np.abs(_gpu_mel(ms, x).T.astype(np.float64) - stored).max())
            print(f"{clip} {tag}: max |gpu - stored| {err:.3e}, gate {gate:.3e}")
            assert err <= gate, (clip, tag, err, gate)


def _old_and_new_640(st, x, n_samples=None):
    B, S = x.shape
    T = audio.num_frames(S)
    basis, fb, rng = st.tables(x.device)
    old, new = torch.full((B, T, 80), 7.0, device="cuda"), torch.full((B, T, 80), -7.0, device="cuda")
    ops.mel_spectrogram(x, old, basis, fb, rng, B=B, S=S, T_rows=T, n_samples=n_samples)
    ops.stft_mel(x, new, basis, fb, rng, B=B, S=S, T_rows=T, n_samples=n_samples, n_fft=640, hop=160, pad=320, mag_eps=0.0)
    return old, new


def test_the_640_instantiation_is_the_old_entry_bit_for_bit(fx):
    """l2s_stft_mel at (640, 160, pad 320, eps 0) against l2s_mel_spectrogram: two fixture clips alone and the padded five-clip
    batch - the generalised kernel tied to the one section 12 validated."""
    st = audio.TacotronSTFT()
    for _, pcm, mel, _ in fx[1:3]:
        old, new = _old_and_new_640(st, torch.from_numpy(pcm)[None].cuda())
        assert torch.equal(old, new) and old.shape[1] == mel.shape[0]
    S = max(p.shape[0] for _, p, _, _ in fx)
    batch = np.full((len(fx), S), 12345, np.int16)
    for i, (_, p, _, _) in enumerate(fx):
        batch[i, : p.shape[0]] = p
    lens = torch.tensor([p.shape[0] for _, p, _, _ in fx], dtype=torch.int32).cuda()
    old, new = _old_and_new_640(st, torch.from_numpy(batch).cuda(), lens)
    assert torch.equal(old, new)
    assert torch.equal(old, st.mel_rows(torch.from_numpy(batch).cuda(), lens))


def test_clip_alone_semantics_in_a_padded_batch(ms, fx):
    """1024 / 256: the five clips in one batch padded with garbage - each clip's rows are bit-identical to its single-clip launch,
    rows past T_b are exactly zero, a clip of <= 384 samples has only zero rows, int16 and fp32 inputs give the same bits."""
    S = max(p.shape[0] for _, p, _, _ in fx)
    batch = np.full((len(fx) + 1, S), 12345, np.int16)
    for i, (_, p, _, _) in enumerate(fx):
        batch[i, : p.shape[0]] = p
    lens = [p.shape[0] for _, p, _, _ in fx] + [384]
    with pytest.raises(ValueError):
        ms.mel_rows(torch.from_numpy(batch).cuda(), lens)                 # a host list is checked: 384 has no valid reflection
    out = ms.mel_rows(torch.from_numpy(batch).cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
    assert out.shape == (len(fx) + 1, hr.num_frames(S), 80)
    out32 = ms.mel_rows(torch.from_numpy(batch.astype(np.float32) / 32768.0).cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
    assert torch.equal(out, out32)
    out = out.cpu().numpy()
    for i, (clip, p, _, _) in enumerate(fx):
        T = hr.num_frames(p.shape[0])
        assert T == ms.num_frames(p.shape[0]) == p.shape[0] // 256
        assert np.array_equal(out[i, :T], _gpu_mel(ms, p)), clip
        assert np.isfinite(out[i, :T]).all() and not out[i, T:].any(), clip
    assert not out[len(fx)].any()
    assert np.array_equal(ms(torch.from_numpy(fx[4][1])[None].cuda())[0].t().cpu().numpy(), _gpu_mel(ms, fx[4][1]))
    with pytest.raises(ops.L2SError):
        ms.mel_rows(torch.zeros(1, 8960))
    with pytest.raises(ValueError):
        ms.mel_rows(torch.zeros(1, 255).cuda())


def test_graph_capture_replays_bit_identically(ms, fx):
    pcm = fx[4][1]
    S = pcm.shape[0]
    x = torch.from_numpy(pcm)[None].cuda()
    basis, fb, rng = ms.tables(x.device)
    T = ms.num_frames(S)
    kw = dict(B=1, S=S, T_rows=T, n_fft=1024, hop=256, pad=384, mag_eps=1e-9)
    eager = torch.empty(1, T, 80, device="cuda")
    ops.stft_mel(x, eager, basis, fb, rng, **kw)
    out = torch.zeros(1, T, 80, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.stft_mel(x, out, basis, fb, rng, **kw)                        # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.stft_mel(x, out, basis, fb, rng, **kw)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and np.array_equal(eager[0].cpu().numpy(), _gpu_mel(ms, pcm))
    x.copy_(torch.from_numpy(pcm[::-1].copy())[None])                     # new audio in the captured buffer, same graph
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), _gpu_mel(ms, pcm[::-1].copy()))


def _e_f64(y, y_hat):
    return float(np.abs(hr.mel_f64(y) - hr.mel_f64(y_hat)).mean())


def _e_gate(y, y_hat):
    """Two mels, each within its cell gate, enter an absolute difference: the mean moves by at most the sum of the two gates
    (<= 2 x the larger)."""
    return _cell_gate(y)[1] + _cell_gate(y_hat)[1]


def test_per_clip_error_from_the_reference_audio(ms, gold, segments):
    """e_i on the device - two analyses and l2s_mel_l1_sc - from the fixture's stored y_g_hat and the ground-truth segment, against
    the float64 evaluation of the same; the stored e_i (the reference's fp32 figure) is printed beside it."""
    from lip2speech_unit_amd.vocoder_validate import device_clip_l1
    idx = [i for i in range(len(gold["clips"])) if f"c{i}_y_g_hat" in gold]
    assert idx == [0, 1, 5]
    y = torch.from_numpy(np.stack([segments[i] for i in idx])).cuda()
    y_hat = torch.from_numpy(np.stack([gold[f"c{i}_y_g_hat"] for i in idx])).cuda()
    y_mel, y_hat_mel = ms.mel_rows(y), ms.mel_rows(y_hat)
    assert y_mel.shape == (3, 35, 80)
    l1 = device_clip_l1(y_hat_mel, y_mel, [35, 35, 35])
    for k, i in enumerate(idx):
        e_gpu, e_ref = l1[k] / (80 * 35), _e_f64(segments[i], gold[f"c{i}_y_g_hat"])
        gate = _e_gate(segments[i], gold[f"c{i}_y_g_hat"])
        print(f"{gold['clips'][i]}: e gpu {e_gpu:.7f}, f64 {e_ref:.7f}, |diff| {abs(e_gpu - e_ref):.3e}, gate {gate:.3e}; "
              f"stored fp32 e {float(gold['e'][i]):.7f}")
        assert abs(e_gpu - e_ref) <= gate, (i, e_gpu, e_ref, gate)


def _cfg(tmp_path):
    from tests.test_models_gpu import VOC_H
    cfg = str(tmp_path / "cfg.json")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000, segment_size=8960, batch_size=16, n_fft=1024,
                   hop_size=256, win_size=1024, fmin=0, fmax=8000, fmax_for_loss=None), open(cfg, "w"))
    return cfg


def test_cli_end_to_end(tmp_path, golden_dir, gold, segments, capsys):
    """vocoder_validate on the materialised six-item data set, synthetic weights (the fixture's seed), fp16: every e_i within the
    two-mel gate of the float64 mel error the test evaluates on the waveform the device generated; val_err is the mean of the
    JSON's e_i; |e_i - fixture e_i| is printed for f16 and --precise (an fp16 / hi-lo generator against the fp32 reference's - what
    the waveform tests bound - so it is recorded in DESIGN.md section 16, not gated); whole-clip mode yields
    (cut + 768 - 1024) // 256 + 1 frames per clip."""
    from lip2speech_unit_amd import vocoder_validate as vv
    lab, names = hr.materialise_six(str(tmp_path / "ds"), golden_dir)
    base = [_cfg(tmp_path), os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--synthetic_weights", "--synthetic_seed",
            str(int(gold["seed"]))]
    log = []                                                              # capsys swallows prints made before readouterr()
    for tag, extra in (("f16", []), ("precise", ["--precise"])):
        wavs = []
        out = str(tmp_path / ("out_" + tag))
        rep = vv.main(base + ["--output_dir", out] + extra, on_batch=lambda b0, y, ns: wavs.append(y.float().cpu().numpy()))
        assert f"validation/mel_spec_error {rep['val_err']:.6f}" in capsys.readouterr().out
        js = json.load(open(os.path.join(out, "valid-mel.json")))
        es = [c["e"] for c in js["clips"]]
        assert js["val_err"] == rep["val_err"] == sum(es) / len(es) and len(es) == 6
        assert [c["name"] for c in js["clips"]] == names and [c["start"] for c in js["clips"]] == [int(s) for s in gold["start_step"]]
        assert all(c["frames"] == 35 for c in js["clips"])
        y_hat = np.concatenate(wavs)
        assert y_hat.shape == (6, hr.SEGMENT)
        for i in range(6):
            diff = abs(es[i] - float(gold["e"][i]))
            log.append(f"{tag} {names[i]}: e {es[i]:.6f}, fixture e {float(gold['e'][i]):.6f}, |e_i - fixture e_i| {diff:.3e}")
            if tag == "f16":
                e_ref, gate = _e_f64(segments[i], y_hat[i]), _e_gate(segments[i], y_hat[i])
                log.append(f"    f64 on the device's waveform {e_ref:.6f}, |diff| {abs(es[i] - e_ref):.3e}, gate {gate:.3e}")
                assert abs(es[i] - e_ref) <= gate, (log, i, es[i], e_ref, gate)
        log.append(f"{tag}: val_err {rep['val_err']:.6f}, fixture val_err {float(gold['val_err']):.6f}")
    print("\n".join(log))
    out = str(tmp_path / "out_whole")
    rep = vv.main(base + ["--output_dir", out, "--segment_size", "-1", "--batch_size", "4"])
    unt = open(os.path.join(lab, "test.unt")).read().splitlines()
    n_audio = [p.shape[0] for _, p, _, _ in mr.load_fixture(golden_dir)] + [hr.SHORT_SAMPLES]
    n_mel = [m.shape[0] for _, _, m, _ in mr.load_fixture(golden_dir)]
    n_mel.append(n_mel[names.index(hr.SHORT_CLIP)])
    cuts = [min(min(n // 160, m) * 160, min(n // 320, len(u.split())) * 320) for n, m, u in zip(n_audio, n_mel, unt)]
    stored = np.load(os.path.join(golden_dir, "vocoder_lrs3.npz"))
    assert (cuts[0], cuts[4], cuts[5]) == (int(stored["c0_code_len"]) * 320, int(stored["c1_code_len"]) * 320, hr.SHORT_SAMPLES)
    assert [c["frames"] for c in rep["clips"]] == [(c + 768 - 1024) // 256 + 1 for c in cuts]
    assert all(c["start"] == 0 and np.isfinite(c["e"]) and c["e"] > 0 for c in rep["clips"])
