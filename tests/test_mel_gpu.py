"""Log-mel analysis on the device (csrc/melspec.hip through audio.TacotronSTFT) against the reference-held (wav, mel) pairs
and the float64 restatement of tests/_mel_reference.py.  Gates are stated in the fixture's / float32's own distance from
float64 (DESIGN.md sections 11 and 12), never in absolute figures picked from a run."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import audio, ops  # noqa: E402
from tests import _mel_reference as mr  # noqa: E402


@pytest.fixture(scope="module")
def stft():
    return audio.TacotronSTFT()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return mr.load_fixture(golden_dir)


def _gpu_mel(stft, x):
    """[T, 80] numpy of one clip analysed alone; x: int16 or float32 numpy."""
    return stft.mel_rows(torch.from_numpy(np.ascontiguousarray(x))[None].cuda())[0].cpu().numpy()


def test_real_clips_against_the_reference_mels(stft, fx):
    """Each fixture clip alone, from int16 and from fp32: max |gpu - file| <= 4 x max |float64 restatement - file| over every one
    of the T_b x 80 cells."""
    for clip, pcm, mel, _ in fx:
        gate = 4.0 * np.abs(mr.mel_f64(pcm) - mel).max()
        for tag, x in (("int16", pcm), ("fp32", (pcm.astype(np.float32) / 32768.0))):
            got = _gpu_mel(stft, x)
            assert got.shape == mel.shape and got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - mel).max()
            print(f"{clip} {tag}: max |gpu - file| {err:.3e}, gate {gate:.3e}")
            assert err <= gate, (clip, tag, err, gate)


def test_any_input_against_the_float64_restatement(stft, fx):
    """The five clips and a synthetic one (tones + noise + digital silence, so the clamp floor is hit):
    max |gpu - f64| <= 4 x max |float32 CPU evaluation - f64| per clip."""
    clips = [(c, p) for c, p, _, _ in fx] + [("synthetic", mr.synthetic_clip())]
    for clip, pcm in clips:
        ref = mr.mel_f64(pcm)
        cpu32 = np.abs(mr.mel_f32(pcm).astype(np.float64) - ref).max()
        got = _gpu_mel(stft, pcm)
        err = np.abs(got.astype(np.float64) - ref).max()
        print(f"{clip}: max |gpu - f64| {err:.3e}, max |f32 cpu - f64| {cpu32:.3e}, gate {4 * cpu32:.3e}")
        if clip == "synthetic":
            floor_rows = (ref == np.log(1e-5)).all(1)
            assert floor_rows.sum() >= 10 and (got[floor_rows] == got[floor_rows][0, 0]).all()
        assert err <= 4.0 * cpu32, (clip, err, cpu32)


def test_clip_alone_semantics_in_a_padded_batch(stft, fx):
    """The five clips in one batch padded to the longest: each clip's rows are bit-identical to its own single-clip launch (the
    reflection is taken against the clip's own length), rows t >= T_b are exactly zero; padding content does not matter."""
    S = max(p.shape[0] for _, p, _, _ in fx)
    batch = np.full((len(fx), S), 12345, np.int16)                    # garbage, not zeros, behind every clip
    for i, (_, p, _, _) in enumerate(fx):
        batch[i, : p.shape[0]] = p
    lens = [p.shape[0] for _, p, _, _ in fx]
    out = stft.mel_rows(torch.from_numpy(batch).cuda(), lens)
    assert out.shape == (len(fx), 1 + S // 160, 80)
    out_dev_lens = stft.mel_rows(torch.from_numpy(batch).cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
    assert torch.equal(out, out_dev_lens)
    out = out.cpu().numpy()
    for i, (clip, p, mel, _) in enumerate(fx):
        T = mel.shape[0]
        alone = _gpu_mel(stft, p)
        assert np.array_equal(out[i, :T], alone), clip
        assert not out[i, T:].any(), clip


def test_short_clips_and_length_checks(stft, fx):
    pcm = fx[2][1]
    x = torch.from_numpy(np.stack([pcm, pcm])).cuda()
    with pytest.raises(ValueError):
        stft.mel_rows(x, [pcm.shape[0], 320])
    with pytest.raises(ValueError):
        stft.mel_rows(x, [pcm.shape[0] + 1, 4000])
    with pytest.raises(ValueError):
        stft.mel_rows(x[:, :320])
    with pytest.raises(ops.L2SError):
        stft.mel_rows(x.cpu())
    out = stft.mel_rows(x, torch.tensor([320, 321], dtype=torch.int32).cuda()).cpu().numpy()
    assert not out[0].any()                                           # no valid reflect padding: all rows zero
    assert np.array_equal(out[1, :3], _gpu_mel(stft, pcm[:321])) and not out[1, 3:].any()
    ref = mr.mel_f64(pcm[:321])                                       # the shortest clip that has frames, same gate as above
    assert np.abs(out[1, :3] - ref).max() <= 4.0 * np.abs(mr.mel_f32(pcm[:321]) - ref).max()


def test_int16_and_fp32_inputs_are_bit_identical(stft, fx):
    for clip, pcm, _, _ in fx[1:3]:
        a = _gpu_mel(stft, pcm)
        b = _gpu_mel(stft, pcm.astype(np.float32) / 32768.0)
        assert np.array_equal(a, b), clip
    m = stft.mel_spectrogram(torch.from_numpy(fx[2][1].astype(np.float32) / 32768.0)[None].cuda())
    assert m.shape == (1, 80, fx[2][2].shape[0]) and np.array_equal(m[0].t().cpu().numpy(), _gpu_mel(stft, fx[2][1]))


def test_graph_capture_replays_bit_identically(stft, fx):
    pcm = fx[4][1]
    x = torch.from_numpy(pcm)[None].cuda()
    basis, fb, rng = stft.tables(x.device)
    T = 1 + pcm.shape[0] // 160
    eager = torch.empty(1, T, 80, device="cuda")
    ops.mel_spectrogram(x, eager, basis, fb, rng, B=1, S=pcm.shape[0], T_rows=T)
    out = torch.zeros(1, T, 80, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mel_spectrogram(x, out, basis, fb, rng, B=1, S=pcm.shape[0], T_rows=T)       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.mel_spectrogram(x, out, basis, fb, rng, B=1, S=pcm.shape[0], T_rows=T)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    x.copy_(torch.from_numpy(fx[4][1][::-1].copy())[None])            # new audio in the captured buffer, same graph
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), _gpu_mel(stft, fx[4][1][::-1].copy()))


def test_through_the_vocoder_against_the_reference_waveform(tmp_path, golden_dir, fx):
    """Fixture audio -> GPU mel -> trimming rule (MelCodeDataset) -> forward_rows_precise, against the reference PCM / wav of
    vocoder_lrs3.npz.  The gate is the stored-mel test's (<= 2 LSB, 4e-5) widened by 2 x the waveform change the CPU oracle itself
    shows when it is fed the float64-restated mel instead of the stored one (computed here)."""
    from lip2speech_unit_amd import data, weights
    from lip2speech_unit_amd.vocoder import AttrDict, MelCodeGenerator
    from oracle import vocoder as ov
    from tests.test_models_gpu import VOC_H, sd_removed
    d = np.load(os.path.join(golden_dir, "vocoder_lrs3.npz"))
    lab, _ = mr.materialise_audio_dataset(str(tmp_path), golden_dir, with_mel=False)
    mds = data.MelCodeDataset(data.parse_manifest(os.path.join(lab, "test.tsv")), 320, 160,
                              code_dict_path=os.path.join(lab, "dict.unt.txt"), mel_from_audio=True)
    g = MelCodeGenerator(AttrDict(VOC_H), dtype=ops.F16)
    g.load_state_dict(weights.synth_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], seed=int(d["seed"])))
    g.remove_weight_norm()
    g = g.cuda().eval()
    sd = sd_removed(g)
    names = [c for c, _, _, _ in fx]
    for ci, clip in enumerate(d["clips"]):
        i = names.index(str(clip))
        f = mds[i][0]
        L = f["code"].shape[0]
        assert L == int(d[f"c{ci}_code_len"]) and f["mel"].shape == (80, 2 * L)
        code, spk = torch.from_numpy(f["code"])[None], torch.from_numpy(f["spkr"])[None]
        stored = torch.from_numpy(np.ascontiguousarray(fx[i][2][: 2 * L].T))[None]
        restated = torch.from_numpy(np.ascontiguousarray(mr.mel_f64(fx[i][1])[: 2 * L].T.astype(np.float32)))[None]
        with torch.no_grad():
            o_stored = ov.mel_code_generator(sd, VOC_H, code, stored, spk)[0, 0].numpy()
            o_rest = ov.mel_code_generator(sd, VOC_H, code, restated, spk)[0, 0].numpy()
            wav, pcm = g.forward_rows_precise(code.cuda(), torch.from_numpy(f["mel"])[None].cuda(), spk.cuda())
        widen = 2.0 * float(np.abs(o_rest - o_stored).max())
        ref_wav, ref_pcm = d[f"c{ci}_wav"], d[f"c{ci}_pcm"].astype(np.int32)
        assert np.abs(o_stored - ref_wav).max() < 4e-5          # the oracle on the stored mel is the fixture's generator
        err = float(np.abs(wav[0].cpu().numpy() - ref_wav).max())
        lsb = int(np.abs(pcm[0].cpu().numpy().astype(np.int32) - ref_pcm).max())
        print(f"{clip}: wav max abs err {err:.3e} ({lsb} LSB); oracle change f64-mel vs stored mel {widen / 2:.3e}; "
              f"gates {4e-5 + widen:.3e}, {2 + widen * 32768:.2f} LSB")
        assert err < 4e-5 + widen and lsb <= 2 + widen * 32768, (clip, err, lsb, widen)


def test_cli_extract_mel_and_vocoder_from_audio(tmp_path, golden_dir, fx):
    """extract_mel on a data set without mel/ writes the five [T, 80] float32 files (real-clip gate); vocoder_inference
    --mel_from_audio writes five wavs of 320 x code_len samples within WAV_TOL[F16] of the same CLI on the stored mel files."""
    from scipy.io import wavfile
    from lip2speech_unit_amd import extract_mel
    from lip2speech_unit_amd import vocoder_inference as s2
    from tests.test_fulldepth_gpu import WAV_TOL
    from tests.test_models_gpu import VOC_H
    root_a, root_m = str(tmp_path / "a"), str(tmp_path / "m")
    lab_a, _ = mr.materialise_audio_dataset(root_a, golden_dir, with_mel=False)
    lab_m, _ = mr.materialise_audio_dataset(root_m, golden_dir, with_mel=True)
    mel_out = str(tmp_path / "mel_out")
    extract_mel.main([os.path.join(root_a, "audio"), mel_out, "--batch", "3"])
    for clip, pcm, mel, _ in fx:
        got = np.load(os.path.join(mel_out, clip + ".npy"))
        assert got.shape == mel.shape and got.dtype == np.float32
        gate = 4.0 * np.abs(mr.mel_f64(pcm) - mel).max()
        err = np.abs(got.astype(np.float64) - mel).max()
        print(f"extract_mel {clip}: max |gpu - file| {err:.3e}, gate {gate:.3e}")
        assert err <= gate, (clip, err, gate)
    assert not os.path.exists(os.path.join(root_a, "mel"))
    cfg = str(tmp_path / "cfg.json")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000), open(cfg, "w"))
    outs = {}
    for tag, lab, extra in (("audio", lab_a, ["--mel_from_audio"]), ("mel", lab_m, [])):
        outs[tag] = str(tmp_path / ("out_" + tag))
        s2.main([cfg, os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--output_dir", outs[tag], "-n", "-1",
                 "--synthetic_weights"] + extra)
    assert not os.path.exists(os.path.join(root_a, "mel"))
    unt = open(os.path.join(lab_a, "test.unt")).read().splitlines()
    for (clip, pcm, _, _), line in zip(fx, unt):
        rel = os.path.join("pred_wav", *clip.split("/")[-2:]) + ".wav"
        sr_a, wa = wavfile.read(os.path.join(outs["audio"], rel))
        sr_m, wm = wavfile.read(os.path.join(outs["mel"], rel))
        code_len = min(pcm.shape[0] // 320, len(line.split("|")[-1].split()))
        assert sr_a == sr_m == 16000 and wa.dtype == np.int16 and wa.shape == wm.shape == (320 * code_len,)
        diff = np.abs(wa.astype(np.int32) - wm.astype(np.int32)).max() / 32768.0
        print(f"vocoder_inference {clip}: --mel_from_audio vs stored mel, max |wav diff| {diff:.3e} (tolerance {WAV_TOL[ops.F16]:.0e})")
        assert diff < WAV_TOL[ops.F16], (clip, diff)
