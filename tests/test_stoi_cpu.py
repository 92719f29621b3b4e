"""STOI / ESTOI without a GPU: the float64 restatement (tests/_stoi_reference.py) against the facts recorded for the five committed
LRS3 clips, the host tables of intelligibility.py (checked by running the kernels' index arithmetic in numpy), the registration and
argument guards of the four l2s_stoi_* entries, and the evaluate CLI on injected parts."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import _stoi_reference as R

EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219)]
ENTRIES = ("l2s_stoi_resample", "l2s_stoi_frames", "l2s_stoi_bands", "l2s_stoi_scores")


@pytest.fixture(scope="module")
def clips(golden_dir):
    a = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    return [a[f"c{i}_pcm"].astype(np.float64) / 32768.0 for i in range(5)]


@pytest.fixture(scope="module")
def clean_stages(clips):
    return [R.stages(x, x) for x in clips]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_frames_kept_segments_margins(clips, clean_stages):
    want = [(333, 287, 257, 0.207), (193, 180, 150, 0.016), (98, 95, 65, 0.055), (278, 252, 222, 0.130), (118, 116, 86, 0.267)]
    for x, r, (frames, kept, segs, margin) in zip(clips, clean_stages, want):
        assert (r["n_frames"], len(r["kept"]), r["n_segments"]) == (frames, kept, segs)
        assert abs(r["margin_db"] - margin) < 5e-4, r["margin_db"]
        assert r["X"].shape == (15, len(r["kept"]) - 1)                  # the "< len - 256" rule on (kept + 1) * 128 samples


def test_restatement_identity_is_one(clean_stages):
    for r in clean_stages:
        assert abs(r["stoi"] - 1.0) < 1e-12 and abs(r["estoi"] - 1.0) < 1e-12


def test_restatement_falls_with_noise(clips):
    for i, x in enumerate(clips):
        got = [R.stages(x, R.add_noise(x, snr, seed=100 + i)) for snr in (20, 5, -5)]
        for key in ("stoi", "estoi"):
            assert 1.0 > got[0][key] > got[1][key] > got[2][key] > 0.0, (i, key, [g[key] for g in got])
        if i == 2:                                                       # scale only: about 0.997 / 0.922 / 0.714
            assert [round(g["stoi"], 1) for g in got] == [1.0, 0.9, 0.7]


def test_restatement_on_a_vocoder_output(clips, golden_dir):
    w = np.load(os.path.join(golden_dir, "vocoder_lrs3.npz"))["c0_wav"].astype(np.float64).reshape(-1)
    assert w.shape[0] == 68480
    r = R.stages(clips[0][:68480], w)
    assert abs(r["stoi"] - 0.259675) < 1e-6 and abs(r["estoi"] - 0.041061) < 1e-6, (r["stoi"], r["estoi"])


def test_restatement_without_a_segment(clips):
    r = R.stages(clips[2][:4000], clips[2][:4000])
    assert (r["n_frames"], r["n_segments"], r["stoi"], r["estoi"]) == (18, 0, 1e-5, 1e-5)


def test_restatement_against_pystoi(clips):
    pystoi = pytest.importorskip("pystoi")
    x = clips[2]
    y = R.add_noise(x, 5, seed=3)
    for ext in (False, True):
        assert abs(pystoi.stoi(x, y, 16000, extended=ext) - R.stoi(x, y, extended=ext)) < 1e-9


# ---- the host tables, through the kernels' own index arithmetic -------------------------------------------------------------------
def test_tables(clips):
    from lip2speech_unit_amd import intelligibility as I
    w = I.resample_taps()
    assert w.shape == (581,) and abs(w.sum() - 1.0) < 1e-12 and np.array_equal(w, R.resample_taps())
    e = I.band_edges()
    assert e.dtype == np.int32 and [(int(a), int(b)) for a, b in zip(e[:-1], e[1:])] == EDGES
    assert np.array_equal(e, R.band_edges()) and np.array_equal(I.window(), R.window())
    t = I.polyphase_taps()
    assert t.shape == (5, 117) and abs(t.sum() - 5.0) < 1e-11 and (t[1:, 116] == 0).all() and t[0, 116] == 5 * w[580]
    st = I.STOI()
    assert st.taps.dtype == np.float32 and st.basis.shape == (256, 512) and st.basis.dtype == np.float32 and st.window.shape == (256,)
    # the polyphase form of csrc/stoi.hip: out[m] = sum_q taps[p][q] x[(8 m + 290 - p) / 5 - q], p = 3 m mod 5
    x = clips[2][:3001]
    ref = R.resample(x)
    assert len(ref) == (5 * len(x) + 7) // 8
    xp = np.concatenate([np.zeros(200), x, np.zeros(200)])
    for m in list(range(0, 40)) + list(range(900, 940)) + list(range(len(ref) - 40, len(ref))):
        p = (3 * m) % 5
        assert (8 * m + 290 - p) % 5 == 0
        base = (8 * m + 290 - p) // 5
        got = sum(t[p, q] * xp[200 + base - q] for q in range(117))
        assert abs(got - ref[m]) < 1e-13, (m, got, ref[m])
    # the packed basis: frames of a compacted signal times the basis, unpacked by the column map = the reference's band matrix
    xr = R.resample(clips[2])
    kept, _ = R.kept_frames(xr)
    z = R.compact(xr, kept)
    frames = np.array([z[i:i + 256] for i in range(0, len(z) - 256, 128)])
    prod = frames @ I.packed_basis()
    k, part = I.basis_bin(np.arange(512))
    power = np.zeros((frames.shape[0], 257 + 8))
    for c in range(512):
        power[:, k[c]] += prod[:, c] ** 2
    got = np.sqrt(np.array([power[:, a:b].sum(1) for a, b in EDGES]))
    want = R.band_matrix(z)
    assert got.shape == want.shape and np.abs(got - want).max() < 1e-11 * want.max()


# ---- registration and guards ------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_wrapped():
    import torch

    from lip2speech_unit_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lip2speech_hip.h")).read()
    for e in ENTRIES:
        assert re.search(r"\bint\s+" + e + r"\s*\(", hdr), e
        assert e in _lib.SIGNATURES
        name = e[len("l2s_"):]
        assert ops.ENTRY_OF[name] == e and callable(getattr(ops, name)) and hasattr(torch.ops.lip2speech, name)
    assert "Taal" in hdr and "Jensen" in hdr and "DESIGN.md section 17" in hdr
    assert _lib.ABI_VERSION == 16
    with pytest.raises(ops.L2SError):
        ops.stoi_resample(torch.zeros(1, 100), torch.zeros(5, 117), torch.zeros(1, 63), B=1, S=100, R=63)


def test_argument_guards_return_codes_without_a_device():
    from lip2speech_unit_amd import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                       # an aligned host address: the guards return before any launch
    p = ctypes.addressof(buf)
    EINVAL, ESHAPE, EALIGN, EUNSUP = -1, -2, -3, -4
    S, big = 4000, ops.STOI_MAX_SAMPLES + 1
    R = ops.stoi_len10k(S)
    assert lib.l2s_stoi_resample(None, 0, S, None, 1, S, p, p, R, R, None) == EINVAL
    assert lib.l2s_stoi_resample(p, 0, S, None, 1, S, p, None, R, R, None) == EINVAL
    assert lib.l2s_stoi_resample(p, 0, S, None, 0, S, p, p, R, R, None) == ESHAPE
    assert lib.l2s_stoi_resample(p, 0, S, None, 1, S, p, p, R, R - 1, None) == ESHAPE
    assert lib.l2s_stoi_resample(p, 0, S, None, 1, S, p, p + 2, R, R, None) == EALIGN
    assert lib.l2s_stoi_resample(p, 0, big, None, 1, big, p, p, ops.stoi_len10k(big), ops.stoi_len10k(big), None) == EUNSUP
    assert lib.l2s_stoi_resample(p, 0, S, None, 70000, S, p, p, R, R, None) == EUNSUP
    assert lib.l2s_stoi_frames(p, R, None, 1, S, p, p, 18, None, None) == EINVAL
    assert lib.l2s_stoi_frames(p, R, None, 1, S, p, p, 17, p, None) == ESHAPE          # 4 000 samples are 18 frames
    assert lib.l2s_stoi_frames(p, R - 1, None, 1, S, p, p, 18, p, None) == ESHAPE
    assert lib.l2s_stoi_frames(p, R, None, 1, big, p, p, 4096, p, None) == EUNSUP
    assert lib.l2s_stoi_bands(p, p, R, None, 1, S, p, 18, p, p, None, p, p, 17, None) == EINVAL
    assert lib.l2s_stoi_bands(p, p, R, None, 1, S, p, 18, p, p, p, p, p, 16, None) == ESHAPE
    assert lib.l2s_stoi_bands(p, p, R, None, 1, S, p, 18, p, p, p + 4, p, p, 17, None) == EALIGN
    assert lib.l2s_stoi_bands(p, p, R, None, 1, big, p, 4096, p, p, p, p, p, 2048, None) == EUNSUP
    assert lib.l2s_stoi_scores(p, 17, p, 1, None, 1, p, p, p, None) == EINVAL
    assert lib.l2s_stoi_scores(p, 100, p, 1, p, 70, p, p, p, None) == ESHAPE           # 100 frames are 71 segments
    assert lib.l2s_stoi_scores(p, 17, p, 1, p + 4, 1, p, p, p, None) == EALIGN
    assert lib.l2s_stoi_scores(p, 4096, p, 1, p, 4096, p, p, p, None) == EUNSUP
    assert ops.stoi_frames_of(ops.stoi_len10k(384000)) == 1873 and ops.stoi_frames_of(ops.stoi_len10k(ops.STOI_MAX_SAMPLES)) == 2048


def test_host_class_refuses_host_tensors_and_other_rates():
    import torch

    from lip2speech_unit_amd import intelligibility as I
    from lip2speech_unit_amd._lib import L2SError
    with pytest.raises(ValueError):
        I.STOI(sampling_rate=22050)
    with pytest.raises(ValueError):
        I.stoi(torch.zeros(1, 4000), torch.zeros(1, 4000), sampling_rate=8000)
    x = torch.zeros(2, 4000)
    with pytest.raises(L2SError):
        I.STOI().scores(x, x)
    with pytest.raises(L2SError):
        I.estoi(x, x)


# ---- the CLI on injected parts ----------------------------------------------------------------------------------------------------
def _reference_score(clean, processed, n_samples):
    out = {"stoi": [], "estoi": [], "n_segments": [], "n_kept": []}
    for x, y, n in zip(clean, processed, n_samples):
        assert not x[n:].any() and not y[n:].any()                       # zero padding past the clip's own length
        r = R.stages(x[:n].astype(np.float64) / 32768.0, y[:n].astype(np.float64) / 32768.0)
        for k in ("stoi", "estoi", "n_segments"):
            out[k].append(r[k])
        out["n_kept"].append(len(r["kept"]))
    return out


def test_cli_pairs_truncates_and_reports(tmp_path, golden_dir, capsys):
    from scipy.io.wavfile import write

    from lip2speech_unit_amd import evaluate
    a = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    pcm = [a[f"c{i}_pcm"] for i in (2, 4)]
    noisy = [np.clip(np.round(R.add_noise(p.astype(np.float64), 5, seed=i)), -32768, 32767).astype(np.int16) for i, p in enumerate(pcm)]
    ref, pred = tmp_path / "audio", tmp_path / "pred_wav"
    for d in (ref / "spk0", ref / "spk1", pred / "spk0", pred / "spk1"):
        d.mkdir(parents=True)
    write(ref / "spk0" / "a.wav", 16000, pcm[0])
    write(pred / "spk0" / "a.wav", 16000, noisy[0][:-300])               # the prediction is 300 samples short
    write(ref / "spk1" / "b.wav", 16000, pcm[1])
    write(pred / "spk1" / "b.wav", 16000, noisy[1])
    write(ref / "spk1" / "short.wav", 16000, pcm[0][:4000])              # 18 frames: no segment
    write(pred / "spk1" / "short.wav", 16000, noisy[0][:4000])
    write(ref / "spk1" / "lonely.wav", 16000, pcm[1][:8000])
    write(pred / "spk0" / "extra.wav", 16000, pcm[1][:8000])
    rep = evaluate.main([str(ref), str(pred), "--batch_size", "2", "--output_dir", str(tmp_path / "out")], score=_reference_score)
    assert [c["name"] for c in rep["clips"]] == ["spk0/a.wav", "spk1/b.wav", "spk1/short.wav"]
    assert [c["samples"] for c in rep["clips"]] == [len(pcm[0]) - 300, len(pcm[1]), 4000]
    assert rep["unpaired"] == {"ref_only": ["spk1/lonely.wav"], "pred_only": ["spk0/extra.wav"]}
    want = [R.stages(p[:len(q)].astype(np.float64) / 32768.0, q.astype(np.float64) / 32768.0)
            for p, q in ((pcm[0], noisy[0][:-300]), (pcm[1], noisy[1]))]
    for c, r in zip(rep["clips"], want):
        assert c["stoi"] == r["stoi"] and c["estoi"] == r["estoi"] and c["segments"] == r["n_segments"] and c["kept_frames"] == len(r["kept"])
    short = rep["clips"][2]
    assert (short["segments"], short["stoi"], short["estoi"]) == (0, 1e-5, 1e-5)
    assert rep["n_clips"] == 2 and rep["n_no_segment"] == 1
    assert rep["stoi"] == (want[0]["stoi"] + want[1]["stoi"]) / 2 and rep["estoi"] == (want[0]["estoi"] + want[1]["estoi"]) / 2
    out = capsys.readouterr().out
    assert f"STOI {rep['stoi']:.3f} | ESTOI {rep['estoi']:.3f} (2 clips)" in out and "spk1/lonely.wav" in out and "spk0/extra.wav" in out
    stored = json.load(open(tmp_path / "out" / "eval-stoi.json"))
    assert stored == rep and set(stored["clips"][0]) == {"name", "samples", "kept_frames", "segments", "stoi", "estoi"}


def test_vocoder_inference_namespace_is_unchanged_without_the_flag():
    from lip2speech_unit_amd import vocoder_inference
    p = vocoder_inference.build_parser()
    a = vars(p.parse_args(["c.json", "test.tsv", "dict.txt"]))
    assert a == {"config_file": "c.json", "input_code_file": "test.tsv", "code_dict_path": "dict.txt", "code_file": None,
                 "output_dir": "generated_files", "checkpoint_file": None, "pad": None, "debug": False, "n": 10,
                 "synthetic_weights": False, "dtype": "f16", "mel_from_audio": False, "units_from_audio": False, "hubert": None,
                 "kmeans": None, "units_layer": 6, "units_dtype": "f32"}
    assert vars(p.parse_args(["c.json", "test.tsv", "dict.txt", "--stoi"]))["stoi"] is True
