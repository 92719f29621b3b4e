"""STOI / ESTOI on the device (csrc/stoi.hip, intelligibility.STOI) against the float64 restatement tests/_stoi_reference.py, on the
five committed LRS3 clips.  Every input is int16-representable, so the same samples go in as int16 PCM and as fp32.

Masking precondition of every case: on the restatement no frame of the clean signal lies within MARGIN_DB = 0.01 dB of the 40 dB
threshold (a 256-term fp32 norm is off by at most ~1.5e-5 relative = 1.3e-4 dB; the cap is 75 x that), so the kept list is exact.

Tolerances: 8 x the maximum measured on the MI355X over the cases below, the scores' floored at 1e-6 and
capped at the hard ceiling 5e-4 (the reference publishes three decimals: the metric must not move the last printed digit by
rounding alone).  Each test prints its figures before it asserts.
"""
import os

import numpy as np
import pytest
import torch

from tests import _stoi_reference as R

pytestmark = pytest.mark.gpu

MARGIN_DB = 0.01
SCORE_CEILING = 5e-4
# measured maxima on the MI355X (cases: stages, all clips x noise levels, silence, the 24 s cap), each times the customary 8:
TOL_SCORE = 1e-6          # |device - fp64| of stoi / estoi: measured 5.72e-8 (c2 at 5 dB); 8 x = 4.6e-7, floored at 1e-6
TOL_RESAMPLE = 3.9e-6     # resampled signal, max-abs over max|x|: measured 4.87e-7 (c4, processed side)
TOL_BANDS = 4.0e-6        # band magnitudes, max-abs over the band's maximum: measured 4.92e-7 (c2, clean side)
SNRS = (None, 20, 5, -5)
assert 1e-6 <= TOL_SCORE <= SCORE_CEILING


def _quantise(v):
    return np.clip(np.round(np.asarray(v) * 32768.0), -32768, 32767).astype(np.int16)


def _f64(pcm):
    return pcm.astype(np.float64) / 32768.0


@pytest.fixture(scope="module")
def pcm(golden_dir):
    a = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    return [a[f"c{i}_pcm"] for i in range(5)]


@pytest.fixture(scope="module")
def cases(pcm):
    """{(clip, snr): (x int16, y int16, restatement)} for the five clips at no noise, 20, 5 and -5 dB; computed once."""
    out = {}
    for i, x in enumerate(pcm):
        for snr in SNRS:
            y = x if snr is None else _quantise(R.add_noise(_f64(x), snr, seed=10 * i + 1))
            r = R.stages(_f64(x), _f64(y))
            assert r["margin_db"] > MARGIN_DB, (i, r["margin_db"])
            out[i, snr] = (x, y, r)
    return out


@pytest.fixture(scope="module")
def stoi():
    from lip2speech_unit_amd.intelligibility import STOI
    return STOI()


def _dev(a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype == torch.float32:
        t = t.to(torch.float32) / 32768.0                                # exact
    return t.cuda()


def _batch(stoi, xs, ys, dtype=torch.int16, stages=False):
    """One ragged call on a list of int16 clip pairs."""
    ns = [len(x) for x in xs]
    X, Y = (np.zeros((len(xs), max(ns)), dtype=np.int16) for _ in range(2))
    for b, (x, y) in enumerate(zip(xs, ys)):
        X[b, :ns[b]] = x
        Y[b, :ns[b]] = y
    f = stoi.stages if stages else stoi.scores
    r = f(_dev(X, dtype), _dev(Y, dtype), ns if len(set(ns)) > 1 else None)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def _score_err(got, b, r):
    assert int(got["n_segments"][b]) == r["n_segments"]
    return max(abs(float(got["stoi"][b]) - r["stoi"]), abs(float(got["estoi"][b]) - r["estoi"]))


def test_each_stage_against_the_restatement(stoi, cases):
    sel = [2, 4]
    xs, ys, refs = zip(*(cases[i, 5] for i in sel))
    got = _batch(stoi, xs, ys, stages=True)
    for b, r in enumerate(refs):
        n10 = len(r["xr"])
        scale = np.abs(_f64(xs[b])).max()
        for s, key in enumerate(("xr", "yr")):
            d = got["resampled"][b, s].numpy().astype(np.float64)
            err = np.abs(d[:n10] - r[key]).max() / scale
            print(f"STOI_MEASURE resample clip{sel[b]} {key} {err:.3e}")
            assert err < TOL_RESAMPLE and not d[n10:].any()
        K = len(r["kept"])
        assert int(got["n_kept"][b]) == K
        assert got["kept"][b, :K].tolist() == r["kept"].tolist() and (got["kept"][b, K:] == -1).all()
        F = K - 1
        for s, key in enumerate(("X", "Y")):
            d = got["bands"][b, s].numpy().astype(np.float64)
            err = (np.abs(d[:, :F] - r[key]).max(1) / r[key].max(1)).max()
            print(f"STOI_MEASURE bands clip{sel[b]} {key} {err:.3e}")
            assert err < TOL_BANDS and not d[:, F:].any()
        e = _score_err(got, b, r)
        print(f"STOI_MEASURE score stages clip{sel[b]} {e:.3e}")
        assert e < TOL_SCORE


@pytest.mark.parametrize("snr", SNRS)
def test_scores_on_all_clips_fp32_and_int16(stoi, cases, snr):
    xs, ys, refs = zip(*(cases[i, snr] for i in range(5)))
    a = _batch(stoi, xs, ys, torch.int16)
    f = _batch(stoi, xs, ys, torch.float32)
    for k in ("stoi", "estoi", "n_segments"):
        assert torch.equal(a[k], f[k]), k                                # the same samples: the same bits
    for b, r in enumerate(refs):
        e = _score_err(a, b, r)
        print(f"STOI_MEASURE score clip{b} snr{snr} {e:.3e}  stoi {float(a['stoi'][b]):.6f} estoi {float(a['estoi'][b]):.6f}")
        assert e < TOL_SCORE
    if snr is None:
        assert all(abs(float(v) - 1.0) < TOL_SCORE for v in a["stoi"]) and all(abs(float(v) - 1.0) < TOL_SCORE for v in a["estoi"])


def test_batch_independence_and_determinism(stoi, cases):
    xs, ys, _ = zip(*(cases[i, 5] for i in range(5)))
    together = _batch(stoi, xs, ys)
    again = _batch(stoi, xs, ys)
    for k in ("stoi", "estoi", "n_segments"):
        assert torch.equal(together[k], again[k]), k
    for b in range(5):
        alone = _batch(stoi, xs[b:b + 1], ys[b:b + 1])
        for k in ("stoi", "estoi", "n_segments"):
            assert torch.equal(alone[k][0], together[k][b]), (k, b)


def test_explicit_silence_across_tile_edges(stoi, pcm):
    x4 = pcm[4]
    x = np.concatenate([x4[:12000], np.zeros(5000, np.int16), x4[12000:], np.zeros(3000, np.int16)])
    y = _quantise(R.add_noise(_f64(x), 5, seed=41))
    r = R.stages(_f64(x), _f64(y))
    assert (r["n_frames"], len(r["kept"]), r["n_segments"]) == (158, 117, 87) and r["margin_db"] > 7.0
    got = _batch(stoi, [x], [y], stages=True)
    assert got["kept"][0, :117].tolist() == r["kept"].tolist() and int(got["n_kept"][0]) == 117
    e = _score_err(got, 0, r)
    print(f"STOI_MEASURE score silence {e:.3e}")
    assert e < TOL_SCORE


def test_no_segment(stoi, cases):
    x2, y2, _ = cases[2, 5]
    x4, y4, r4 = cases[4, 5]
    assert R.stages(_f64(x2[:4000]), _f64(y2[:4000]))["n_segments"] == 0
    got = _batch(stoi, [x2[:4000]], [y2[:4000]])
    assert int(got["n_segments"][0]) == 0
    assert float(got["stoi"][0]) == float(np.float32(1e-5)) and float(got["estoi"][0]) == float(np.float32(1e-5))
    both = _batch(stoi, [x2[:4000], x4], [y2[:4000], y4])
    alone = _batch(stoi, [x4], [y4])
    assert int(both["n_segments"][0]) == 0 and float(both["stoi"][0]) == float(np.float32(1e-5))
    for k in ("stoi", "estoi", "n_segments"):
        assert torch.equal(both[k][1], alone[k][0]), k


def test_service_cap_and_one_sample_over(stoi, pcm):
    from lip2speech_unit_amd import ops
    x = np.concatenate(pcm * 2)[:384000]
    y = _quantise(_f64(x) + 0.01 * np.random.default_rng(6).standard_normal(x.shape))
    r = R.stages(_f64(x), _f64(y))
    assert (r["n_frames"], len(r["kept"]), r["n_segments"]) == (1873, 1650, 1620) and r["margin_db"] > MARGIN_DB
    got = _batch(stoi, [x], [y], stages=True)
    assert int(got["n_kept"][0]) == 1650 and got["kept"][0, :1650].tolist() == r["kept"].tolist()
    e = _score_err(got, 0, r)
    print(f"STOI_MEASURE score cap {e:.3e}")
    assert e < TOL_SCORE
    over = torch.zeros(1, ops.STOI_MAX_SAMPLES + 1, dtype=torch.int16, device="cuda")
    with pytest.raises(ops.L2SError):
        stoi.scores(over, over)
    at = torch.zeros(1, ops.STOI_MAX_SAMPLES, dtype=torch.int16, device="cuda")     # the largest supported size, as digital silence:
    z = stoi.stages(at, at)                                                          # every frame is "the loudest", none is dropped
    assert int(z["n_kept"][0]) == 2048 and int(z["n_segments"][0]) == 2018 and float(z["stoi"][0]) == 0.0 and float(z["estoi"][0]) == 0.0


def test_cli_end_to_end(stoi, cases, tmp_path, capsys):
    from scipy.io.wavfile import write

    from lip2speech_unit_amd import evaluate
    ref, pred = tmp_path / "audio" / "spk", tmp_path / "pred_wav" / "spk"
    ref.mkdir(parents=True)
    pred.mkdir(parents=True)
    want = []
    for i in (1, 2, 4):
        x, y, _ = cases[i, 5]
        write(ref / f"c{i}.wav", 16000, x)
        write(pred / f"c{i}.wav", 16000, y)
        want.append(_batch(stoi, [x], [y]))
    rep = evaluate.main([str(tmp_path / "audio"), str(tmp_path / "pred_wav"), "--batch_size", "2", "--output_dir", str(tmp_path / "out")])
    for c, w in zip(rep["clips"], want):
        assert c["stoi"] == float(w["stoi"][0]) and c["estoi"] == float(w["estoi"][0]) and c["segments"] == int(w["n_segments"][0])
    assert rep["stoi"] == sum(float(w["stoi"][0]) for w in want) / 3 and rep["estoi"] == sum(float(w["estoi"][0]) for w in want) / 3
    assert f"STOI {rep['stoi']:.3f} | ESTOI {rep['estoi']:.3f} (3 clips)" in capsys.readouterr().out
    assert os.path.exists(tmp_path / "out" / "eval-stoi.json")


def test_vocoder_inference_scores_what_it_wrote(stoi, tmp_path, golden_dir, capsys):
    """`vocoder_inference --stoi` (synthetic weights, two clips): eval-stoi.json holds, per clip, the scores of a direct call on the
    manifest's audio and the wav just written, both truncated to the shorter."""
    import json

    from scipy.io import wavfile

    from lip2speech_unit_amd import vocoder_inference as s2
    from tests import _mel_reference as mr
    from tests.test_models_gpu import VOC_H
    root = str(tmp_path / "d")
    lab, fx = mr.materialise_audio_dataset(root, golden_dir, with_mel=True)
    cfg, out = str(tmp_path / "cfg.json"), str(tmp_path / "out")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000), open(cfg, "w"))
    s2.main([cfg, os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--output_dir", out, "-n", "2", "--synthetic_weights",
             "--stoi"])
    rep = json.load(open(os.path.join(out, "eval-stoi.json")))
    assert [c["name"] for c in rep["clips"]] == ["/".join(clip.split("/")[-2:]) for clip, _, _, _ in fx[:2]]
    for c, (clip, pcm, _, _) in zip(rep["clips"], fx[:2]):
        sr, w = wavfile.read(os.path.join(out, "pred_wav", *clip.split("/")[-2:]) + ".wav")
        n = min(len(w), len(pcm))
        assert sr == 16000 and c["samples"] == n
        want = _batch(stoi, [pcm[:n]], [w[:n]])
        assert c["stoi"] == float(want["stoi"][0]) and c["estoi"] == float(want["estoi"][0]) and c["segments"] == int(want["n_segments"][0])
        assert c["segments"] > 0 and -1.0 <= c["stoi"] <= 1.0 and -1.0 <= c["estoi"] <= 1.0
    assert f"STOI {rep['stoi']:.3f} | ESTOI {rep['estoi']:.3f} (2 clips)" in capsys.readouterr().out
