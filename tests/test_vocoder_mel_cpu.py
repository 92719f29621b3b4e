"""Vocoder validation, the parts that need no GPU: the reference-made fixture against a float64 restatement of the HiFi-GAN mel
analysis, the product's 1024-point tables against that restatement, l2s_stft_mel's argument checks, the data set's segment
sampling against the reference's recorded draws, and the host logic of `vocoder_validate` on stand-ins."""
import json
import os

import numpy as np
import pytest
import torch

from tests import _hifigan_mel_reference as hr
from tests import _mel_reference as mr

TABLE = [("test/UmvOgW6iV2s/00007", 112, 35), ("test/UmvOgW6iV2s/00001", 14, 35), ("test/UmvOgW6iV2s/00002", 0, 35),
         ("test/UmvOgW6iV2s/00004", 23, 35), ("test/62cNtvx6P8E/00001", 37, 35), ("test/UmvOgW6iV2s/00002_short", 0, 35)]
WITH_WAV = (0, 1, 5)
GATE = 2e-4          # log units: the bound tests/test_mel_cpu.py holds the 640-point restatement to


@pytest.fixture(scope="module")
def gold(golden_dir):
    return hr.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return mr.load_fixture(golden_dir)


def _source_audio(fx, i):
    """float64 normalised audio the item is cut from, the code line index and the mel file's rows (the short item reuses its
    parent's)."""
    k = i if i < 5 else [c for c, _, _, _ in fx].index(hr.SHORT_CLIP)
    pcm = fx[k][1] if i < 5 else fx[k][1][: hr.SHORT_SAMPLES]
    return hr.normalise(pcm), k, fx[k][2]


def test_fixture_matches_the_issue_table(golden_dir, gold):
    got = [(str(c), int(s), gold[f"c{i}_y_mel"].shape[1]) for i, (c, s) in enumerate(zip(gold["clips"], gold["start_step"]))]
    assert got == TABLE
    for i in range(6):
        assert gold[f"c{i}_y_mel"].shape == gold[f"c{i}_y_g_hat_mel"].shape == (80, 35)
        assert gold[f"c{i}_y_mel"].dtype == gold[f"c{i}_y_g_hat_mel"].dtype == np.float32
        assert (f"c{i}_y_g_hat" in gold) == (i in WITH_WAV)
    for i in WITH_WAV:
        assert gold[f"c{i}_y_g_hat"].shape == (8960,) and np.abs(gold[f"c{i}_y_g_hat"]).max() <= 1.0
    e = [float(np.abs(gold[f"c{i}_y_mel"].astype(np.float64) - gold[f"c{i}_y_g_hat_mel"]).mean()) for i in range(6)]
    assert np.allclose(e, gold["e"], rtol=1e-6) and abs(float(gold["val_err"]) - np.mean(e)) < 1e-6
    assert int(gold["seed"]) == 13 and int(gold["dataset_seed"]) == 1234 and int(gold["segment_size"]) == 8960
    assert os.path.getsize(os.path.join(golden_dir, "vocoder_mel_loss.npz")) <= 512 * 1024


def test_float64_restatement_reproduces_the_fixture_mels(gold, fx):
    for i, (clip, start, _) in enumerate(TABLE):
        x, _, _ = _source_audio(fx, i)
        x = x if i < 5 else np.hstack([x, x])
        seg = x[start * 320: start * 320 + 8960].astype(np.float32)
        pairs = [("y_mel", seg)] + ([("y_g_hat_mel", gold[f"c{i}_y_g_hat"])] if i in WITH_WAV else [])
        for tag, y in pairs:
            err = np.abs(hr.mel_f64(y).T - gold[f"c{i}_{tag}"]).max()
            print(f"{clip} {tag}: max |f64 restatement - stored| = {err:.3e}")
            assert err <= GATE, (clip, tag, err)
            if tag == "y_mel":                                         # fp32 torch.stft on the item alone: the reference's bits
                assert np.array_equal(hr.mel_f32(y).T, gold[f"c{i}_y_mel"])


def _frames_f64(x, n_fft=1024, hop=256, pad=384):
    p = np.pad(x, pad, mode="reflect")
    T = (x.shape[0] + 2 * pad - n_fft) // hop + 1
    return np.stack([p[t * hop: t * hop + n_fft] for t in range(T)])


def test_product_tables_equal_the_restatement(fx):
    """The 1024 x 1024 packed basis and the 80 x 513 filterbank in float64, applied to reflect-padded frames: linear mel equal to the
    torch.stft restatement to 1e-9; the device gets those arrays rounded once; fb_range brackets exactly the non-zero weights; a bin
    feeds at most two bands."""
    from lip2speech_unit_amd import audio
    basis, fb = audio.packed_basis(1024), audio.mel_filterbank(16000, 1024, 80, 0.0, 8000.0)
    assert basis.shape == (1024, 1024) and fb.shape == (80, 513) and basis.dtype == fb.dtype == np.float64
    worst = 0.0
    for clip, x in [(c, hr.normalise(p)) for c, p, _, _ in fx[1:3]] + [("synthetic", mr.as_float64(mr.synthetic_clip()))]:
        re, im = audio.unpack_spectrum(_frames_f64(x) @ basis, 1024)
        lin = np.sqrt(re ** 2 + im ** 2 + 1e-9) @ fb.T
        ref = hr.linear_mel_f64(x)
        assert lin.shape == ref.shape == (hr.num_frames(x.shape[0]), 80)
        err = np.abs(lin - ref).max()
        worst = max(worst, err)
        assert err <= 1e-9, (clip, err)
    print(f"packed tables vs restatement, linear mel: max abs diff {worst:.2e}")
    ms = audio.MelSpectrogram()
    assert (ms.n_fft, ms.hop, ms.pad, ms.mag_eps, ms.floor) == (1024, 256, 384, 1e-9, 1e-5)
    assert ms.basis.dtype == np.float32 and np.array_equal(ms.basis, basis.astype(np.float32))
    assert ms.fb.dtype == np.float32 and np.array_equal(ms.fb, fb.astype(np.float32))
    assert np.array_equal(audio.MelSpectrogram(fmax=8000).fb, ms.fb)                       # fmax=None means sr/2
    assert ms.fb_range.shape == (80, 2) and ms.fb_range.dtype == np.int32
    for j, (lo, hi) in enumerate(ms.fb_range):
        assert 0 <= lo < hi <= 513 and ms.fb[j, lo] != 0 and ms.fb[j, hi - 1] != 0
        assert not ms.fb[j, :lo].any() and not ms.fb[j, hi:].any()
    assert ((ms.fb != 0).sum(0) <= 2).all()
    w = audio.hann_periodic(1024)
    assert np.allclose(basis[:, 32], w * np.cos(np.pi * np.arange(1024)), atol=1e-15) and np.allclose(basis[:, 0], w, atol=1e-15)
    assert [ms.num_frames(n) for n in (384, 385, 511, 512, 8960, 64000)] == [0, 1, 1, 2, 35, 250]
    with pytest.raises(ValueError):
        audio.MelSpectrogram(win_size=800)


def test_abi_entry_rejects_bad_arguments_without_a_gpu():
    from lip2speech_unit_amd import _lib
    lib = _lib.load()
    assert lib.l2s_abi_version() == 16 == _lib.ABI_VERSION
    f = lib.l2s_stft_mel
    ok = dict(wav=0x1000, i16=0, ldw=64000, ns=None, B=1, S=64000, basis=0x2000, fb=0x3000, rng=0x4000, mel=0x5000, ldm=80, T=250,
              n_fft=1024, hop=256, n_mels=80, pad=384, eps=1e-9, floor=1e-5, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["wav"], a["i16"], a["ldw"], a["ns"], a["B"], a["S"], a["basis"], a["fb"], a["rng"], a["mel"], a["ldm"], a["T"],
                 a["n_fft"], a["hop"], a["n_mels"], a["pad"], a["eps"], a["floor"], a["stream"])
    for name in ("wav", "basis", "fb", "rng", "mel"):
        assert call(**{name: None}) == -1, name                                            # L2S_EINVAL, nothing launched
        assert call(**{name: None}, n_fft=640, hop=160, pad=320) == -1, name
    assert call(B=0) == -2 and call(ldw=63999) == -2 and call(ldm=79) == -2 and call(T=0) == -2 and call(n_fft=0) == -2   # L2S_ESHAPE
    assert call(pad=513) == -4 and call(pad=-1) == -4 and call(n_fft=640, hop=160, pad=321) == -4     # L2S_EUNSUPPORTED
    assert call(n_fft=512, hop=128, pad=192) == -4 and call(n_mels=64) == -4 and call(hop=160) == -4 and call(n_fft=640) == -4
    assert call(eps=-1.0) == -4
    assert call(basis=0x2004) == -3 and call(mel=0x5002) == -3 and call(wav=0x1001, i16=1) == -3 and call(wav=0x1002) == -3   # L2S_EALIGN
    assert call(n_fft=640, hop=160, pad=320, basis=0x2008) == -3


def test_operator_is_registered_and_has_no_cpu_path():
    from lip2speech_unit_amd import audio, ops
    assert ops.ENTRY_OF["stft_mel"] == "l2s_stft_mel" and hasattr(torch.ops.lip2speech, "stft_mel")
    ms = audio.MelSpectrogram()
    with pytest.raises(ops.L2SError):
        ms.mel_rows(torch.zeros(1, 8960))
    with pytest.raises(ops.L2SError):
        ms(torch.zeros(1, 8960, dtype=torch.int16))
    tabs = (torch.from_numpy(ms.basis), torch.from_numpy(ms.fb), torch.from_numpy(ms.fb_range))
    with pytest.raises(ops.L2SError):
        ops.stft_mel(torch.zeros(1, 8960), torch.zeros(1, 35, 80), *tabs, B=1, S=8960, T_rows=35, n_fft=1024, hop=256, pad=384, mag_eps=1e-9)
    with pytest.raises(NotImplementedError):
        torch.ops.lip2speech.stft_mel(torch.zeros(1, 8960), torch.zeros(1, 35, 80), *tabs, B=1, S=8960, T_rows=35, n_fft=1024, hop=256,
                                      pad=384)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        mel = torch.empty(1, 35, 80, device="cuda")
        assert torch.ops.lip2speech.stft_mel(
            torch.empty(1, 8960, device="cuda"), mel, torch.empty(1024, 1024, device="cuda"), torch.empty(80, 513, device="cuda"),
            torch.empty(80, 2, device="cuda", dtype=torch.int32), B=1, S=8960, T_rows=35, n_fft=1024, hop=256, pad=384, mag_eps=1e-9) is None


class _HostAnalysis:
    """Stands in for the device analysis (the _HostSTFT pattern of tests/test_mel_cpu.py): answers with the float64 restatement."""

    def num_frames(self, n):
        return hr.num_frames(int(n))

    def mel_rows(self, wav, n_samples=None):
        ns = [wav.shape[1]] * wav.shape[0] if n_samples is None else list(n_samples)
        out = torch.zeros(wav.shape[0], hr.num_frames(wav.shape[1]), 80, dtype=torch.float64)
        for b, n in enumerate(ns):
            m = hr.mel_f64(wav[b, :n].numpy())
            out[b, : m.shape[0]] = torch.from_numpy(m)
        return out


def _dataset(tmp_path, golden_dir, **kw):
    from lip2speech_unit_amd import data
    lab, names = hr.materialise_six(str(tmp_path / "ds"), golden_dir)
    files = data.parse_manifest(os.path.join(lab, "test.tsv"))
    return data.MelCodeDataset(files, 320, 160, code_dict_path=os.path.join(lab, "dict.unt.txt"), **kw), names, lab


def test_dataset_with_a_segment_size(tmp_path, golden_dir, gold, fx):
    """MelCodeDataset(segment_size=8960) reproduces the reference's six draws; the code and conditioning-mel slices are those
    recomputed from the stored inputs; the short item is doubled; the audio slice analysed by the float64 stand-in is the fixture's
    y_mel; without a segment size the items are today's."""
    from lip2speech_unit_amd import data
    ds, names, lab = _dataset(tmp_path, golden_dir, segment_size=8960)
    plain, _, _ = _dataset(tmp_path, golden_dir)
    unt = open(os.path.join(lab, "test.unt")).read().splitlines()
    code_dict = data.load_code_dict(os.path.join(lab, "dict.unt.txt"))
    an = _HostAnalysis()
    assert len(ds) == 6 and names == [t[0] for t in TABLE]
    for i, (clip, start, frames) in enumerate(TABLE):
        feats, wav, fn, last = ds[i]
        assert ds.starts[i] == start and last is None and fn.endswith(clip + ".wav")
        assert wav.dtype == np.float32 and wav.shape == (8960,) and set(feats) == {"code", "mel", "spkr"}
        x, k, mel_file = _source_audio(fx, i)
        code = np.array([code_dict[c] for c in unt[i].split()])
        L = min(x.shape[0] // 320, code.shape[0])
        cut = min(min(x.shape[0] // 160, mel_file.shape[0]) * 160, L * 320)
        x, code, mel = x[:cut], code[: cut // 320], mel_file[: cut // 160].T
        if i == 5:                                                     # 6 400 samples < 8 960: doubled once, 40 code frames
            assert cut == 6400
            x, code, mel = np.hstack([x, x]), np.hstack([code, code]), np.hstack([mel, mel])
            assert start == 0 and np.array_equal(feats["code"][20:], feats["code"][:8]) and np.array_equal(feats["mel"][:, 40:], feats["mel"][:, :16])
            assert np.array_equal(wav[6400:], wav[: 8960 - 6400])
        assert np.array_equal(feats["code"], code[start: start + 28]) and feats["code"].dtype == np.int64
        assert np.array_equal(feats["mel"], mel[:, 2 * start: 2 * start + 56]) and feats["mel"].dtype == np.float32
        assert np.array_equal(wav, x[320 * start: 320 * start + 8960].astype(np.float32))
        assert np.array_equal(feats["spkr"], fx[k][3])
        got = an.mel_rows(torch.from_numpy(wav)[None])[0].numpy().T
        err = np.abs(got - gold[f"c{i}_y_mel"]).max()
        assert got.shape == (80, frames) and err <= GATE, (clip, err)
        # without a segment size: the item of before this option existed
        f0, a0, fn0, l0 = plain[i]
        assert a0 is None and l0 is None and fn0 == fn and set(f0) == {"code", "mel", "spkr"}
        assert np.array_equal(f0["code"], code[: cut // 320] if i < 5 else code[:20])
        assert np.array_equal(f0["mel"], mel[:, : cut // 160] if i < 5 else mel[:, :40]) and f0["mel"].flags["C_CONTIGUOUS"]
    # the draws belong to the object: a fresh one starts the sequence again, another seed gives another sequence
    again = _dataset(tmp_path, golden_dir, segment_size=8960)[0]
    assert [again[i] and again.starts[i] for i in range(6)] == [t[1] for t in TABLE]
    other = _dataset(tmp_path, golden_dir, segment_size=8960, seed=7)[0]
    assert [other[i] and other.starts[i] for i in range(6)] != [t[1] for t in TABLE]
    # whole clips: start 0, nothing doubled, audio of cut samples
    whole = _dataset(tmp_path, golden_dir, segment_size=-1)[0]
    f, a, _, _ = whole[5]
    assert a.shape == (6400,) and f["code"].shape == (20,) and f["mel"].shape == (80, 40) and whole.starts[5] == 0
    f, a, _, _ = whole[4]
    assert a.shape == (24320,) and f["code"].shape == (76,) and f["mel"].shape == (80, 152)


def test_dataset_refuses_another_sampling_rate(tmp_path, golden_dir):
    import wave
    ds, _, _ = _dataset(tmp_path, golden_dir, segment_size=8960)
    with wave.open(ds.audio_files[0], "rb") as w:
        raw = w.readframes(w.getnframes())
    with wave.open(ds.audio_files[0], "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(22050)
        w.writeframes(raw)
    with pytest.raises(ValueError):
        ds[0]


def _host_l1(pred, targ, frames):
    return [float((pred[b, :T].double() - targ[b, :T].double()).abs().sum()) for b, T in enumerate(frames)]


def test_cli_host_logic_on_stand_ins(tmp_path, golden_dir, gold):
    """vocoder_validate.validate with a stand-in generator (the fixture's y_g_hat where it is stored, a tone elsewhere), the float64
    stand-in analysis and a host sum: val_err is the mean of the e_i it reports, in manifest order; the three items whose reference
    waveform is stored land on the fixture's e_i; --drop_last with a batch larger than the set is an error."""
    from lip2speech_unit_amd import vocoder_validate as vv
    seen = []

    def generate(code, mel, spkr, lens, t_label):
        B, L = code.shape
        assert mel.shape == (B, 80, 2 * L) and spkr.shape == (B, 256) and lens is None and t_label is None
        out = torch.zeros(B, 320 * L)
        for b in range(B):
            i = len(seen)
            seen.append(i)
            tone = 0.3 * np.sin(2 * np.pi * 440.0 * np.arange(320 * L) / 16000.0)
            out[b] = torch.from_numpy(gold[f"c{i}_y_g_hat"] if i in WITH_WAV else tone.astype(np.float32))
        return out
    for bs in (4, 16):
        del seen[:]
        ds, names, _ = _dataset(tmp_path, golden_dir, segment_size=8960)
        rep = vv.validate(ds, generate, _HostAnalysis(), _host_l1, bs, device="cpu")
        es = [c["e"] for c in rep["clips"]]
        assert rep["val_err"] == sum(es) / len(es) and rep["n_clips"] == 6
        assert [(c["name"], c["start"], c["frames"]) for c in rep["clips"]] == TABLE
        for i in WITH_WAV:
            assert abs(es[i] - float(gold["e"][i])) <= 2 * GATE, (i, es[i], float(gold["e"][i]))
    del seen[:]
    ds, _, _ = _dataset(tmp_path, golden_dir, segment_size=8960)
    rep = vv.validate(ds, generate, _HostAnalysis(), _host_l1, 4, drop_last=True, device="cpu")
    assert rep["n_clips"] == 4 and [c["name"] for c in rep["clips"]] == [t[0] for t in TABLE[:4]]
    with pytest.raises(ValueError):
        vv.validate(ds, generate, _HostAnalysis(), _host_l1, 16, drop_last=True, device="cpu")


def test_cli_writes_the_report(monkeypatch, tmp_path, golden_dir, capsys):
    """main() with the generator, the analysis and the device sum replaced by stand-ins: the printed line and valid-mel.json carry
    val_err and, per clip, name, start, frames and e; --drop_last with a batch larger than the set errors out."""
    from lip2speech_unit_amd import audio, vocoder_validate as vv

    class FakeGen:
        def __init__(self, *a, **k): pass
        def load_state_dict(self, sd): pass
        def cuda(self): return self
        def eval(self): return self
        def remove_weight_norm(self): pass
        def forward_rows(self, code, mel, spkr, lens=None, t_label=None):
            return torch.zeros(code.shape[0], 320 * code.shape[1]) + 0.25, None
    _, _, lab = _dataset(tmp_path, golden_dir)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(dict(code_hop_size=320, mel_hop_size=160, sampling_rate=16000, segment_size=8960, batch_size=4,
                                   fmax_for_loss=None)))
    monkeypatch.setattr(vv, "MelCodeGenerator", FakeGen)
    monkeypatch.setattr(vv.weights, "spec_of", lambda g: None)
    monkeypatch.setattr(vv.weights, "synth_state_dict", lambda spec, seed: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(audio, "MelSpectrogram", lambda *a, **k: _HostAnalysis())
    monkeypatch.setattr(vv, "device_clip_l1", _host_l1)
    import functools
    monkeypatch.setattr(vv, "validate", functools.partial(vv.validate, device="cpu"))
    args = [str(cfg), os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--synthetic_weights", "--output_dir",
            str(tmp_path / "out")]
    rep = vv.main(args)
    assert f"validation/mel_spec_error {rep['val_err']:.6f}" in capsys.readouterr().out
    js = json.load(open(tmp_path / "out" / "valid-mel.json"))
    assert js["val_err"] == rep["val_err"] == sum(c["e"] for c in js["clips"]) / 6 and js["segment_size"] == 8960 and js["seed"] == 1234
    assert [(c["name"], c["start"], c["frames"]) for c in js["clips"]] == TABLE
    assert all(set(c) == {"name", "start", "frames", "e"} and c["e"] > 0 for c in js["clips"])
    with pytest.raises(ValueError):
        vv.main(args + ["--drop_last", "--batch_size", "16"])
