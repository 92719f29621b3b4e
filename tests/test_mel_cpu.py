"""Log-mel analysis of waveforms, the parts that need no GPU: the reference-held (wav, mel) pairs against a float64
restatement of the recipe, the product's packed basis and filterbank against that restatement, the ABI entry's argument checks
and the host logic of the `--mel_from_audio` route."""
import os
import wave

import numpy as np
import pytest
import torch

from tests import _mel_reference as mr


def _frames_f64(x, n_fft=640, hop=160):
    """[T, n_fft] reflect-padded frames of a 1-d float64 signal."""
    p = np.pad(x, n_fft // 2, mode="reflect")
    T = 1 + x.shape[0] // hop
    return np.stack([p[t * hop: t * hop + n_fft] for t in range(T)])


def test_fixture_matches_the_issue_table(golden_dir):
    fx = mr.load_fixture(golden_dir)
    want = [("test/UmvOgW6iV2s/00007", 68608, 429), ("test/UmvOgW6iV2s/00001", 39936, 250), ("test/UmvOgW6iV2s/00002", 20480, 129),
            ("test/UmvOgW6iV2s/00004", 57344, 359), ("test/62cNtvx6P8E/00001", 24576, 154)]
    assert [(c, p.shape[0], m.shape[0]) for c, p, m, _ in fx] == want
    for _, pcm, mel, spk in fx:
        assert pcm.dtype == np.int16 and mel.dtype == np.float32 and mel.shape[1] == 80 and spk.shape == (256,)
    for fn in ("mel_lrs3.npz", "mel_lrs3_audio.npz"):
        assert os.path.getsize(os.path.join(golden_dir, fn)) <= 688 * 1024


def test_float64_restatement_reproduces_the_reference_mels(golden_dir):
    for clip, pcm, mel, _ in mr.load_fixture(golden_dir):
        err = np.abs(mr.mel_f64(pcm) - mel).max()
        print(f"{clip}: max |f64 restatement - stored mel| = {err:.3e}")
        assert err <= 2e-4, (clip, err)


def test_frame_count_is_one_plus_n_over_hop(golden_dir):
    from lip2speech_unit_amd import audio
    for _, pcm, mel, _ in mr.load_fixture(golden_dir):
        assert audio.num_frames(pcm.shape[0]) == 1 + pcm.shape[0] // 160 == mel.shape[0] == mr.mel_f64(pcm).shape[0]
    for n in (321, 479, 480, 64000):
        assert audio.num_frames(n) == 1 + n // 160


def test_product_tables_equal_the_restatement(golden_dir):
    """The packed basis (the column map of include/lip2speech_hip.h) and the filterbank, in float64 before their one rounding,
    applied to reflect-padded frames: linear mel equal to the torch.stft restatement to 1e-9; the fp32 tables the device gets
    are those arrays rounded once, and fb_range brackets exactly the non-zero weights."""
    from lip2speech_unit_amd import audio
    basis, fb = audio.packed_basis(640), audio.mel_filterbank(16000, 640, 80, 0.0, 8000.0)
    assert basis.shape == (640, 640) and fb.shape == (80, 321) and basis.dtype == fb.dtype == np.float64
    worst = 0.0
    for clip, pcm, _, _ in mr.load_fixture(golden_dir)[1:3] + [("synthetic", mr.synthetic_clip(), None, None)]:
        x = mr.as_float64(pcm)
        re, im = audio.unpack_spectrum(_frames_f64(x) @ basis)
        lin = np.sqrt(re ** 2 + im ** 2) @ fb.T
        err = np.abs(lin - mr.linear_mel_f64(x)).max()
        worst = max(worst, err)
        assert err <= 1e-9, (clip, err)
    print(f"packed tables vs restatement, linear mel: max abs diff {worst:.2e}")
    st = audio.TacotronSTFT()
    assert st.basis.dtype == np.float32 and np.array_equal(st.basis, basis.astype(np.float32))
    assert st.fb.dtype == np.float32 and np.array_equal(st.fb, fb.astype(np.float32))
    assert st.fb_range.shape == (80, 2) and st.fb_range.dtype == np.int32
    for j, (lo, hi) in enumerate(st.fb_range):
        assert 0 <= lo < hi <= 321 and st.fb[j, lo] != 0 and st.fb[j, hi - 1] != 0
        assert not st.fb[j, :lo].any() and not st.fb[j, hi:].any()
    assert ((st.fb != 0).sum(0) <= 2).all()          # the sparse triangular form: a bin feeds at most two bands
    # bins 0 and n_fft/2 are the real-only ones: column 32 carries cos(pi n) * window, not a sine
    w = audio.hann_periodic(640)
    assert np.allclose(basis[:, 32], w * np.cos(np.pi * np.arange(640)), atol=1e-15) and np.allclose(basis[:, 0], w, atol=1e-15)


def test_abi_entry_rejects_bad_arguments_without_a_gpu():
    from lip2speech_unit_amd import _lib
    lib = _lib.load()
    assert lib.l2s_abi_version() == 16 == _lib.ABI_VERSION
    f = lib.l2s_mel_spectrogram
    ok = dict(wav=0x1000, i16=0, ldw=64000, ns=None, B=1, S=64000, basis=0x2000, fb=0x3000, rng=0x4000, mel=0x5000, ldm=80, T=401,
              n_fft=640, hop=160, n_mels=80, floor=1e-5, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["wav"], a["i16"], a["ldw"], a["ns"], a["B"], a["S"], a["basis"], a["fb"], a["rng"], a["mel"], a["ldm"], a["T"],
                 a["n_fft"], a["hop"], a["n_mels"], a["floor"], a["stream"])
    for name in ("wav", "basis", "fb", "rng", "mel"):
        assert call(**{name: None}) == -1, name                       # L2S_EINVAL, nothing launched
    assert call(B=0) == -2 and call(ldw=63999) == -2 and call(ldm=79) == -2 and call(T=0) == -2      # L2S_ESHAPE
    assert call(n_fft=1024) == -4 and call(hop=256) == -4 and call(n_mels=64) == -4                  # L2S_EUNSUPPORTED
    assert call(basis=0x2004) == -3 and call(mel=0x5002) == -3 and call(wav=0x1001, i16=1) == -3     # L2S_EALIGN


def test_operator_is_registered_and_has_no_cpu_path():
    from lip2speech_unit_amd import audio, ops
    assert ops.ENTRY_OF["mel_spectrogram"] == "l2s_mel_spectrogram" and hasattr(torch.ops.lip2speech, "mel_spectrogram")
    st = audio.TacotronSTFT()
    with pytest.raises(ops.L2SError):
        st.mel_rows(torch.zeros(1, 16000))
    with pytest.raises(ops.L2SError):
        st.mel_spectrogram(torch.zeros(1, 16000, dtype=torch.int16))
    with pytest.raises(ops.L2SError):
        ops.mel_spectrogram(torch.zeros(1, 16000), torch.zeros(1, 101, 80), torch.from_numpy(st.basis), torch.from_numpy(st.fb),
                            torch.from_numpy(st.fb_range), B=1, S=16000, T_rows=101)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        mel = torch.empty(1, 101, 80, device="cuda")
        assert torch.ops.lip2speech.mel_spectrogram(
            torch.empty(1, 16000, device="cuda"), mel, torch.empty(640, 640, device="cuda"), torch.empty(80, 321, device="cuda"),
            torch.empty(80, 2, device="cuda", dtype=torch.int32), B=1, S=16000, T_rows=101) is None


class _HostSTFT:
    """Stands in for the device analysis: records what it was handed, answers with the float64 restatement."""

    def __init__(self):
        self.seen = []

    def mel_rows(self, wav, n_samples=None):
        assert wav.dtype == torch.int16 and wav.dim() == 2 and wav.shape[0] == 1 and n_samples is None
        self.seen.append(wav[0].numpy().copy())
        return torch.from_numpy(mr.mel_f64(wav[0].numpy()).astype(np.float32))[None]


@pytest.mark.parametrize("pad", [None, 1280])
def test_mel_from_audio_dataset_host_logic(tmp_path, golden_dir, pad):
    """MelCodeDataset(mel_from_audio=True) on a layout WITHOUT mel/: the wav is read, zero-extended to the padded length, analysed,
    and the trimming rule leaves the same shapes (and, to the restatement's accuracy, values) as the stored mels give."""
    from lip2speech_unit_amd import data
    root_a, root_m = str(tmp_path / "a"), str(tmp_path / "m")
    lab_a, fx = mr.materialise_audio_dataset(root_a, golden_dir, with_mel=False)
    lab_m, _ = mr.materialise_audio_dataset(root_m, golden_dir, with_mel=True)
    assert not os.path.exists(os.path.join(root_a, "mel"))
    stft = _HostSTFT()
    kw = dict(code_dict_path=os.path.join(lab_a, "dict.unt.txt"), pad=pad)
    ds_a = data.MelCodeDataset(data.parse_manifest(os.path.join(lab_a, "test.tsv")), 320, 160, mel_from_audio=True, stft=stft, **kw)
    ds_m = data.MelCodeDataset(data.parse_manifest(os.path.join(lab_m, "test.tsv")), 320, 160, **kw)
    assert len(ds_a) == 5
    for i, (clip, pcm, mel, _) in enumerate(fx):
        fa, fm = ds_a[i][0], ds_m[i][0]
        n_audio = data.audio_num_samples(os.path.join(root_a, "audio", clip + ".wav"), pad)
        assert stft.seen[i].shape[0] == n_audio and np.array_equal(stft.seen[i][: pcm.shape[0]], pcm)
        assert not stft.seen[i][pcm.shape[0]:].any()
        assert fa["mel"].shape == fm["mel"].shape and fa["mel"].dtype == np.float32 and np.array_equal(fa["code"], fm["code"])
        assert fa["mel"].shape[1] == 2 * fa["code"].shape[0]
        T = min(fa["mel"].shape[1], mel.shape[0] - 3)            # the zero extension changes the clip's last frames only
        assert np.abs(fa["mel"][:, :T] - fm["mel"][:, :T]).max() <= 2e-4
    assert not os.path.exists(os.path.join(root_a, "mel"))


def test_cli_flag_reaches_the_dataset(monkeypatch, tmp_path):
    """`vocoder_inference --mel_from_audio` hands mel_from_audio=True to MelCodeDataset; without the flag it is False."""
    from lip2speech_unit_amd import vocoder_inference as s2
    seen = []

    class Stop(Exception):
        pass

    def fake_dataset(*a, **k):
        seen.append(k.get("mel_from_audio"))
        raise Stop

    class FakeGen:
        def __init__(self, *a, **k): pass
        def load_state_dict(self, sd): pass
        def cuda(self): return self
        def eval(self): return self
        def remove_weight_norm(self): pass

    import json
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(dict(code_hop_size=320, mel_hop_size=160, sampling_rate=16000)))
    monkeypatch.setattr(s2, "MelCodeDataset", fake_dataset)
    monkeypatch.setattr(s2, "MelCodeGenerator", FakeGen)
    monkeypatch.setattr(s2, "parse_manifest", lambda p: None)
    monkeypatch.setattr(s2.weights, "spec_of", lambda g: None)
    monkeypatch.setattr(s2.weights, "synth_state_dict", lambda spec, seed: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for extra, want in (([], False), (["--mel_from_audio"], True)):
        with pytest.raises(Stop):
            s2.main([str(cfg), "x.tsv", "d.txt", "--synthetic_weights"] + extra)
        assert seen[-1] is want


def test_read_wav_refuses_other_formats(tmp_path):
    from lip2speech_unit_amd import audio
    p = str(tmp_path / "x.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(8000)
        w.writeframes(np.zeros(100, np.int16).tobytes())
    with pytest.raises(ValueError):
        audio.read_wav_s16(p)
    with wave.open(p, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.arange(-50, 50, dtype="<i2").tobytes())
    assert np.array_equal(audio.read_wav_s16(p), np.arange(-50, 50, dtype=np.int16))
