"""Speaker embeddings from audio, the parts that need no GPU: the float64 restatement tests/_spk_reference.py pinned against
torch / the package's own tables, the partial-window rule, the checkpoint loader, the registration of the four entries, their
host-side guards, and the CLI on a stubbed embedder."""
import ctypes
import os
import re
import wave

import numpy as np
import pytest
import torch

from tests import _spk_reference as R

ENTRIES = ("l2s_wav_gain", "l2s_stft_mel_power", "l2s_lstm_layer", "l2s_spk_embed_head")
WORKED = {64000: ([0, 77, 154, 231], 64000), 68608: ([0, 77, 154, 231, 308], 74880), 31520: ([0, 77], 37920),
          31519: ([0], 31519), 16000: ([0], 25600)}


# ---- the partial-window rule --------------------------------------------------------------------------------------------------------
def test_partial_slices_worked_values_and_sweep():
    from lip2speech_unit_amd.speaker_encoder import compute_partial_slices
    for n, want in WORKED.items():
        assert compute_partial_slices(n) == want and R.partial_slices(n) == want, n
    lengths = [1, 16000, 25599, 25600, 31519, 31520, 37920, 64000, 68608]
    lengths += [int(v) for v in np.random.default_rng(2024).integers(1, 400000, size=200)]
    for n in lengths:
        starts, n_pad = compute_partial_slices(n)
        assert (starts, n_pad) == R.partial_slices(n), n
        assert starts[0] == 0 and n_pad >= 160 * (starts[-1] + 160) and n_pad >= n
        assert 1 + n_pad // 160 >= starts[-1] + 160                      # every window lies inside the mel frames
    with pytest.raises(ValueError):
        compute_partial_slices(0)


# ---- the yardstick itself -----------------------------------------------------------------------------------------------------------
def test_restated_lstm_is_torch_lstm():
    torch.manual_seed(5)
    ref = torch.nn.LSTM(40, 256, 3, batch_first=True).double()
    with torch.no_grad():
        for p in ref.parameters():
            p.uniform_(-3.0 / 16.0, 3.0 / 16.0)
    sd = {"lstm." + k: v.detach() for k, v in ref.state_dict().items()}
    x = torch.randn(3, 23, 40, dtype=torch.float64)
    with torch.no_grad():
        want, (hn, _) = ref(x)
    got = R.lstm(x, sd)
    assert float((got - want).abs().max()) < 1e-12
    assert float((got[:, -1] - hn[-1]).abs().max()) < 1e-12
    assert float(want.abs().max()) > 0.5                                  # the weight scale drives the gates out of the linear range


def test_restated_filterbank_is_the_package_slaney_function_at_40_bands():
    from lip2speech_unit_amd import audio
    fb = R.filterbank()
    own = audio.mel_filterbank(16000, 400, 40, 0.0, 8000.0)
    assert fb.shape == own.shape == (40, 201)
    assert np.abs(fb - own).max() < 1e-15 * max(1.0, np.abs(fb).max()) * 8
    assert (fb.sum(1) > 0).all()                                          # no empty band at 40 bands over 201 bins


def test_power_basis_is_the_windowed_dft():
    from lip2speech_unit_amd import speaker_encoder as se
    basis = se.power_basis()
    assert basis.shape == (400, 448)
    x = np.random.default_rng(0).standard_normal((5, 400))
    y = (x @ basis).reshape(5, 7, 2, 32)
    re, im = y[:, :, 0].reshape(5, 224), y[:, :, 1].reshape(5, 224)
    spec = np.fft.rfft(x * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)), axis=1)
    assert np.abs(re[:, :201] - spec.real).max() < 1e-11 and np.abs(im[:, 1:200] - spec.imag[:, 1:200]).max() < 1e-11
    assert not re[:, 201:].any() and not im[:, 201:].any() and not im[:, 0].any() and not im[:, 200].any()
    c, s = R._dft()                                                       # and the restatement's dense DFT is the same transform
    assert np.abs(x @ c - spec.real).max() < 1e-11 and np.abs(x @ s - spec.imag).max() < 1e-11


def test_restated_mel_shapes_gain_and_head_edge_cases():
    rng = np.random.default_rng(1)
    assert R.mel_power(rng.standard_normal(25600) * 0.1).shape == (161, 40)
    assert R.mel_power(rng.standard_normal(201)).shape == (2, 40)
    quiet, loud = rng.standard_normal(4000) * 1e-3, rng.standard_normal(4000) * 0.5
    g = R.gain(quiet)
    assert g > 1 and abs(10 * np.log10(np.mean((quiet * g) ** 2)) + 30.0) < 1e-9
    assert R.gain(loud) == 1.0 and R.gain(np.zeros(100)) == 1.0
    w, b = torch.randn(256, 256, dtype=torch.float64) / 16, torch.full((256,), -0.5, dtype=torch.float64)
    assert not R.head(torch.zeros(2, 256, dtype=torch.float64), w, b).any()           # all-zero ReLU output: zeros, not NaN
    v = R.head(torch.randn(5, 256, dtype=torch.float64) * 4, w, b)
    assert abs(float(torch.linalg.norm(v)) - 1.0) < 1e-12


def test_packed_lstm_operands_hold_the_torch_parameters():
    from lip2speech_unit_amd.speaker_encoder import pack_lstm_layer
    g = torch.Generator().manual_seed(3)
    w_ih, w_hh = torch.randn(1024, 40, generator=g), torch.randn(1024, 256, generator=g)
    b_ih, b_hh = torch.randn(1024, generator=g), torch.randn(1024, generator=g)
    w_ih_p, bias_p, w_hh_p = pack_lstm_layer(w_ih, w_hh, b_ih, b_hh)
    assert w_ih_p.shape == (1024, 40) and bias_p.shape == (1024,) and w_hh_p.shape == (256, 256, 4)
    for gate, u, k in ((0, 0, 0), (1, 5, 7), (2, 255, 39), (3, 128, 17)):
        assert w_ih_p[4 * u + gate, k] == w_ih[256 * gate + u, k]
        assert bias_p[4 * u + gate] == b_ih[256 * gate + u] + b_hh[256 * gate + u]
        assert w_hh_p[k, u, gate] == w_hh[256 * gate + u, k]
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (w_ih_p, bias_p, w_hh_p))


# ---- the parameter holder -----------------------------------------------------------------------------------------------------------
def test_state_dict_loads_from_both_checkpoint_shapes(tmp_path):
    from lip2speech_unit_amd import speaker_encoder as se
    sd = se.synthetic_state_dict()
    assert set(sd) == {f"lstm.{n}_l{l}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for l in range(3)} | {
        "linear.weight", "linear.bias"}
    assert sd["lstm.weight_ih_l0"].shape == (1024, 40) and sd["linear.weight"].shape == (256, 256)
    assert all(float(v.abs().max()) <= 3.0 / 16.0 for v in sd.values()) and float(sd["lstm.weight_hh_l1"].abs().max()) > 0.18
    full = dict(sd, similarity_weight=torch.tensor([10.0]), similarity_bias=torch.tensor([-5.0]))
    torch.save({"model_state": full, "step": 1}, tmp_path / "wrapped.pt")
    torch.save(full, tmp_path / "bare.pt")
    for name in ("wrapped.pt", "bare.pt"):
        enc = se.SpeakerEncoder().load_checkpoint(str(tmp_path / name))
        got = enc.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd), name
    small = {k: v[:, :128] if k.startswith("lstm.weight_hh") else v for k, v in sd.items()}
    with pytest.raises(ValueError):
        se.SpeakerEncoder().load_state_dict(small)
    with pytest.raises(RuntimeError):
        se.SpeakerEncoder().load_state_dict({k: v for k, v in sd.items() if k != "linear.bias"})


def test_host_class_refuses_host_tensors_and_bad_lengths():
    from lip2speech_unit_amd import speaker_encoder as se
    from lip2speech_unit_amd._lib import L2SError
    enc = se.SpeakerEncoder()
    with pytest.raises(L2SError):
        enc.embed(torch.zeros(1, 16000), [16000])
    with pytest.raises(L2SError):
        enc.pack("cpu")
    with pytest.raises(L2SError):
        se.PowerMel().mel_rows(torch.zeros(1, 16000))
    assert "webrtcvad" in se.__doc__ and "NOT built" in se.__doc__


# ---- registration and guards --------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_wrapped():
    from lip2speech_unit_amd import _lib, ops
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lip2speech_hip.h")).read()
    for e in ENTRIES:
        m = re.search(r"\bint\s+" + e + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, e
        assert e in _lib.SIGNATURES and len(_lib.SIGNATURES[e][0]) == len(m.group(1).split(",")), e
        name = e[len("l2s_"):]
        assert ops.ENTRY_OF[name] == e and callable(getattr(ops, name)) and hasattr(torch.ops.lip2speech, name)
    assert "helpers.py:185-198" in hdr and "DESIGN.md section 18" in hdr
    assert _lib.ABI_VERSION == 16
    f32, i32 = torch.zeros(4, 1024), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ops.L2SError):
        ops.wav_gain(torch.zeros(1, 100), torch.zeros(1), B=1, S=100)
    with pytest.raises(ops.L2SError):
        ops.stft_mel_power(torch.zeros(1, 1000), torch.zeros(1, 7, 40), torch.zeros(400, 448), torch.zeros(40, 201),
                           torch.zeros(40, 2, dtype=torch.int32), B=1, S=1000, T_rows=7)
    with pytest.raises(ops.L2SError):
        ops.lstm_layer(f32, i32, torch.zeros(256, 256, 4), S=4, T=1, h_last=torch.zeros(4, 256))
    with pytest.raises(ops.L2SError):
        ops.spk_embed_head(torch.zeros(4, 256), i32, i32, torch.zeros(256, 256), torch.zeros(256), torch.zeros(4, 256), B=4)


def test_argument_guards_return_codes_without_a_device():
    from lip2speech_unit_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()                       # an aligned host address: the guards return before any launch
    p = ctypes.addressof(buf)
    EINVAL, ESHAPE, EALIGN, EUNSUP = -1, -2, -3, -4
    assert lib.l2s_lstm_layer(None, 1024, 160, p, p, 1, 160, 256, p, None, None) == EINVAL
    assert lib.l2s_lstm_layer(p, 1024, 160, p, p, 1, 160, 256, None, None, None) == EINVAL        # no output at all
    assert lib.l2s_lstm_layer(p, 1024, 160, p, p, 0, 160, 256, p, None, None) == ESHAPE
    assert lib.l2s_lstm_layer(p, 1024, 160, p, p, 1, 0, 256, p, None, None) == ESHAPE
    assert lib.l2s_lstm_layer(p, 1020, 160, p, p, 1, 160, 256, p, None, None) == ESHAPE           # ldx < 4 hidden
    assert lib.l2s_lstm_layer(p, 1024, 159, p, p, 1, 160, 256, p, None, None) == ESHAPE           # fewer rows than steps
    assert lib.l2s_lstm_layer(p, 1024, 160, p, p, 1, 160, 128, p, None, None) == EUNSUP
    assert lib.l2s_lstm_layer(p, 1024, 160, p, p, 1, 160, 512, p, None, None) == EUNSUP
    assert lib.l2s_lstm_layer(p, 1026, 160, p, p, 1, 160, 256, p, None, None) == EALIGN
    assert lib.l2s_lstm_layer(p + 4, 1024, 160, p, p, 1, 160, 256, p, None, None) == EALIGN
    assert lib.l2s_spk_embed_head(p, 4, p, p, p, None, 1, 256, p, None) == EINVAL
    assert lib.l2s_spk_embed_head(p, 0, p, p, p, p, 1, 256, p, None) == ESHAPE
    assert lib.l2s_spk_embed_head(p, 4, p, p, p, p, 1, 128, p, None) == EUNSUP
    assert lib.l2s_spk_embed_head(p, 4, p + 2, p, p, p, 1, 256, p, None) == EALIGN
    assert lib.l2s_wav_gain(None, 0, 100, None, 1, 100, -30.0, p, None) == EINVAL
    assert lib.l2s_wav_gain(p, 0, 99, None, 1, 100, -30.0, p, None) == ESHAPE
    assert lib.l2s_wav_gain(p, 0, 100, None, 1, 100, -30.0, p + 2, None) == EALIGN
    order = ("wav", "i16", "ldw", "n", "nv", "sc", "B", "S", "basis", "fb", "fbr", "mel", "ldm", "T", "n_fft", "hop", "n_mels", "pad", "st")
    good = dict(wav=p, i16=0, ldw=1000, n=None, nv=None, sc=None, B=1, S=1000, basis=p, fb=p, fbr=p, mel=p, ldm=40, T=7, n_fft=400,
                hop=160, n_mels=40, pad=200, st=None)

    def mel(**k):
        return lib.l2s_stft_mel_power(*[{**good, **k}[a] for a in order])
    assert mel(wav=None) == EINVAL and mel(ldm=39) == ESHAPE and mel(ldw=999) == ESHAPE
    assert mel(n_fft=640) == EUNSUP and mel(n_mels=80, ldm=80) == EUNSUP and mel(hop=200) == EUNSUP and mel(pad=201) == EUNSUP
    assert mel(B=70000) == EUNSUP and mel(mel=p + 2) == EALIGN and mel(sc=p + 2) == EALIGN


# ---- the CLIs on injected parts -----------------------------------------------------------------------------------------------------
def _write_wav(path, pcm, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(pcm, np.int16).tobytes())


def test_cli_arguments_and_output_naming(tmp_path, capsys):
    from lip2speech_unit_amd import extract_spk_emb as cli
    a = cli.build_parser().parse_args(["in", "out", "--encoder", "e.pt"])
    assert vars(a) == {"audio_root": "in", "spk_emb_root": "out", "encoder": "e.pt", "batch": 64, "synthetic_weights": False}
    assert cli.output_path("/o", "/a", "/a/spk/x/clip.wav") == "/o/spk/x/clip.npy"
    root = tmp_path / "audio"
    (root / "s0").mkdir(parents=True)
    (root / "s1" / "deep").mkdir(parents=True)
    rng = np.random.default_rng(0)
    clips = {"s0/b.wav": rng.integers(-3000, 3000, 9000), "s0/a.wav": rng.integers(-3000, 3000, 20000),
             "s1/deep/c.wav": rng.integers(-3000, 3000, 400)}
    for rel, pcm in clips.items():
        _write_wav(root / rel, pcm)
    seen = []

    def stub(pcms):
        seen.extend(p.shape[0] for p in pcms)
        return np.stack([np.full(256, float(p.shape[0]), np.float32) for p in pcms])

    with pytest.raises(SystemExit):
        cli.main([str(root), str(tmp_path / "o")], embed=stub)                       # neither --encoder nor --synthetic_weights
    with pytest.raises(SystemExit):
        cli.main([str(root), str(tmp_path / "o"), "--encoder", str(tmp_path / "missing.pt")], embed=stub)
    written = cli.main([str(root), str(tmp_path / "spk_emb"), "--synthetic_weights", "--batch", "2"], embed=stub)
    assert seen == [20000, 9000, 400]                                                # sorted paths: s0/a, s0/b, s1/deep/c
    assert [os.path.relpath(w, tmp_path / "spk_emb") for w in written] == ["s0/a.npy", "s0/b.npy", "s1/deep/c.npy"]
    for rel, pcm in clips.items():
        v = np.load(tmp_path / "spk_emb" / (rel[:-4] + ".npy"))
        assert v.shape == (256,) and v.dtype == np.float32 and (v == len(pcm)).all()
    assert "embedded 3 clips" in capsys.readouterr().out
    _write_wav(root / "s0" / "rate.wav", clips["s0/b.wav"], rate=22050)              # no resampler: refused
    with pytest.raises(ValueError):
        cli.main([str(root), str(tmp_path / "o2"), "--synthetic_weights"], embed=stub)


def test_vocoder_inference_flag_is_absent_unless_given():
    from lip2speech_unit_amd import vocoder_inference
    p = vocoder_inference.build_parser()
    base = vars(p.parse_args(["c.json", "test.tsv", "dict.txt"]))
    assert "spk_emb_from_audio" not in base and "speaker_encoder" not in base
    a = vars(p.parse_args(["c.json", "test.tsv", "dict.txt", "--spk_emb_from_audio", "--speaker_encoder", "enc.pt"]))
    assert a["spk_emb_from_audio"] is True and a["speaker_encoder"] == "enc.pt"
    assert {k: v for k, v in a.items() if k not in ("spk_emb_from_audio", "speaker_encoder")} == base


def test_dataset_takes_the_embedding_from_the_hook(tmp_path, golden_dir):
    from lip2speech_unit_amd.data import MelCodeDataset, parse_manifest
    from tests._lrs3_sample import materialise
    lab, _, _ = materialise(str(tmp_path), golden_dir)
    files = parse_manifest(os.path.join(lab, "test.tsv"))
    calls = []

    def hook(path):
        calls.append(path)
        return np.full(256, 0.25, np.float64)

    kw = dict(code_dict_path=os.path.join(lab, "dict.unt.txt"))
    plain, hooked = MelCodeDataset(files, **kw), MelCodeDataset(files, spk_embedder=hook, **kw)
    f0, f1 = plain[0][0], hooked[0][0]
    assert calls == [files[0][0]] and f1["spkr"].dtype == np.float32 and (f1["spkr"] == 0.25).all()
    assert np.array_equal(f0["code"], f1["code"]) and np.array_equal(f0["mel"], f1["mel"]) and not (f0["spkr"] == 0.25).all()
