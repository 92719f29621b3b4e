"""Speaker embeddings from audio on the device (csrc/lstm.hip, csrc/spkemb.hip, speaker_encoder.SpeakerEncoder) against the float64
restatement tests/_spk_reference.py.

Weights are uniform in +-3/16: default initialisation (+-1/16) leaves |h| <= 0.09 and no gate saturates; at this scale |h|
reaches 0.77.  Every tolerance is the error the same recipe has when a CPU evaluates it in float32, times 4 - the factor covers
a different summation order and expf / tanhf implementation, not a wrong algorithm (a swapped gate or a dropped bias is off by
1e-2 or more).  Each test prints its figures before it asserts.

Measured on the MI355X: l2s_lstm_layer max |h - f64| 1.98e-6 over the 48 cases against E32 = 1.81e-6 (gate
7.25e-6); power mel 1.17e-6 band-relative against 7.3e-7 for the float32 CPU evaluation (gate 2.9e-6); embeddings 1.35e-7
against 8.5e-8 (gate 3.4e-7), 1 - cos <= 1.1e-13; head 7.6e-8 against the fixed 1e-6.
"""
import os
import wave

import numpy as np
import pytest
import torch

from tests import _spk_reference as R

pytestmark = pytest.mark.gpu

TILE = 16                                                 # sequences per workgroup of l2s_lstm_layer
S_MAX = 2 * TILE + 3
W_SCALE = 3.0 / 16.0
LSTM_T = (1, 2, 160)
LSTM_IN = (40, 256)


def _uniform(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 2.0 - 1.0) * W_SCALE


def _torch_lstm(params, dtype):
    w_ih, w_hh, b_ih, b_hh = params
    m = torch.nn.LSTM(w_ih.shape[1], 256, 1, batch_first=True).to(dtype)
    with torch.no_grad():
        m.weight_ih_l0.copy_(w_ih), m.weight_hh_l0.copy_(w_hh), m.bias_ih_l0.copy_(b_ih), m.bias_hh_l0.copy_(b_hh)
    return m


@pytest.fixture(scope="module")
def lstm_cases():
    """{(T, in): (x fp32 [S_MAX, T, in], params, h float64 [S_MAX, T, 256])} and E32, the largest max-abs error of torch's own
    fp32 CPU nn.LSTM against the float64 one over these inputs.  Computed once; a case with fewer sequences uses a prefix."""
    gen = torch.Generator().manual_seed(11)
    params = {n_in: (_uniform(gen, 1024, n_in), _uniform(gen, 1024, 256), _uniform(gen, 1024), _uniform(gen, 1024)) for n_in in LSTM_IN}
    cases, e32 = {}, 0.0
    with torch.no_grad():
        for n_in in LSTM_IN:
            m64, m32 = _torch_lstm(params[n_in], torch.float64), _torch_lstm(params[n_in], torch.float32)
            for T in LSTM_T:
                x = torch.randn(S_MAX, T, n_in, generator=gen)
                ref = m64(x.double())[0]
                e32 = max(e32, float((m32(x)[0].double() - ref).abs().max()))
                cases[T, n_in] = (x, params[n_in], ref)
    assert float(cases[160, 40][2].abs().max()) > 0.5     # the gates do leave their linear range
    return cases, e32


def _device_layer(x, params, row_off=None, S=None, T=None, want_seq=True, want_last=True):
    """One layer on the device: x fp32 [rows, in] on the host -> (h_seq [S, T, 256] or None, h_last [S, 256] or None)."""
    from lip2speech_unit_amd import ops
    from lip2speech_unit_amd.speaker_encoder import input_projection, pack_lstm_layer
    w_ih_p, bias_p, w_hh_p = (t.cuda() for t in pack_lstm_layer(*params))
    xp = input_projection(x.cuda().contiguous(), w_ih_p, bias_p)
    h_seq = torch.full((S, T, 256), float("nan"), device="cuda") if want_seq else None
    h_last = torch.full((S, 256), float("nan"), device="cuda") if want_last else None
    ops.lstm_layer(xp, torch.tensor(row_off, dtype=torch.int32).cuda(), w_hh_p, S=S, T=T, h_seq=h_seq, h_last=h_last)
    torch.cuda.synchronize()
    return (None if h_seq is None else h_seq.cpu()), (None if h_last is None else h_last.cpu())


@pytest.mark.parametrize("with_seq", [True, False])
@pytest.mark.parametrize("n_in", LSTM_IN)
@pytest.mark.parametrize("T", LSTM_T)
@pytest.mark.parametrize("S", [1, TILE - 1, TILE + 1, S_MAX])
def test_lstm_layer_against_float64(lstm_cases, S, T, n_in, with_seq):
    cases, e32 = lstm_cases
    x, params, ref = cases[T, n_in]
    h_seq, h_last = _device_layer(x[:S].reshape(S * T, n_in), params, [s * T for s in range(S)], S, T, want_seq=with_seq)
    err = float((h_last.double() - ref[:S, -1]).abs().max())
    if with_seq:
        err = max(err, float((h_seq.double() - ref[:S]).abs().max()))
        assert torch.equal(h_seq[:, -1], h_last)
    print(f"S{S} T{T} in{n_in} seq{int(with_seq)}: max |h - f64| {err:.3e}, E32 {e32:.3e}, gate {4 * e32:.3e}")
    assert err <= 4.0 * e32, (err, e32)


def test_lstm_layer_overlapping_and_unordered_row_offsets(lstm_cases):
    """Windows 0 / 77 / 154 of ONE clip's projection rows, gathered by offset in a non-monotone order with repeats."""
    cases, e32 = lstm_cases
    _, params, _ = cases[160, 40]
    x = torch.randn(154 + 160, 40, generator=torch.Generator().manual_seed(12))
    offs = [154, 0, 77, 77, 0]
    with torch.no_grad():
        ref = _torch_lstm(params, torch.float64)(torch.stack([x[o:o + 160] for o in offs]).double())[0]
    h_seq, h_last = _device_layer(x, params, offs, len(offs), 160)
    err = float((h_seq.double() - ref).abs().max())
    print(f"overlapping offsets {offs}: max |h - f64| {err:.3e}, gate {4 * e32:.3e}")
    assert err <= 4.0 * e32
    assert torch.equal(h_seq[1], h_seq[4]) and torch.equal(h_seq[2], h_seq[3]) and torch.equal(h_last[2], h_last[3])


def test_lstm_layer_is_independent_of_tile_mates_and_repeatable(lstm_cases):
    cases, _ = lstm_cases
    x, params, _ = cases[160, 40]
    T = 160
    alone, _ = _device_layer(x[:1].reshape(T, 40), params, [0], 1, T)
    full, last = _device_layer(x.reshape(S_MAX * T, 40), params, [s * T for s in range(S_MAX)], S_MAX, T)
    again, last2 = _device_layer(x.reshape(S_MAX * T, 40), params, [s * T for s in range(S_MAX)], S_MAX, T)
    assert torch.equal(alone[0], full[0])
    assert torch.equal(full, again) and torch.equal(last, last2)
    moved, _ = _device_layer(x.reshape(S_MAX * T, 40), params, [(S_MAX - 1 - s) * T for s in range(S_MAX)], S_MAX, T)
    assert torch.equal(moved.flip(0), full)               # a sequence's bits do not depend on its place in the tile either


def test_spk_embed_head_against_float64():
    """Clips with 1, 2 and 5 windows and one whose ReLU output is all zero (h = 0 under a negative bias) in one batch.  There the
    mean is the zero vector and the final division is 0 / 0: the kernel and the restatement both return zeros."""
    from lip2speech_unit_amd import ops
    gen = torch.Generator().manual_seed(13)
    w, b = _uniform(gen, 256, 256), -0.05 - torch.rand(256, generator=gen) * 0.1
    h = (torch.rand(10, 256, generator=gen) * 2.0 - 1.0) * 0.8
    h[3:5] = 0.0
    first, count = [0, 1, 5, 3], [1, 2, 5, 2]             # clip 3 = rows 3, 4: zeros; not in row order on purpose
    out = torch.full((4, 256), float("nan"), device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()   # noqa: E731
    ops.spk_embed_head(h.cuda(), i32(first), i32(count), w.t().contiguous().cuda(), b.cuda(), out, B=4)
    out = out.cpu()
    for c, (f, n) in enumerate(zip(first, count)):
        ref = R.head(h[f:f + n].double(), w.double(), b.double())
        err = float((out[c].double() - ref).abs().max())
        print(f"clip {c} ({n} windows): max |e - f64| {err:.3e}, |e| {float(out[c].norm()):.7f}")
        assert err <= 1e-6
    assert not out[3].any() and abs(float(out[2].double().norm()) - 1.0) < 1e-6


# ---- gain and power mel --------------------------------------------------------------------------------------------------------------
def _speechlike(n, seed, level=0.1):
    """int16 noise under a slow envelope with a stretch of digital silence in the middle."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    x = rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) + 0.5 * np.sin(2 * np.pi * 440.0 * t)
    if n >= 16000:
        x[n // 2: n // 2 + 4000] = 0.0
    return np.clip(np.round(x * level * 32768.0), -32768, 32767).astype(np.int16)


def _band_relative(got, ref):
    """max over bands of max_t |got - ref| / max_t |ref| (bands without energy: absolute)."""
    scale = np.abs(ref).max(0)
    return float((np.abs(got - ref).max(0) / np.where(scale > 0, scale, 1.0)).max())


def test_wav_gain_against_float64():
    from lip2speech_unit_amd import ops
    clips = [_speechlike(20000, 1, 0.002), _speechlike(30000, 2, 0.3), np.zeros(5000, np.int16), _speechlike(777, 3, 0.01)]
    S = max(c.shape[0] for c in clips)
    batch = np.full((len(clips), S), 4321, np.int16)      # garbage behind every clip
    for i, c in enumerate(clips):
        batch[i, : c.shape[0]] = c
    lens = torch.tensor([c.shape[0] for c in clips], dtype=torch.int32).cuda()
    want = np.array([R.gain(c.astype(np.float64) / 32768.0) for c in clips])
    for x in (torch.from_numpy(batch).cuda(), (torch.from_numpy(batch).float() / 32768.0).cuda()):
        g = torch.empty(len(clips), device="cuda")
        ops.wav_gain(x, g, B=len(clips), S=S, n_samples=lens)
        got = g.cpu().numpy().astype(np.float64)
        print("gain", got, "f64", want)
        assert np.abs(got / want - 1.0).max() <= 2.0 ** -23   # one rounding of the float64 factor to float32
    assert want[0] > 1.0 and want[1] == 1.0 and want[2] == 1.0


def test_power_mel_against_float64():
    """Clip lengths {25600, 64000, 74880, 201} and a clip of 200 samples (no valid reflection: zero rows) in one ragged batch, from
    int16 and from fp32.  Per band, relative to the band's largest value in the clip (the outputs are linear power; an fp32
    dense DFT is accurate relative to the frame's energy, not to each bin): gpu <= 4 x the float32 CPU evaluation.  Frames of
    digital silence are exactly zero in float64, float32 and on the device - the absolute floor is 0."""
    from lip2speech_unit_amd.speaker_encoder import PowerMel
    lens = [25600, 64000, 74880, 201, 200]
    clips = [_speechlike(n, 20 + i) for i, n in enumerate(lens)]
    S = max(lens)
    batch = np.full((len(clips), S), -1234, np.int16)
    for i, c in enumerate(clips):
        batch[i, : c.shape[0]] = c
    n_dev = torch.tensor(lens, dtype=torch.int32).cuda()
    pm = PowerMel()
    out16 = pm.mel_rows(torch.from_numpy(batch).cuda(), n_samples=n_dev).cpu().numpy()
    out32 = pm.mel_rows((torch.from_numpy(batch).float() / 32768.0).cuda(), n_samples=n_dev).cpu().numpy()
    assert out16.shape == (5, 1 + S // 160, 40) and np.array_equal(out16, out32)
    worst32 = 0.0
    errs = []
    for i, c in enumerate(clips[:4]):
        x = c.astype(np.float64) / 32768.0
        ref = R.mel_power(x)
        T = ref.shape[0]
        assert T == 1 + lens[i] // 160
        e32 = _band_relative(R.mel_power(x, torch.float32).astype(np.float64), ref)
        err = _band_relative(out16[i, :T].astype(np.float64), ref)
        silent = ~ref.any(1)
        print(f"n {lens[i]}: band-relative gpu {err:.3e}, f32 cpu {e32:.3e}; {int(silent.sum())} silent frames")
        assert not out16[i, :T][silent].any() and not out16[i, T:].any()
        if lens[i] >= 16000:
            assert silent.sum() >= 10
        worst32 = max(worst32, e32)
        errs.append(err)
    print(f"gate {4 * worst32:.3e}")
    assert max(errs) <= 4.0 * worst32
    assert not out16[4].any()                             # n <= 200: no frames
    alone = pm.mel_rows(torch.from_numpy(clips[1][None]).cuda()).cpu().numpy()
    assert np.array_equal(alone[0], out16[1, : alone.shape[1]])


def test_power_mel_zero_extension_and_scale():
    """The analysis length beyond the real samples (a clip shorter than its partial window) and the per-clip factor."""
    from lip2speech_unit_amd.speaker_encoder import PowerMel
    c = _speechlike(16000, 31, 0.004)
    x = c.astype(np.float64) / 32768.0
    g = np.float32(R.gain(x))
    ref = R.mel_power(np.concatenate([(x.astype(np.float32) * g).astype(np.float64), np.zeros(9600)]))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()   # noqa: E731
    buf = np.concatenate([c, np.full(3000, 999, np.int16)])[None]
    got = PowerMel().mel_rows(torch.from_numpy(buf).cuda(), n_samples=i32([25600]), n_valid=i32([16000]),
                              scale=torch.tensor([g]).cuda(), T_rows=161).cpu().numpy()[0].astype(np.float64)
    e32 = _band_relative(R.mel_power(np.concatenate([(x.astype(np.float32) * g).astype(np.float64), np.zeros(9600)]),
                                     torch.float32).astype(np.float64), ref)
    err = _band_relative(got, ref)
    print(f"zero-extended, scaled: band-relative gpu {err:.3e}, f32 cpu {e32:.3e}")
    assert g > 1.0 and err <= 4.0 * e32 and not got[102:].any() and got[:40].any(1).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder():
    from lip2speech_unit_amd import speaker_encoder as se
    enc = se.SpeakerEncoder()
    enc.load_state_dict(se.synthetic_state_dict())
    return enc.eval()


@pytest.fixture(scope="module")
def clips(golden_dir):
    a = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    lrs3 = [a[f"c{i}_pcm"] for i in range(5)]
    synth = [_speechlike(16000, 41, 0.004), _speechlike(31519, 42, 0.3), _speechlike(31520, 43, 0.05), _speechlike(68608, 44, 0.02)]
    return lrs3 + synth


def test_embed_against_float64(encoder, clips):
    sd = {k: v.detach() for k, v in encoder.state_dict().items()}
    lens = [c.shape[0] for c in clips]
    S = max(lens)
    batch = np.full((len(clips), S), 77, np.int16)
    for i, c in enumerate(clips):
        batch[i, : c.shape[0]] = c
    out = encoder.embed(torch.from_numpy(batch).cuda(), lens).cpu()
    assert out.shape == (len(clips), 256) and out.dtype == torch.float32
    gains = [R.gain(c.astype(np.float64) / 32768.0) for c in clips]
    assert gains[5] > 1.0 and gains[6] == 1.0             # the quiet and the loud synthetic clip: both sides of the increase-only rule
    e32, errs = 0.0, []
    for i, c in enumerate(clips):
        x = c.astype(np.float64) / 32768.0
        ref = R.embed(x, sd)
        e32 = max(e32, float(np.abs(R.embed(x, sd, torch.float32).astype(np.float64) - ref).max()))
        got = out[i].double().numpy()
        cos = float(got @ ref / (np.linalg.norm(got) * np.linalg.norm(ref)))
        errs.append(float(np.abs(got - ref).max()))
        print(f"clip {i} ({lens[i]} samples, {len(R.partial_slices(lens[i])[0])} windows, gain {gains[i]:.3f}): "
              f"max |gpu - f64| {errs[-1]:.3e}, 1 - cos {1 - cos:.3e}, |v| {np.linalg.norm(got):.8f}")
        assert cos >= 1.0 - 1e-6
        alone = encoder.embed(torch.from_numpy(c[None]).cuda(), [lens[i]]).cpu()
        assert torch.equal(alone[0], out[i]), i
    print(f"f32 cpu pipeline max |e32 - f64| {e32:.3e}, gate {4 * e32:.3e}")
    assert max(errs) <= 4.0 * e32
    f32 = encoder.embed((torch.from_numpy(batch).float() / 32768.0).cuda(), lens).cpu()
    assert torch.equal(f32, out)                          # int16 and fp32 input of the same samples
    small = encoder.embed(torch.from_numpy(batch).cuda(), lens, max_seqs=7).cpu()
    assert torch.equal(small, out)                        # chunking the sequences changes nothing


def test_cli_writes_what_embed_returns(tmp_path, encoder, clips):
    from lip2speech_unit_amd import extract_spk_emb
    root = tmp_path / "audio" / "spk"
    root.mkdir(parents=True)
    for name, pcm in (("a", clips[2]), ("b", clips[7])):
        with wave.open(str(root / (name + ".wav")), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
            w.writeframes(pcm.tobytes())
    extract_spk_emb.main([str(tmp_path / "audio"), str(tmp_path / "spk_emb"), "--synthetic_weights", "--batch", "2"])
    for name, pcm in (("a", clips[2]), ("b", clips[7])):
        v = np.load(tmp_path / "spk_emb" / "spk" / (name + ".npy"))
        assert v.shape == (256,) and v.dtype == np.float32 and abs(float(np.linalg.norm(v.astype(np.float64))) - 1.0) <= 1e-6
        want = encoder.embed(torch.from_numpy(pcm[None]).cuda(), [pcm.shape[0]])[0].cpu().numpy()
        assert np.array_equal(v, want)
        assert np.array_equal(encoder.embed_file(str(root / (name + ".wav"))), want)


def test_vocoder_inference_takes_the_embedding_from_audio(tmp_path, golden_dir):
    """vocoder_inference --spk_emb_from_audio writes the same bytes as the same CLI reading the spk_emb/ tree that extract_spk_emb
    wrote for the data set: the flag computes per clip what the data-set tool computes in batches."""
    import json
    import shutil

    from scipy.io import wavfile

    from lip2speech_unit_amd import extract_spk_emb
    from lip2speech_unit_amd import vocoder_inference as s2
    from tests import _mel_reference as mr
    from tests.test_models_gpu import VOC_H
    root = str(tmp_path / "d")
    lab, _ = mr.materialise_audio_dataset(root, golden_dir, with_mel=True)
    cfg = str(tmp_path / "cfg.json")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000), open(cfg, "w"))
    args = [cfg, os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "-n", "-1", "--synthetic_weights"]
    s2.main(args + ["--output_dir", str(tmp_path / "flag"), "--spk_emb_from_audio"])
    s2.main(args + ["--output_dir", str(tmp_path / "stored")])
    written = extract_spk_emb.main([os.path.join(root, "audio"), str(tmp_path / "spk_out"), "--synthetic_weights", "--batch", "3"])
    assert len(written) == 5
    shutil.copytree(str(tmp_path / "spk_out"), os.path.join(root, "spk_emb"), dirs_exist_ok=True)
    s2.main(args + ["--output_dir", str(tmp_path / "tool")])
    n = 0
    for dirpath, _, files in os.walk(str(tmp_path / "flag" / "pred_wav")):
        for f in files:
            rel = os.path.relpath(os.path.join(dirpath, f), str(tmp_path / "flag"))
            a, b, c = (wavfile.read(str(tmp_path / t / rel))[1] for t in ("flag", "tool", "stored"))
            assert np.array_equal(a, b), rel
            assert not np.array_equal(a, c), rel                      # the fixture's own embedding is another vector
            n += 1
    assert n == 5
