"""Whisper on the device against the float64 restatement (tests/_whisper_reference.py, pinned to transformers by
tests/test_whisper_cpu.py): the log-mel front end, the encoder, teacher-forced logits, greedy decoding and the CLIs.

Bounds: 8 x the largest error measured on an MI355X (MEASURED), under a ceiling computed on the CPU that no measurement can loosen:
for the front end's fp32 values 4 x the float32 CPU evaluation of the same clip, for the model's quantities 4 x the error of the
restatement itself with weights and features rounded to the 16-bit type (eps).  Greedy ids are compared exactly where the CPU test
shows the case to be decisive: every step for fp16, the decisive steps for bf16.  Every figure is printed before it is asserted."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import asr_text, ops  # noqa: E402
from lip2speech_unit_amd import whisper as W  # noqa: E402
from tests import _whisper_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [ops.F16, ops.BF16]
DNAME = {ops.F16: "f16", ops.BF16: "bf16"}
TORCH16 = {ops.F16: torch.float16, ops.BF16: torch.bfloat16}
# largest |device - float64| seen on an MI355X over the cases of this file (the MEASURE lines)
MEASURED = {
    "features_f32": 1.53e-5,                           # the clip with digital silence; 2.4e-7 .. 1.5e-5 over the clips, float32 CPU 2.4e-7 .. 1.5e-5
    "encoder_f16": 8.17e-3, "encoder_bf16": 3.90e-2,   # eps (CPU, 16-bit restatement) 6.2e-3 / 3.8e-2
    "logits_f16": 2.81e-2, "logits_bf16": 2.21e-1,     # eps 2.86e-2 / 2.79e-1
}
NEVER = 331                    # a suppressed id as eot: the decode runs its 10 steps


def _bound(key, value, ceiling):
    print(f"MEASURE {key} {value:.3e} ceiling {ceiling:.3e}")
    return min(8.0 * MEASURED[key], ceiling)


def _r16(dtype):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(TORCH16[dtype]).double().numpy()


@pytest.fixture(scope="module")
def case():
    return R.tiny_case()


_EPS = {}


def _eps(case, dtype):
    """CPU: (eps of the encoder output, eps of the logits) of the restatement with 16-bit weights and features."""
    if dtype not in _EPS:
        r16 = _r16(dtype)
        sdq = R.round_state_dict(case["sd"], r16)
        e_enc = max(float(np.abs(R.encoder(sdq, R.TINY_DIMS, r16(f)) - x).max()) for f, x in zip(case["feats"], case["xa"]))
        _EPS[dtype] = (e_enc, R.quantised_logit_error(case, r16)[0])
    return _EPS[dtype]


_MODELS = {}


def _model(case, dtype):
    if dtype not in _MODELS:
        m = W.Whisper(W.WhisperDims(**R.TINY_DIMS), dtype=dtype)
        m.load_state_dict({k: torch.from_numpy(v).float() for k, v in case["sd"].items()})
        _MODELS[dtype] = m.cuda().eval()
    return _MODELS[dtype]


def _batch(clips, S=None, seed=5):
    """int16 [B, S] with seeded noise behind each clip's end, and the lengths."""
    S = S or max(len(c) for c in clips)
    buf = np.random.default_rng(seed).integers(-20000, 20000, size=(len(clips), S), dtype=np.int16)
    for b, c in enumerate(clips):
        buf[b, : len(c)] = c
    return buf, [len(c) for c in clips]


def _config(eot, max_new=R.TINY_STEPS):
    return asr_text.WhisperDecodeConfig(sot_sequence=R.TINY_SOT, eot=eot, suppress=R.TINY_SUPPRESS, begin_suppress=R.TINY_BEGIN_SUPPRESS,
                                        max_new_tokens=max_new)


# ---- front end ---------------------------------------------------------------------------------------------------------------------

def _frontend_clips(golden_dir):
    g = np.load(os.path.join(golden_dir, "mel_lrs3_audio.npz"))
    clips = [g[f"c{i}_pcm"] for i in range(5)]
    t = np.arange(40000) / 16000.0
    tone = np.round(9000.0 * np.sin(2 * np.pi * 330.0 * t)).astype(np.int16)
    tone[12000:25000] = 0                                       # digital silence: log10 hits its floor and the max - 8 clamp binds
    rng = np.random.default_rng(3)
    clips.append(tone)
    for n in (0, 1, 200, 201):
        clips.append(rng.integers(-20000, 20000, size=n, dtype=np.int16))
    return clips


@pytest.fixture(scope="module")
def frontend_case(golden_dir):
    clips = _frontend_clips(golden_dir)
    wav = [c.astype(np.float64) / 32768.0 for c in clips]
    return clips, [R.log_mel(w) for w in wav], [R.log_mel_f32(w) for w in wav]


def _check_features(out16, out32, refs, refs32, dtype, B):
    out32 = out32.view(B, 3000, 80).double().cpu().numpy()
    pad = out16.view(B, 3000, W.MEL_LD)[:, :, 80:]
    assert not pad.any(), "the padding columns of conv1's operand must be zero"
    assert torch.equal(out16.view(B, 3000, W.MEL_LD)[:, :, :80].cpu(), torch.from_numpy(out32).to(TORCH16[dtype])), "one rounding of the fp32 value"
    for b in range(B):
        err = float(np.abs(out32[b] - refs[b]).max())
        e32 = float(np.abs(refs32[b].astype(np.float64) - refs[b]).max())
        assert err <= _bound("features_f32", err, 4.0 * max(e32, 2.0 ** -23)), b


@pytest.mark.parametrize("i16", [True, False], ids=["int16_in", "fp32_in"])
def test_logmel_against_float64(frontend_case, i16):
    clips, refs, refs32 = frontend_case
    buf, lens = _batch(clips)
    wav = torch.from_numpy(buf).cuda() if i16 else torch.from_numpy(buf.astype(np.float32) / 32768.0).cuda()
    ns = torch.tensor(lens, dtype=torch.int32).cuda()
    lm = W.LogMel()
    o16, o32 = lm.features(wav, ns, dtype=ops.F16, want_f32=True)
    torch.cuda.synchronize()
    # the digital silence reaches the clamp: the floor value (max - 8 + 4) / 4 is present in the reference
    assert (refs[5] == refs[5].min()).sum() > 80 * 50 and refs[5].min() == pytest.approx(refs[5].max() - 2.0)
    _check_features(o16, o32, refs, refs32, ops.F16, len(clips))
    # a clip's bytes alone = in the batch; bf16 output is the same fp32 values rounded the other way
    for b in (0, 5, 7):
        a16, a32 = lm.features(wav[b:b + 1, : max(lens[b], 1)].contiguous(), ns[b:b + 1], dtype=ops.F16, want_f32=True)
        assert torch.equal(a32, o32.view(len(clips), 3000, 80)[b]) and torch.equal(a16, o16.view(len(clips), 3000, W.MEL_LD)[b])
    b16, b32 = lm.features(wav, ns, dtype=ops.BF16, want_f32=True)
    assert torch.equal(b32, o32) and torch.equal(b16[:, :80], o32.to(torch.bfloat16))


def test_logmel_full_window_and_limits():
    clip = np.random.default_rng(9).integers(-20000, 20000, size=480000, dtype=np.int16)
    lm = W.LogMel()
    o16, o32 = lm.features(torch.from_numpy(clip[None]).cuda(), None, dtype=ops.F16, want_f32=True)
    w = clip.astype(np.float64) / 32768.0
    _check_features(o16, o32, [R.log_mel(w)], [R.log_mel_f32(w)], ops.F16, 1)
    e16 = lm.features(torch.zeros(2, 0, device="cuda"), None)                # no samples at all
    assert (e16[:, :80].float() == -1.5).all()
    with pytest.raises(ValueError):
        lm.features(torch.zeros(1, 480001, device="cuda"))
    with pytest.raises(ops.L2SError):
        lm.features(torch.zeros(1, 100))


# ---- the model, stage by stage -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
def test_encoder_and_teacher_forced_logits_against_float64(case, dtype):
    m = _model(case, dtype)
    buf, lens = _batch(case["clips"])
    enc32, enc16 = m.encode(torch.from_numpy(buf).cuda(), torch.tensor(lens, dtype=torch.int32).cuda())
    e_enc, e_log = _eps(case, dtype)
    err = max(float(np.abs(enc32[b].double().cpu().numpy() - case["xa"][b]).max()) for b in range(3))
    assert err <= _bound("encoder_" + DNAME[dtype], err, 4.0 * e_enc)
    P = len(R.TINY_SOT)
    toks = np.array([list(R.TINY_SOT) + f[0][:-1] for f in case["free"]])
    got = m.teacher_forced_logits(enc16, torch.from_numpy(toks)).double().cpu().numpy()
    ref = np.stack([R.decoder_logits(case["sd"], R.TINY_DIMS, case["xa"][b], toks[b]) for b in range(3)])
    err = float(np.abs(got - ref).max())
    assert err <= _bound("logits_" + DNAME[dtype], err, 4.0 * e_log)
    # at every decisive step (all of them for fp16, tests/test_whisper_cpu.py) the device's choice is the float64 id
    forbid = np.zeros(R.TINY_DIMS["n_vocab"], bool)
    forbid[list(R.TINY_SUPPRESS)] = True
    first = forbid.copy()
    first[list(R.TINY_BEGIN_SUPPRESS)] = True
    n_checked = 0
    for b in range(3):
        for s in range(R.TINY_STEPS):
            if case["free"][b][1][s] >= 8.0 * e_log:
                ids, _, _ = R.masked_argmax(got[b, P - 1 + s][None], first if s == 0 else forbid)
                assert ids[0] == case["free"][b][0][s], (b, s)
                n_checked += 1
    assert n_checked == (30 if dtype == ops.F16 else 11)


# ---- greedy decoding ---------------------------------------------------------------------------------------------------------------

def _decode(case, dtype, eot, which=(0, 1, 2), **kw):
    m = _model(case, dtype)
    asr = W.WhisperASR(m, _config(eot), **kw)
    buf, lens = _batch([case["clips"][i] for i in which], S=max(R.CLIP_SAMPLES))
    ids, lengths, mean_lp = asr.tokens(torch.from_numpy(buf).cuda(), lens)
    return ids, lengths.cpu().tolist(), mean_lp.double().cpu().numpy(), asr


def test_greedy_ids_equal_float64_fp16(case):
    ids, lengths, mean_lp, asr = _decode(case, ops.F16, NEVER)
    assert ids == [f[0] for f in case["free"]] and lengths == [R.TINY_STEPS] * 3 and asr.steps_run == R.TINY_STEPS
    _, e_log = _eps(case, ops.F16)
    ref = np.array([f[2] / (R.TINY_STEPS + 1) for f in case["free"]])
    err = float(np.abs(mean_lp - ref).max())
    print(f"mean log-probability: max error {err:.3e}, bound {2 * e_log:.3e}")
    assert err <= 2.0 * e_log                        # a log softmax moves by at most twice the largest logit error


def test_termination_fp16(case):
    """eot = an ordinary id of the float64 decode: the clips end at steps 4, 6 and 6, eot follows, and the loop stops before the cap."""
    ids, lengths, mean_lp, asr = _decode(case, ops.F16, R.TINY_EOT)
    assert ids == [e[0] for e in case["ended"]] and lengths == [4, 6, 6]
    assert asr.steps_run == 8 < R.TINY_STEPS                                  # polled every 8 steps
    S = next(iter(asr._states.values()))["S"]
    P = len(R.TINY_SOT)
    toks = S["tokens"][:, P - 1:P - 1 + 8].cpu().numpy()
    for b, n in enumerate(lengths):
        assert (toks[b, n:] == R.TINY_EOT).all()
    _, e_log = _eps(case, ops.F16)
    ref = np.array([e[2] / (len(e[0]) + 1) for e in case["ended"]])
    assert np.abs(mean_lp - ref).max() <= 2.0 * e_log
    ids1, lengths1, mean1, asr1 = _decode(case, ops.F16, R.TINY_EOT, poll=1)
    assert ids1 == ids and lengths1 == lengths and asr1.steps_run == 7 and np.array_equal(mean1, mean_lp)


@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
def test_greedy_is_the_same_alone_plain_and_polled(case, dtype):
    ids, lengths, mean_lp, _ = _decode(case, dtype, R.TINY_EOT)
    idp, lengthp, meanp, _ = _decode(case, dtype, R.TINY_EOT, graph=False)
    assert idp == ids and lengthp == lengths and np.array_equal(meanp, mean_lp), "graph replay and plain launches differ"
    id1, _, mean1, _ = _decode(case, dtype, R.TINY_EOT, poll=1)
    assert id1 == ids and np.array_equal(mean1, mean_lp)
    for b in range(3):
        ida, _, meana, _ = _decode(case, dtype, R.TINY_EOT, which=(b,))
        assert ida[0] == ids[b] and meana[0] == mean_lp[b], b
    free, _, _, _ = _decode(case, dtype, NEVER)
    for b in range(3):                                                        # a clip's ids do not depend on when its mates end
        assert free[b][: len(ids[b])] == ids[b]


def test_graph_is_recaptured_when_the_weights_change(case):
    m = W.Whisper(W.WhisperDims(**R.TINY_DIMS), dtype=ops.F16)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in case["sd"].items()})
    m.cuda().eval()
    asr = W.WhisperASR(m, _config(NEVER))
    buf, lens = _batch(case["clips"])
    wav = torch.from_numpy(buf).cuda()
    assert asr.tokens(wav, lens)[0] == [f[0] for f in case["free"]]
    other = R.tiny_state_dict(20)
    m.load_state_dict({k: torch.from_numpy(v).float() for k, v in other.items()})
    got = asr.tokens(wav, lens)[0]
    plain = W.WhisperASR(m, _config(NEVER), graph=False).tokens(wav, lens)[0]
    assert got == plain and got != [f[0] for f in case["free"]]


# ---- CLIs --------------------------------------------------------------------------------------------------------------------------

def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(pcm.tobytes())


def _tiny_files(case, tmp_path):
    m = _model(case, ops.F16)
    ck = tmp_path / "tiny.pt"
    W.save_openai_checkpoint(m, str(ck))
    # a vocabulary whose tokens are words, so that transcripts have several of them
    import base64
    vocab = tmp_path / "tiny.tiktoken"
    vocab.write_bytes(b"".join(base64.b64encode(f" w{i}".encode()) + f" {i}\n".encode() for i in range(329)))
    cfg = tmp_path / "decode.json"
    cfg.write_text(json.dumps({"decoder_start_token_id": R.TINY_SOT[0], "forced_decoder_ids": [[1, R.TINY_SOT[1]]], "eos_token_id": R.TINY_EOT,
                               "suppress_tokens": list(R.TINY_SUPPRESS), "begin_suppress_tokens": list(R.TINY_BEGIN_SUPPRESS)}))
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    for i, c in enumerate(case["clips"]):
        _write_wav(wavs / f"clip{i}.wav", c)
    return ck, vocab, cfg, wavs


def _cli(*args):
    r = subprocess.run([sys.executable, "-m", *args], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_transcribe_and_evaluate_wer_clis(case, tmp_path):
    ck, vocab, cfg, wavs = _tiny_files(case, tmp_path)
    m = _model(case, ops.F16)
    config = asr_text.WhisperDecodeConfig.from_generation_config(str(cfg), max_new_tokens=R.TINY_STEPS)
    asr = W.WhisperASR(m, config, vocab=str(vocab))
    buf, lens = _batch(case["clips"])
    want = asr.run(torch.from_numpy(buf).cuda(), lens)
    assert want[0] == "w193 w122 w71 w71"
    out = tmp_path / "out"
    _cli("lip2speech_unit_amd.transcribe", str(wavs), "--whisper", str(ck), "--vocab", str(vocab), "--decode_config", str(cfg),
         "--max_new_tokens", str(R.TINY_STEPS), "--output_dir", str(out))
    for i in range(3):
        assert (out / "pred_asr" / f"clip{i}.txt").read_text().strip() == want[i]
    refs = ["w193 w122 w71 w71", "w193 w122 w71", "nothing alike here at all"]
    tr = tmp_path / "transcripts"
    tr.mkdir()
    for i, r in enumerate(refs):
        (tr / f"clip{i}.txt").write_text(r + "\n")
    ev = tmp_path / "eval"
    _cli("lip2speech_unit_amd.evaluate", str(wavs), str(wavs), "--output_dir", str(ev), "--wer", "--whisper", str(ck), "--vocab", str(vocab),
         "--decode_config", str(cfg), "--max_new_tokens", str(R.TINY_STEPS), "--transcripts", str(tr))
    got = json.load(open(ev / "eval-wer.json"))
    exp = asr_text.wer(refs, want)
    assert got["wer"] == pytest.approx(exp["wer"]) and got["n_err"] == exp["n_err"] and got["n_total"] == exp["n_total"] == 12
    assert [c["errors"] for c in got["clips"]] == [0, 3, 6] and [c["hyp"] for c in got["clips"]] == [c["hyp"] for c in exp["clips"]]


def test_vocoder_inference_asr_takes_a_tiny_model(case, tmp_path, capsys):
    """--asr transcribes the clips stage 2 just wrote (the way --stoi scores them): pred_asr/<spk>/<utt>.txt = WhisperASR.run on them."""
    from lip2speech_unit_amd import audio
    from lip2speech_unit_amd import vocoder_inference as s2
    from tests._synth_dataset import make
    from tests.test_models_gpu import VOC_H
    ck, vocab, cfg, _ = _tiny_files(case, tmp_path)
    lab = make(str(tmp_path / "ds"), frames=(12, 9))
    vc = str(tmp_path / "cfg.json")
    json.dump(dict(VOC_H, code_hop_size=320, mel_hop_size=160, sampling_rate=16000), open(vc, "w"))
    out = str(tmp_path / "out")
    s2.main([vc, os.path.join(lab, "test.tsv"), os.path.join(lab, "dict.unt.txt"), "--output_dir", out, "-n", "-1", "--synthetic_weights",
             "--asr", "--whisper", str(ck), "--vocab", str(vocab), "--decode_config", str(cfg), "--max_new_tokens", str(R.TINY_STEPS)])
    config = asr_text.WhisperDecodeConfig.from_generation_config(str(cfg), max_new_tokens=R.TINY_STEPS)
    asr = W.WhisperASR(_model(case, ops.F16), config, vocab=str(vocab))
    for utt in ("spk0/00000", "spk1/00001"):
        pcm = audio.read_wav_s16(os.path.join(out, "pred_wav", utt + ".wav"))
        want = asr.run(torch.from_numpy(pcm[None].copy()).cuda(), [len(pcm)])[0]
        got = open(os.path.join(out, "pred_asr", utt + ".txt")).read().strip()
        assert got == want and len(got.split()) >= 1
