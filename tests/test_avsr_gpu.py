"""Audio-visual speech recognition on the device: a tiny AV-HuBERT seq2seq model (one encoder layer, a one-layer decoder, 40
symbols, synthetic weights) on 2 clips of 8 and 5 video frames with audio of matching and of mismatching length.

Encoder rows from audio + video, audio alone and 'add' fusion are held against the float64 reference tests/_avsr_reference.py
(oracle.avhubert plus the audio branch of hubert.py:703-727, fed with the float64 audio features) at the tolerance
tests/test_models_gpu.py:56 applies to the video-only extract_finetune output at the same dtype: err < 1e-2 * max|ref| at F16.
Video alone is bit-equal to extract_rows and LipReader.generate; the search equals generate_from_encoder on the same rows; the
CLI writes its two files for ['audio','video'] and ['audio'].

The audio stream must matter: audio + video rows differ from video-only rows by at least 100 * TOL = 1.0.  (100 x the gate's absolute
bound, TOL * max|ref| = 0.049 here, is max|ref| itself, which no two outputs of the final LayerNorm reach - the float64 reference's own
two row sets are 2.39 apart - so the factor is applied to the figure TOL, not to the product.)"""
import json
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import weights  # noqa: E402
from lip2speech_unit_amd.av_recogniser import SpeechRecogniser, load_speech_recogniser  # noqa: E402
from lip2speech_unit_amd.hubert import AVHubertConfig  # noqa: E402
from lip2speech_unit_amd.lip_reader import AVHubertSeq2Seq, BeamSearchConfig, DecoderConfig, LipReader, save_checkpoint  # noqa: E402
from tests import _avsr_reference as AR  # noqa: E402
from tests import _logfbank_reference as LR  # noqa: E402

TOL = 1e-2            # tests/test_models_gpu.py:56, (ops.F16, 1e-2): err < tol * ref.abs().max() over the valid rows
EOS, PAD = 2, 1
FRAMES = (8, 5)
# clip 0: 5200 samples = 8 rows (the video's count) or 3000 samples = 5 rows (padded to 8); clip 1: 4400 samples = 7 rows (trimmed to 5)
SAMPLES = {"match_trim": (5200, 4400), "pad_trim": (3000, 4400)}
# largest err / max|ref| on an MI355X at F16, the models' default type (MEASURE lines of this file)
MEASURED = {"av": 5.86e-4, "av_padded": 4.81e-4, "audio": 7.45e-4, "add_av": 6.03e-4, "add_audio": 6.04e-4, "add_video": 6.35e-4,
            "gap_concat": 2.387, "gap_add": 2.199}     # gap: max |audio+video rows - video-only rows| on the device


def _model(fuse):
    torch.manual_seed(0)
    w2v = AVHubertConfig(encoder_layers=1, modality_fuse=fuse)
    cfg = DecoderConfig(decoder_embed_dim=128, decoder_ffn_embed_dim=256, decoder_layers=1, decoder_attention_heads=2,
                        encoder_embed_dim=w2v.encoder_embed_dim)
    model = AVHubertSeq2Seq(w2v, cfg, n_vocab=40).eval()
    model.load_state_dict(weights.synth_state_dict(weights.spec_of(model), seed=0))
    with torch.no_grad():
        model.decoder.layer_norm.weight.mul_(4.0)
    return model, w2v


@pytest.fixture(scope="module")
def models():
    return {fuse: _model(fuse) for fuse in ("concat", "add")}


@pytest.fixture(scope="module")
def clips():
    g = torch.Generator().manual_seed(1)
    video = torch.randn(2, 1, 8, 88, 88, generator=g)
    mask = torch.zeros(2, 8, dtype=torch.bool)
    mask[1, 5:] = True
    wavs = {k: [LR.signal("noise", n[0], 11), LR.signal("tone", n[1], 12)] for k, n in SAMPLES.items()}
    return video, mask, wavs


def _padded(wavs):
    pcm = np.zeros((len(wavs), max(len(w) for w in wavs)), dtype=np.int16)
    for i, w in enumerate(wavs):
        pcm[i, :len(w)] = w
    return torch.from_numpy(pcm).cuda(), [len(w) for w in wavs]


def _reader(model, mods, **kw):
    return SpeechRecogniser(model.cuda(), None, BeamSearchConfig(beam=3, max_len_a=0.5, max_len_b=2, nbest=3), modalities=mods, **kw)


_REF = {}


def _reference(models, clips, fuse, mods, key):
    """float64 rows and the padding mask of a case, computed once."""
    k = (fuse, mods, key)
    if k not in _REF:
        video, mask, wavs = clips
        sd = models[fuse][0].state_dict()
        if "video" in mods:
            a = AR.audio_rows(wavs[key], list(FRAMES), 8) if "audio" in mods else None
            _REF[k] = (AR.extract_finetune(sd, a, video, mask, fuse), mask)
        else:
            rows = [LR.audio_rows(w).shape[0] for w in wavs[key]]
            m = torch.arange(max(rows))[None, :] >= torch.tensor(rows)[:, None]
            _REF[k] = (AR.extract_finetune(sd, AR.audio_rows(wavs[key], None, max(rows)), None, m, fuse), m)
    return _REF[k]


@pytest.mark.parametrize("fuse,mods,key", [("concat", ("audio", "video"), "match_trim"), ("concat", ("audio", "video"), "pad_trim"),
                                           ("concat", ("audio",), "match_trim"), ("add", ("audio", "video"), "match_trim"),
                                           ("add", ("audio",), "match_trim"), ("add", ("video",), "match_trim")],
                         ids=["av", "av_padded", "audio", "add_av", "add_audio", "add_video"])
def test_encoder_rows_against_float64(models, clips, fuse, mods, key):
    video, mask, wavs = clips
    ref, m = _reference(models, clips, fuse, mods, key)
    rec = _reader(models[fuse][0], mods)
    wav, n = _padded(wavs[key])
    rows, lens, B, T = rec.encode(video.cuda(), wav, n, mask.cuda())
    got = rows.view(B, T, -1).cpu().double()
    valid = ~m
    assert got.shape == ref.shape and lens.cpu().tolist() == valid.sum(1).tolist()
    assert torch.isfinite(got[valid]).all()
    err, top = (got - ref)[valid].abs().max().item(), ref[valid].abs().max().item()
    print(f"MEASURE rows_{fuse}_{'+'.join(mods)}_{key} err={err:.3e} max|ref|={top:.3e} err/max={err / top:.3e} gate={TOL:.1e}")
    assert err < TOL * top, err
    if mods == ("audio", "video"):                       # a silently ignored audio stream fails here
        only = _reader(models[fuse][0], ("video",)).encode(video.cuda(), None, None, mask.cuda())[0].view(B, T, -1).cpu().double()
        gap = (got - only)[valid].abs().max().item()
        print(f"MEASURE gap_{fuse}_{key} |audio+video - video| = {gap:.3e}")
        assert gap >= 100.0 * TOL


def test_video_only_is_bit_equal_to_the_lip_reader(models, clips):
    video, mask, _ = clips
    model = models["concat"][0].cuda()
    v, m = video.cuda(), mask.cuda()
    w2v = model.encoder.w2v_model
    a, b = w2v.extract_av_rows(video=v, padding_mask=m), w2v.extract_rows(v, m)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:]
    cfg = BeamSearchConfig(beam=3, max_len_a=0.5, max_len_b=2, nbest=3)
    want = LipReader(model, None, cfg).generate(v, m)
    assert _reader(model, ("video",)).generate(v, padding_mask=m) == want
    wav, n = _padded(clips[2]["match_trim"])
    assert _reader(model, ("video",)).generate(v, wav, n, m) == want          # audio outside the modalities is dropped
    with pytest.raises(NotImplementedError):             # the lip reader and extract_finetune go on refusing an audio source
        LipReader(model, None, cfg).generate({"video": v, "audio": v}, None)
    with pytest.raises(NotImplementedError):
        w2v.extract_finetune({"video": v, "audio": v}, m)


@pytest.mark.parametrize("mods", [("audio", "video"), ("audio",)], ids=["av", "audio"])
def test_search_equals_generate_from_encoder(models, clips, mods):
    video, mask, wavs = clips
    rec = _reader(models["concat"][0], mods)
    wav, n = _padded(wavs["match_trim"])
    got = rec.generate(video.cuda(), wav, n, mask.cuda())
    rows, lens, B, T = rec.encode(video.cuda(), wav, n, mask.cuda())
    assert rec.generate_from_encoder(rows.view(B, T, -1), lens.cpu().tolist()) == got
    assert len(got) == 2 and lens.cpu().tolist() == (list(FRAMES) if "video" in mods else [8, 7])
    for b, frames in enumerate(lens.cpu().tolist()):
        assert 1 <= len(got[b]) <= 3
        for h in got[b]:
            assert h["tokens"][-1] == EOS and len(h["tokens"]) <= rec.max_len(frames) + 1 and np.isfinite(h["score"])
            assert all(0 <= t < 40 and t != PAD for t in h["tokens"])
    with pytest.raises(ValueError):
        rec.generate(video.cuda(), wav, [n[0], 0], mask.cuda())                # a clip without samples


def test_cli_round_trip(models, tmp_path, golden_dir):
    """infer_avsr on two clips of tests/golden/lrs3_sample's manifest (synthetic mouth crops as .npy sidecars, short synthetic wavs)
    with a saved tiny audio-visual checkpoint, once with ['audio','video'] and once with ['audio']."""
    from lip2speech_unit_amd import infer_avsr
    from lip2speech_unit_amd.asr_text import wer
    model, w2v = models["concat"]
    ck = str(tmp_path / "ck.pt")
    save_checkpoint(model.half(), ck, w2v, modalities=["video", "audio"], task={"stack_order_audio": 4, "normalize": True})
    model.float()
    loaded = load_speech_recogniser(ck)
    assert set(loaded.state_dict()) == set(model.state_dict()) and loaded.modalities == ("audio", "video")
    root, lab = str(tmp_path / "data"), str(tmp_path / "data" / "label")
    os.makedirs(lab)
    rows = open(os.path.join(golden_dir, "lrs3_sample", "test.tsv")).read().splitlines()[1:3]
    rng = np.random.default_rng(0)
    with open(os.path.join(lab, "test.tsv"), "w") as f:
        f.write(root + "\n")
        for i, (r, n, ns) in enumerate(zip(rows, (6, 9), (3840, 5000))):
            c = r.split("\t")
            c[3], c[4] = str(n), str(ns)
            f.write("\t".join(c) + "\n")
            p = os.path.join(root, os.path.splitext(c[1])[0] + ".npy")
            os.makedirs(os.path.dirname(p), exist_ok=True)
            np.save(p, rng.integers(0, 256, (n, 96, 96), dtype=np.uint8))
            p = os.path.join(root, c[2])
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with wave.open(p, "wb") as w:
                w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
                w.writeframes(LR.signal("noise", ns, 20 + i).astype("<i2").tobytes())
    syms = ["▁" + w for w in ("the", "lip", "reads", "a", "word")] + [chr(97 + i) for i in range(26)] + ["▁", "'", "s", "ing", "ed"]
    with open(os.path.join(lab, "dict.wrd.txt"), "w", encoding="utf-8") as f:
        f.write("".join(f"{s} 1\n" for s in syms))
    refs = ["the lip reads a word", "a word"]
    with open(os.path.join(lab, "test.wrd"), "w") as f:
        f.write("\n".join(refs) + "\n")
    for fid, extra in ((7, ["override.modalities=['audio','video']"]), (8, ["override.modalities=['audio']"])):
        res = str(tmp_path / f"res{fid}")
        out = infer_avsr.main([f"common_eval.path={ck}", f"common_eval.results_path={res}", f"override.data={lab}", f"override.label_dir={lab}",
                               "dataset.gen_subset=test", "generation.beam=3", "generation.max_len_a=0.5", f"fid={fid}"] + extra)
        hypo = json.load(open(os.path.join(res, f"hypo-{fid}.json")))
        assert hypo["utt_id"] == [r.split("\t")[0] for r in rows] and hypo["ref"] == refs and len(hypo["hypo"]) == 2
        assert all(isinstance(h, str) for h in hypo["hypo"]) and hypo["hypo"] == out["hypo"]
        w = wer(refs, hypo["hypo"])
        text = open(os.path.join(res, f"wer.{fid}")).read()
        assert text.startswith(f"WER: {w['wer']}\n") and f"err / num_ref_words = {w['n_err']} / {w['n_total']}" in text
    with pytest.raises(SystemExit):
        infer_avsr.main([f"common_eval.path={ck}", f"common_eval.results_path={res}", f"override.label_dir={lab}", "override.noise_prob=0.5"])
