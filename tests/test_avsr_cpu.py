"""Audio-visual speech recognition without a GPU: the float64 restatement of the audio features (tests/_logfbank_reference.py) is
pinned - band edges, frame counts, the dense DFT against numpy's FFT, the stacker's 0.0 padding, the alignment, the row norm - the
package's tables equal it to one fp32 rounding, the new entry is declared, bound and registered at ABI 16, and the checkpoint
loader and the CLI's overrides accept and refuse what they should."""
import os
import re

import numpy as np
import pytest
import torch

from lip2speech_unit_amd import _lib, audio, ops
from tests import _logfbank_reference as R

HDR = os.path.join(os.path.dirname(__file__), "..", "include", "lip2speech_hip.h")


def test_filterbank_edges_and_weights():
    assert R.edges().tolist() == R.EDGES
    fb = R.filterbank()
    assert fb.shape == (26, 257) and fb.min() >= 0.0 and fb.max() <= 1.0
    assert (fb[:, 256] == 0).all()                       # the last edge is bin 256 exactly: no filter reaches it
    assert (fb.max(axis=1) == 1.0).all() and (fb[np.arange(26), R.EDGES[1:-1]] == 1.0).all()


@pytest.mark.parametrize("n,want", [(1, 1), (399, 1), (400, 1), (401, 2), (560, 2), (561, 3), (16000, 99)])
def test_frame_counts(n, want):
    assert R.n_frames(n) == want and audio.logfbank_frames(n) == want
    assert R.frames(np.ones(n)).shape == (want, 400)
    assert audio.logfbank_rows(n, 4) == -(-want // 4) and audio.logfbank_rows(n, 1) == want


def test_dense_dft_restatement_equals_the_fft_route():
    worst = 0.0
    for kind, n, seed in (("noise", 4000, 1), ("tone", 10801, 2), ("walk", 561, 3)):
        x = R.signal(kind, n, seed)
        worst = max(worst, np.abs(R.logfbank(x) - R.logfbank_fft(x)).max())
    print(f"MEASURE dense_vs_fft {worst:.3e}")
    assert worst <= 1e-10
    assert (R.logfbank(np.zeros(700)) == np.log(R.EPS)).all()          # a zero energy is taken as eps


def test_preemphasis_keeps_the_first_sample():
    x = np.array([100, 200, -50] + [0] * 5, dtype=np.int16)
    f = R.frames(x)
    assert f[0, 0] == 100.0 and f[0, 1] == 200.0 - 0.97 * 100.0 and f[0, 2] == -50.0 - 0.97 * 200.0 and f[0, 3] == 0.97 * 50.0


def test_stacker_alignment_and_row_norm():
    f = np.arange(1.0, 6 * 26 + 1).reshape(6, 26)
    s = R.stacker(f, 4)
    assert s.shape == (2, 104) and (s[0] == f[:4].ravel()).all() and (s[1, :52] == f[4:].ravel()).all()
    assert (s[1, 52:] == 0.0).all()                      # the missing frames are 0.0, not log(eps)
    assert R.stacker(f[:4], 4).shape == (1, 104) and R.stacker(f, 1).shape == (6, 26)
    a = R.align(s, 5)
    assert a.shape == (5, 104) and (a[:2] == s).all() and (a[2:] == 0).all()
    assert (R.align(s, 1) == s[:1]).all() and R.align(s, None) is s and (R.align(s, 2) == s).all()
    n = R.layer_norm(a)
    assert (n[2:] == 0).all()                            # LN of a zero row is zero
    assert np.abs(n[:2].mean(axis=1)).max() < 1e-12 and np.abs((n[:2] ** 2).mean(axis=1) - 1.0).max() < 1e-6
    x = R.signal("noise", 1000, 4)
    assert R.audio_rows(x, 4, 3).shape == (3, 104) and R.audio_rows(x, 1, None, False).shape == (5, 26)


def test_package_tables_equal_the_restatement_to_one_rounding():
    t = audio.LogFbank()
    assert t.stack == 4 and t.normalize and t.width == 104 and t.edges.tolist() == R.EDGES
    c, s = R.dft_tables()
    k, part = audio.packed_bins(np.arange(512))
    assert t.basis.shape == (400, 512) and t.basis.dtype == np.float32
    assert sorted(set(k.tolist())) == list(range(256))   # bins 0 .. 255, each with a cos and a -sin column
    want = np.where(part[None, :] == 0, c[:, k], s[:, k])
    assert (t.basis == want.astype(np.float32)).all()
    assert t.fb.shape == (26, 257) and (t.fb == R.filterbank().astype(np.float32)).all()
    assert t.fb_range.dtype == np.int32 and t.fb_range.tolist() == [[R.EDGES[j] + 1, R.EDGES[j + 2]] for j in range(26)]
    assert t.fb_range.max() <= 256
    with pytest.raises(ValueError):
        audio.LogFbank(stack=3)
    with pytest.raises(ops.L2SError):
        t.rows(torch.zeros(1, 800))


def test_entry_is_declared_bound_and_registered():
    hdr = open(HDR).read()
    assert re.search(r"#define L2S_ABI_VERSION 16\b", hdr) and _lib.ABI_VERSION == 16
    m = re.search(r"int l2s_logfbank\(([^;]*)\);", hdr)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["l2s_logfbank"][0])
    assert ops.ENTRY_OF["logfbank"] == "l2s_logfbank" and hasattr(torch.ops.lip2speech, "logfbank")
    schema = str(torch.ops.lip2speech.logfbank.default._schema)
    assert schema.rstrip().endswith("-> ()") and "Tensor(a!) out" in schema
    t = audio.LogFbank()
    with pytest.raises(ops.L2SError):                    # the dispatcher has a HIP kernel only
        ops.logfbank(torch.zeros(1, 800), torch.zeros(1, 1, 104), torch.from_numpy(t.basis), torch.from_numpy(t.fb),
                     torch.from_numpy(t.fb_range), B=1, S=800, T_rows=1)


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from lip2speech_unit_amd import weights
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.lip_reader import AVHubertSeq2Seq, DecoderConfig
    w2v = AVHubertConfig(encoder_layers=1)
    cfg = DecoderConfig(decoder_embed_dim=128, decoder_ffn_embed_dim=256, decoder_layers=1, decoder_attention_heads=2,
                        encoder_embed_dim=w2v.encoder_embed_dim)
    model = AVHubertSeq2Seq(w2v, cfg, n_vocab=40).eval()
    model.load_state_dict(weights.synth_state_dict(weights.spec_of(model), seed=0))
    return model.half(), w2v


def test_load_speech_recogniser(tiny, tmp_path):
    from lip2speech_unit_amd.av_recogniser import load_speech_recogniser
    from lip2speech_unit_amd.lip_reader import load_lip_reader, save_checkpoint
    model, w2v = tiny
    for i, mods in enumerate((["video", "audio"], ["audio", "video"])):
        p = str(tmp_path / f"av{i}.pt")
        save_checkpoint(model, p, w2v, modalities=mods)
        got = load_speech_recogniser(p)
        assert got.modalities == ("audio", "video") and got.stack_order_audio == 4 and got.normalize is True
        assert set(got.state_dict()) == set(model.state_dict())
        assert load_speech_recogniser(p, modalities=["audio"]).modalities == ("audio",)     # the argument overrides the file
        with pytest.raises(NotImplementedError):
            load_lip_reader(p)
    p = str(tmp_path / "task.pt")
    save_checkpoint(model, p, w2v, modalities=["audio"], task={"stack_order_audio": 1, "normalize": False})
    with pytest.raises(ValueError, match="audio_feat_dim"):                                 # 104 columns are not 26 * 1
        load_speech_recogniser(p)
    got = load_speech_recogniser(p, modalities=["video"])
    assert got.modalities == ("video",) and got.stack_order_audio == 1 and got.normalize is False
    # today's default output of save_checkpoint is unchanged and loads as video
    p = str(tmp_path / "v.pt")
    save_checkpoint(model, p, w2v)
    ck = torch.load(p, weights_only=False)
    assert ck["cfg"]["task"] == {"modalities": ["video"]}
    assert load_speech_recogniser(p).modalities == ("video",) and load_lip_reader(p) is not None
    # a checkpoint without the audio sub-model's weights serves video, and is refused by name when audio is asked for
    ck["model"] = {k: v for k, v in ck["model"].items() if "feature_extractor_audio" not in k}
    torch.save(ck, p)
    assert load_speech_recogniser(p).modalities == ("video",)
    with pytest.raises(ValueError, match="feature_extractor_audio.proj.weight"):
        load_speech_recogniser(p, modalities=["audio", "video"])
    with pytest.raises(ValueError):
        load_speech_recogniser(p, modalities=["text"])


def test_add_fusion_is_constructed_and_other_refusals_stay():
    from lip2speech_unit_amd.hubert import AVHubertConfig, AVHubertModel
    m = AVHubertModel(AVHubertConfig(encoder_layers=1, modality_fuse="add"))
    assert m.embed == 1024 and m.post_extract_proj.weight.shape == (1024, 1024) and m.layer_norm.weight.shape == (1024,)
    assert AVHubertModel(AVHubertConfig(encoder_layers=1)).embed == 2048
    with pytest.raises(NotImplementedError):
        AVHubertModel(AVHubertConfig(encoder_layers=1, modality_fuse="mul"))
    with pytest.raises(NotImplementedError):
        AVHubertModel(AVHubertConfig(encoder_layers=1, sub_encoder_layers=2))
    with pytest.raises(NotImplementedError):
        m.extract_finetune({"audio": torch.zeros(1, 104, 4), "video": None})


def test_cli_overrides():
    from lip2speech_unit_amd import infer_avsr, infer_s2s
    for text, want in (("['video']", ["video"]), ("['audio']", ["audio"]), ("['audio','video']", ["audio", "video"]),
                       ("['video','audio']", ["audio", "video"])):
        assert infer_avsr.parse_overrides([f"override.modalities={text}"])["override.modalities"] == want
    cfg = infer_avsr.parse_overrides(["generation.beam=5", "override.noise_prob=0"])
    assert cfg["override.modalities"] is None and cfg["generation.beam"] == 5
    assert infer_s2s.search_config(cfg).beam == 5
    for bad in (["override.noise_prob=0.5"], ["override.modalities=['text']"], ["override.modalities=[]"], ["no.such.key=1"], ["--beam", "5"],
                ["dtype=f32"]):
        with pytest.raises(SystemExit):
            infer_avsr.parse_overrides(bad)
    with pytest.raises(SystemExit):                      # the lip reader's CLI goes on refusing audio
        infer_s2s.parse_overrides(["override.modalities=['audio','video']"])


def test_manifest_audio_column(tmp_path, golden_dir):
    from lip2speech_unit_amd import infer_s2s
    lab = os.path.join(golden_dir, "lrs3_sample")
    root, clips, _ = infer_s2s.read_manifest(lab, "test", audio=True)
    plain = infer_s2s.read_manifest(lab, "test")[1]
    assert [c[:3] for c in clips] == plain and all(c[3].endswith(".wav") and c[4] > 0 for c in clips)
