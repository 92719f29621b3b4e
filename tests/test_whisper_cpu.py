"""Whisper without a GPU: the float64 restatement (tests/_whisper_reference.py) against transformers - live where it is installed,
and against its recorded results (tests/golden/whisper_tiny.npz, tools/make_whisper_golden.py) always; the properties that keep the
GPU tests' cases from being vacuous; and the host code (WER, detokeniser, decoding configuration, rename table, ABI and operator
registration).

Observed with transformers 5.15 in float64: encoder rows within 8.5e-15, teacher-forced logits within 4.1e-14, the
greedy ids equal; WhisperFeatureExtractor returns float32 whatever it is given, so its features bound the restatement's only to
6.7e-8 (one float32 rounding of values up to 1.3) - the filterbanks themselves are equal to the last bit."""
import base64
import json
import os

import numpy as np
import pytest
import torch

from lip2speech_unit_amd import _lib, asr_text, ops
from lip2speech_unit_amd import whisper as W
from tests import _whisper_reference as R

TOL64 = 1e-10                  # float64 against float64 (observed 4.1e-14)
TOL_FEATURES = 2e-7            # against float32 features (observed 6.7e-8)
ENC_ROWS = (0, 700, 1499)
P = len(R.TINY_SOT)


@pytest.fixture(scope="module")
def case():
    return R.tiny_case()


def _r16(td):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(td).double().numpy()


def _own_logits(case, c):
    toks = list(R.TINY_SOT) + case["free"][c][0]
    return R.decoder_logits(case["sd"], R.TINY_DIMS, case["xa"][c], toks[:-1])[P - 1:]


def test_restatement_matches_the_recorded_transformers_results(case, golden_dir):
    g = np.load(os.path.join(golden_dir, "whisper_tiny.npz"))
    assert np.abs(g["features_clip0"] - case["feats"][0][::25]).max() <= TOL_FEATURES
    for c in range(3):
        assert np.abs(g[f"encoder_rows_{c}"] - case["xa"][c][list(ENC_ROWS)]).max() <= TOL64
        assert np.abs(g[f"logits_{c}"] - _own_logits(case, c)).max() <= TOL64
        assert g[f"greedy_{c}"].tolist() == case["free"][c][0]


def test_restatement_matches_transformers_live(case):
    pytest.importorskip("transformers")
    from tests import _whisper_hf as HF
    assert np.abs(HF.hf_features(case["clips"][0]) - case["feats"][0]).max() <= TOL_FEATURES
    m = HF.hf_model(case["sd"])
    for c in range(3):
        xa = HF.hf_encoder(m, case["feats"][c])
        assert np.abs(xa - case["xa"][c]).max() <= TOL64
        toks = list(R.TINY_SOT) + case["free"][c][0]
        assert np.abs(HF.hf_logits(m, xa, toks[:-1])[P - 1:] - _own_logits(case, c)).max() <= TOL64
        assert HF.hf_greedy(m, xa, R.TINY_STEPS) == case["free"][c][0]


def test_the_tiny_case_is_not_degenerate(case):
    ids = [f[0] for f in case["free"]]
    assert all(len(i) == R.TINY_STEPS for i in ids)
    assert len({tuple(i) for i in ids}) == 3, "the clips must decode differently"
    assert all(len(set(i)) >= 4 for i in ids), [len(set(i)) for i in ids]
    # eot is an ordinary id of this decode: nobody's first token, one clip's early, the others' later
    ends = [i.index(R.TINY_EOT) for i in ids]
    assert ends == [4, 6, 6] and all(i[0] != R.TINY_EOT for i in ids)
    for c, (got, _, _, end) in enumerate(case["ended"]):
        assert end == ends[c] < R.TINY_STEPS and got == ids[c][: ends[c]]


def test_every_fp16_step_is_decisive(case):
    """The float64 margin between the best and the runner-up allowed logit is >= 8 eps at every greedy step of every clip, eps = the
    largest logit error of the restatement with fp16-rounded weights and features (a CPU quantity)."""
    eps, _ = R.quantised_logit_error(case, _r16(torch.float16))
    margins = np.array([f[1] for f in case["free"]])
    print(f"fp16: eps {eps:.4f}, smallest margin {margins.min():.4f}")
    assert margins.shape == (3, R.TINY_STEPS) and margins.min() >= 8.0 * eps


def test_bf16_decisive_steps_are_counted(case):
    """bf16's eps is ten times fp16's and no seed of 0 .. 59 keeps all 30 margins above 8 eps; the GPU test holds bf16 to the float64
    id at the steps that are decisive, so there must be enough of them, in every clip."""
    eps, _ = R.quantised_logit_error(case, _r16(torch.bfloat16))
    margins = np.array([f[1] for f in case["free"]])
    decisive = margins >= 8.0 * eps
    print(f"bf16: eps {eps:.4f}, decisive steps per clip {decisive.sum(axis=1).tolist()}")
    assert decisive.sum(axis=1).tolist() == [3, 5, 3]                     # 11 of the 30 steps (eps 0.279: margins of 2.23 and more)


# ---- host code ---------------------------------------------------------------------------------------------------------------------

def test_wer_on_handmade_pairs():
    r = asr_text.wer(["Hello, world!", "it's a fine day"], ["hello world", "its a day"])
    assert [c["errors"] for c in r["clips"]] == [0, 2] and r["n_total"] == 6 and r["wer"] == pytest.approx(100.0 * 2 / 6)
    assert r["clips"][1]["ref"] == "it's a fine day"                       # the apostrophe stays, the comma went
    # an empty hypothesis: every reference word is a deletion; an insertion-only clip adds errors but no words
    r = asr_text.wer(["one two three", ""], ["", "extra words"])
    assert [c["errors"] for c in r["clips"]] == [3, 2] and r["n_total"] == 3 and r["wer"] == pytest.approx(100.0 * 5 / 3)
    # pooled, not the mean of the per-clip rates: (1 + 0) / (1 + 9) against (100 + 0) / 2
    r = asr_text.wer(["yes", "a b c d e f g h i"], ["no", "a b c d e f g h i"])
    assert r["wer"] == pytest.approx(10.0)
    assert asr_text.wer([], [])["wer"] is None and asr_text.wer([""], [""])["wer"] is None
    with pytest.raises(ValueError):
        asr_text.wer(["a"], [])
    assert asr_text.edit_distance("a b c".split(), "a x c d".split()) == 2
    assert asr_text.normalize_text("  Mr. O'Neil --  said: \"HI\"\n") == "mr o'neil said hi"


def test_detokeniser_joins_split_characters_in_both_formats(tmp_path):
    # a vocabulary in which the three bytes of the euro sign are split over two tokens
    euro = "€".encode("utf-8")
    toks = [b"he", b"llo", b" ", euro[:1], euro[1:], b"5", b"<|endoftext|>"]
    tk = tmp_path / "v.tiktoken"
    tk.write_bytes(b"".join(base64.b64encode(t) + b" " + str(i).encode() + b"\n" for i, t in enumerate(toks[:-1])))
    enc = {b: c for c, b in asr_text._gpt2_byte_decoder().items()}
    vj = tmp_path / "vocab.json"
    vj.write_text(json.dumps({"".join(enc[b] for b in t): i for i, t in enumerate(toks)}, ensure_ascii=False), encoding="utf-8")
    ids = [0, 1, 2, 3, 4, 5, 6, 40]                                       # 6 is special, 40 is in no table
    for path in (tk, vj):
        d = asr_text.Detokenizer.load(str(path))
        assert d.decode(ids) == "hello €5"
        assert d.decode([3]) == "�"                                  # half a character alone cannot decode
    assert asr_text.Detokenizer.load(str(tk), special_start=5).decode(ids) == "hello €"
    assert len(asr_text._gpt2_byte_decoder()) == 256


def test_decode_config_ids_for_both_vocabularies(tmp_path):
    en = asr_text.WhisperDecodeConfig.english()
    assert en.sot_sequence == (50257, 50362) and en.eot == 50256 and en.begin_suppress == (220, 50256) and en.max_new_tokens == 224
    assert {50257, 50358, 50359, 50360, 50361, 50362, 50363, 51863} <= set(en.suppress) and 50256 not in en.suppress and min(en.suppress) == 50257
    ml = asr_text.WhisperDecodeConfig.multilingual("de")
    assert ml.sot_sequence == (50258, 50261, 50359, 50363) and ml.eot == 50257 and 50257 not in ml.suppress
    assert asr_text.WhisperDecodeConfig.multilingual("en").sot_sequence[1] == 50259
    assert asr_text.WhisperDecodeConfig.multilingual("yue", n_vocab=51866).sot_sequence == (50258, 50358, 50360, 50364)
    with pytest.raises(ValueError):
        asr_text.WhisperDecodeConfig.multilingual("yue")                    # the 99-language vocabulary has no Cantonese token
    with pytest.raises(ValueError):
        asr_text.special_ids(333)
    assert 11 in asr_text.WhisperDecodeConfig.english(non_speech=(11,)).suppress
    g = {"decoder_start_token_id": 50257, "forced_decoder_ids": [[1, 50362]], "eos_token_id": 50256, "suppress_tokens": [1, 2, 7],
         "begin_suppress_tokens": [220, 50256]}
    p = tmp_path / "generation_config.json"
    p.write_text(json.dumps(g))
    c = asr_text.WhisperDecodeConfig.from_generation_config(str(p))
    assert c.sot_sequence == en.sot_sequence and c.eot == en.eot and c.suppress == (1, 2, 7) and c.begin_suppress == en.begin_suppress
    with pytest.raises(ValueError):
        asr_text.WhisperDecodeConfig.from_generation_config(dict(g, forced_decoder_ids=[[1, None], [2, 50359]]))


def test_rename_round_trip_and_checkpoint_files(tmp_path):
    dims = W.WhisperDims(**R.TINY_DIMS)
    m = W.Whisper(dims)
    sd = m.state_dict()
    assert set(sd) == set(R.tiny_state_dict(0)), set(sd) ^ set(R.tiny_state_dict(0))      # openai-whisper's names
    hf = W.openai_to_hf(sd)
    assert "model.decoder.layers.1.encoder_attn.q_proj.weight" in hf and "model.encoder.layers.0.self_attn.k_proj.weight" in hf
    assert "model.encoder.layer_norm.bias" in hf and "model.decoder.embed_positions.weight" in hf and "model.encoder.layers.1.fc2.bias" in hf
    assert "model.decoder.layers.0.final_layer_norm.weight" in hf and "model.encoder.layers.0.self_attn_layer_norm.weight" in hf
    back = W.hf_to_openai(hf)
    assert set(back) == set(sd) and all(back[k] is sd[k] for k in sd)
    assert W.dims_of(sd) == dims
    W.save_openai_checkpoint(m, str(tmp_path / "tiny.pt"))
    m2 = W.load_whisper(str(tmp_path / "tiny.pt"))
    assert m2.dims == dims and all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), sd.values()))
    torch.save(hf, str(tmp_path / "hf.pt"))
    m3 = W.load_whisper(str(tmp_path / "hf.pt"))
    assert m3.dims == dims and all(torch.equal(m3.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(NotImplementedError, match="n_mels"):
        W.Whisper(W.WhisperDims(n_mels=128))


def test_abi_signatures_and_operators_are_registered():
    for name in ("l2s_whisper_logmel", "l2s_whisper_logmel_workspace", "l2s_kv_attention", "l2s_vocab_argmax", "l2s_vocab_argmax_workspace",
                 "l2s_whisper_advance"):
        assert name in _lib.SIGNATURES
    for name in ("whisper_logmel", "kv_attention", "vocab_argmax", "whisper_advance"):
        assert ops.ENTRY_OF[name] == "l2s_" + name and hasattr(torch.ops.lip2speech, name)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "lip2speech_hip.h")).read()
    assert "#define L2S_ABI_VERSION 16" in hdr


def test_fake_implementations_trace_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        h = dict(device="cuda", dtype=torch.float16)
        q, out = torch.empty(3, 128, **h), torch.empty(3, 128, **h)
        kc, vc = torch.empty(3, 64, 128, **h), torch.empty(3, 64, 128, **h)
        pos = torch.empty(1, device="cuda", dtype=torch.int32)
        assert torch.ops.lip2speech.kv_attention(q, kc, vc, out, B=3, H=2, pos=pos) is None
        tok, lp = torch.empty(3, device="cuda", dtype=torch.int32), torch.empty(3, device="cuda")
        ws = torch.empty(1024, device="cuda", dtype=torch.uint8)
        assert torch.ops.lip2speech.vocab_argmax(q, torch.empty(333, 128, **h), ws, tok, lp, B=3, V=333, d=128) is None
        wav = torch.empty(2, 16000, device="cuda")
        assert torch.ops.lip2speech.whisper_logmel(wav, ws, torch.empty(6000, 128, **h), torch.empty(400, 448, device="cuda"),
                                                   torch.empty(80, 201, device="cuda"), torch.empty(80, 2, device="cuda", dtype=torch.int32),
                                                   B=2, S=16000) is None
    with pytest.raises(ops.L2SError):                                       # no CPU path
        ops.kv_attention(torch.zeros(1, 64), torch.zeros(1, 4, 64), torch.zeros(1, 4, 64), torch.zeros(1, 64), B=1, H=1, n_valid=1)
