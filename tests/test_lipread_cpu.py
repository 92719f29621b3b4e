"""The lip reader's host side without a GPU: tests/_s2s_reference.py (the float64 yardstick of the device tests) pinned
independently - against torch.nn.TransformerDecoderLayer, against its own teacher-forced pass, against greedy decoding and
against hand-computed position entries - the dictionary, the detokeniser, the CLI's arguments, the new ABI entries, and the
decisiveness census of the seeded tiny cases the GPU tests decode."""
import math
import os
import re

import numpy as np
import pytest
import torch

from lip2speech_unit_amd import _lib, ops
from lip2speech_unit_amd.asr_text import FairseqDictionary
from tests import _s2s_reference as R

ROOT = os.path.join(os.path.dirname(__file__), "..")


def test_decoder_layer_equals_torch_transformer_decoder_layer():
    """One pre-LN layer in float64 against torch.nn.TransformerDecoderLayer(norm_first=True, activation="relu") with q / k / v
    packed into in_proj: 1e-12."""
    d, H, F, T, M = 128, 2, 256, 7, 11
    sd = R.tiny_state_dict(3, d, H, layers=1, ffn=F)
    p = "decoder.layers.0."
    layer = torch.nn.TransformerDecoderLayer(d, H, dim_feedforward=F, dropout=0.0, activation="relu", norm_first=True, batch_first=True).double().eval()
    t = lambda k: torch.from_numpy(sd[p + k])
    with torch.no_grad():
        for a, name in ((layer.self_attn, "self_attn"), (layer.multihead_attn, "encoder_attn")):
            a.in_proj_weight.copy_(torch.cat([t(f"{name}.{m}_proj.weight") for m in "qkv"]))
            a.in_proj_bias.copy_(torch.cat([t(f"{name}.{m}_proj.bias") for m in "qkv"]))
            a.out_proj.weight.copy_(t(name + ".out_proj.weight")), a.out_proj.bias.copy_(t(name + ".out_proj.bias"))
        for mod, name in ((layer.norm1, "self_attn_layer_norm"), (layer.norm2, "encoder_attn_layer_norm"), (layer.norm3, "final_layer_norm"),
                          (layer.linear1, "fc1"), (layer.linear2, "fc2")):
            mod.weight.copy_(t(name + ".weight")), mod.bias.copy_(t(name + ".bias"))
    rng = np.random.default_rng(0)
    x, enc = rng.normal(size=(T, d)), rng.normal(size=(M, d))
    causal = torch.triu(torch.full((T, T), float("-inf"), dtype=torch.float64), 1)
    with torch.no_grad():
        want = layer(torch.from_numpy(x)[None], torch.from_numpy(enc)[None], tgt_mask=causal)[0].numpy()
    got = R.Decoder(sd, H).layer(x, 0, enc)
    assert np.max(np.abs(got - want)) <= 1e-12


@pytest.mark.parametrize("d,H", R.TINY_SHAPES)
def test_incremental_decoding_equals_the_teacher_forced_pass(d, H):
    sd = R.tiny_state_dict(11, d, H)
    enc = np.random.default_rng(1).normal(size=(7, d))
    dec = R.Decoder(sd, H)
    tokens = [R.EOS, 5, 9, 30, 4, 17]
    full = dec.logits(tokens, enc)
    inc = R.Incremental(dec, enc)
    for i, tk in enumerate(tokens):
        assert np.max(np.abs(inc.step(tk) - full[i])) <= 1e-11


def test_beam_one_equals_greedy():
    d, H = 128, 2
    sd = R.tiny_state_dict(2, d, H)
    enc = np.random.default_rng(2).normal(size=(9, d))
    dec = R.Decoder(sd, H)
    max_len = 6
    hyps, _ = R.search_clip(dec, enc, 1, max_len)
    inc, tok, out, total = R.Incremental(dec, enc), R.EOS, [], 0.0
    for step in range(max_len + 1):
        lp = R.log_softmax_rows(inc.step(tok)[None])[0]
        lp[R.PAD] = -np.inf
        if step >= max_len:
            keep = lp[R.EOS]
            lp[:] = -np.inf
            lp[R.EOS] = keep
        if step < 1:
            lp[R.EOS] = -np.inf
        tok = int(np.argmax(lp))
        total += lp[tok]
        out.append(tok)
        if tok == R.EOS:
            break
    assert hyps[0][0] == out and abs(hyps[0][1] - total / len(out)) <= 1e-12


def test_search_bookkeeping_on_a_scripted_model():
    """A 'decoder' whose logits depend on the last token only: the best hypotheses are known by hand."""
    class Fake:
        V, d, n_layers = 8, 4, 0

        def all_cross(self, enc):
            return []

        def logits(self, tokens, enc, cross):
            row = np.full(self.V, -20.0)
            last = tokens[-1]
            if last == R.EOS:
                row[4], row[5] = 2.0, 1.0
            elif last == 4:
                row[R.EOS], row[6] = 3.0, 1.0
            else:
                row[R.EOS] = 5.0
            return row[None]
    hyps, trace = R.search_clip(Fake(), None, 2, 5)
    assert [h[0] for h in hyps] == [[4, R.EOS], [5, R.EOS]] and hyps[0][1] > hyps[1][1]
    assert len(trace) == 2 and list(trace[0]["slot"][:4]) == [0, 0, 0, 0]      # step 0: slot 0 only


def test_position_table_against_hand_computed_entries():
    d = 8
    tab = R.sinusoidal_table(6, d)
    assert not tab[1].any()                                      # the padding row
    assert np.allclose(tab[0], [0, 0, 0, 0, 1, 1, 1, 1], atol=0)
    inv = [1.0, 10000 ** (-1 / 3), 10000 ** (-2 / 3), 1e-4]
    for pos in (2, 3, 5):
        want = [math.sin(pos * k) for k in inv] + [math.cos(pos * k) for k in inv]
        assert np.max(np.abs(tab[pos] - want)) <= 1e-15
    assert np.array_equal(R.token_positions(3, d), tab[2:5])     # token index t reads row t + 2
    from lip2speech_unit_amd.lip_reader import sinusoidal_table
    assert np.array_equal(sinusoidal_table(6, d).numpy(), tab.astype(np.float32))


def test_per_clip_length_limit():
    assert R.clip_max_len(100) == 100 and R.clip_max_len(5000) == 2047 and R.clip_max_len(7, 0.15, 2) == 3
    from lip2speech_unit_amd.lip_reader import BeamSearchConfig
    c = BeamSearchConfig()
    assert (c.beam, c.max_len_a, c.max_len_b, c.min_len, c.lenpen, c.unk_penalty, c.temperature, c.normalize_scores, c.nbest) == \
        (50, 1.0, 0, 1, 1.0, 0, 1, True, 1)


def test_fairseq_dictionary_and_detokeniser(tmp_path):
    p = tmp_path / "dict.wrd.txt"
    p.write_text("▁the 100\n▁lip 50\ns 40\n▁read 30\ner 20\n' 5\n", encoding="utf-8")
    d = FairseqDictionary.load(str(p))
    assert d.nspecial == 4 and len(d) == 10 and d.symbols[:4] == ["<s>", "<pad>", "</s>", "<unk>"]
    assert (d.pad(), d.eos(), d.unk()) == (1, 2, 3) and d.index["▁the"] == 4 and d.index["er"] == 8
    assert d.string([4, 5, 7, 8, 6, 2]) == "the lip readers"
    assert d.string([2, 4, 1, 1]) == "the"
    assert d.encode_pieces(["▁lip", "zzz"]) == [5, 3]
    bad = tmp_path / "bad.txt"
    bad.write_text("nocount\n")
    with pytest.raises(ValueError):
        FairseqDictionary.load(str(bad))


def test_cli_arguments():
    from lip2speech_unit_amd import infer_s2s
    cfg = infer_s2s.parse_overrides(["dataset.gen_subset=test", "common_eval.path=/m/ck.pt", "common_eval.results_path=/r",
                                     "override.data=/d", "override.label_dir=/d", "generation.beam=20", "generation.lenpen=0.5",
                                     "override.modalities=['video']"])
    assert cfg["common_eval.path"] == "/m/ck.pt" and cfg["generation.beam"] == 20 and cfg["override.modalities"] == ["video"]
    s = infer_s2s.search_config(cfg)
    assert (s.beam, s.lenpen, s.max_len_a, s.normalize_scores) == (20, 0.5, 1.0, True)
    assert infer_s2s.search_config(infer_s2s.parse_overrides([])).beam == 50
    for bad in (["override.modalities=['audio','video']"], ["override.modalities=['audio']"], ["generation.nope=1"], ["--beam=5"]):
        with pytest.raises(SystemExit):
            infer_s2s.parse_overrides(bad)


def test_audio_checkpoint_is_refused(tmp_path):
    from lip2speech_unit_amd.lip_reader import load_lip_reader
    p = str(tmp_path / "ck.pt")
    torch.save({"cfg": {"model": {"w2v_args": {"model": {"encoder_layers": 1}}}, "task": {"modalities": ["audio", "video"]}}, "model": {}}, p)
    with pytest.raises(NotImplementedError):
        load_lip_reader(p)


def test_model_state_dict_names_and_small_vocabulary():
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.lip_reader import AVHubertSeq2Seq, DecoderConfig, TransformerDecoder
    cfg = DecoderConfig(decoder_embed_dim=128, decoder_ffn_embed_dim=256, decoder_layers=2, decoder_attention_heads=2, encoder_embed_dim=128,
                        share_decoder_input_output_embed=False)
    dec = TransformerDecoder(cfg, 36)
    names = set(dec.state_dict())
    for n in ("embed_tokens.weight", "layers.1.self_attn.q_proj.weight", "layers.0.encoder_attn.k_proj.bias", "layers.0.encoder_attn.out_proj.weight",
              "layers.1.self_attn_layer_norm.weight", "layers.0.encoder_attn_layer_norm.bias", "layers.0.final_layer_norm.weight",
              "layers.1.fc1.weight", "layers.1.fc2.bias", "layer_norm.weight", "embed_out"):
        assert n in names, n
    assert not any("embed_positions" in n for n in names)        # sinusoidal positions are no parameters
    with pytest.raises(NotImplementedError):
        TransformerDecoder(DecoderConfig(decoder_embed_dim=128, decoder_attention_heads=4), 36)      # heads 32 wide
    m = AVHubertSeq2Seq(AVHubertConfig(encoder_layers=1), DecoderConfig(decoder_layers=1), n_vocab=40)
    keys = set(m.state_dict())
    assert "encoder.w2v_model.post_extract_proj.weight" in keys and "decoder.layers.0.encoder_attn.v_proj.weight" in keys


def test_new_abi_entries_are_declared_bound_and_registered():
    hdr = open(os.path.join(ROOT, "include", "lip2speech_hip.h")).read()
    assert re.search(r"#define\s+L2S_ABI_VERSION\s+16\b", hdr) and _lib.ABI_VERSION == 16
    for name in ("l2s_beam_attention", "l2s_beam_select", "l2s_beam_select_workspace", "l2s_beam_advance"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    for op in ("beam_attention", "beam_select", "beam_advance"):
        assert ops.ENTRY_OF[op] == "l2s_" + op and hasattr(torch.ops.lip2speech, op)
    assert "l2s_beam_select_workspace" in ops.HOST_QUERIES
    lib = os.path.join(ROOT, "lip2speech_unit_amd", "liblip2speech_hip.so")
    if os.path.exists(lib):
        import ctypes
        so = ctypes.CDLL(lib)
        for name in ("l2s_beam_attention", "l2s_beam_select", "l2s_beam_select_workspace", "l2s_beam_advance"):
            assert hasattr(so, name)
    with pytest.raises(ops.L2SError):            # HIP only: no CPU path
        ops.beam_select(torch.zeros(2, 40), torch.zeros(2, 1, 2), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                        torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32), B=1, beam=2, V=40,
                        pad=1, unk=3, eos=2)


def test_decisiveness_census_of_the_tiny_cases():
    """The seeded tiny cases of tests/test_lipread_gpu.py: a case (d, heads, beam; three clips of 1, 7 and 20 encoder rows) is
    decisive when, at every step of every clip, every adjacent gap among the best 2 beam + 1 candidate scores and among the final
    scores exceeds 4 x the score error of the restatement run with fp16-rounded weights and activations.  At least 75 % of the
    cases must be decisive for fp16 - by the restatement alone, no device involved."""
    census = R.tiny_census("fp16")
    assert len(census) == 9
    n = sum(1 for ok, _ in census.values() if ok)
    for key, (ok, clips) in census.items():
        print(key, ok, [(round(c[1], 4), round(c[2], 5)) for c in clips])
    assert n / len(census) >= 0.75, n
    # the searches are not trivial: several hypotheses, different lengths, the clips differ
    for (d, H, beam), (ok, clips) in census.items():
        assert all(len(c[3]) >= 1 for c in clips)
        if beam > 1:
            assert any(len(c[3]) > 1 for c in clips)
    assert len({tuple(c[3][0][0]) for _, clips in census.values() for c in clips}) >= 12


def test_the_long_tiny_case_is_decisive_and_long():
    ok, gap, eps, hyps = R.tiny_long_census("fp16")
    print(ok, gap, eps, [len(h[0]) for h in hyps])
    assert ok and gap > 4 * eps
    assert len(hyps) == R.TINY_LONG["beam"] and all(len(h[0]) >= R.TINY_LONG["min_len"] + 1 for h in hyps)
    assert max(len(h[0]) for h in hyps) == R.TINY_LONG["max_len"] + 1           # the search reaches position 20
