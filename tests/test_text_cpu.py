"""Text supervision (TEXT_SUPERVISION=1) without a GPU: the CPU restatement of ctcdecode's prefix beam search against exact
CTC prefix probabilities, the trie (revival) semantics, the conformer's text head and its checkpoint keys, and the
dispatcher-visible ops."""
import numpy as np
import pytest
import torch

from lip2speech_unit_amd import ops
from lip2speech_unit_amd.conformer import Conformer, ConformerConfig
from tests import _ctc_reference as R

# seeded search (tests/_ctc_reference.py fresh_ids=False vs True): the first seed whose answer differs
REVIVAL = dict(seed=941, T=12, V=5, scale=1.5, beam=3)


def revival_logits():
    r = np.random.default_rng(REVIVAL["seed"])
    return (r.normal(size=(REVIVAL["T"], REVIVAL["V"])).astype(np.float32) * REVIVAL["scale"]).astype(np.float32)


@pytest.mark.parametrize("T,seed", [(1, 0), (3, 1), (4, 2), (5, 3), (6, 4)])
def test_beam_search_equals_exact_prefix_probabilities(T, seed):
    """With the beam and the cutoff wider than every prefix, the prefix beam search is exact: each prefix's score is the
    log of the summed probability of its alignments (brute force over all V^T paths)."""
    rng = np.random.default_rng(seed)
    p = R.softmax32(rng.normal(size=(T, 4)).astype(np.float32) * 2)
    exact = R.exact_prefix_logprobs(p)
    out = R.beam_search(p, beam=100000, cutoff_top_n=4)
    real = [(lab, s) for lab, s in out if s < float(R.FLT_MAX)]   # -FLT_MAX-scored members are prefixes of probability 0
    assert {lab for lab, _ in real} == set(exact)
    for lab, s in real:
        assert abs(-s - exact[lab]) < 1e-5 * max(1.0, abs(exact[lab])), (lab, -s, exact[lab])
    best = sorted(exact.items(), key=lambda kv: -kv[1])[:5]
    assert [lab for lab, _ in real[:5]] == [lab for lab, _ in best]


def test_revival_input_needs_the_trie():
    """The recorded input: a prefix pruned from the beam is extended into again and must merge with the beam that already
    extends it (PathTrie::get_path_trie).  Fresh per-step ids give a different answer (duplicate strings)."""
    p = R.softmax32(revival_logits())
    good = R.beam_search(p, beam=REVIVAL["beam"], cutoff_top_n=REVIVAL["V"])
    bad = R.beam_search(p, beam=REVIVAL["beam"], cutoff_top_n=REVIVAL["V"], fresh_ids=True)
    assert good != bad
    assert len({lab for lab, _ in good}) == len(good)


def test_lse_guard_and_pruning():
    assert R.lse(R.NEG, np.float32(-3.0)) == np.float32(-3.0)
    assert R.lse(np.float32(-3.0), R.NEG) == np.float32(-3.0)
    assert R.lse(R.NEG, R.NEG) == R.NEG
    assert R.lse(np.float32(-1.0), np.float32(-2.0)) == R.lse(np.float32(-2.0), np.float32(-1.0))
    top = R.pruned_log_probs(np.array([0.25, 0.25, 0.5, 0.0], np.float32), 3)
    assert [c for c, _ in top] == [2, 0, 1]
    assert top[0][1] == np.float32(np.log(np.float32(0.5) + R.FLT_MIN))


def _tiny_conformer(text):
    cfg = ConformerConfig(conformer_layers=1, conformer_ffn_embed_dim=64, text_supervision=text)
    return Conformer(cfg)


def test_text_head_config_and_names(monkeypatch):
    monkeypatch.delenv("TEXT_SUPERVISION", raising=False)
    assert ConformerConfig().text_supervision is False
    monkeypatch.setenv("TEXT_SUPERVISION", "1")
    assert ConformerConfig().text_supervision is True            # the reference dataclass default (model.py:43)
    c = _tiny_conformer(True)
    names = {k: tuple(v.shape) for k, v in c.state_dict().items() if "text" in k}
    assert names == {"text_classifier.classifier.weight": (4000, 512), "text_classifier.classifier.bias": (4000,)}
    assert _tiny_conformer(False).text_classifier is None


def test_text_head_keys_load_or_are_ignored():
    from lip2speech_unit_amd.hubert import AVHubertConfig
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    from lip2speech_unit_amd import weights

    def build(text):
        return MultiTargetAVHubertEncoderModel.build_model(
            dtype=ops.F16, w2v_cfg=AVHubertConfig(encoder_layers=1),
            conformer_cfg=ConformerConfig(conformer_layers=1, text_supervision=text))
    on = build(True)
    sd = weights.synth_state_dict(weights.spec_of(build(False)), seed=0)
    # V_text comes from the checkpoint (39 = CHAR_LEVEL): the head is resized before the load
    sd["conformer.text_classifier.classifier.weight"] = torch.randn(39, 512)
    sd["conformer.text_classifier.classifier.bias"] = torch.randn(39)
    r = on.load_checkpoint_state(sd, check_resnet_sum=False)
    assert not [k for k in r.unexpected_keys if "text" in k]
    assert on.conformer.text_classes == 39
    assert torch.equal(on.conformer.text_classifier.classifier.weight.detach(), sd["conformer.text_classifier.classifier.weight"])
    off = build(False)
    r = off.load_checkpoint_state(sd, check_resnet_sum=False)            # still tolerated when the head is off
    assert {k for k in r.unexpected_keys if "text" in k} == {"conformer.text_classifier.classifier.weight",
                                                             "conformer.text_classifier.classifier.bias"}
    del sd["conformer.text_classifier.classifier.weight"], sd["conformer.text_classifier.classifier.bias"]
    from lip2speech_unit_amd.model_avhubert import CheckpointMismatch
    with pytest.raises(CheckpointMismatch):                              # a head that the checkpoint lacks is an error
        build(True).load_checkpoint_state(sd, check_resnet_sum=False)


def test_task_accepts_text_supervision(tmp_path):
    from lip2speech_unit_amd.task import Lip2SpeechTask, UnitDictionary, decode_config
    cfg = decode_config(data=str(tmp_path))
    cfg.text_supervision = True
    d = tmp_path / "dict.unt.txt"
    d.write_text("".join(f"{i} 1\n" for i in range(200)))
    Lip2SpeechTask(cfg, UnitDictionary.load(str(d)))


def test_ctc_ops_schemas_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("ctc_frames", "ctc_beam_search"):
        schema = str(getattr(torch.ops.lip2speech, name).default._schema)
        assert schema.rstrip().endswith("-> ()") and "!" in schema
    assert "l2s_ctc_beam_workspace" in ops.HOST_QUERIES
    with FakeTensorMode():
        B, L, V, K = 2, 9, 40, 8
        logits = torch.empty(B * L, V)
        lab = torch.empty(B, L, dtype=torch.int32)
        tc, tl = torch.empty(B, L, K, dtype=torch.int32), torch.empty(B, L, K)
        assert torch.ops.lip2speech.ctc_frames(logits, lab, tc, tl, B=B, L=L, V=39, K=K, ldl=V) is None
        ws = torch.empty(64, dtype=torch.int64)
        beams, blen, bsc = torch.empty(B, 3, L, dtype=torch.int32), torch.empty(B, 3, dtype=torch.int32), torch.empty(B, 3)
        assert torch.ops.lip2speech.ctc_beam_search(tc, tl, ws, beams, blen, bsc, B=B, L=L, K=K, beam=4, nbest=3) is None
    with pytest.raises(ops.L2SError):                                    # HIP only: no CPU path
        ops.ctc_frames(torch.zeros(4, 8), torch.zeros(1, 4, dtype=torch.int32), None, None, B=1, L=4, V=8, K=0)


def test_restatement_equals_literal_pathtrie_port():
    """The member-centric restatement (the kernel's form) against a literal port of ctcdecode's DecoderState::next / PathTrie
    (characters outer, prefixes inner, exists_ / get_path_trie revival / remove), with pruning on: narrow beams over many
    seeded inputs and the recorded revival input."""
    inputs = [(R.softmax32(revival_logits()), REVIVAL["beam"], REVIVAL["V"])]
    for seed in range(120):
        r = np.random.default_rng(seed)
        T, V, beam = int(r.integers(8, 25)), int(r.integers(4, 9)), int(r.integers(2, 9))
        inputs.append((R.softmax32((r.normal(size=(T, V)) * 1.5).astype(np.float32)), beam, int(r.integers(3, V + 1))))
    for p, beam, K in inputs:
        assert R.beam_search(p, beam=beam, cutoff_top_n=K) == R.beam_search_trie(p, beam=beam, cutoff_top_n=K)


def _voc_h(text=True, model_in_dim=925):
    from lip2speech_unit_amd.vocoder import AttrDict
    from tests.test_models_gpu import VOC_H
    h = dict(VOC_H, text_supervision=text, model_in_dim=model_in_dim)
    if text:
        h.update(num_embeddings_text=4000, embedding_dim_text=589)
    return AttrDict(h)


def test_vocoder_text_names_match_the_reference(golden_dir):
    import json
    import os
    from lip2speech_unit_amd import weights
    from lip2speech_unit_amd.vocoder import MelCodeGenerator
    d = np.load(os.path.join(golden_dir, "vocoder_text.npz"))
    cfg = json.loads(str(d["config"]))
    assert cfg == {"num_embeddings_text": 4000, "embedding_dim_text": 589, "model_in_dim": 925}
    g = MelCodeGenerator(_voc_h())
    ref = {str(n): tuple(int(x) for x in str(s).split(",")) if str(s) else () for n, s in zip(d["names"], d["shapes"])}
    assert dict(weights.spec_of(g)) == ref
    assert {k for k in ref if k.startswith("layer_text.")} == {
        "layer_text.0.weight", "layer_text.2.weight", "layer_text.2.bias", "layer_text.6.weight", "layer_text.6.bias"}
    with pytest.raises(ValueError, match="model_in_dim"):
        MelCodeGenerator(_voc_h(model_in_dim=336))
    assert not hasattr(MelCodeGenerator(_voc_h(text=False, model_in_dim=336)), "layer_text")


def test_synth_rule_for_the_text_embedding_only():
    from lip2speech_unit_amd import weights
    e = weights.synth_tensor("layer_text.0.weight", (4000, 589), 17)
    assert abs(e.std().item() - 1.0) < 0.01                  # unit scale like `dict`, not 589^-0.5
    assert torch.equal(weights.synth_tensor("dict.weight", (200, 128), 13), weights.synth_tensor("dict.weight", (200, 128), 13))


def test_conv_pre_weight_padded_for_the_text_columns():
    from lip2speech_unit_amd import weights
    from lip2speech_unit_amd.vocoder import MelCodeGenerator
    g = MelCodeGenerator(_voc_h())
    g.load_state_dict(weights.synth_state_dict(weights.spec_of(g), seed=3))
    g.remove_weight_norm()
    w, wp = g.conv_pre.effective_weight(), g._conv_pre_weight()
    assert wp.shape == (512, 928, 7)
    c = 80 + 128 + 589
    assert torch.equal(wp[:, :c], w[:, :c]) and torch.equal(wp[:, c + 3:], w[:, c:]) and not wp[:, c:c + 3].any()


def test_repeat_text_labels_is_the_reference_fill():
    from lip2speech_unit_amd.data import repeat_text_labels
    assert repeat_text_labels([0, 0, 5, 0, 5, 7, 0, 0, 3]) == [0, 0, 5, 5, 5, 7, 7, 7, 3]
    assert repeat_text_labels([4, 0, 0, 9]) == [4, 4, 4, 9]


def test_parse_manifest_reads_text_labels(tmp_path, monkeypatch):
    from lip2speech_unit_amd import data
    from tests._synth_dataset import make
    lab = make(str(tmp_path / "ds"), frames=(12, 9, 5))
    rows = [[0, 3, 3, 0, 7] + [0] * 19, [2] + [0] * 17, [0, 0, 9] + [0] * 7]
    with open(f"{lab}/test.txt", "w") as f:
        f.write("\n".join(" ".join(str(x) for x in r) for r in rows) + "\n")
    monkeypatch.delenv("TEXT_SUPERVISION", raising=False)
    assert len(data.parse_manifest(f"{lab}/test.tsv")) == 3                      # off: the label file is not read
    monkeypatch.setenv("TEXT_SUPERVISION", "1")
    monkeypatch.delenv("REPEAT_TEXT_LABELS", raising=False)
    fl = data.parse_manifest(f"{lab}/test.tsv")
    assert len(fl) == 4 and fl[3] == rows
    monkeypatch.setenv("REPEAT_TEXT_LABELS", "1")
    fl = data.parse_manifest(f"{lab}/test.tsv")
    assert fl[3][0][:6] == [0, 3, 3, 3, 7, 7] and fl[3][1] == [2] * 18
    ds = data.MelCodeDataset(fl, 320, 160, code_dict_path=f"{lab}/dict.unt.txt")
    for i in range(3):
        feats = ds[i][0]
        assert feats["t_label"].shape == feats["code"].shape                      # trimmed with the code
    # min_keep drops a row without consuming a label line (dataset_multi_input.py:75-90)
    fl = data.parse_manifest(f"{lab}/test.tsv", min_keep=6)
    assert len(fl[0]) == 2 and fl[3] == [[0, 3, 3, 3, 7] + [7] * 19, [2] * 18]


def test_multi_target_family_has_no_text_head(monkeypatch):
    from lip2speech_unit_amd.model import Conformer as MTConformer
    monkeypatch.setenv("TEXT_SUPERVISION", "1")
    assert MTConformer(ConformerConfig(conformer_layers=1, conformer_ffn_embed_dim=64)).text_classifier is None


def test_repeat_op_schema():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.lip2speech.ctc_repeat_labels.default._schema).rstrip().endswith("-> ()")
    with FakeTensorMode():
        x = torch.empty(2, 9, dtype=torch.int32)
        assert torch.ops.lip2speech.ctc_repeat_labels(x, torch.empty_like(x), B=2, L=9) is None
