"""tests/golden/criterion.npz was written by the reference's own criterion (tools/make_criterion_golden.py); the float64 restatement
in tests/_criterion_reference.py - the yardstick of the GPU tests - has to reproduce every value in it.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _criterion_reference as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "criterion.npz")
LOG_KEYS = ("loss", "nll_loss", "mel_loss", "ctc_loss", "ntokens", "nsentences", "sample_size", "n_correct", "total")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def _inputs(g):
    net = {k: torch.from_numpy(g[k]) for k in ("encoder_out", "encoder_out_mel", "encoder_out_text")}
    sample = {k: torch.from_numpy(g[k]) for k in ("target", "mel", "input_lengths", "text_labels", "text_labels_lengths")}
    sample["ntokens"] = int(g["ntokens"])
    return net, sample


def _restate(g, sentence_avg, **kw):
    net, sample = _inputs(g)
    return R.forward(net, sample, pad=int(g["pad"]), label_smoothing=float(g["label_smoothing"]), mel_weight=float(g["mel_weight"]),
                     sentence_avg=sentence_avg, text_supervision=True, **kw)


def test_the_file_holds_the_cases_the_gates_need(gold):
    g = gold
    frames, tl = g["input_lengths"], g["text_labels_lengths"]
    labels = (g["target"] != int(g["pad"])).sum(1)
    assert g["encoder_out"].shape[0] <= 6 and frames.max() <= 100
    assert (labels <= 2 * frames).all() and (labels == 2 * frames).any() and (labels == 2 * frames - 1).any()
    mel_rows = np.array([np.flatnonzero(np.abs(m).sum(1))[-1] + 1 for m in g["mel"]])
    assert (mel_rows > 4 * frames).any() and (mel_rows < 4 * frames).any()
    assert (tl == 0).any() and (tl > 2 * frames).any()                      # empty target; more labels than frames
    off = np.concatenate([[0], np.cumsum(tl)])
    assert any((np.diff(g["text_labels"][off[b]:off[b + 1]]) == 0).any() for b in range(len(tl)) if tl[b] > 1)    # repeats
    assert g["f64_sa0_clip_ctc_loss"][tl > 2 * frames].max() == 0.0 and g["f64_sa0_clip_ctc_loss"][tl == 0].min() > 0


@pytest.mark.parametrize("sentence_avg", [False, True])
def test_float64_restatement_reproduces_every_stored_value(gold, sentence_avg):
    g, tag = gold, f"sa{int(sentence_avg)}_"
    log, clip = _restate(g, sentence_avg)
    for k in LOG_KEYS:
        want64, want32 = float(g["f64_" + tag + k]), float(g["f32_" + tag + k])
        assert abs(log[k] - want64) <= 1e-12 * abs(want64), (k, log[k], want64)
        assert abs(log[k] - want32) <= abs(want32 - want64) + 1e-12 * abs(want64), (k, log[k], want32)
    per = {"loss": clip["loss"], "nll_loss": clip["nll"], "mel_loss": clip["mel_loss"], "ctc_loss": clip["ctc_loss"],
           "n_correct": clip["n_correct"], "total": clip["n_tok"]}
    for k, v in per.items():
        want64, want32 = g["f64_" + tag + "clip_" + k], g["f32_" + tag + "clip_" + k]
        got = v.double().numpy()
        assert (np.abs(got - want64) <= 1e-12 * np.abs(want64)).all(), (k, got, want64)
        assert (np.abs(got - want32) <= np.abs(want32 - want64) + 1e-12 * np.abs(want64)).all(), k
    metrics = R.reduce_metrics([log])
    for k in ("loss", "nll_loss", "ppl", "accuracy", "mel_loss", "ctc_loss"):
        want = float(g["f64_" + tag + "metric_" + k])
        assert abs(metrics[k] - want) <= 1e-12 * abs(want), (k, metrics[k], want)


def test_float32_restatement_is_what_the_reference_computes_in_float32(gold):
    """The same text evaluated in float32 lands on the file's float32 values up to float32 rounding of the totals (the per-clip
    order of the restatement's sums differs from the reference's flat ones)."""
    log, _ = _restate(gold, False, dtype=torch.float32)
    for k in ("loss", "nll_loss", "mel_loss", "ctc_loss"):
        want = float(gold["f32_sa0_" + k])
        assert abs(log[k] - want) <= 8 * 2.0 ** -24 * abs(want), (k, log[k], want)


def test_alpha_recursion_agrees_with_torch_ctc(gold):
    g = gold
    text = torch.from_numpy(g["encoder_out_text"]).double().transpose(0, 1)
    lp = torch.log_softmax(text, -1).numpy()
    off = np.concatenate([[0], np.cumsum(g["text_labels_lengths"])])
    for b, frames in enumerate(g["input_lengths"]):
        nll = R.ctc_alpha_nll(lp[b, : 2 * frames], g["text_labels"][off[b]:off[b + 1]])
        nll = 0.0 if math.isinf(nll) else nll
        want = float(g["f64_sa0_clip_ctc_loss"][b])
        assert abs(nll - want) <= 1e-12 * max(abs(want), 1.0), (b, nll, want)


def test_clip_alone_rule_deviates_only_past_two_labels_per_frame(gold):
    """a clip whose label file holds more labels than 2 * frames.  The reference scores the surplus labels against
    logits computed from padding; the product stops at the clip's own frames.  Restatement only - nothing here is pinned."""
    g = gold
    net, sample = _inputs(g)
    lens = sample["input_lengths"].clone()
    same = R.unit_ce_per_clip(net["encoder_out"], sample["target"], lens, int(g["pad"]), clip_alone=False)
    mine = R.unit_ce_per_clip(net["encoder_out"], sample["target"], lens, int(g["pad"]), clip_alone=True)
    assert torch.equal(same["nll"], mine["nll"]) and torch.equal(same["n_tok"], mine["n_tok"])
    lens[3] -= 1                                                     # clip 3 now carries 30 labels over 2 * 15 frames... and
    lens[0] -= 1                                                     # clip 0 32 labels over 30 frames: two labels too many
    ref = R.unit_ce_per_clip(net["encoder_out"], sample["target"], lens, int(g["pad"]), clip_alone=False)
    mine = R.unit_ce_per_clip(net["encoder_out"], sample["target"], lens, int(g["pad"]), clip_alone=True)
    assert int(ref["n_tok"][0]) == 32 and int(mine["n_tok"][0]) == 30 and float(ref["nll"][0]) > float(mine["nll"][0])
    assert torch.equal(ref["nll"][1:], mine["nll"][1:])
