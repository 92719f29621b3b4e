#!/usr/bin/env python3
"""Writes tests/golden/criterion.npz by RUNNING the reference's own criterion (multi_target_lip2speech/criterion.py, imported as a
single file) on seeded net_outputs and samples, on the CPU, in float32 and in float64.

  python tools/make_criterion_golden.py <reference>/multi_target_lip2speech

fairseq is not vendored in the reference tree, so the names criterion.py imports from it are stand-ins defined HERE:
`metrics.log_scalar` (a recorder), `utils.item`, `register_criterion` (a no-op) and the base class
`LabelSmoothedCrossEntropyCriterion` with `label_smoothed_nll_loss` / `compute_accuracy` / `reduce_metrics` - recalled from fairseq,
not pinned.  `SentenceProcessor` is the reference's own (helpers.py; needs sentencepiece and its data/ model file).

Stored per case: the inputs, every logging_output value of the batch run, the `reduce_metrics` scalars, and each clip's values from a
one-clip run of the same program (`clip_*`, [B]) - all as f32_* and f64_*.  Cases: both sentence_avg values on a 5-clip batch with a
label count equal to and one short of 2 * frames, a mel target longer and one shorter than 4 * frames, text targets with repeats, an
empty text target and a clip too short for its text (zero_infinity).  No label count exceeds 2 * frames.
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
from tests import _criterion_reference as R  # noqa: E402

GOLDEN = os.path.join(HERE, "..", "tests", "golden", "criterion.npz")
PAD, EPS, MEL_W = 1, 0.1, 10.0
FRAMES = [16, 12, 9, 16, 5]
LABELS = [32, 23, 18, 30, 10]                    # = 2 * frames, one short of it, ...
MEL_LENS = [70, 44, 36, 64, 20]                  # longer than 4 * 16, shorter than 4 * 12, ...
TEXT = [[5, 5, 9, 12], [], [7, 8, 9], [3, 3, 3, 4], [11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22]]   # repeats, empty, too long for 10 frames
SCALARS = []


def install_standins():
    fairseq = types.ModuleType("fairseq")
    metrics = types.ModuleType("fairseq.metrics")
    metrics.log_scalar = lambda key, value, weight=1, round=None, priority=10: SCALARS.append((key, float(value)))
    utils = types.ModuleType("fairseq.utils")
    utils.item = lambda t: t.item() if hasattr(t, "item") else t
    crit = types.ModuleType("fairseq.criterions")
    crit.register_criterion = lambda name, dataclass=None: (lambda cls: cls)
    lsce = types.ModuleType("fairseq.criterions.label_smoothed_cross_entropy")

    class LabelSmoothedCrossEntropyCriterionConfig:
        pass

    def label_smoothed_nll_loss(lprobs, target, epsilon, ignore_index=None, reduce=True):
        if target.dim() == lprobs.dim() - 1:
            target = target.unsqueeze(-1)
        nll_loss = -lprobs.gather(dim=-1, index=target)
        smooth_loss = -lprobs.sum(dim=-1, keepdim=True)
        if ignore_index is not None:
            pad_mask = target.eq(ignore_index)
            nll_loss.masked_fill_(pad_mask, 0.0)
            smooth_loss.masked_fill_(pad_mask, 0.0)
        if reduce:
            nll_loss, smooth_loss = nll_loss.sum(), smooth_loss.sum()
        eps_i = epsilon / (lprobs.size(-1) - 1)
        return (1.0 - epsilon - eps_i) * nll_loss + eps_i * smooth_loss, nll_loss

    class LabelSmoothedCrossEntropyCriterion(torch.nn.Module):
        def __init__(self, task, sentence_avg, label_smoothing, ignore_prefix_size=0, report_accuracy=False):
            super().__init__()
            self.task, self.padding_idx = task, task.target_dictionary.pad()
            self.sentence_avg, self.eps = sentence_avg, label_smoothing
            self.ignore_prefix_size, self.report_accuracy = ignore_prefix_size, report_accuracy

        def compute_loss(self, model, net_output, sample, reduce=True):
            lprobs, target = self.get_lprobs_and_target(model, net_output, sample)
            return label_smoothed_nll_loss(lprobs, target, self.eps, ignore_index=self.padding_idx, reduce=reduce)

        def compute_accuracy(self, model, net_output, sample):
            lprobs, target = self.get_lprobs_and_target(model, net_output, sample)
            mask = target.ne(self.padding_idx)
            n_correct = torch.sum(lprobs.argmax(1).masked_select(mask).eq(target.masked_select(mask)))
            return n_correct, torch.sum(mask)

        @classmethod
        def reduce_metrics(cls, logging_outputs):
            s = lambda k: sum(float(log.get(k, 0)) for log in logging_outputs)     # noqa: E731
            metrics.log_scalar("loss", s("loss") / s("sample_size") / math.log(2))
            nll = s("nll_loss") / s("ntokens") / math.log(2)
            metrics.log_scalar("nll_loss", nll)
            metrics.log_scalar("ppl", 2 ** nll)
            if s("total") > 0:
                metrics.log_scalar("accuracy", s("n_correct") * 100.0 / s("total"))

    lsce.LabelSmoothedCrossEntropyCriterion = LabelSmoothedCrossEntropyCriterion
    lsce.LabelSmoothedCrossEntropyCriterionConfig = LabelSmoothedCrossEntropyCriterionConfig
    fairseq.metrics, fairseq.utils, fairseq.criterions = metrics, utils, crit
    for m in (fairseq, metrics, utils, crit, lsce):
        sys.modules[m.__name__] = m


def load_reference(ref_dir):
    pkg = types.ModuleType("_mtl_ref")          # a package shell: criterion.py's `from .helpers import ...` resolves, __init__ never runs
    pkg.__path__ = [ref_dir]
    sys.modules["_mtl_ref"] = pkg
    return importlib.import_module("_mtl_ref.criterion")


class _Dict:
    def pad(self):
        return PAD


class _Task:
    cfg = types.SimpleNamespace(text_supervision=True)
    target_dictionary = _Dict()


class _Model:
    def __init__(self, net_output):
        self.net_output = net_output

    def __call__(self, **net_input):
        return self.net_output

    def get_normalized_probs(self, net_output, log_probs):
        return torch.log_softmax(net_output["encoder_out"], dim=-1)

    def get_targets(self, sample, net_output):
        return sample["target"]


def run(mod, case, dtype, sentence_avg, clips=None):
    sl = slice(None) if clips is None else clips
    B = len(FRAMES)
    off = np.concatenate([[0], np.cumsum(case["text_labels_lengths"].numpy())])
    idx = list(range(B))[sl]
    text_labels = torch.cat([case["text_labels"][off[b]:off[b + 1]] for b in idx]) if idx else case["text_labels"][:0]
    net_output = {"encoder_out": case["encoder_out"][sl].to(dtype), "encoder_out_mel": case["encoder_out_mel"][sl].to(dtype),
                  "encoder_out_text": case["encoder_out_text"][:, sl].to(dtype)}
    sample = {"net_input": {"padding_mask": case["padding_mask"][sl]}, "target": case["target"][sl],
              "ntokens": int(sum(LABELS[b] for b in idx)), "mel": case["mel"][sl].to(dtype),
              "input_lengths": case["input_lengths"][sl], "text_labels": text_labels,
              "text_labels_lengths": case["text_labels_lengths"][sl]}
    crit = mod.LabelSmoothedCrossEntropyCriterionLengthMatch(_Task(), sentence_avg, EPS, MEL_W, report_accuracy=True)
    crit.step = 1                               # keeps the every-100-steps text print out of the run
    loss, sample_size, log = crit.forward(_Model(net_output), sample)
    log = {k: (v.item() if hasattr(v, "item") else v) for k, v in log.items()}
    assert float(loss) == log["loss"] and sample_size == log["sample_size"]
    return log, type(crit)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    install_standins()
    mod = load_reference(os.path.abspath(sys.argv[1]))
    case = R.draw_case(2024, FRAMES, LABELS, MEL_LENS, TEXT, V=204, Vt=96, pad=PAD)
    out = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in case.items()}
    out.update(pad=np.asarray(PAD), label_smoothing=np.asarray(EPS), mel_weight=np.asarray(MEL_W))
    for sa in (False, True):
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            tag = f"{name}_sa{int(sa)}_"
            log, cls = run(mod, case, dtype, sa)
            for k, v in log.items():
                out[tag + k] = np.asarray(v, np.float64)
            SCALARS.clear()
            cls.reduce_metrics([log])
            for k, v in SCALARS:
                out[tag + "metric_" + k] = np.asarray(v, np.float64)
            per = [run(mod, case, dtype, sa, clips=slice(b, b + 1))[0] for b in range(len(FRAMES))]
            for k in per[0]:
                out[tag + "clip_" + k] = np.asarray([p[k] for p in per], np.float64)
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
    for k in ("nll_loss", "mel_loss", "ctc_loss", "loss"):
        a, b = out["f32_sa0_" + k], out["f64_sa0_" + k]
        print(f"  {k}: f64 {b:.9g}  |f32 - f64| / |f64| = {abs(a - b) / abs(b):.2e}")


if __name__ == "__main__":
    main()
