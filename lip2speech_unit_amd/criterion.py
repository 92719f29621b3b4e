"""`multi_target` criterion, forward (scoring) only — multi_target_lip2speech/criterion.py:19-179 on the HIP kernels of
csrc/criterion.hip.  It gives the figures a checkpoint is judged by (`loss`, `nll_loss`, `accuracy`, `mel_loss`, `ctc_loss`);
gradients and training are not built.

`forward` runs the model's training-time `forward`, then three launches over its fp32 row outputs (unit logits, mel rows, text
logits) that leave PER-CLIP partials on the device; batch totals are sums of those in clip order.  No log-probability tensor is
written (`get_normalized_probs` is not used) and nothing is copied to the host: every value of the logging output that depends on
the network is a 0-dim device tensor, so the whole call can be captured in a hipGraph.  `last_partials` keeps the per-clip
tensors of the latest call for callers that report per clip (validate.py copies them out once per batch).

The base class `LabelSmoothedCrossEntropyCriterion` is fairseq's and not in the reference tree; its arithmetic (loss =
(1 - eps - eps/(V-1)) nll + eps/(V-1) smooth; accuracy = argmax == target over non-pad; base-2 losses, ppl, accuracy in percent
in `reduce_metrics`) is restated from recollection - see tests/_criterion_reference.py.
"""
import math
from dataclasses import dataclass, field

import torch

from . import ops
from .plugin import CriterionBase, DataclassBase, cfg_get, interpolation, log_scalar, register_criterion

CTC_BLANK = 0          # helpers.py:22 SentenceProcessor.blank
CTC_WEIGHT = 1.0       # criterion.py:46
MAX_TEXT_LABELS = 511  # l2s_ctc_loss: 2 S + 1 extended labels, one lane each


def _total(per_clip):
    """Batch total of per-clip fp32 partials: summed in fp64, where the order of B <= a few thousand additions cannot show at
    fp32 resolution - the total is a function of the per-clip values alone."""
    return per_clip.double().sum()


@dataclass
class MultiTargetCriterionConfig(DataclassBase):
    """criterion.py:19-21 over fairseq's LabelSmoothedCrossEntropyCriterionConfig (field for field)."""
    label_smoothing: float = field(default=0.0, metadata={"help": "epsilon for label smoothing, 0 means no label smoothing"})
    report_accuracy: bool = field(default=False, metadata={"help": "report accuracy metric"})
    ignore_prefix_size: int = field(default=0, metadata={"help": "Ignore first N tokens"})
    sentence_avg: bool = interpolation("optimization.sentence_avg", False)
    mel_weight: float = field(default=1.0, metadata={"help": "weight for mel loss"})


@register_criterion("multi_target", dataclass=MultiTargetCriterionConfig)
class MultiTargetCriterion(CriterionBase):
    def __init__(self, task, sentence_avg, label_smoothing, mel_weight, ignore_prefix_size=0, report_accuracy=False):
        super().__init__(task)
        if ignore_prefix_size and int(ignore_prefix_size) > 0:
            raise NotImplementedError("multi_target criterion: ignore_prefix_size > 0 (criterion.py:154-160) is not built - the unit "
                                      "targets of this path carry no prefix token")
        self.sentence_avg = bool(sentence_avg)
        self.eps = float(label_smoothing)
        self.mel_weight = float(mel_weight)
        self.ignore_prefix_size = 0
        self.report_accuracy = bool(report_accuracy)
        self.text_supervision = bool(cfg_get(getattr(task, "cfg", None), "text_supervision", False))
        self.ctc_weight = CTC_WEIGHT
        self.step = 0
        self.last_partials = None

    def log_text_sample(self, *a, **k):
        raise NotImplementedError("multi_target criterion: the every-100-steps ground-truth / prediction text print "
                                  "(criterion.py:114-134) needs sentencepiece and a host copy of the logits; it is not built")

    # ---- the three device reductions ----------------------------------------------------------------------------------
    @staticmethod
    def _rows(t):
        """A [B, T, C] fp32 view whose rows (b, t) lie ld apart -> (tensor, ld); anything else is made dense."""
        t = t.float()
        if t.stride(2) == 1 and t.stride(0) == t.size(1) * t.stride(1) and t.stride(1) >= t.size(2):
            return t, t.stride(1)
        t = t.contiguous()
        return t, t.size(2)

    def unit_partials(self, logits, target, lens):
        """logits [B, T2, V] fp32, target [B, Lt] -> per-clip (nll, smooth, n_correct, n_tok)."""
        logits, ldl = self._rows(logits)
        B, T2, V = logits.shape
        dev = logits.device
        tgt = target.to(device=dev, dtype=torch.int32).contiguous()
        nll, smooth = torch.empty(B, device=dev), torch.empty(B, device=dev)
        n_correct, n_tok = torch.empty(B, device=dev, dtype=torch.int32), torch.empty(B, device=dev, dtype=torch.int32)
        ops.unit_ce(logits, tgt, nll, smooth, n_correct, n_tok, B=B, T2=T2, V=V, ldl=ldl, ldt=tgt.size(1), lens=lens, len_mul=2,
                    pad_idx=self.padding_idx)
        return nll, smooth, n_correct, n_tok

    def mel_partials(self, pred, targ, lens, frames):
        """pred [B, Tp, 80] fp32, targ [B, Tt, 80] -> per-clip (sum|p-t|, sum (p-t)^2, sum t^2, rows).  crop_len (criterion.py:67)
        = min(4 * longest clip, Tp, Tt) from shapes alone: the batch is padded to its longest clip."""
        pred = pred.float().contiguous()
        dev = pred.device
        targ = targ.to(device=dev, dtype=torch.float32).contiguous()
        B, Tp, C = pred.shape
        Tt = targ.size(1)
        l1, sq, tsq = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
        rows = torch.empty(B, device=dev, dtype=torch.int32)
        ops.mel_l1_sc(pred, targ, l1, sq, tsq, rows, B=B, Tm_pred=Tp, Tm_targ=Tt, crop_len=min(4 * frames, Tp, Tt), lens=lens,
                      len_mul=4, n_mels=C)
        return l1, sq, tsq, rows

    def ctc_partials(self, text, labels, label_lens, lens):
        """text [B, L, V] fp32 view, labels 1-D, label_lens [B] -> per-clip CTC nll (inf -> 0)."""
        text, ldl = self._rows(text)
        B, L, V = text.shape
        dev = text.device
        if label_lens.is_cuda:
            # the workspace is sized on the host: a device tensor only bounds S by the total label count
            s_max = int(labels.numel())
            if s_max > MAX_TEXT_LABELS:
                raise ops.L2SError("multi_target criterion: pass text_labels_lengths as a host tensor (as the collater does) when a "
                                   f"batch holds more than {MAX_TEXT_LABELS} text labels")
        else:
            s_max = int(label_lens.max()) if label_lens.numel() else 0
        tl = label_lens.to(device=dev, dtype=torch.int32).contiguous()
        offs = (torch.cumsum(tl, 0, dtype=torch.int32) - tl).contiguous()
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        work = torch.empty(ops.ctc_loss_workspace_bytes(B, L, s_max) // 4, device=dev, dtype=torch.float32)
        nll = torch.empty(B, device=dev)
        ops.ctc_loss(text, lab, tl, offs, work, nll, B=B, L=L, V=V, S_max=s_max, blank=CTC_BLANK, ldl=ldl, lens=lens, len_mul=2)
        return nll

    # ---- criterion.py:52-146 ---------------------------------------------------------------------------------------
    def forward(self, model, sample, reduce=True):
        """Returns (loss, sample_size, logging_output); losses are 0-dim device tensors, counts from the sample are ints."""
        if not reduce:
            raise NotImplementedError("multi_target criterion: reduce=False (per-position losses) is a training-time option")
        net_output = model(**sample["net_input"])
        return self.score(net_output, sample)

    def score(self, net_output, sample):
        unit = net_output["encoder_out"]                                   # [B, T2, V]
        B, dev = unit.size(0), unit.device
        pm = sample["net_input"]["padding_mask"]
        frames = pm.size(1)
        lens = ops.lens_from_mask(pm.to(device=dev, dtype=torch.bool).contiguous(), B, frames, dev)
        nll, smooth, n_correct, n_tok = self.unit_partials(unit, sample["target"], lens)
        eps_i = self.eps / (unit.size(-1) - 1)
        clip_loss = (1.0 - self.eps - eps_i) * nll + eps_i * smooth
        part = {"nll": nll, "smooth": smooth, "n_correct": n_correct, "n_tok": n_tok}
        mel_loss = None
        if net_output.get("encoder_out_mel") is not None:
            l1, sq, tsq, rows = self.mel_partials(net_output["encoder_out_mel"], sample["mel"], lens, frames)
            rows_f = rows.float()
            l1m, sc = l1 / net_output["encoder_out_mel"].size(-1), sq.sqrt() / tsq.sqrt()       # :80-82, :199
            clip_mel = l1m / rows_f + sc if self.sentence_avg else l1m + sc * rows_f             # :78-82, :200
            clip_loss = clip_loss + self.mel_weight * clip_mel                                   # :89
            mel_loss = _total(clip_mel)
            part.update(l1=l1, sq=sq, tsq=tsq, rows=rows, mel_loss=clip_mel)
        sample_size = sample["target"].size(0) if self.sentence_avg else sample["ntokens"]       # :91-93
        log = {"nll_loss": _total(nll), "mel_loss": mel_loss, "ntokens": sample["ntokens"], "nsentences": sample["target"].size(0),
               "sample_size": sample_size}
        if self.text_supervision and "text_labels" in sample and "text_labels_lengths" in sample:   # :103-112
            if net_output.get("encoder_out_text") is None:
                raise ops.L2SError("multi_target criterion: text_supervision is on but the model has no text head "
                                   "(build it with TEXT_SUPERVISION=1)")
            text = net_output["encoder_out_text"].transpose(0, 1)           # T x B x C as the models give it -> [B, L, V] view
            ctc = self.ctc_partials(text, sample["text_labels"], sample["text_labels_lengths"], lens)
            clip_loss = clip_loss + self.ctc_weight * ctc                   # :111
            log["ctc_loss"] = _total(ctc)
            part["ctc_loss"] = ctc
        part["loss"] = clip_loss
        loss = _total(clip_loss)
        log["loss"] = loss
        if self.report_accuracy:                                            # :138-141
            log["n_correct"], log["total"] = n_correct.sum(), n_tok.sum()   # integers: exact
        self.last_partials = part
        self.step += 1
        return loss, sample_size, log

    # ---- criterion.py:163-179 over fairseq's reduce_metrics -----------------------------------------------------------
    @staticmethod
    def aggregate(logging_outputs):
        """The scalars `reduce_metrics` logs, as a dict: loss (base 2, per sample_size), nll_loss (base 2, per token), ppl,
        accuracy (percent), mel_loss and ctc_loss (per sample_size)."""
        def tot(key):
            return sum(float(log.get(key, 0) or 0) for log in logging_outputs)
        sample_size, ntokens = tot("sample_size"), tot("ntokens")
        out = {"loss": tot("loss") / sample_size / math.log(2), "nll_loss": tot("nll_loss") / ntokens / math.log(2)}
        out["ppl"] = 2 ** out["nll_loss"]
        if tot("total") > 0:
            out["accuracy"] = tot("n_correct") * 100.0 / tot("total")
        if logging_outputs[0].get("mel_loss") is not None:
            out["mel_loss"] = tot("mel_loss") / sample_size
        if "ctc_loss" in logging_outputs[0]:
            out["ctc_loss"] = tot("ctc_loss") / sample_size
        return out

    @classmethod
    def reduce_metrics(cls, logging_outputs) -> None:
        agg = cls.aggregate(logging_outputs)
        sample_size = sum(float(log.get("sample_size", 0)) for log in logging_outputs)
        ntokens = sum(float(log.get("ntokens", 0)) for log in logging_outputs)
        log_scalar("loss", agg["loss"], sample_size, round=3)
        log_scalar("nll_loss", agg["nll_loss"], ntokens, round=3)
        log_scalar("ppl", agg["ppl"], 0, round=3)
        if "accuracy" in agg:
            log_scalar("accuracy", round(agg["accuracy"], 3), 0)
        for k in ("mel_loss", "ctc_loss"):
            if k in agg:
                log_scalar(k, agg[k], sample_size, round=5)

    @staticmethod
    def logging_outputs_can_be_summed() -> bool:
        return True
