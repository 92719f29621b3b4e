#!/usr/bin/env python3
"""Validation CLI: the `multi_target` criterion's figures for a checkpoint on a labelled subset (what `fairseq-validate` prints
for the reference's fine-tuning config, conf/lrs3/multi_target_avhubert.yaml:46-64).

  python -m lip2speech_unit_amd.validate common_eval.path=<ckpt.pt> common_eval.results_path=<dir> override.data=<label_dir> \
      override.label_dir=<label_dir> [dataset.gen_subset=test] [dataset.max_tokens=3600] [dataset.batch_size=N] \
      [criterion.label_smoothing=0.1 criterion.mel_weight=10 criterion.report_accuracy=true criterion.sentence_avg=true] \
      [dtype=f16|bf16|f32] [synthetic_weights=true]
`key=value` overrides as inference.py takes them; the defaults are the yaml's (max_tokens 3600 frames, label_smoothing 0.1,
mel_weight 10, report_accuracy, optimization.sentence_avg true).  TEXT_SUPERVISION=1 adds the CTC term when <label_dir>/<subset>.txt
(one line of piece ids per clip) exists.

Clips are batched longest first under `dataset.max_tokens` (frames of the padded batch) and `dataset.batch_size`; a clip's partials
do not depend on its batch, and the per-clip partials of a batch come to the host in ONE copy.  Prints
  valid | loss … | nll_loss … | ppl … | accuracy … | mel_loss … [| ctc_loss …]
and writes <results_path>/valid-<subset>.json (the aggregate, the summed logging output and every clip's partials).
Single process: validation is not sharded over ranks.
"""
import json
import logging
import os
import sys

import numpy as np
import torch

from . import inference as s1
from .criterion import MultiTargetCriterion
from .task import Lip2SpeechTask, decode_config

DEFAULTS = {
    "common_eval.path": None, "common_eval.results_path": None, "override.data": None, "override.label_dir": None,
    "dataset.gen_subset": "test", "dataset.max_tokens": 3600, "dataset.batch_size": None,
    "criterion._name": "multi_target", "criterion.label_smoothing": 0.1, "criterion.mel_weight": 10.0,
    "criterion.report_accuracy": True, "criterion.ignore_prefix_size": 0, "criterion.sentence_avg": None,
    "optimization.sentence_avg": True,
    "dtype": "f16", "synthetic_weights": False, "fp16": False,
    "model.encoder_layers": 24, "model.conformer_layers": 12, "model.check_resnet_checksum": True,
}
PARTIAL_KEYS = ("loss", "nll", "smooth", "n_correct", "n_tok", "mel_loss", "l1", "sq", "tsq", "rows", "ctc_loss")


def parse_overrides(argv):
    cfg = dict(DEFAULTS)
    for a in argv:
        if a.startswith("--") or "=" not in a:
            raise SystemExit(f"cannot parse argument '{a}' (hydra-style key=value overrides expected)")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k not in DEFAULTS:
            raise SystemExit(f"unknown override '{k}' (known: {', '.join(sorted(DEFAULTS))})")
        cfg[k] = s1._scalar(v)
    if cfg["criterion.sentence_avg"] is None:
        cfg["criterion.sentence_avg"] = bool(cfg["optimization.sentence_avg"])      # II("optimization.sentence_avg")
    return cfg


def criterion_config(cfg):
    return {k.split(".", 1)[1]: v for k, v in cfg.items() if k.startswith("criterion.")}


def form_batches(sizes, max_tokens=None, batch_size=None):
    """Lists of dataset indices, longest clip first (ties in manifest order): a batch is closed when one more clip would take its
    padded size - clips x frames of its longest clip, fairseq's `max_tokens` for this dataset - past max_tokens, or its clip
    count past batch_size."""
    order = [int(i) for i in np.lexsort((np.arange(len(sizes)), -np.asarray(sizes, dtype=np.int64)))]
    batches, cur = [], []
    for i in order:
        if max_tokens and sizes[i] > max_tokens:
            raise ValueError(f"clip {i} has {sizes[i]} frames: more than dataset.max_tokens={max_tokens}")
        full = cur and ((batch_size and len(cur) >= batch_size) or (max_tokens and (len(cur) + 1) * sizes[cur[0]] > max_tokens))
        if full:
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def to_device(batch, dev):
    ni = batch["net_input"]
    ni["source"]["video"] = ni["source"]["video"].to(dev)
    ni["padding_mask"], ni["spk_emb"] = ni["padding_mask"].to(dev), ni["spk_emb"].to(dev)
    batch["target"], batch["mel"] = batch["target"].to(dev), batch["mel"].to(dev)
    if "text_labels" in batch:
        batch["text_labels"] = batch["text_labels"].to(dev)      # the lengths stay on the host: they size the CTC workspace
    return batch


def pack_partials(part, keys):
    """[len(keys), B] fp64 device tensor: the batch's per-clip partials in one block (fp64 holds the int32 counts exactly)."""
    return torch.stack([part[k].double() for k in keys])


def validate_dataset(cfg, task, model, criterion, ds, logger=None):
    dev = next(model.parameters()).device
    clips, logs = {}, []
    for idx in form_batches(ds.sizes, cfg["dataset.max_tokens"], cfg["dataset.batch_size"]):
        batch = ds.collater([ds[i] for i in idx])
        if batch["target"] is None:
            raise SystemExit("validation needs unit labels (<label_dir>/<subset>.unt)")
        batch = to_device(batch, dev)
        _, sample_size, log = task.valid_step(batch, model, criterion)
        keys = [k for k in PARTIAL_KEYS if k in criterion.last_partials]
        host = pack_partials(criterion.last_partials, keys).cpu().numpy()          # the batch's one device -> host copy
        for j, i in enumerate(idx):
            clips[i] = {"utt_id": batch["utt_id"][j], "frames": int(ds.sizes[i]), "ntokens": int(batch["target_lengths"][j]),
                        **{k: (int(host[r, j]) if k in ("n_correct", "n_tok", "rows") else float(host[r, j]))
                           for r, k in enumerate(keys)}}
        # the batch's logging output, formed on the host from the per-clip rows in clip order
        col = {k: host[r] for r, k in enumerate(keys)}
        out = {"loss": float(sum(col["loss"])), "nll_loss": float(sum(col["nll"])), "ntokens": int(log["ntokens"]),
               "nsentences": int(log["nsentences"]), "sample_size": int(sample_size),
               "mel_loss": float(sum(col["mel_loss"])) if "mel_loss" in col else None}
        if "ctc_loss" in col:
            out["ctc_loss"] = float(sum(col["ctc_loss"]))
        if criterion.report_accuracy:
            out["n_correct"], out["total"] = int(sum(col["n_correct"])), int(sum(col["n_tok"]))
        logs.append(out)
    agg = MultiTargetCriterion.aggregate(logs)
    totals = {k: sum(log[k] for log in logs) for k in logs[0] if logs[0][k] is not None}
    return agg, totals, [clips[i] for i in sorted(clips)]


def format_line(agg):
    order = ("loss", "nll_loss", "ppl", "accuracy", "mel_loss", "ctc_loss")
    rnd = {"loss": 3, "nll_loss": 3, "ppl": 2, "accuracy": 3, "mel_loss": 5, "ctc_loss": 5}
    return "valid | " + " | ".join(f"{k} {agg[k]:.{rnd[k]}f}" for k in order if k in agg)


def main(argv=None):
    cfg = parse_overrides(sys.argv[1:] if argv is None else argv)
    results_path = cfg["common_eval.results_path"]
    assert results_path, "common_eval.results_path is required"
    os.makedirs(results_path, exist_ok=True)
    logging.basicConfig(format="%(asctime)s | %(levelname)s | %(name)s | %(message)s", level=logging.INFO, force=True,
                        handlers=[logging.StreamHandler(sys.stdout)])
    logger = logging.getLogger("lip2speech.validate")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    tcfg = decode_config(data=cfg["override.data"], label_dir=cfg["override.label_dir"], fp16=bool(cfg["fp16"]))
    task = Lip2SpeechTask(tcfg)
    model = s1.build_model(cfg, task, logger)
    criterion = task.build_criterion(criterion_config(cfg))
    subset = cfg["dataset.gen_subset"]
    ds = task.load_dataset(subset)
    agg, totals, clips = validate_dataset(cfg, task, model, criterion, ds, logger)
    line = format_line(agg)
    print(line)
    out = {"subset": subset, "aggregate": agg, "totals": totals, "clips": clips, "criterion": criterion_config(cfg)}
    with open(os.path.join(results_path, f"valid-{subset}.json"), "w") as f:
        json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
