#!/usr/bin/env python3
"""Lip-reading CLI: the reference's `avhubert/infer_s2s.py` with `conf/s2s_decode.yaml` - decode a labelled subset with the
fine-tuned AV-HuBERT seq2seq model and report the word error rate.

  python -m lip2speech_unit_amd.infer_s2s common_eval.path=<ckpt.pt> common_eval.results_path=<dir> override.data=<label_dir> \
      override.label_dir=<label_dir> [dataset.gen_subset=test] [dataset.max_tokens=1000] [dataset.batch_size=N] \
      [generation.beam=50 generation.max_len_a=1.0 generation.max_len_b=0 generation.min_len=1 generation.lenpen=1.0 \
       generation.unkpen=0 generation.temperature=1.0 generation.unnormalized=false generation.nbest=1] \
      [override.modalities=['video']] [dtype=f16|bf16] [graph=true]
`key=value` overrides as validate.py takes them.  <label_dir> holds <subset>.tsv (the manifest), <subset>.wrd (one reference
sentence per clip) and dict.wrd.txt (the sentencepiece units).  Video only: a checkpoint or an override that asks for the audio
modality is refused.  Writes <results_path>/hypo-<fid>.json ({"utt_id", "ref", "hypo"}, lists over the clips) and
<results_path>/wer.<fid> ("WER: <percent>" and "err / num_ref_words = <e> / <n>"), fid = the process id as in the reference
(infer_s2s.py:254-262); the figures are asr_text.wer's."""
import json
import logging
import os
import sys

import numpy as np
import torch

from . import inference as s1
from .asr_text import FairseqDictionary, wer
from .validate import form_batches

DEFAULTS = {
    "common_eval.path": None, "common_eval.results_path": None, "override.data": None, "override.label_dir": None,
    "override.modalities": None, "override.noise_prob": 0.0, "override.noise_snr": 0,
    "dataset.gen_subset": "test", "dataset.max_tokens": 1000, "dataset.batch_size": None,
    "generation.beam": 50, "generation.max_len_a": 1.0, "generation.max_len_b": 0, "generation.min_len": 1, "generation.lenpen": 1.0,
    "generation.unkpen": 0.0, "generation.temperature": 1.0, "generation.unnormalized": False, "generation.nbest": 1,
    "dtype": "f16", "graph": True, "fid": None,
}


def read_overrides(argv):
    """DEFAULTS updated by the `key=value` arguments; what the values mean is the caller's check."""
    cfg = dict(DEFAULTS)
    for a in argv:
        if a.startswith("--") or "=" not in a:
            raise SystemExit(f"cannot parse argument '{a}' (hydra-style key=value overrides expected)")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k not in DEFAULTS:
            raise SystemExit(f"unknown override '{k}' (known: {', '.join(sorted(DEFAULTS))})")
        cfg[k] = s1._scalar(v)
    return cfg


def modality_names(mods):
    return [m.strip(" '\"") for m in str(mods).strip("[]").split(",") if m.strip(" '\"")]


def parse_overrides(argv):
    cfg = read_overrides(argv)
    mods = cfg["override.modalities"]
    if mods is not None:
        names = modality_names(mods)
        if names != ["video"]:
            raise SystemExit(f"override.modalities={mods}: the lip reader takes video only")
        cfg["override.modalities"] = names
    if cfg["dtype"] not in ("f16", "bf16"):
        raise SystemExit("dtype: f16 or bf16")
    return cfg


def search_config(cfg):
    from .lip_reader import BeamSearchConfig
    g = lambda k: cfg["generation." + k]
    return BeamSearchConfig(beam=int(g("beam")), max_len_a=float(g("max_len_a")), max_len_b=int(g("max_len_b")), min_len=int(g("min_len")),
                            lenpen=float(g("lenpen")), unk_penalty=float(g("unkpen")), temperature=float(g("temperature")),
                            normalize_scores=not bool(g("unnormalized")), nbest=int(g("nbest")))


def read_manifest(label_dir, subset, audio=False):
    """(root, [(fid, video path, n_frames)], references or None); audio=True: the clips also carry the tsv's audio column and
    sample count, (fid, video path, n_frames, audio path, n_samples)."""
    with open(os.path.join(label_dir, subset + ".tsv")) as f:
        root = f.readline().strip()
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    refs = None
    p = os.path.join(label_dir, subset + ".wrd")
    if os.path.exists(p):
        refs = open(p, encoding="utf-8").read().splitlines()
        if len(refs) != len(rows):
            raise SystemExit(f"{p} has {len(refs)} lines for {len(rows)} clips")
    if audio:
        if any(len(r) < 5 for r in rows):
            raise SystemExit(f"{label_dir}/{subset}.tsv: id, video path, audio path, frame count, sample count expected")
        return root, [(r[0], r[1], int(r[-2]), r[2], int(r[-1])) for r in rows], refs
    return root, [(r[0], r[1], int(r[-2])) for r in rows], refs


def load_batch(root, clips, dev):
    from .data import load_video, normalize_frames
    frames = [normalize_frames(load_video(os.path.join(root, c[1]))) for c in clips]
    T = max(f.shape[0] for f in frames)
    video = torch.zeros(len(frames), 1, T, frames[0].shape[1], frames[0].shape[2])
    mask = torch.zeros(len(frames), T, dtype=torch.bool)
    for i, f in enumerate(frames):
        video[i, 0, :f.shape[0]] = torch.from_numpy(np.ascontiguousarray(f))
        mask[i, f.shape[0]:] = True
    return video.to(dev), mask.to(dev)


def main(argv=None):
    cfg = parse_overrides(sys.argv[1:] if argv is None else argv)
    results_path = cfg["common_eval.results_path"]
    if not results_path or not cfg["common_eval.path"]:
        raise SystemExit("common_eval.path and common_eval.results_path are required")
    label_dir = cfg["override.label_dir"] or cfg["override.data"]
    if not label_dir:
        raise SystemExit("override.label_dir (or override.data) is required")
    os.makedirs(results_path, exist_ok=True)
    logging.basicConfig(format="%(asctime)s | %(levelname)s | %(name)s | %(message)s", level=logging.INFO, force=True,
                        handlers=[logging.StreamHandler(sys.stdout)])
    logger = logging.getLogger("lip2speech.infer_s2s")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    from . import ops
    from .lip_reader import LipReader, load_lip_reader
    dev = torch.device("cuda")
    model = load_lip_reader(cfg["common_eval.path"], dtype=ops.F16 if cfg["dtype"] == "f16" else ops.BF16).to(dev)
    dictionary = FairseqDictionary.load(os.path.join(label_dir, "dict.wrd.txt"))
    reader = LipReader(model, dictionary, search_config(cfg), graph=bool(cfg["graph"]))
    subset = cfg["dataset.gen_subset"]
    root, clips, refs = read_manifest(label_dir, subset)
    hyps = [""] * len(clips)
    for idx in form_batches([c[2] for c in clips], cfg["dataset.max_tokens"], cfg["dataset.batch_size"]):
        video, mask = load_batch(root, [clips[i] for i in idx], dev)
        for i, text in zip(idx, reader.transcribe(video, mask)):
            hyps[i] = text
            logger.info("HYP (%s): %s", clips[i][0], text)
    return write_results(cfg, clips, refs, hyps, logger)


def write_results(cfg, clips, refs, hyps, logger):
    """hypo-<fid>.json and, with references, wer.<fid> under common_eval.results_path; returns what the json holds (and the WER)."""
    results_path = cfg["common_eval.results_path"]
    fid = cfg["fid"] if cfg["fid"] is not None else os.getpid()
    out = {"utt_id": [c[0] for c in clips], "ref": refs if refs is not None else [""] * len(clips), "hypo": hyps}
    with open(os.path.join(results_path, f"hypo-{fid}.json"), "w") as f:
        json.dump(out, f, indent=4)
    if refs is not None:
        w = wer(refs, hyps)
        with open(os.path.join(results_path, f"wer.{fid}"), "w") as f:
            f.write(f"WER: {w['wer']}\nerr / num_ref_words = {w['n_err']} / {w['n_total']}\n\n")
        logger.info("WER: %s%%", w["wer"])
        out["wer"] = w
    return out


if __name__ == "__main__":
    main()
