#!/usr/bin/env python3
"""Audio-visual speech recognition CLI: the reference's `avhubert/infer_s2s.py` with `conf/s2s_decode.yaml` for the audio and
audio-visual models - decode a labelled subset from audio, video or both and report the word error rate.

  python -m lip2speech_unit_amd.infer_avsr common_eval.path=<ckpt.pt> common_eval.results_path=<dir> override.data=<label_dir> \
      override.label_dir=<label_dir> [override.modalities=['audio','video']] [dataset.* generation.* dtype graph as infer_s2s]
The overrides and the output files (hypo-<fid>.json, wer.<fid>) are infer_s2s's.  `override.modalities` is ['video'], ['audio']
or both in any order; its default is the checkpoint's `task.modalities`.  <label_dir>/<subset>.tsv holds id, video path, audio
path, frame count, sample count per clip; the audio is 16 kHz mono s16 wav.  Noise mixing (`override.noise_prob` > 0) is refused."""
import logging
import os
import sys

import numpy as np
import torch

from . import infer_s2s
from .asr_text import FairseqDictionary
from .infer_s2s import modality_names, read_manifest, read_overrides, search_config, write_results
from .validate import form_batches


def parse_overrides(argv):
    cfg = read_overrides(argv)
    mods = cfg["override.modalities"]
    if mods is not None:
        from .av_recogniser import modality_set
        try:
            cfg["override.modalities"] = list(modality_set(modality_names(mods), "override.modalities"))
        except ValueError as e:
            raise SystemExit(str(e))
    if float(cfg["override.noise_prob"]) > 0:
        raise SystemExit("override.noise_prob > 0: noise mixing (add_noise) is not built; decode clean audio")
    if cfg["dtype"] not in ("f16", "bf16"):
        raise SystemExit("dtype: f16 or bf16")
    return cfg


def load_wavs(root, clips, dev):
    """int16 [B, S] on the device, zero padded, and the clips' sample counts."""
    from .audio import read_wav_s16
    wavs = [read_wav_s16(os.path.join(root, c[3])) for c in clips]
    out = np.zeros((len(wavs), max(len(w) for w in wavs)), dtype=np.int16)
    for i, w in enumerate(wavs):
        out[i, :len(w)] = w
    return torch.from_numpy(out).to(dev), [len(w) for w in wavs]


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
    logger = logging.getLogger("lip2speech.infer_avsr")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    from . import ops
    from .av_recogniser import SpeechRecogniser, load_speech_recogniser
    dev = torch.device("cuda")
    model = load_speech_recogniser(cfg["common_eval.path"], dtype=ops.F16 if cfg["dtype"] == "f16" else ops.BF16,
                                   modalities=cfg["override.modalities"]).to(dev)
    dictionary = FairseqDictionary.load(os.path.join(label_dir, "dict.wrd.txt"))
    reader = SpeechRecogniser(model, dictionary, search_config(cfg), graph=bool(cfg["graph"]))
    logger.info("modalities: %s", list(reader.modalities))
    subset = cfg["dataset.gen_subset"]
    root, clips, refs = read_manifest(label_dir, subset, audio="audio" in reader.modalities)
    hyps = [""] * len(clips)
    for idx in form_batches([c[2] for c in clips], cfg["dataset.max_tokens"], cfg["dataset.batch_size"]):
        batch = [clips[i] for i in idx]
        video, mask = infer_s2s.load_batch(root, batch, dev) if "video" in reader.modalities else (None, None)
        wav, n_samples = load_wavs(root, batch, dev) if "audio" in reader.modalities else (None, None)
        for i, text in zip(idx, reader.transcribe(video, wav, n_samples, mask)):
            hyps[i] = text
            logger.info("HYP (%s): %s", clips[i][0], text)
    return write_results(cfg, clips, refs, hyps, logger)


if __name__ == "__main__":
    main()
