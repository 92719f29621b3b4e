#!/usr/bin/env python3
"""Writes the speech units of a folder of wavs - what extract_speech_units.sh:6-11 stores as label/<split>.unt (HuBERT-base
layer-6 features quantised by km.bin, `--hide-fname`: ids only), computed on the device.

  python -m lip2speech_unit_amd.extract_units <audio_root> <out.unt> --hubert <ckpt> --kmeans <km.bin|centers.npy>
      [--layer 6] [--manifest <x_unit_manifest.txt>] [--batch N] [--dtype f32|f16|bf16]
Walks <audio_root>/**/*.wav (16 kHz mono s16) in sorted order, or takes the files of a manifest (first line: root, then one
`<rel path>\\t<samples>` per line, the format extract_speech_units.sh feeds its quantiser) in manifest order; runs
length-sorted batches, one forward per batch, and writes one line of space-separated ids per clip in that order.
"""
import argparse
import glob
import os

import numpy as np
import torch

from . import audio, ops, speech_units

DTYPES = {"f32": ops.F32, "f16": ops.F16, "bf16": ops.BF16}


def list_clips(audio_root, manifest=None):
    if manifest is None:
        return sorted(glob.glob(os.path.join(audio_root, "**", "*.wav"), recursive=True))
    with open(manifest) as f:
        lines = [ln.rstrip("\n") for ln in f if ln.strip()]
    if not lines:
        raise SystemExit(f"{manifest}: empty manifest")
    return [os.path.join(audio_root, ln.split("\t")[0]) for ln in lines[1:]]


def extract(extractor, clips, batch=16):
    """clips: a list of int16 arrays.  Returns their unit ids in the same order (length-sorted batches, one forward each)."""
    order = sorted(range(len(clips)), key=lambda i: clips[i].shape[0])
    out = [None] * len(clips)
    for i in range(0, len(order), max(batch, 1)):
        group = order[i:i + max(batch, 1)]
        lens = [clips[j].shape[0] for j in group]
        pcm = np.zeros((len(group), max(lens)), np.int16)
        for r, j in enumerate(group):
            pcm[r, : lens[r]] = clips[j]
        for j, ids in zip(group, extractor.units(torch.from_numpy(pcm).cuda(), lens)):
            out[j] = ids
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("audio_root")
    p.add_argument("out_unt")
    p.add_argument("--hubert", required=True)
    p.add_argument("--kmeans", required=True)
    p.add_argument("--layer", type=int, default=6)
    p.add_argument("--manifest", default=None)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--dtype", default="f32", choices=sorted(DTYPES))
    a = p.parse_args(argv)
    if a.layer < 1:
        p.error("--layer must be at least 1")
    if a.batch < 1:
        p.error("--batch must be at least 1")
    for path in (a.hubert, a.kmeans) + ((a.manifest,) if a.manifest else ()):
        if not os.path.isfile(path):
            p.error(f"{path}: no such file")
    if not os.path.isdir(a.audio_root):
        p.error(f"{a.audio_root}: no such directory")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    dt = DTYPES[a.dtype]
    extractor = speech_units.SpeechUnitExtractor(speech_units.load_hubert(a.hubert, dtype=dt), speech_units.load_kmeans(a.kmeans),
                                                 layer=a.layer, dtype=dt)
    paths = list_clips(a.audio_root, a.manifest)
    clips = [audio.read_wav_s16(pth) for pth in paths]
    short = [pth for pth, c in zip(paths, clips) if c.shape[0] < speech_units.MIN_SAMPLES]
    if short:
        raise SystemExit(f"clips under {speech_units.MIN_SAMPLES} samples have no feature frame: " + ", ".join(short))
    units = extract(extractor, clips, a.batch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out_unt)), exist_ok=True)
    with open(a.out_unt, "w") as f:
        for ids in units:
            f.write(" ".join(str(int(v)) for v in ids) + "\n")
    print(f"quantised {len(clips)} clips, {sum(len(u) for u in units)} units -> {a.out_unt}")


if __name__ == "__main__":
    main()
