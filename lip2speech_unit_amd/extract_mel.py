#!/usr/bin/env python3
"""Writes the vocoder's mel conditioning for a folder of wavs - what create_dataset.py:221-224 stores as mel/<rel>.npy
(extract_mel_spec, :62-75), analysed on the device.

  python -m lip2speech_unit_amd.extract_mel <audio_root> <mel_root> [--batch N]
Walks <audio_root>/**/*.wav (16 kHz mono s16), analyses length-sorted batches in one launch each and writes
<mel_root>/<rel>.npy as float32 [T, 80], T = 1 + samples // 160.
"""
import argparse
import glob
import os

import numpy as np
import torch

from . import audio


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("audio_root")
    p.add_argument("mel_root")
    p.add_argument("--batch", type=int, default=64)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    stft = audio.default_stft()
    paths = sorted(glob.glob(os.path.join(a.audio_root, "**", "*.wav"), recursive=True))
    clips = [(pth, audio.read_wav_s16(pth, stft.sr)) for pth in paths]
    clips.sort(key=lambda c: c[1].shape[0])
    frames = 0
    for i in range(0, len(clips), max(a.batch, 1)):
        group = clips[i:i + max(a.batch, 1)]
        lens = [c[1].shape[0] for c in group]
        pcm = np.zeros((len(group), max(lens)), np.int16)
        for r, (_, x) in enumerate(group):
            pcm[r, : x.shape[0]] = x
        mel = stft.mel_rows(torch.from_numpy(pcm).cuda(), lens).cpu().numpy()
        for r, (pth, x) in enumerate(group):
            out = os.path.join(a.mel_root, os.path.relpath(pth, a.audio_root))[:-4] + ".npy"
            os.makedirs(os.path.dirname(out), exist_ok=True)
            T = audio.num_frames(x.shape[0], stft.hop)
            np.save(out, np.ascontiguousarray(mel[r, :T]))
            frames += T
    print(f"analysed {len(clips)} clips, {frames} frames -> {a.mel_root}")


if __name__ == "__main__":
    main()
