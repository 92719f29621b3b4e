#!/usr/bin/env python3
"""Writes the speaker embedding of every wav of a folder - what create_dataset.py:94,133 stores as spk_emb/<rel>.npy
(helpers.py:185-198, _get_speaker_embedding: a float32 (256,) vector per clip), computed on the device.

  python -m lip2speech_unit_amd.extract_spk_emb <audio_root> <spk_emb_root> --encoder <encoder.pt> [--batch N]
      [--synthetic_weights]
Walks <audio_root>/**/*.wav (16 kHz mono s16), embeds length-sorted batches (speaker_encoder.SpeakerEncoder.embed) and writes
<spk_emb_root>/<rel>.npy.  --encoder is an RTVC encoder checkpoint ({"model_state": ...} or a bare state dict);
--synthetic_weights replaces it by the build-owned weights (speaker_encoder.synthetic_state_dict), like the other CLIs.
"""
import argparse
import glob
import os

import numpy as np
import torch

from . import audio, speaker_encoder


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("audio_root")
    p.add_argument("spk_emb_root")
    p.add_argument("--encoder", default=None)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--synthetic_weights", action="store_true")
    return p


def output_path(spk_emb_root, audio_root, wav_path):
    """<spk_emb_root>/<path of the wav under audio_root, .wav -> .npy>"""
    return os.path.join(spk_emb_root, os.path.relpath(wav_path, audio_root))[:-4] + ".npy"


def load_encoder(a):
    enc = speaker_encoder.SpeakerEncoder()
    if a.synthetic_weights:
        enc.load_state_dict(speaker_encoder.synthetic_state_dict())
    else:
        enc.load_checkpoint(a.encoder)
    return enc.eval()


def extract(enc, clips, batch=64):
    """clips: a list of int16 arrays.  Returns float32 [len(clips), 256] in the same order (length-sorted batches)."""
    order = sorted(range(len(clips)), key=lambda i: clips[i].shape[0])
    out = np.zeros((len(clips), speaker_encoder.EMBED), np.float32)
    for i in range(0, len(order), max(batch, 1)):
        group = order[i:i + max(batch, 1)]
        lens = [clips[j].shape[0] for j in group]
        pcm = np.zeros((len(group), max(lens)), np.int16)
        for r, j in enumerate(group):
            pcm[r, : lens[r]] = clips[j]
        emb = enc.embed(torch.from_numpy(pcm).cuda(), lens)
        out[group] = np.asarray(emb.cpu(), dtype=np.float32)
    return out


def main(argv=None, embed=None):
    """embed (tests): a callable list of int16 clips -> float32 [N, 256] used instead of the encoder on the device."""
    p = build_parser()
    a = p.parse_args(argv)
    if a.batch < 1:
        p.error("--batch must be at least 1")
    if not a.synthetic_weights and not a.encoder:
        p.error("--encoder <encoder.pt> is needed (or --synthetic_weights)")
    if a.encoder and not a.synthetic_weights and not os.path.isfile(a.encoder):
        p.error(f"{a.encoder}: no such file")
    if not os.path.isdir(a.audio_root):
        p.error(f"{a.audio_root}: no such directory")
    if embed is None:
        if not torch.cuda.is_available():
            raise SystemExit("this build runs on MI355X only: no CPU path")
        enc = load_encoder(a)
        embed = lambda clips: extract(enc, clips, a.batch)   # noqa: E731
    paths = sorted(glob.glob(os.path.join(a.audio_root, "**", "*.wav"), recursive=True))
    clips = [audio.read_wav_s16(pth, speaker_encoder.SAMPLING_RATE) for pth in paths]   # another rate is refused: no resampler
    empty = [pth for pth, c in zip(paths, clips) if c.shape[0] < 1]
    if empty:
        raise SystemExit("clips without samples: " + ", ".join(empty))
    emb = np.asarray(embed(clips))
    for pth, v in zip(paths, emb):
        out = output_path(a.spk_emb_root, a.audio_root, pth)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        assert v.shape == (speaker_encoder.EMBED,) and v.dtype == np.float32
        np.save(out, v)
    print(f"embedded {len(clips)} clips -> {a.spk_emb_root}")
    return [output_path(a.spk_emb_root, a.audio_root, pth) for pth in paths]


if __name__ == "__main__":
    main()
