#!/usr/bin/env python3
"""Writes tests/golden/mel_lrs3*.npz: the reference's own (audio/*.wav, mel/*.npy) pairs for the five clips of
tests/golden/lrs3_sample/test.tsv.  Copies data only - the PCM int16 of each wav, the mel its create_dataset.py stored
(float32 [T, 80]) and the clip's speaker embedding (so that a test can lay a whole data set out) - and runs no reference code.

  python tools/make_mel_golden.py <reference>/datasets/lrs3
Audio and mel go to two files when one would exceed the largest fixture already committed.
"""
import os
import sys
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden")
LIMIT = 688 * 1024


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    root = sys.argv[1]
    rows = open(os.path.join(GOLDEN, "lrs3_sample", "test.tsv")).read().splitlines()[1:]
    clips = [r.split("\t")[0] for r in rows]
    audio, mel = {"clips": np.array(clips)}, {"clips": np.array(clips)}
    for i, (clip, row) in enumerate(zip(clips, rows)):
        with wave.open(os.path.join(root, "audio", clip + ".wav"), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000), clip
            pcm = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16)
        assert pcm.shape[0] == int(row.split("\t")[-1]), clip
        m = np.load(os.path.join(root, "mel", clip + ".npy"))
        assert m.dtype == np.float32 and m.shape == (1 + pcm.shape[0] // 160, 80), (clip, m.shape)
        audio[f"c{i}_pcm"] = pcm
        mel[f"c{i}_mel"] = m
        mel[f"c{i}_spk"] = np.load(os.path.join(root, "spk_emb", clip + ".npy")).astype(np.float32)
    one = os.path.join(GOLDEN, "mel_lrs3.npz")
    np.savez_compressed(one, **audio, **{k: v for k, v in mel.items() if k != "clips"})
    if os.path.getsize(one) > LIMIT:
        os.remove(one)
        np.savez_compressed(os.path.join(GOLDEN, "mel_lrs3_audio.npz"), **audio)
        np.savez_compressed(os.path.join(GOLDEN, "mel_lrs3.npz"), **mel)
    for fn in ("mel_lrs3.npz", "mel_lrs3_audio.npz"):
        pth = os.path.join(GOLDEN, fn)
        if os.path.exists(pth):
            print(fn, os.path.getsize(pth), "bytes")
            assert os.path.getsize(pth) <= LIMIT, fn


if __name__ == "__main__":
    main()
