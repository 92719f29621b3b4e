#!/usr/bin/env python3
"""Generate tests/golden/vocoder_mel_loss.npz by RUNNING THE REFERENCE's own validation step (multi_input_vocoder/train.py:214-240)
on CPU fp32: its MelCodeDataset (dataset_multi_input.py:144-291, segment_size 8960), its mel_spectrogram
(speech-resynthesis/dataset.py:44-67), its MelCodeGenerator (synthetic weights, seed 13, weight norm removed) and F.l1_loss.

Runs only where a checkout of the reference is at hand (REF below, as in tools/make_golden.py); the fixture is data and travels with
the repo - the reference itself never does.
Inputs: the five datasets/lrs3 test clips in manifest order plus a sixth item, the first 6 400 samples of test/UmvOgW6iV2s/00002
written to a temporary data set (tests/_hifigan_mel_reference.py::materialise_six) - shorter than a segment, so the reference's
doubling branch (:249-252) runs.

Three of the reference's imports are not installed here and are stood in for, in sys.modules, before the reference is imported:
  librosa.filters.mel     the test-side Slaney filterbank (tests/_hifigan_mel_reference.py::slaney_filterbank), float32;
  librosa.util.normalize  division by the peak (what it does to a 1-d signal with its default norm=inf);
  soundfile.read          stdlib `wave` (int16 samples, the file's rate);
  amfm_decompy, torchvision  empty modules (pitch tracking and the blur augmentation are not on the validation path).
Everything else - the padding, torch.stft, the magnitude with its 1e-9, the matmul, log(clamp) and the data set's trimming, doubling
and random.randint segment draw - is the reference's code running under this torch.

Per item i the file holds the clip name, start_step, y_mel [80, 35] (ground-truth segment), y_g_hat_mel [80, 35] (generated
segment) and e_i = F.l1_loss of the two; y_g_hat [8960] of items 0, 1 and 5; val_err = F.l1_loss over the batch of six; the seed.
"""
import json
import os
import sys
import tempfile
import types
import wave

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")

from lip2speech_unit_amd import weights  # noqa: E402
from tests import _hifigan_mel_reference as hr  # noqa: E402

KEEP_WAV = (0, 1, 5)


def install_stand_ins():
    def mel(sr, n_fft, n_mels, fmin, fmax):
        assert (sr, n_fft, n_mels, fmin) == (hr.SR, hr.N_FFT, hr.N_MELS, 0) and fmax in (None, hr.FMAX)
        return hr.slaney_filterbank().astype(np.float32)

    def sf_read(path, dtype="int16"):
        assert dtype == "int16"
        with wave.open(str(path), "rb") as w:
            assert w.getnchannels() == 1 and w.getsampwidth() == 2
            return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").astype(np.int16), w.getframerate()
    mods = {n: types.ModuleType(n) for n in ("librosa", "librosa.filters", "librosa.util", "soundfile", "amfm_decompy", "torchvision")}
    mods["librosa.filters"].mel = mel
    mods["librosa.util"].normalize = lambda a: a / np.abs(a).max()
    mods["librosa"].filters, mods["librosa"].util = mods["librosa.filters"], mods["librosa.util"]
    mods["soundfile"].read = sf_read
    for n, m in mods.items():
        assert n not in sys.modules, f"{n} is installed: use it, not the stand-in"
        sys.modules[n] = m


def main():
    install_stand_ins()
    sys.path.insert(0, f"{REF}/speech-resynthesis")
    sys.path.insert(0, f"{REF}/multi_input_vocoder")
    import dataset_multi_input as dmi
    from dataset import mel_spectrogram
    from models_multi_input import MelCodeGenerator
    from utils import AttrDict
    h = AttrDict(json.load(open(f"{REF}/multi_input_vocoder/configs/lrs3/multi_input.json")))
    h.text_supervision = False
    g = MelCodeGenerator(h).eval()
    g.load_state_dict(weights.synth_state_dict([(k, tuple(v.shape)) for k, v in g.state_dict().items()], seed=13), strict=True)
    g.remove_weight_norm()
    with tempfile.TemporaryDirectory() as tmp:
        lab, names = hr.materialise_six(tmp, OUT)
        for clip in names[:5]:                               # the materialised wavs are the reference's own files
            a, b = (wave.open(p, "rb") for p in (f"{REF}/datasets/lrs3/audio/{clip}.wav", os.path.join(tmp, "audio", clip + ".wav")))
            assert a.readframes(a.getnframes()) == b.readframes(b.getnframes()) and a.getframerate() == b.getframerate()
        files = dmi.parse_manifest(os.path.join(lab, "test.tsv"), h.get("max_keep", None), h.get("min_keep", None))
        ds = dmi.MelCodeDataset(files, h.segment_size, h.code_hop_size, h.mel_hop_size, h.n_fft, h.num_mels, h.hop_size, h.win_size,
                                h.sampling_rate, h.fmin, h.fmax, False, n_cache_reuse=0, fmax_loss=h.fmax_for_loss, device=None,
                                multispkr=h.get("multispkr", None), code_dict_path=os.path.join(lab, "dict.unt.txt"))   # train.py:116-118
        # the draw is inside _sample_interval: record what random.randint hands it (the call itself is untouched)
        import random
        draws, randint = [], random.randint

        def recording_randint(lo, hi):
            draws.append((lo, hi, randint(lo, hi)))
            return draws[-1][2]
        random.randint = recording_randint
        try:
            items = [ds[i] for i in range(len(ds))]
        finally:
            random.randint = randint
        assert len(draws) == len(items) == 6 and all(lo == 0 for lo, _, _ in draws)
        starts = [d[2] for d in draws]
        assert draws[5][1] == 2 * hr.SHORT_SAMPLES // 320 - h.segment_size // 320          # the short item was doubled once
        x = {k: torch.from_numpy(np.stack([np.asarray(it[0][k]) for it in items])) for k in ("code", "mel", "spkr")}
        y_mel = torch.stack([it[3] for it in items])
        with torch.no_grad():
            y_g_hat = g(**x)                                                                     # train.py:222
            y_g_hat_mel = mel_spectrogram(y_g_hat.squeeze(1), h.n_fft, h.num_mels, h.sampling_rate, h.hop_size, h.win_size, h.fmin,
                                          h.fmax_for_loss)                                       # :224-225
            val_err = F.l1_loss(y_mel, y_g_hat_mel).item()                                       # :226, one batch of six
            e = [F.l1_loss(y_mel[i], y_g_hat_mel[i]).item() for i in range(len(items))]
        assert y_mel.shape == y_g_hat_mel.shape == (6, 80, 35) and y_g_hat.shape == (6, 1, 8960)
        # the reference's function against its float32 restatement (torch.stft called directly): the same bits
        for i, it in enumerate(items):
            assert np.array_equal(hr.mel_f32(it[1].numpy()).T, y_mel[i].numpy()), i
        out = {"seed": 13, "dataset_seed": 1234, "segment_size": h.segment_size, "clips": np.array(names),
               "start_step": np.array(starts, np.int32), "e": np.array(e, np.float64), "val_err": np.float64(val_err)}
        for i in range(len(items)):
            out[f"c{i}_y_mel"] = y_mel[i].numpy()
            out[f"c{i}_y_g_hat_mel"] = y_g_hat_mel[i].numpy()
            if i in KEEP_WAV:
                out[f"c{i}_y_g_hat"] = y_g_hat[i, 0].numpy()
            print(names[i], "start_step", starts[i], "e_i", e[i])
        print("val_err", val_err, "mean e_i", float(np.mean(e)))
    path = os.path.join(OUT, "vocoder_mel_loss.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 512 * 1024, os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
