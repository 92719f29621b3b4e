#!/usr/bin/env python3
"""Stage-2 CLI — mirrors multi_input_vocoder/inference.py:167-259 (argparse surface :170-180, worker :85-165).

  python -m lip2speech_unit_amd.vocoder_inference <config.json> <label/test.tsv> <dict.unt.txt> \
      --output_dir D --checkpoint_file C -n -1 [--pad N] [--synthetic_weights] [--mel_from_audio]
      [--units_from_audio --hubert <ckpt> --kmeans <km.bin|centers.npy> [--units_layer 6] [--units_dtype f32|f16|bf16]] [--stoi]
      [--spk_emb_from_audio --speaker_encoder <encoder.pt>]
--mel_from_audio: the mel conditioning is analysed from audio/*.wav on the device (audio.TacotronSTFT); mel/ is not read.
--units_from_audio: the units are computed from audio/*.wav on the device (speech_units.SpeechUnitExtractor); the .unt file is
not read.  With both flags stage 2 runs from a folder of wavs and speaker embeddings alone.
--spk_emb_from_audio (off by default): the speaker embedding is computed from audio/*.wav on the device
(speaker_encoder.SpeakerEncoder; with --synthetic_weights its build-owned weights); spk_emb/ is not read.  With all three flags
stage 2 runs from a folder of wavs alone.
Writes D/pred_wav/<spk>/<utt>.wav (int16, 16 kHz) like :157-165.
--stoi (off by default): the clips just written are scored against the manifest's audio on the device (evaluate.report: STOI and
ESTOI, the summary line and D/eval-stoi.json).
"""
import argparse
import json
import os
import time

import numpy as np
import torch
from scipy.io.wavfile import write

from . import weights
from .data import MelCodeDataset, parse_manifest
from .vocoder import AttrDict, MelCodeGenerator


def manifest_from_audio(manifest_path, extractor, batch=16):
    """parse_manifest's (audio_files, mel_files, codes) with the codes computed from the wavs instead of read from <manifest>.unt."""
    from . import audio
    from .extract_units import extract
    with open(manifest_path) as f:
        root = f.readline().strip()
        audio_files = [os.path.join(root, line.strip().split("\t")[2]) for line in f if line.strip()]
    units = extract(extractor, [audio.read_wav_s16(pth) for pth in audio_files], batch)
    mels = [pth.replace("/audio/", "/mel/")[:-4] + ".npy" for pth in audio_files]
    return audio_files, mels, [" ".join(str(int(v)) for v in ids) for ids in units]


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("config_file")
    p.add_argument("input_code_file")
    p.add_argument("code_dict_path")
    p.add_argument("--code_file", default=None)
    p.add_argument("--output_dir", default="generated_files")
    p.add_argument("--checkpoint_file", required=False, default=None)
    p.add_argument("--pad", default=None, type=int)
    p.add_argument("--debug", action="store_true")
    p.add_argument("-n", type=int, default=10)
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    p.add_argument("--mel_from_audio", action="store_true")
    p.add_argument("--units_from_audio", action="store_true")
    p.add_argument("--hubert", default=None)
    p.add_argument("--kmeans", default=None)
    p.add_argument("--units_layer", type=int, default=6)
    p.add_argument("--units_dtype", default="f32", choices=["f32", "f16", "bf16"])
    p.add_argument("--stoi", action="store_true", default=argparse.SUPPRESS)   # absent: the namespace is what it was without the flag
    p.add_argument("--spk_emb_from_audio", action="store_true", default=argparse.SUPPRESS)   # absent likewise, and so is the next
    p.add_argument("--speaker_encoder", default=argparse.SUPPRESS)
    p.add_argument("--asr", action="store_true", default=argparse.SUPPRESS)    # absent likewise, and so are the recogniser's options
    from .transcribe import add_asr_arguments
    add_asr_arguments(p, suppress=True)
    return p


def main(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    if a.units_from_audio and not (a.hubert and a.kmeans):
        p.error("--units_from_audio needs --hubert and --kmeans")
    spk_from_audio = getattr(a, "spk_emb_from_audio", False)
    if spk_from_audio and not (a.synthetic_weights or getattr(a, "speaker_encoder", None)):
        p.error("--spk_emb_from_audio needs --speaker_encoder (or --synthetic_weights)")
    if a.code_file is not None:
        raise NotImplementedError("--code_file (units without mel/speaker) is not the multi-input path")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    from . import ops
    h = AttrDict(json.load(open(a.config_file)))
    h.code_dict_path = a.code_dict_path
    h.text_supervision = bool(int(os.environ.get("TEXT_SUPERVISION", 0)))
    gen = MelCodeGenerator(h, dtype=ops.BF16 if a.dtype == "bf16" else ops.F16)
    if a.synthetic_weights:
        gen.load_state_dict(weights.synth_state_dict(weights.spec_of(gen), seed=1))
    else:
        gen.load_state_dict(torch.load(a.checkpoint_file, map_location="cpu")["generator"])   # :119-120
    gen.cuda().eval()
    gen.remove_weight_norm()                                                                   # :142-143
    if a.units_from_audio:
        from . import speech_units
        from .extract_units import DTYPES
        udt = DTYPES[a.units_dtype]
        extractor = speech_units.SpeechUnitExtractor(speech_units.load_hubert(a.hubert, dtype=udt), speech_units.load_kmeans(a.kmeans),
                                                     layer=a.units_layer, dtype=udt)
        file_list = manifest_from_audio(a.input_code_file, extractor)
    else:
        file_list = parse_manifest(a.input_code_file)
    ds_kw = {}
    if spk_from_audio:
        from . import speaker_encoder
        enc = speaker_encoder.SpeakerEncoder()
        if a.synthetic_weights:
            enc.load_state_dict(speaker_encoder.synthetic_state_dict())
        else:
            enc.load_checkpoint(a.speaker_encoder)
        ds_kw["spk_embedder"] = enc.eval().embed_file
    ds = MelCodeDataset(file_list, h.code_hop_size, h.mel_hop_size, code_dict_path=a.code_dict_path,
                        pad=a.pad, mel_from_audio=a.mel_from_audio, **ds_kw)
    os.makedirs(a.output_dir, exist_ok=True)
    n = len(ds) if a.n == -1 else min(a.n, len(ds))
    audio_s, wall = 0.0, 0.0
    written = []
    for i in range(n):
        feats, _, filename, _ = ds[i]
        code = {k: torch.from_numpy(v).cuda().unsqueeze(0) for k, v in feats.items()}        # :155
        t0 = time.perf_counter()
        with torch.no_grad():
            _, pcm = gen.forward_rows(code["code"], code["mel"], code["spkr"], t_label=code.get("t_label"))
        audio = pcm[0].cpu().numpy()                                                          # :79-81
        wall += time.perf_counter() - t0
        audio_s += audio.shape[0] / h.sampling_rate
        out = os.path.join(a.output_dir, os.path.join("pred_wav", *(filename.split("/")[-2:]))[:-4] + ".wav")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        write(out, h.sampling_rate, audio.astype(np.int16))
        written.append(("/".join(filename.split("/")[-2:])[:-4], filename, out))
    print(f"synthesised {n} clips, {audio_s:.1f} s of audio in {wall:.2f} s (RTF {audio_s / max(wall, 1e-9):.1f}x)")
    if getattr(a, "stoi", False):
        from . import evaluate
        evaluate.report(written, a.output_dir)
    if getattr(a, "asr", False):
        from . import audio, transcribe
        asr = transcribe.asr_from_args(a)
        texts = transcribe.transcribe_clips(asr, [audio.read_wav_s16(out) for _, _, out in written], getattr(a, "asr_batch_size", 16))
        transcribe.write_transcripts([name for name, _, _ in written], texts, a.output_dir)
        for (name, _, _), t in zip(written, texts):
            print(f"{name}\t{t}")


if __name__ == "__main__":
    main()
