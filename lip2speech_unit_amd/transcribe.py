#!/usr/bin/env python3
"""Speech recognition CLI - what the reference's server does with every clip it synthesises (`server.py:337-342`,
`asr.run(pred_audio_path)` with Whisper base.en), on the device (whisper.WhisperASR).

  python -m lip2speech_unit_amd.transcribe <wav_dir> --whisper <ckpt> --vocab <file> [--output_dir D] [--batch_size N]
      [--language en] [--decode_config generation_config.json] [--max_new_tokens 224] [--dtype f16|bf16]

<ckpt>: openai-whisper's `.pt` file (or a HuggingFace state dict saved with torch.save); <file>: its `.tiktoken` vocabulary or a
HuggingFace `vocab.json`.  The decoding ids follow from the vocabulary size (English-only or multilingual with --language) unless
--decode_config names a HuggingFace generation_config.json.  Every *.wav below <wav_dir> (16 kHz mono s16, at most 30 s) is
transcribed; D/pred_asr/<relative name>.txt holds the text, and the texts are printed as `<name>\t<text>`.
"""
import argparse
import os

import numpy as np

DTYPES = ("f16", "bf16")


def add_asr_arguments(p, suppress=False):
    """The recogniser's options; suppress: absent options leave no trace in the namespace (for CLIs that gained them later)."""
    d = (lambda v: argparse.SUPPRESS) if suppress else (lambda v: v)
    p.add_argument("--whisper", default=d(None), help="openai-whisper .pt checkpoint (or a HuggingFace state dict)")
    p.add_argument("--vocab", default=d(None), help=".tiktoken vocabulary or HuggingFace vocab.json")
    p.add_argument("--language", default=d("en"))
    p.add_argument("--decode_config", default=d(None), help="HuggingFace generation_config.json (default: ids from the vocabulary size)")
    p.add_argument("--max_new_tokens", type=int, default=d(224))
    p.add_argument("--asr_batch_size", type=int, default=d(16))
    p.add_argument("--asr_dtype", default=d("f16"), choices=DTYPES)


def build_asr(whisper, vocab, language="en", decode_config=None, max_new_tokens=224, dtype="f16"):
    from . import ops
    from .asr_text import Detokenizer, WhisperDecodeConfig
    from .whisper import WhisperASR, load_whisper
    model = load_whisper(whisper, dtype=ops.BF16 if dtype == "bf16" else ops.F16).cuda()
    V = model.dims.n_vocab
    if decode_config:
        cfg = WhisperDecodeConfig.from_generation_config(decode_config, max_new_tokens=max_new_tokens)
    elif V == 51864:
        cfg = WhisperDecodeConfig.english(max_new_tokens=max_new_tokens)
    else:
        cfg = WhisperDecodeConfig.multilingual(language, n_vocab=V, max_new_tokens=max_new_tokens)
    return WhisperASR(model, cfg, vocab=Detokenizer.load(vocab, special_start=cfg.special_start))


def asr_from_args(a):
    g = lambda k, v: getattr(a, k, v)  # noqa: E731
    if not g("whisper", None) or not g("vocab", None):
        raise SystemExit("the recogniser needs --whisper <ckpt> and --vocab <file>")
    return build_asr(a.whisper, a.vocab, g("language", "en"), g("decode_config", None), g("max_new_tokens", 224), g("asr_dtype", "f16"))


def transcribe_clips(asr, clips, batch_size=16):
    """clips: int16 arrays (16 kHz) -> texts, in batches of clips sorted by length."""
    import torch
    from .whisper import N_SAMPLES
    for c in clips:
        if len(c) > N_SAMPLES:
            raise ValueError(f"a clip of {len(c)} samples is longer than one 30-s window ({N_SAMPLES})")
    out = [None] * len(clips)
    order = sorted(range(len(clips)), key=lambda i: (len(clips[i]), i))
    for b0 in range(0, len(order), batch_size):
        idx = order[b0:b0 + batch_size]
        ns = [len(clips[i]) for i in idx]
        buf = np.zeros((len(idx), max(max(ns), 1)), dtype=np.int16)
        for r, i in enumerate(idx):
            buf[r, :ns[r]] = clips[i]
        for i, t in zip(idx, asr.run(torch.from_numpy(buf).cuda(), ns)):
            out[i] = t
    return out


def write_transcripts(names, texts, output_dir):
    for n, t in zip(names, texts):
        path = os.path.join(output_dir, "pred_asr", (n[:-4] if n.endswith(".wav") else n) + ".txt")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w", encoding="utf-8") as f:
            f.write(t + "\n")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("wav_dir")
    p.add_argument("--output_dir", default="generated_files")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--dtype", default="f16", choices=DTYPES)
    add_asr_arguments(p)
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    from .audio import read_wav_s16
    from .evaluate import list_wavs
    names = list_wavs(a.wav_dir)
    if not names:
        raise SystemExit(f"no *.wav below {a.wav_dir}")
    a.asr_dtype = a.dtype
    asr = asr_from_args(a)
    texts = transcribe_clips(asr, [read_wav_s16(os.path.join(a.wav_dir, n)) for n in names], a.batch_size)
    write_transcripts(names, texts, a.output_dir)
    for n, t in zip(names, texts):
        print(f"{n}\t{t}")
    return dict(zip(names, texts))


if __name__ == "__main__":
    main()
