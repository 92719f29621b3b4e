#!/usr/bin/env python3
"""End-to-end intelligibility CLI - STOI and ESTOI of generated audio against the ground truth, the two numbers the reference
publishes per model (README.md:103-122), computed on the device (intelligibility.STOI, csrc/stoi.hip).

  python -m lip2speech_unit_amd.evaluate <ref_audio_dir> <pred_wav_dir> [--batch_size N] [--output_dir DIR]

Every *.wav below <pred_wav_dir> is paired with the file of the same relative name below <ref_audio_dir> (16 kHz mono s16, read by
audio.read_wav_s16); files without a partner are listed and not scored.  Each pair is truncated to the shorter of the two and that
length is reported.  Pairs are sorted by length and scored in batches of --batch_size, every clip against its own length.
Prints `STOI 0.xxx | ESTOI 0.xxx (n clips)` - the means over the clips that have at least one 30-frame segment; the others (both
scores 1e-5 by the published code's convention) are counted apart - and writes DIR/eval-stoi.json: the means and, per clip, name,
samples, kept frames, segments, stoi, estoi.
"""
import argparse
import json
import os

import numpy as np


def list_wavs(root):
    """Relative names (posix separators, sorted) of the *.wav files below root."""
    out = []
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".wav"):
                out.append(os.path.relpath(os.path.join(d, f), root).replace(os.sep, "/"))
    return sorted(out)


def pair_files(ref_dir, pred_dir):
    """([(name, ref_path, pred_path)], names only below ref_dir, names only below pred_dir)."""
    ref, pred = list_wavs(ref_dir), list_wavs(pred_dir)
    both = sorted(set(ref) & set(pred))
    return ([(n, os.path.join(ref_dir, n), os.path.join(pred_dir, n)) for n in both], sorted(set(ref) - set(pred)),
            sorted(set(pred) - set(ref)))


def evaluate(pairs, read, score, batch_size=16):
    """The protocol on injected parts: `read(path) -> int16 [n]`, `score(clean int16 [B, S], processed int16 [B, S], n_samples) ->
    {"stoi", "estoi", "n_segments", "n_kept": sequences of B}`.  Returns the report dict (clips in the order of `pairs`)."""
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    clips = []
    for name, ref_path, pred_path in pairs:
        x, y = read(ref_path), read(pred_path)
        n = min(len(x), len(y))                                          # both truncated to the shorter
        clips.append({"name": name, "samples": int(n), "_x": x[:n], "_y": y[:n]})
    order = sorted(range(len(clips)), key=lambda i: (clips[i]["samples"], i))
    for b0 in range(0, len(order), batch_size):
        idx = [i for i in order[b0:b0 + batch_size] if clips[i]["samples"] > 0]
        if not idx:
            continue
        ns = [clips[i]["samples"] for i in idx]
        clean = np.zeros((len(idx), max(ns)), dtype=np.int16)
        proc = np.zeros_like(clean)
        for r, i in enumerate(idx):
            clean[r, :ns[r]] = clips[i]["_x"]
            proc[r, :ns[r]] = clips[i]["_y"]
        res = score(clean, proc, ns)
        for r, i in enumerate(idx):
            clips[i].update(kept_frames=int(res["n_kept"][r]), segments=int(res["n_segments"][r]), stoi=float(res["stoi"][r]),
                            estoi=float(res["estoi"][r]))
    for c in clips:
        del c["_x"], c["_y"]
        if "segments" not in c:                                          # an empty pair
            c.update(kept_frames=0, segments=0, stoi=1e-5, estoi=1e-5)
    scored = [c for c in clips if c["segments"] > 0]
    mean = (lambda k: sum(c[k] for c in scored) / len(scored)) if scored else (lambda k: None)
    return {"stoi": mean("stoi"), "estoi": mean("estoi"), "n_clips": len(scored), "n_no_segment": len(clips) - len(scored),
            "batch_size": batch_size, "clips": clips}


def device_score(clean, processed, n_samples, device="cuda"):
    """`score` of evaluate() on the HIP device."""
    import torch

    from .intelligibility import default_stoi
    r = default_stoi().stages(torch.from_numpy(clean).to(device), torch.from_numpy(processed).to(device), n_samples)
    return {k: r[k].tolist() for k in ("stoi", "estoi", "n_segments", "n_kept")}


def summary_line(rep):
    if rep["n_clips"] == 0:
        line = "STOI n/a | ESTOI n/a (0 clips)"
    else:
        line = f"STOI {rep['stoi']:.3f} | ESTOI {rep['estoi']:.3f} ({rep['n_clips']} clips)"
    if rep["n_no_segment"]:
        line += f"; {rep['n_no_segment']} too short for a segment, not averaged"
    return line


def report(pairs, output_dir, batch_size=16, read=None, score=None, unpaired=None):
    """Score, print the summary line, write <output_dir>/eval-stoi.json; returns the report."""
    if read is None:
        from .audio import read_wav_s16 as read
    rep = evaluate(pairs, read, score if score is not None else device_score, batch_size)
    rep["unpaired"] = unpaired if unpaired is not None else {"ref_only": [], "pred_only": []}
    print(summary_line(rep))
    for side, names in rep["unpaired"].items():
        if names:
            print(f"not scored ({side}, no partner): " + " ".join(names))
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "eval-stoi.json"), "w") as f:
        json.dump(rep, f, indent=1)
    return rep


def read_transcripts(path, names):
    """Reference texts of the clips `names` (relative *.wav names): a directory of <name>.txt files, or a tsv of `<name>\\t<text>`
    lines (name with or without .wav).  Returns {name: text} for the names that have one."""
    stem = lambda n: n[:-4] if n.endswith(".wav") else n  # noqa: E731
    out = {}
    if os.path.isdir(path):
        for n in names:
            f = os.path.join(path, stem(n) + ".txt")
            if os.path.exists(f):
                out[n] = open(f, encoding="utf-8").read().strip()
        return out
    table = {}
    for line in open(path, encoding="utf-8"):
        if line.strip():
            k, _, t = line.rstrip("\n").partition("\t")
            table[stem(k.strip())] = t.strip()
    return {n: table[stem(n)] for n in names if stem(n) in table}


def wer_report(items, transcripts, output_dir, transcribe):
    """WER of the predicted clips against reference texts, the fourth number the reference publishes (README.md:103-122; formula
    inference_server.py:364-373): items = [(name, pred_path)], transcribe(paths) -> texts.  Prints `WER xx.xx (n clips)`, writes
    <output_dir>/eval-wer.json (wer, n_err, n_total and per clip name, ref, hyp, errors, words), returns the report."""
    from .asr_text import wer
    refs = read_transcripts(transcripts, [n for n, _ in items])
    scored = [(n, pth) for n, pth in items if n in refs]
    if not scored:
        raise SystemExit(f"no clip has a transcript in {transcripts}")
    hyps = transcribe([pth for _, pth in scored])
    rep = wer([refs[n] for n, _ in scored], hyps)
    for c, (n, _) in zip(rep["clips"], scored):
        c["name"] = n
    rep["no_transcript"] = [n for n, _ in items if n not in refs]
    print("WER n/a (no reference words)" if rep["wer"] is None else f"WER {rep['wer']:.2f} ({len(scored)} clips, {rep['n_err']} / {rep['n_total']})")
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "eval-wer.json"), "w") as f:
        json.dump(rep, f, indent=1)
    return rep


def main(argv=None, read=None, score=None):
    p = argparse.ArgumentParser()
    p.add_argument("ref_audio_dir")
    p.add_argument("pred_wav_dir")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--output_dir", default="generated_files")
    # --wer: also transcribe the predicted clips (whisper.WhisperASR) and score them against --transcripts; absent, nothing changes
    p.add_argument("--wer", action="store_true", default=argparse.SUPPRESS)
    p.add_argument("--transcripts", default=argparse.SUPPRESS, help="directory of <name>.txt files or a tsv of <name>\\t<text>")
    from .transcribe import add_asr_arguments
    add_asr_arguments(p, suppress=True)
    a = p.parse_args(argv)
    if getattr(a, "wer", False) and not getattr(a, "transcripts", None):
        p.error("--wer needs --transcripts (and --whisper, --vocab)")
    if score is None:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("this build runs on MI355X only: no CPU path")
    pairs, ref_only, pred_only = pair_files(a.ref_audio_dir, a.pred_wav_dir)
    if not pairs:
        raise SystemExit(f"no *.wav of {a.pred_wav_dir} has a partner of the same relative name below {a.ref_audio_dir}")
    rep = report(pairs, a.output_dir, a.batch_size, read, score, {"ref_only": ref_only, "pred_only": pred_only})
    if getattr(a, "wer", False):
        from . import transcribe
        from .audio import read_wav_s16
        asr = transcribe.asr_from_args(a)
        wer_report([(n, pred) for n, _, pred in pairs], a.transcripts, a.output_dir,
                   lambda paths: transcribe.transcribe_clips(asr, [read_wav_s16(pth) for pth in paths], getattr(a, "asr_batch_size", 16)))
    return rep


if __name__ == "__main__":
    main()
