#!/usr/bin/env python3
"""Stage-2 validation CLI - the number the reference picks vocoder checkpoints by, `validation/mel_spec_error`
(multi_input_vocoder/train.py:214-240): generate audio for a validation segment, analyse it and the ground-truth segment with the
HiFi-GAN mel_spectrogram (speech-resynthesis/dataset.py:44-67) and take F.l1_loss of the two log-mels.

  python -m lip2speech_unit_amd.vocoder_validate <config.json> <label/valid.tsv> <dict.unt.txt> --checkpoint_file <g_...>
      [--segment_size N] [--batch_size N] [--seed 1234] [--drop_last] [--dtype f16|bf16] [--precise] [--synthetic_weights
      [--synthetic_seed 1]] [--output_dir DIR]

Per batch, all on the device: the generator's float waveform (not its PCM) and the ground-truth segment go through
audio.MelSpectrogram; the per-clip sums sum |y_mel - y_g_hat_mel| come from l2s_mel_l1_sc (deterministic, fp64 carries) with
lens = the clips' frame counts, len_mul = 1 and a crop_len that never truncates; e_i = l1_i / (80 T_i).  The reported val_err is
the mean of e_i over the clips in manifest order.  With equal-length segments that is the reference's mean of per-batch
F.l1_loss whenever the clip count is a multiple of the batch size; --drop_last drops the tail as train.py:120 does (and is an
error when no clip is left, where the reference would meet an unbound `j`).  --segment_size defaults to the config's; -1 takes
whole clips: the batch is zero-padded, every clip is analysed against its own length and averaged over its own cells.
Prints `validation/mel_spec_error <val_err>` and writes DIR/valid-mel.json: val_err and, per clip, name, start (code frames),
frames and e.
"""
import argparse
import json
import os

import numpy as np
import torch

from . import weights
from .data import MelCodeDataset, parse_manifest
from .vocoder import AttrDict, MelCodeGenerator


def clip_name(filename):
    return filename.split("/audio/")[-1][:-4]


def validate(ds, generate, analysis, clip_l1, batch_size, drop_last=False, device="cuda", on_batch=None):
    """The protocol on injected parts: `generate(code, mel, spkr, lens, t_label) -> wav [B, S]`, `analysis` with mel_rows and
    num_frames, `clip_l1(pred, targ, frames) -> [B]` per-clip sums of |pred - targ| over each clip's first frames[b] rows.
    `on_batch(first_index, y_g_hat, n_samples_per_clip)` sees every generated batch (tools and tests).  Returns the report dict."""
    n = len(ds)
    if drop_last:
        n -= n % batch_size
    if n <= 0:
        raise ValueError(f"--drop_last with {len(ds)} clips and batch size {batch_size} leaves no clip to validate")
    clips = []
    for b0 in range(0, n, batch_size):
        items = [ds[i] for i in range(b0, min(b0 + batch_size, n))]                # index order: one segment draw each
        B = len(items)
        L = [it[0]["code"].shape[0] for it in items]
        ns = [it[1].shape[0] for it in items]
        Lm, S = max(L), max(ns)
        code = torch.zeros(B, Lm, dtype=torch.int64)
        mel = torch.zeros(B, items[0][0]["mel"].shape[0], 2 * Lm)
        wav = torch.zeros(B, S)
        t_label = torch.zeros(B, Lm, dtype=torch.int64) if "t_label" in items[0][0] else None
        for i, (f, a, _, _) in enumerate(items):
            assert f["mel"].shape[1] == 2 * L[i] and ns[i] == L[i] * ds.code_hop_size, (f["mel"].shape, L[i], ns[i])
            code[i, : L[i]] = torch.from_numpy(f["code"])
            mel[i, :, : 2 * L[i]] = torch.from_numpy(f["mel"])
            wav[i, : ns[i]] = torch.from_numpy(a)
            if t_label is not None:
                t_label[i, : L[i]] = torch.from_numpy(f["t_label"])
        spkr = torch.from_numpy(np.stack([it[0]["spkr"] for it in items]))
        ragged = min(ns) != S
        lens = torch.tensor(L, dtype=torch.int32).to(device)
        y_g_hat = generate(code.to(device), mel.to(device), spkr.to(device), lens if ragged else None,
                           None if t_label is None else t_label.to(device))        # train.py:222
        assert y_g_hat.shape == (B, S), f"Mismatch in vocoder output shape - {tuple(y_g_hat.shape)} != {(B, S)}"   # :149
        if on_batch is not None:
            on_batch(b0, y_g_hat, ns)
        n_samples = ns if ragged else None
        y_g_hat_mel = analysis.mel_rows(y_g_hat, n_samples)                         # :224-225
        y_mel = analysis.mel_rows(wav.to(device), n_samples)                        # dataset_multi_input.py:275
        frames = [analysis.num_frames(v) for v in ns]
        l1 = clip_l1(y_g_hat_mel, y_mel, frames)
        for i, (it, T) in enumerate(zip(items, frames)):
            clips.append({"name": clip_name(it[2]), "start": int(ds.starts.get(b0 + i, 0)), "frames": int(T),
                          "e": float(l1[i]) / (y_mel.shape[2] * T)})               # :226 F.l1_loss = the mean over the clip's cells
    return {"val_err": sum(c["e"] for c in clips) / len(clips), "n_clips": len(clips), "batch_size": batch_size,
            "segment_size": ds.segment_size, "clips": clips}


def device_clip_l1(pred, targ, frames):
    """Per-clip sum |pred - targ| over rows t < frames[b] of two dense fp32 [B, T, 80] device tensors: l2s_mel_l1_sc."""
    from . import ops
    B, T, nm = pred.shape
    dev = pred.device
    l1, sq, tsq = (torch.empty(B, device=dev, dtype=torch.float32) for _ in range(3))
    rows = torch.empty(B, device=dev, dtype=torch.int32)
    lens = torch.tensor(frames, dtype=torch.int32).to(dev)
    ops.mel_l1_sc(pred.contiguous(), targ.contiguous(), l1, sq, tsq, rows, B=B, Tm_pred=T, Tm_targ=T, crop_len=max(T, max(frames)),
                  lens=lens, len_mul=1, n_mels=nm)
    assert rows.tolist() == [int(f) for f in frames]
    return l1.tolist()


def main(argv=None, on_batch=None):
    p = argparse.ArgumentParser()
    p.add_argument("config_file")
    p.add_argument("input_code_file")
    p.add_argument("code_dict_path")
    p.add_argument("--checkpoint_file", required=False, default=None)
    p.add_argument("--segment_size", type=int, default=None)
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--drop_last", action="store_true")
    p.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    p.add_argument("--precise", action="store_true")
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--synthetic_seed", type=int, default=1)
    p.add_argument("--output_dir", default="generated_files")
    a = p.parse_args(argv)
    if not a.synthetic_weights and a.checkpoint_file is None:
        p.error("--checkpoint_file is required (or --synthetic_weights)")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    from . import audio, ops
    h = AttrDict(json.load(open(a.config_file)))
    h.code_dict_path = a.code_dict_path
    h.text_supervision = bool(int(os.environ.get("TEXT_SUPERVISION", 0)))
    gen = MelCodeGenerator(h, dtype=ops.BF16 if a.dtype == "bf16" else ops.F16)
    if a.synthetic_weights:
        gen.load_state_dict(weights.synth_state_dict(weights.spec_of(gen), seed=a.synthetic_seed))
    else:
        gen.load_state_dict(torch.load(a.checkpoint_file, map_location="cpu")["generator"])
    gen.cuda().eval()
    gen.remove_weight_norm()
    sr = h.get("sampling_rate", 16000)
    analysis = audio.MelSpectrogram(h.get("n_fft", 1024), h.get("num_mels", 80), sr, h.get("hop_size", 256), h.get("win_size", 1024),
                                    h.get("fmin", 0), h.get("fmax_for_loss", None))
    segment = a.segment_size if a.segment_size is not None else h.get("segment_size", 8960)
    ds = MelCodeDataset(parse_manifest(a.input_code_file, h.get("max_keep", None), h.get("min_keep", None)), h.code_hop_size,
                        h.mel_hop_size, code_dict_path=a.code_dict_path, segment_size=segment, seed=a.seed, sampling_rate=sr)
    forward = gen.forward_rows_precise if a.precise else gen.forward_rows

    def generate(code, mel, spkr, lens, t_label):
        with torch.no_grad():
            return forward(code, mel, spkr, lens=lens, t_label=t_label)[0]
    rep = validate(ds, generate, analysis, device_clip_l1, a.batch_size if a.batch_size is not None else h.get("batch_size", 16),
                   a.drop_last, on_batch=on_batch)
    rep.update(seed=a.seed, dtype="precise" if a.precise else a.dtype)
    print(f"validation/mel_spec_error {rep['val_err']:.6f}  ({rep['n_clips']} clips)")
    os.makedirs(a.output_dir, exist_ok=True)
    with open(os.path.join(a.output_dir, "valid-mel.json"), "w") as f:
        json.dump(rep, f, indent=1)
    return rep


if __name__ == "__main__":
    main()
