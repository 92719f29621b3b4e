#!/usr/bin/env python3
"""Milliseconds of the on-device speaker embedding (speaker_encoder.SpeakerEncoder.embed) at the bench's operating point, 640
four-second clips = 2560 partial windows of 160 steps, split by launch: gain, power mel, the three input projections, the three
recurrences, the head.  No threshold: the figures are recorded in DESIGN.md section 18.

  python tools/spk_emb_bench.py [--clips 640] [--seconds 4] [--iters 5]

Every launch is timed with HIP events on its own stream position (ops.KernelProfiler); the per-launch figure is the median over
`iters` whole embed() calls after one warm-up call, the whole-path figure is timed without the profiler.  The recurrence's rate is
stated against the fp32 matrix-instruction peak of the MI355X (157.3 TFLOP/s).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
STAGES = ("gain", "mel", "proj0", "rec0", "proj1", "rec1", "proj2", "rec2", "head")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--clips", type=int, default=640)
    p.add_argument("--seconds", type=float, default=4.0)
    p.add_argument("--iters", type=int, default=5)
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spk_emb_bench measures the MI355X path: no GPU, no figure")
    from lip2speech_unit_amd import ops
    from lip2speech_unit_amd import speaker_encoder as se
    g = np.load(os.path.join(ROOT, "tests", "golden", "mel_lrs3_audio.npz"))
    n = int(a.seconds * 16000)
    pcm = np.stack([np.tile(g[f"c{b % 5}_pcm"], (n + b * 160) // len(g[f"c{b % 5}_pcm"]) + 1)[b * 160:b * 160 + n] for b in range(a.clips)])
    wav = torch.from_numpy(pcm).cuda()
    lens = [n] * a.clips
    windows = a.clips * len(se.compute_partial_slices(n)[0])
    enc = se.SpeakerEncoder()
    enc.load_state_dict(se.synthetic_state_dict())
    enc.eval()
    out = enc.embed(wav, lens, max_seqs=windows)            # warm-up: packs the weights, uploads the tables
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = enc.embed(wav, lens, max_seqs=windows)
    e1.record()
    torch.cuda.synchronize()
    whole_ms = e0.elapsed_time(e1) / a.iters
    per_stage = {s: [] for s in STAGES}
    for _ in range(a.iters):
        prof = ops.KernelProfiler()
        ops.set_profiler(prof)
        try:
            enc.embed(wav, lens, max_seqs=windows)
            torch.cuda.synchronize()
        finally:
            ops.set_profiler(None)
        assert len(prof.records) == len(STAGES), [r[0] for r in prof.records]
        for s, (_, _, _, r0, r1, _) in zip(STAGES, prof.records):
            per_stage[s].append(r0.elapsed_time(r1))
    ms = {s: round(statistics.median(v), 4) for s, v in per_stage.items()}
    rec_flops = 2.0 * windows * se.PARTIAL_FRAMES * se.HIDDEN * 4 * se.HIDDEN
    rec_ms = [ms["rec0"], ms["rec1"], ms["rec2"]]
    norms = out.double().norm(dim=1)
    print(json.dumps({"clips": a.clips, "seconds_per_clip": a.seconds, "windows": windows, "whole_path_ms": round(whole_ms, 3),
                      "clips_per_s": round(a.clips / whole_ms * 1e3, 1), "stage_ms": ms,
                      "recurrence_tflops": [round(rec_flops / (t * 1e-3) / 1e12, 2) for t in rec_ms],
                      "recurrence_fraction_of_f32_mfma_peak": [round(rec_flops / (t * 1e-3) / PEAK_F32_MFMA, 4) for t in rec_ms], "max_abs_norm_minus_1": float((norms - 1.0).abs().max())}))


if __name__ == "__main__":
    main()
