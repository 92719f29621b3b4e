#!/usr/bin/env python3
"""Clips per second of on-device STOI / ESTOI scoring (intelligibility.STOI) at a batch of 4-second clips, against the float64
restatement (tests/_stoi_reference.py) on the CPU.  No threshold: the figure is recorded in DESIGN.md section 17.

  python tools/stoi_bench.py [--batch 16] [--seconds 4] [--iters 50] [--cpu_clips 4]

The clips are the committed LRS3 fixture clips tiled / cut to length, the processed side is the clean one plus white noise at
5 dB.  Device time is taken with events around `iters` whole scores() calls (upload excluded) after a warm-up; the CPU time is the
restatement's on `cpu_clips` of the same pairs.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _stoi_reference as R  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--seconds", type=float, default=4.0)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--cpu_clips", type=int, default=4)
    a = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("stoi_bench measures the MI355X path: no GPU, no figure")
    from lip2speech_unit_amd.intelligibility import STOI
    g = np.load(os.path.join(ROOT, "tests", "golden", "mel_lrs3_audio.npz"))
    n = int(a.seconds * 16000)
    xs, ys = [], []
    for b in range(a.batch):
        pcm = g[f"c{b % 5}_pcm"]
        x = np.tile(pcm, (n + b * 160) // len(pcm) + 1)[b * 160:b * 160 + n].astype(np.float64) / 32768.0
        xs.append(x)
        ys.append(R.add_noise(x, 5, seed=b))
    st = STOI()
    X, Y = (torch.from_numpy(np.stack(v).astype(np.float32)).cuda() for v in (xs, ys))
    for _ in range(3):
        out = st.scores(X, Y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = st.scores(X, Y)
    e1.record()
    torch.cuda.synchronize()
    dev_s = e0.elapsed_time(e1) / 1e3 / a.iters
    t0 = time.perf_counter()
    ref = [R.stages(xs[b].astype(np.float32).astype(np.float64), ys[b].astype(np.float32).astype(np.float64)) for b in range(a.cpu_clips)]
    cpu_s = (time.perf_counter() - t0) / max(a.cpu_clips, 1)
    err = max(max(abs(float(out["stoi"][b]) - r["stoi"]), abs(float(out["estoi"][b]) - r["estoi"])) for b, r in enumerate(ref)) if ref else None
    print(json.dumps({"batch": a.batch, "seconds_per_clip": a.seconds, "device_ms_per_batch": round(dev_s * 1e3, 4),
                      "device_clips_per_s": round(a.batch / dev_s, 1), "cpu_fp64_clips_per_s": round(1.0 / cpu_s, 2) if ref else None,
                      "speedup": round(a.batch / dev_s * cpu_s, 1) if ref else None, "max_score_err_vs_fp64": err}))


if __name__ == "__main__":
    main()
