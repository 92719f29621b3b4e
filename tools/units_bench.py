"""Throughput of the speech-unit path (speech_units.SpeechUnitExtractor), for DESIGN.md section 14:

  * clips per second of `units()` on a batch of 4-second clips, f32 (the default, what labels are made with) and f16;
  * per-kernel time of one such forward (ops.KernelProfiler: HIP events around every launch), with the algorithmic bytes and
    FLOPs kept beside each launcher in ops.py.

  python tools/units_bench.py [--steps 10] [--batch 64] [--samples 64000] [--layers 6]

Seeded weights and audio (no checkpoint is needed to time the path).  Each clips/s figure is the median of `steps` timed runs
between HIP events after 3 warm-up runs, with the min - max spread; the per-kernel table is a separate, single profiled run."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.f32_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=64000)
    ap.add_argument("--layers", type=int, default=6)
    a = ap.parse_args()
    from lip2speech_unit_amd import ops, speech_units, weights
    g = torch.Generator().manual_seed(0)
    pcm = torch.randint(-20000, 20000, (a.batch, a.samples), generator=g, dtype=torch.int16).cuda()
    ns = [a.samples] * a.batch
    centers = np.random.default_rng(0).standard_normal((200, 768)).astype(np.float32)
    frames = speech_units.num_frames(a.samples)
    for name, dt in (("f32", ops.F32), ("f16", ops.F16)):
        hub = speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=a.layers), dtype=dt)
        hub.load_state_dict(weights.synth_state_dict(weights.spec_of(hub), seed=0))
        ex = speech_units.SpeechUnitExtractor(hub.eval(), centers, layer=a.layers, dtype=dt)
        with torch.no_grad():
            med, lo, hi = timed(lambda: ex.units(pcm, ns), a.steps)
            print(f"units {name} B{a.batch} S{a.samples} ({frames} frames per clip, {a.layers} layers): {med:8.2f} ms "
                  f"(min {lo:.2f}, max {hi:.2f}) = {a.batch / med * 1e3:7.1f} clips/s", flush=True)
            prof = ops.KernelProfiler()
            ops.set_profiler(prof)
            try:
                ex.units(pcm, ns)
            finally:
                ops.set_profiler(None)
            rows = sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])
            total = sum(v["ms"] for _, v in rows)
            print(f"  per-kernel time of one forward ({total:.2f} ms in kernels):")
            for key, v in rows:
                rate = f"{v['flops'] / v['ms'] / 1e9:7.1f} TFLOP/s" if v["flops"] else " " * 15
                bw = f"{v['bytes'] / v['ms'] / 1e9:6.2f} TB/s" if v["bytes"] else ""
                print(f"    {key:<44s} {v['calls']:3d} calls {v['ms']:8.3f} ms {100 * v['ms'] / total:5.1f} %  {rate} {bw}", flush=True)
        del hub, ex
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
