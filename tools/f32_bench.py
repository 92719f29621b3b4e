"""Rates of the fp32 (ops.F32) mode, for DESIGN.md section "fp32 reference-precision mode":

  * the fp32 tap-GEMM's TFLOP/s on the encoder's FC1 and QKV shapes at M = 6 400 (next to the fp16 kernel on the same shapes);
  * stage-1 milliseconds at B = 32, T = 100 in fp32 next to fp16 (one hipGraph replay per step, full depth).

  python tools/f32_bench.py [--steps 20] [--batch 32]

Each figure is the median of `steps` timed runs between HIP events after 3 warm-up runs, with the min - max spread."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, steps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=100)
    a = ap.parse_args()
    from lip2speech_unit_amd import ops, weights
    from lip2speech_unit_amd.model_avhubert import MultiTargetAVHubertEncoderModel
    from lip2speech_unit_amd.pipeline import GraphCache, LipToSpeechPipeline
    g = torch.Generator().manual_seed(0)
    M = 6400
    for name, N, K, act in (("FC1 (GELU)", 4096, 1024, ops.ACT_GELU), ("QKV", 3072, 1024, ops.ACT_NONE), ("FC2 (+x)", 1024, 4096, None)):
        for dt in (ops.F32, ops.F16):
            t = ops.torch_dtype(dt)
            A = torch.randn(M, K, generator=g).to(t).cuda()
            W = (torch.randn(N, K, generator=g) / K ** 0.5).to(t).cuda()
            b = torch.randn(N, generator=g).cuda()
            if act is None:
                x = torch.randn(M, N, generator=g).cuda()
                fn = lambda: ops.tapgemm(A, W, x, M=M, N=N, Cin=K, bias=b, R=x, ldr=N, flags=ops.F_RES_POST, dtype=dt)  # noqa: E731
            else:
                C = torch.empty(M, N, dtype=t, device="cuda")
                fn = lambda: ops.tapgemm(A, W, C, M=M, N=N, Cin=K, bias=b, act=act, dtype=dt)  # noqa: E731
            med, lo, hi = timed(fn, a.steps)
            fl = 2.0 * M * N * K
            print(f"tapgemm {'f32' if dt == ops.F32 else 'f16'} {name:11s} M{M} N{N} K{K}: {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}) "
                  f"= {fl / med / 1e9:7.1f} TFLOP/s", flush=True)
    B, T = a.batch, a.frames
    u8 = torch.randint(0, 256, (B, T, 88, 88), generator=g)
    video = ((u8.float() / 255.0 - 0.421) / 0.165).unsqueeze(1).cuda()
    spk = torch.rand(B, 256, generator=g).cuda()
    sd = None
    for dt in (ops.F32, ops.F16):
        m = MultiTargetAVHubertEncoderModel.build_model(dtype=dt)
        if sd is None:
            sd = weights.synth_state_dict(weights.spec_of(m), seed=0)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        pipe = LipToSpeechPipeline(m, None)
        cache = GraphCache(lambda v, s: pipe.stage1_device(v, None, s)["tokens"])
        med, lo, hi = timed(lambda: cache(video, spk), a.steps)
        print(f"stage 1 {'f32' if dt == ops.F32 else 'f16'} B{B} T{T} (24 + 12 layers, hipGraph replay): {med:8.2f} ms (min {lo:.2f}, max {hi:.2f}) "
              f"= {med / B:.3f} ms per clip, RTF {med / 1e3 / (B * T / 25.0):.5f}", flush=True)
        del m, pipe, cache
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
