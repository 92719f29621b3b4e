"""Text-supervision decode costs: the CTC text head GEMM (y16 [M, 512] x W [4000, 512] -> fp32 logits),
l2s_ctc_frames (softmax, argmax, top-40) and l2s_ctc_beam_search (beam 30) at 640 x 4-s clips (L = 200 unit frames) and at
one clip, each replayed from a hipGraph as bench.py does.  Prints one JSON line per configuration.

    python tools/text_bench.py [--clips 640] [--reps 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lip2speech_unit_amd import ops  # noqa: E402


def timed(fn, reps):
    """Mean ms of one replay of a graph holding `fn` (captured after two warm-up calls)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench(B, L, V=4000, d=512, K=40, beam=30, reps=20):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    M = B * L
    y16 = torch.randn(M, d, device=dev, generator=g).half()
    w = (torch.randn(V, d, device=dev, generator=g) * d ** -0.5).half()
    bias = torch.zeros(V, device=dev)
    logits = torch.empty(M, V, device=dev)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    lab = torch.empty(B, L, dtype=torch.int32, device=dev)
    tc = torch.empty(B, L, K, dtype=torch.int32, device=dev)
    tl = torch.empty(B, L, K, device=dev)
    work = torch.empty(ops.ctc_beam_workspace_bytes(B, L, beam) // 8, dtype=torch.int64, device=dev)
    beams = torch.empty(B, 3, L, dtype=torch.int32, device=dev)
    blen = torch.empty(B, 3, dtype=torch.int32, device=dev)
    bsc = torch.empty(B, 3, device=dev)

    def head():
        ops.tapgemm(y16, w, logits, M=M, N=V, Cin=d, bias=bias, dtype=ops.F16)

    def greedy():
        ops.ctc_frames(logits, lab, None, None, B=B, L=L, V=V, K=0, lens=lens)

    def frames():
        ops.ctc_frames(logits, lab, tc, tl, B=B, L=L, V=V, K=K, lens=lens)

    def search():
        ops.ctc_beam_search(tc, tl, work, beams, blen, bsc, B=B, L=L, K=K, beam=beam, nbest=3, lens=lens)

    head()
    frames()
    r = {"clips": B, "L": L, "V": V, "K": K, "beam": beam}
    r["head_gemm_ms"] = timed(head, reps)
    r["head_gemm_tflops"] = 2.0 * M * V * d / r["head_gemm_ms"] / 1e9
    r["ctc_frames_argmax_ms"] = timed(greedy, reps)
    r["ctc_frames_top40_ms"] = timed(frames, reps)
    r["ctc_frames_GBps"] = M * V * 4 / r["ctc_frames_top40_ms"] / 1e6
    r["ctc_beam_search_ms"] = timed(search, reps)
    r["ctc_beam_search_us_per_frame"] = r["ctc_beam_search_ms"] * 1e3 / L
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=640)
    ap.add_argument("--L", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for B in (a.clips, 1):
        print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in bench(B, a.L, reps=a.reps).items()}), flush=True)


if __name__ == "__main__":
    main()
