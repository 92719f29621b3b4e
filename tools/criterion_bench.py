"""Times of the three criterion entries (csrc/criterion.hip) at the headline batch, for DESIGN.md section 13, each against the
torch composition the reference runs for the same term, on the same device in the same process, the two ALTERNATING run by run:

  * l2s_unit_ce        vs  log_softmax + gather / sum / argmax (fairseq's label_smoothed_nll_loss + compute_accuracy, restated);
  * l2s_mel_l1_sc      vs  L1Loss(reduction='none').mean(-1) * mask, summed, + the per-clip Frobenius norms;
  * l2s_ctc_loss       vs  log_softmax + F.ctc_loss(reduction='sum', zero_infinity=True)   (text logits [B*2T, 4000] fp32).

  python tools/criterion_bench.py [--steps 20] [--batch 640] [--frames 100] [--text-classes 4000] [--labels 40]

A report only (no gate).  Each figure is the median of `steps` runs between HIP events after 3 warm-up runs, min - max in brackets
(a call from Python includes its launch latency, on both sides; the kernels' own time is that of ten calls replayed from one
hipGraph); the last column is the largest difference between the two results (they are not each other's yardstick: the tests hold the kernels
to float64)."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed_alternating(fa, fb, steps, warm=3):
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(steps):
        for k, fn in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def device_time(fn, steps, reps=10):
    """ms per call with the host out of the picture: `reps` calls captured in one hipGraph, the replay timed."""
    fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    (med, lo, hi), _ = timed_alternating(graph.replay, lambda: None, steps)
    return med / reps


def report(name, nbytes, ours, theirs, diff, dev_ms):
    (a, alo, ahi), (b, blo, bhi) = ours, theirs
    print(f"{name}: call {a:8.3f} ms [{alo:.3f} - {ahi:.3f}] | torch {b:8.3f} ms [{blo:.3f} - {bhi:.3f}] | call / torch = {a / b:.3f} | "
          f"device time in a replayed hipGraph {dev_ms:.3f} ms = {nbytes / dev_ms / 1e6:7.1f} GB/s over the clips' own rows | "
          f"max rel. difference {diff:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=640)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--text-classes", type=int, default=4000)
    ap.add_argument("--labels", type=int, default=40)
    a = ap.parse_args()
    from lip2speech_unit_amd import ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    B, T, V, PAD = a.batch, a.frames, 204, 1
    T2 = 2 * T
    lens = torch.randint(T // 2, T + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    lens[0] = T
    rows2 = torch.arange(T2, device=dev)[None, :] < 2 * lens[:, None]

    # ---- units
    logits = torch.randn(B * T2, V, generator=g, device=dev) * 2
    target = torch.randint(4, V, (B, T2), generator=g, device=dev)
    target[~rows2] = PAD
    t32 = target.int()
    out = [torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32),
           torch.empty(B, device=dev, dtype=torch.int32)]

    def ours_units():
        ops.unit_ce(logits, t32, *out, B=B, T2=T2, V=V, lens=lens, len_mul=2, pad_idx=PAD)

    def torch_units():
        lprobs = F.log_softmax(logits, dim=-1)
        tgt = target.view(-1, 1)
        pad = tgt.eq(PAD)
        nll = (-lprobs.gather(-1, tgt)).masked_fill_(pad, 0.0).sum()
        smooth = (-lprobs.sum(-1, keepdim=True)).masked_fill_(pad, 0.0).sum()
        mask = ~pad.view(-1)
        n_correct = torch.sum(lprobs.argmax(1).masked_select(mask).eq(tgt.view(-1).masked_select(mask)))
        return nll, smooth, n_correct
    r = timed_alternating(ours_units, torch_units, a.steps)
    nll, smooth, nc = torch_units()
    diff = max(abs(out[0].double().sum() - nll.double()).item() / abs(nll.item()),
               abs(out[1].double().sum() - smooth.double()).item() / abs(smooth.item()))
    assert int(out[2].sum()) == int(nc)
    report(f"unit_ce    B{B} x {T2} x {V}", 4.0 * V * float(2 * lens.sum()), r[0], r[1], diff, device_time(ours_units, a.steps))
    del logits

    # ---- mel
    pred = torch.randn(B, 4 * T, 80, generator=g, device=dev) - 5
    targ = torch.randn(B, 4 * T, 80, generator=g, device=dev) - 5
    mask4 = torch.arange(4 * T, device=dev)[None, :] < 4 * lens[:, None]
    mo = [torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32)]

    def ours_mel_launch():
        ops.mel_l1_sc(pred, targ, *mo, B=B, Tm_pred=4 * T, Tm_targ=4 * T, crop_len=4 * T, lens=lens, len_mul=4)

    def ours_mel():
        ours_mel_launch()
        return (mo[0] / 80 / mo[3]).sum() + (mo[1].sqrt() / mo[2].sqrt()).sum()

    def torch_mel():                                     # criterion.py:73-85 with sentence_avg (the per-clip lists as one masked pass)
        l1 = ((F.l1_loss(pred, targ, reduction="none").mean(-1) * mask4).sum(1) / mask4.sum(1)).sum()
        m = mask4[..., None]
        sc = (torch.linalg.vector_norm((targ - pred) * m, dim=(1, 2)) / torch.linalg.vector_norm(targ * m, dim=(1, 2))).sum()
        return l1 + sc
    r = timed_alternating(ours_mel, torch_mel, a.steps)
    diff = abs(ours_mel().double() - torch_mel().double()).item() / abs(torch_mel().item())
    report(f"mel_l1_sc  B{B} x {4 * T} x 80", 8.0 * 80 * float(4 * lens.sum()), r[0], r[1], diff, device_time(ours_mel_launch, a.steps))
    del pred, targ

    # ---- text / CTC
    Vt, S = a.text_classes, a.labels
    text = torch.randn(B * T2, Vt, generator=g, device=dev)
    tl = torch.randint(max(S // 2, 1), S + 1, (B,), generator=g, device=dev, dtype=torch.int32)
    offs = (torch.cumsum(tl, 0, dtype=torch.int32) - tl).contiguous()
    labels = torch.randint(1, Vt, (int(tl.sum()),), generator=g, device=dev, dtype=torch.int32)
    work = torch.empty(ops.ctc_loss_workspace_bytes(B, T2, S) // 4, device=dev)
    cn = torch.empty(B, device=dev)
    il = (2 * lens).long()

    def ours_ctc():
        ops.ctc_loss(text, labels, tl, offs, work, cn, B=B, L=T2, V=Vt, S_max=S, lens=lens, len_mul=2)

    def torch_ctc():
        lp = F.log_softmax(text.view(B, T2, Vt).transpose(0, 1), dim=2)
        return F.ctc_loss(lp, labels.long(), il, tl.long(), blank=0, reduction="sum", zero_infinity=True)
    r = timed_alternating(ours_ctc, torch_ctc, a.steps)
    ref = torch_ctc()
    diff = abs(cn.double().sum() - ref.double()).item() / abs(ref.item())
    report(f"ctc_loss   B{B} x {T2} x {Vt}, <= {S} labels", 4.0 * Vt * float(2 * lens.sum()), r[0], r[1], diff, device_time(ours_ctc, a.steps))


if __name__ == "__main__":
    main()
