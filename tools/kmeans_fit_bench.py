#!/usr/bin/env python3
"""Times the mini-batch k-means fit kernels (csrc/kmeans_fit.hip) at corpus scale: seeded features N = 1 000 000 x 768, K = 200,
batch 10 000 - the shapes of avhubert/clustering/learn_kmeans.py's defaults on HuBERT-base features.

  python tools/kmeans_fit_bench.py [--n 1000000] [--dim 768] [--k 200] [--batch 10000] [--steps 50] [--inits 2] [--sklearn_steps 5]
      [--out profiles/kmeans_fit_bench.json]

Reports, from HIP events: the time of a step split by kernel entry (l2s_kmeans_nearest, l2s_kmeans_update), the achieved bytes/s
of a step against the 2 * batch * dim * 4 bytes (61 MB) it must move (the batch is read once by the assignment and once by the
update), the time of one k-means++ init (init_size = 3 batch rows, K - 1 rounds of pick / potentials / closest), and - if
scikit-learn is importable - scikit-learn's CPU time per step on the same data (MiniBatchKMeans.partial_fit on the same batches).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lip2speech_unit_amd import kmeans_fit, ops  # noqa: E402


def features(n, dim, k, seed=0):
    """Seeded planted features generated on the device (float32): k centres of norm ~ sqrt(dim) plus unit noise."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cen = torch.randn(k, dim, device="cuda", generator=g)
    lab = torch.randint(0, k, (n,), device="cuda", generator=g)
    x = torch.empty(n, dim, device="cuda")
    for a in range(0, n, 1 << 18):
        e = min(n, a + (1 << 18))
        x[a:e] = cen[lab[a:e]] + torch.randn(e - a, dim, device="cuda", generator=g)
    return x


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=1000000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--k", type=int, default=200)
    p.add_argument("--batch", type=int, default=10000)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--inits", type=int, default=2)
    p.add_argument("--sklearn_steps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this tool runs on MI355X only")
    n, D, K, M = a.n, a.dim, a.k, a.batch
    x = features(n, D, K)
    rs = np.random.RandomState(0)
    fit = kmeans_fit.MiniBatchKMeansFit(K, batch_size=M, n_init=1, random_state=rs)
    F = kmeans_fit.Features(x, 1 << 62)
    res = {"n": n, "dim": D, "k": K, "batch": M, "device": torch.cuda.get_device_name(0)}

    # k-means++ inits (queued without a host synchronisation; one sync at the end of each)
    isz = kmeans_fit.init_size_of(n, K, M)
    times = []
    for i in range(a.inits + 1):
        sub = rs.randint(0, n, isz)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos, _ = fit._kmeans_pp(F, sub, rs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    res["init_size"] = isz
    res["kmeanspp_init_ms"] = 1e3 * min(times[1:])              # the first call warms up
    cen = x.index_select(0, torch.from_numpy(sub).cuda()[pos.long()]).contiguous()

    # steps, per kernel entry
    cn = kmeans_fit._cnorm(cen)
    counts = torch.zeros(K, device="cuda")
    ids = torch.empty(M, device="cuda", dtype=torch.int32)
    inert = torch.zeros(1, device="cuda", dtype=torch.float64)
    ws_n = torch.empty(ops.kmeans_nearest_workspace_bytes(M), device="cuda", dtype=torch.uint8)
    ws_u = torch.empty(ops.kmeans_update_workspace_bytes(M, K), device="cuda", dtype=torch.uint8)
    batches = [rs.randint(0, n, M) for _ in range(a.steps)]
    rows = torch.from_numpy(np.stack(batches).astype(np.int32)).cuda()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.steps)]
    for s in range(a.steps):
        ev[s][0].record()
        ops.kmeans_nearest(x, cen, cn, M=M, D=D, K=K, rows=rows[s], ids=ids, inertia=inert, workspace=ws_n)
        ev[s][1].record()
        ops.kmeans_update(x, ids, cen, counts, cen, counts, cn, ws_u, M=M, D=D, K=K, rows=rows[s])
        ev[s][2].record()
    torch.cuda.synchronize()
    warm = min(5, a.steps // 2)
    near = np.array([e[0].elapsed_time(e[1]) for e in ev[warm:]])
    upd = np.array([e[1].elapsed_time(e[2]) for e in ev[warm:]])
    must = 2.0 * M * D * 4
    res.update({"nearest_ms": float(np.median(near)), "update_ms": float(np.median(upd)), "step_ms": float(np.median(near + upd)),
                "step_bytes": must, "step_bytes_per_s": must / (1e-3 * float(np.median(near + upd))),
                "nearest_tflops": 2.0 * M * K * D / (1e-3 * float(np.median(near))) / 1e12})

    # the step loop as fit() runs it (chunks, one synchronisation each), wall clock
    t0 = time.perf_counter()
    f2 = kmeans_fit.MiniBatchKMeansFit(K, init=cen.cpu().numpy(), batch_size=M, max_iter=max(1, (a.steps * M) // n + 1), n_init=1,
                                       max_no_improvement=None, seed=1)
    f2.fit(x)
    res["fit_loop_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / f2.n_steps_
    res["fit_loop_steps"] = f2.n_steps_

    try:
        from sklearn.cluster import MiniBatchKMeans
    except ImportError:
        MiniBatchKMeans = None
    if MiniBatchKMeans is not None and a.sklearn_steps > 0:
        km = MiniBatchKMeans(n_clusters=K, init=cen.cpu().numpy(), n_init=1, batch_size=M, compute_labels=False, reassignment_ratio=0.0)
        host = [x[torch.from_numpy(b).cuda()].cpu().numpy() for b in batches[:a.sklearn_steps + 1]]
        km.partial_fit(host[0])
        t0 = time.perf_counter()
        for h in host[1:]:
            km.partial_fit(h)
        res["sklearn_cpu_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / a.sklearn_steps
        res["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", 0)) or None
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
