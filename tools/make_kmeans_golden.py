#!/usr/bin/env python3
"""Writes tests/golden/kmeans_fit.npz by RUNNING the reference's own learn_kmeans.learn_kmeans (avhubert/clustering/learn_kmeans.py,
imported as a single file) on a small seeded shard pair, on the CPU.

  python tools/make_kmeans_golden.py <reference>/avhubert/clustering

The features are small-integer valued (planted integer centres plus integer noise), so that every squared distance and every
k-means++ potential of the run is an integer below 2^24: exact in the float32 the reference computes in, in float64 and on the
device alike - the init of the run is decided without rounding.  Stored: both shards (int8) with their utterance lengths, the
arguments, the rows the reference's `--percent` sampling selected (the features its fit saw), the centres of every init it tried
(recorded by wrapping scikit-learn's MiniBatchKMeans._init_centroids for the duration of the call; the reference's text is not
touched), the fitted centres, n_steps_, n_iter_ and the inertia it printed.  Deterministic: re-running reproduces the arrays.
"""
import importlib.util
import logging
import os
import sys
import tempfile

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden", "kmeans_fit.npz")
D, K, PLANTED = 32, 8, 8
ARGS = dict(n_clusters=K, seed=7, percent=0.5, init="k-means++", max_iter=20, batch_size=128, tol=0.0, n_init=3,
            reassignment_ratio=0.0, max_no_improvement=8)


def make_shards():
    rng = np.random.default_rng(20250311)
    centres = rng.integers(-8, 9, (PLANTED, D))
    shards = []
    for _ in range(2):
        lens = rng.integers(20, 60, 13)
        lab = rng.integers(0, PLANTED, int(lens.sum()))
        feat = centres[lab] + rng.integers(-2, 3, (len(lab), D))
        shards.append((feat.astype(np.float32), lens.astype(np.int64)))
    return shards


def load_reference(clustering_dir):
    spec = importlib.util.spec_from_file_location("learn_kmeans_reference", os.path.join(clustering_dir, "learn_kmeans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(clustering_dir):
    from sklearn.cluster import MiniBatchKMeans
    mod = load_reference(clustering_dir)
    shards = make_shards()
    inits, seen, lines = [], [], []
    real_init = MiniBatchKMeans._init_centroids
    real_fit = MiniBatchKMeans.fit

    def spy_init(self, X, *a, **k):
        c = real_init(self, X, *a, **k)
        inits.append(np.array(c, dtype=np.float64))
        return c

    def spy_fit(self, X, *a, **k):
        seen.append(np.array(X))
        return real_fit(self, X, *a, **k)

    class Keep(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())

    handler = Keep()
    mod.logger.addHandler(handler)
    MiniBatchKMeans._init_centroids, MiniBatchKMeans.fit = spy_init, spy_fit
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for r, (feat, lens) in enumerate(shards):
                np.save(os.path.join(tmp, f"train_{r}_2.npy"), feat)
                with open(os.path.join(tmp, f"train_{r}_2.len"), "w") as f:
                    f.write("".join(f"{n}\n" for n in lens))
            km_path = os.path.join(tmp, "km.bin")
            mod.learn_kmeans(tmp, "train", 2, km_path, **ARGS)
            km = joblib.load(km_path)
    finally:
        MiniBatchKMeans._init_centroids, MiniBatchKMeans.fit = real_init, real_fit
        mod.logger.removeHandler(handler)
    inertia = [float(ln.split(":")[1]) for ln in lines if ln.startswith("total intertia")]
    assert len(inertia) == 1 and len(seen) == 1 and len(inits) == ARGS["n_init"]
    sampled = seen[0]
    assert sampled.dtype == np.float32 and np.array_equal(sampled, np.round(sampled)) and np.abs(sampled).max() < 127
    out = {"sampled": sampled.astype(np.int8), "init_centers": np.stack(inits).astype(np.int8),
           "centers": np.asarray(km.cluster_centers_, dtype=np.float32), "n_steps": np.int64(km.n_steps_), "n_iter": np.int64(km.n_iter_),
           "printed_inertia": np.float64(inertia[0]), "counts": np.asarray(km._counts, dtype=np.float32)}
    assert np.array_equal(out["init_centers"], np.stack(inits))
    for r, (feat, lens) in enumerate(shards):
        out[f"shard{r}"], out[f"lens{r}"] = feat.astype(np.int8), lens
    for k, v in ARGS.items():
        out["arg_" + k] = np.array(v)
    return out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    np.savez_compressed(GOLDEN, **build(sys.argv[1]))
    print("wrote", os.path.normpath(GOLDEN), os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
