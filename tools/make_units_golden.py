#!/usr/bin/env python3
"""Writes tests/golden/units_kmeans.npz by RUNNING the reference's own quantiser (avhubert/clustering/dump_km_label.py,
ApplyKmeans, imported as a single file) on seeded features, on the CPU.

  python tools/make_units_golden.py <reference>/avhubert/clustering

ApplyKmeans loads its model with joblib and reads `cluster_centers_` from it, so the tool dumps a plain object carrying that
attribute (what a fitted sklearn MiniBatchKMeans exposes) and hands the path over.  `tqdm`, which the file imports for its
progress bar only, is replaced by a stand-in when it is not installed.  Stored: the features float32 [130, 64], the centres
float32 [37, 64] (data rows plus noise: every row has a clear nearest centre), `ids` from ApplyKmeans' numpy branch on the float64
copies of both and `ids_f32` from the same branch on the float32 arrays.  Deterministic: re-running reproduces the file's arrays.
"""
import importlib.util
import os
import sys
import tempfile
import types

import joblib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "..", "tests", "golden", "units_kmeans.npz")
M, D, K = 130, 64, 37


def load_reference(clustering_dir):
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, **k: it)
    spec = importlib.util.spec_from_file_location("dump_km_label", os.path.join(clustering_dir, "dump_km_label.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case():
    rng = np.random.default_rng(20240607)
    feats = rng.standard_normal((M, D)).astype(np.float32)
    rows = rng.permutation(M)[:K]
    centers = (feats[rows] + 0.25 * rng.standard_normal((K, D))).astype(np.float32)
    return feats, centers


def run(mod, feats, centers):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "km.bin")
        joblib.dump(types.SimpleNamespace(cluster_centers_=centers), path)
        return np.asarray(mod.ApplyKmeans(path)(feats))


def build(clustering_dir):
    mod = load_reference(clustering_dir)
    feats, centers = make_case()
    return {"features": feats, "centers": centers,
            "ids": run(mod, feats.astype(np.float64), centers.astype(np.float64)).astype(np.int32),
            "ids_f32": run(mod, feats, centers).astype(np.int32)}


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    np.savez_compressed(GOLDEN, **build(sys.argv[1]))
    print("wrote", os.path.normpath(GOLDEN), os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
