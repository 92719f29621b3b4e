#!/usr/bin/env python3
"""Learns the speech-unit codebook (km.bin) on the device - avhubert/clustering/learn_kmeans.py:124-147 with its arguments
and defaults, the fit running on csrc/kmeans_fit.hip instead of scikit-learn's CPU MiniBatchKMeans.

  python -m lip2speech_unit_amd.learn_kmeans <feat_dir> <split> <nshard> <km_path> <n_clusters>
      [--seed 0] [--percent -1] [--init k-means++] [--max_iter 100] [--batch_size 10000] [--tol 0.0]
      [--max_no_improvement 100] [--n_init 20] [--reassignment_ratio 0.0]
  python -m lip2speech_unit_amd.learn_kmeans <km_path> <n_clusters> --audio_root <dir> --hubert <ckpt> [--layer 6]
      [--manifest <x_unit_manifest.txt>] [--dtype f32|f16|bf16] [--batch N]  (+ the options above)

The first form reads the feature shards <feat_dir>/<split>_<rank>_<nshard>.npy / .len (learn_kmeans.py:50-85); `--percent p`
samples ceil(p * utterances) utterances of every shard without replacement, drawing from the RandomState(seed) that the fit
then continues - the reference's global np.random stream after np.random.seed(seed).  The second form computes the features
with speech_units.HubertModel from <audio_root>/**/*.wav (or a manifest's files), `--percent` sampling the clips the same way.
km_path ending in .npy receives the centres; any other name a joblib dump of a scikit-learn MiniBatchKMeans carrying them (what
dump_km_label.py's ApplyKmeans loads).  Prints `total intertia: %.5f` (learn_kmeans.py:119-120: the mean squared distance to the
nearest centre over all features).
"""
import argparse
import os

import numpy as np
import torch

from . import kmeans_fit, ops


def shard_paths(feat_dir, split, nshard, rank):
    stem = f"{feat_dir}/{split}_{rank}_{nshard}"
    return stem + ".npy", stem + ".len"


def load_feature_shard(feat_dir, split, nshard, rank, percent, rs):
    """One shard's features (learn_kmeans.py:50-72): all of them as a memmap (percent < 0), or the utterances rs draws."""
    feat_path, leng_path = shard_paths(feat_dir, split, nshard, rank)
    with open(leng_path) as f:
        lengs = [int(line.rstrip()) for line in f]
    offsets = [0] + np.cumsum(lengs[:-1]).tolist()
    feat = np.load(feat_path, mmap_mode="r")
    if percent < 0:
        return feat
    nsample = int(np.ceil(len(lengs) * percent))
    indices = rs.choice(len(lengs), nsample, replace=False)
    return np.concatenate([feat[offsets[i]: offsets[i] + lengs[i]] for i in indices], axis=0)


def load_feature(feat_dir, split, nshard, percent, rs):
    shards = [load_feature_shard(feat_dir, split, nshard, r, percent, rs) for r in range(nshard)]
    if len(shards) == 1:
        return shards[0]                     # a memmap stays a memmap: the fit gathers its batches from it
    return np.concatenate(shards, axis=0)


def audio_features(audio_root, hubert_path, layer, manifest, dtype, batch, percent, rs):
    """Layer-`layer` HuBERT features of the clips as one float32 device tensor [frames, d]."""
    from . import audio, extract_units, speech_units
    dt = extract_units.DTYPES[dtype]
    hub = speech_units.load_hubert(hubert_path, dtype=dt)
    if not 0 < layer <= len(hub.encoder.layers):
        raise SystemExit(f"--layer {layer}: the model has {len(hub.encoder.layers)} transformer layers")
    paths = extract_units.list_clips(audio_root, manifest)
    if not paths:
        raise SystemExit(f"{audio_root}: no .wav files")
    if percent >= 0:
        paths = [paths[i] for i in rs.choice(len(paths), int(np.ceil(len(paths) * percent)), replace=False)]
    clips = [audio.read_wav_s16(p) for p in paths]
    short = [p for p, c in zip(paths, clips) if c.shape[0] < speech_units.MIN_SAMPLES]
    if short:
        raise SystemExit(f"clips under {speech_units.MIN_SAMPLES} samples have no feature frame: " + ", ".join(short))
    hub.cuda()
    order = sorted(range(len(clips)), key=lambda i: clips[i].shape[0])
    out = [None] * len(clips)
    for i in range(0, len(order), batch):
        group = order[i:i + batch]
        lens = [clips[j].shape[0] for j in group]
        pcm = np.zeros((len(group), max(lens)), np.int16)
        for r, j in enumerate(group):
            pcm[r, : lens[r]] = clips[j]
        rows, _, host_lens, B, T = hub.extract_rows(torch.from_numpy(pcm).cuda(), lens, layer)
        rows = rows.view(B, T, -1)
        for r, j in enumerate(group):
            out[j] = rows[r, : host_lens[r]].clone()
    return torch.cat(out, 0).contiguous()


def build_parser():
    p = argparse.ArgumentParser(description="mini-batch k-means codebook of speech units, fitted on the device")
    p.add_argument("paths", nargs="+", metavar="ARG",
                   help="feat_dir split nshard km_path n_clusters, or (with --audio_root) km_path n_clusters")
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--percent", default=-1, type=float, help="sample a subset; -1 for all")
    p.add_argument("--init", default="k-means++")
    p.add_argument("--max_iter", default=100, type=int)
    p.add_argument("--batch_size", default=10000, type=int)
    p.add_argument("--tol", default=0.0, type=float)
    p.add_argument("--max_no_improvement", default=100, type=int)
    p.add_argument("--n_init", default=20, type=int)
    p.add_argument("--reassignment_ratio", default=0.0, type=float)
    p.add_argument("--audio_root", default=None)
    p.add_argument("--hubert", default=None)
    p.add_argument("--layer", type=int, default=6)
    p.add_argument("--manifest", default=None)
    p.add_argument("--dtype", default="f32", choices=("bf16", "f16", "f32"))
    p.add_argument("--batch", type=int, default=16, help="clips per HuBERT forward (--audio_root)")
    return p


def main(argv=None):
    p = build_parser()
    a = p.parse_args(argv)
    audio_mode = a.audio_root is not None
    if len(a.paths) != (2 if audio_mode else 5):
        p.error("expected km_path n_clusters with --audio_root" if audio_mode else "expected feat_dir split nshard km_path n_clusters")
    try:
        n_clusters = int(a.paths[-1])
        nshard = 0 if audio_mode else int(a.paths[2])
    except ValueError:
        p.error("nshard and n_clusters are integers")
    km_path = a.paths[-2]
    if not 2 <= n_clusters <= 1024:
        p.error("n_clusters: 2 .. 1024")
    if a.percent > 1.0:
        p.error("--percent is a fraction: at most 1.0 (-1 for all)")
    if a.init not in ("k-means++", "random"):
        p.error("--init: k-means++ or random")
    if a.tol > 0:
        p.error("--tol > 0 is not built (the reference's default is 0)")
    if a.reassignment_ratio > 0:
        p.error("--reassignment_ratio > 0 is not built (the reference's default is 0)")
    if a.tol < 0 or a.reassignment_ratio < 0 or min(a.max_iter, a.batch_size, a.n_init, a.batch) < 1 or a.max_no_improvement < 0:
        p.error("--max_iter, --batch_size, --n_init, --batch must be at least 1; --tol, --reassignment_ratio, --max_no_improvement not negative")
    if audio_mode:
        if not a.hubert:
            p.error("--audio_root needs --hubert")
        if a.layer < 1:
            p.error("--layer must be at least 1")
        if not os.path.isdir(a.audio_root):
            p.error(f"{a.audio_root}: no such directory")
        for path in (a.hubert,) + ((a.manifest,) if a.manifest else ()):
            if not os.path.isfile(path):
                p.error(f"{path}: no such file")
    else:
        if a.hubert or a.manifest:
            p.error("--hubert / --manifest go with --audio_root")
        feat_dir, split = a.paths[0], a.paths[1]
        if nshard < 1:
            p.error("nshard must be at least 1")
        if not os.path.isdir(feat_dir):
            p.error(f"{feat_dir}: no such directory")
        for r in range(nshard):
            for path in shard_paths(feat_dir, split, nshard, r):
                if not os.path.isfile(path):
                    p.error(f"{path}: no such file")
    if not str(km_path).endswith(".npy"):
        try:
            import sklearn  # noqa: F401
        except ImportError:
            raise SystemExit("km_path: writing a scikit-learn model needs scikit-learn, which is not importable here; "
                             "give a name ending in .npy to write the centres alone")
    if not torch.cuda.is_available():
        raise SystemExit("this build runs on MI355X only: no CPU path")
    rs = np.random.RandomState(a.seed)
    if audio_mode:
        feat = audio_features(a.audio_root, a.hubert, a.layer, a.manifest, a.dtype, a.batch, a.percent, rs)
    else:
        feat = load_feature(feat_dir, split, nshard, a.percent, rs)
        if feat.dtype != np.float32:
            feat = np.ascontiguousarray(feat, dtype=np.float32)
    print(f"loaded feature with dimension {tuple(feat.shape)}")
    if feat.shape[0] < n_clusters:
        raise SystemExit(f"{feat.shape[0]} feature frames are fewer than n_clusters = {n_clusters}")
    fit = kmeans_fit.MiniBatchKMeansFit(n_clusters, init=a.init, max_iter=a.max_iter, batch_size=a.batch_size, tol=a.tol,
                                        max_no_improvement=a.max_no_improvement, n_init=a.n_init,
                                        reassignment_ratio=a.reassignment_ratio, random_state=rs)
    try:
        F = kmeans_fit.Features(feat, fit.device_budget_bytes)   # uploaded once: the fit and the inertia line read the same copy
        centers = fit.fit(F)
    except (ops.L2SError, ValueError) as e:
        raise SystemExit(f"fit: {e}")
    os.makedirs(os.path.dirname(os.path.abspath(km_path)), exist_ok=True)
    kmeans_fit.save_kmeans(km_path, fit)
    inertia = kmeans_fit.mean_min_distance(F, centers)
    print("total intertia: %.5f" % inertia)
    print(f"finished successfully: {fit.n_steps_} steps -> {km_path}")
    return fit


if __name__ == "__main__":
    main()
