"""The mini-batch k-means fit on the device (lip2speech_unit_amd/kmeans_fit.py, the learn_kmeans CLI) against the float64
restatement of tests/_kmeans_fit_reference.py and the recorded run of the reference's own learn_kmeans."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from lip2speech_unit_amd import kmeans_fit, learn_kmeans, ops, speech_units  # noqa: E402
from tests import _kmeans_fit_reference as KR  # noqa: E402

ARGS = dict(max_iter=20, batch_size=256, n_init=3)
TRAJECTORY_SEED = 2      # assignment margin 0.81 over all 160 steps (float64, found on the CPU)
STOP_SEED = 3            # max_no_improvement = 3 stops after 18 of 160 steps; EWA gap 5.0e-4, assignment margin 4.3e-3


def planted_int(seed, n=2048, D=64, K=16):
    """Integer planted data: centres in [-8, 8] plus noise in [-2, 2].  Every squared distance (< 2^15) and every sum of 768 of
    them is exact in fp32 and fp64, so the k-means++ init is decided without rounding."""
    rng = np.random.default_rng(seed)
    cen = rng.integers(-8, 9, (K, D))
    return (cen[rng.integers(0, K, n)] + rng.integers(-2, 3, (n, D))).astype(np.float32)


_REF = {}


def ref_fit(seed, max_no_improvement):
    key = (seed, max_no_improvement)
    if key not in _REF:
        X = planted_int(seed)
        _REF[key] = (X, KR.fit(X, 16, seed=seed, max_no_improvement=max_no_improvement, p_dtype=np.float32, **ARGS))
    return _REF[key]


def dev_fit(X, seed, max_no_improvement, **kw):
    f = kmeans_fit.MiniBatchKMeansFit(16, max_no_improvement=max_no_improvement, seed=seed, **dict(ARGS, **kw))
    return f, f.fit(X)


def trajectory_gate(X, r):
    """4 x the deviation of a numpy-float32 run of the restatement's step loop (same init, same batches) from its float64 run."""
    c32 = KR.step_loop(X, r["init_centers"], r["batches"], None, dtype=np.float32)[0]
    return 4.0 * np.abs(c32.astype(np.float64) - r["centers"]).max()


def test_init_is_exact_on_integer_data():
    for seed in (TRAJECTORY_SEED, STOP_SEED):
        X, r = ref_fit(seed, 3)
        assert (KR.sq_dists(X.astype(np.float64), X.astype(np.float64)).max() * 768) < 2 ** 24
        f, _ = dev_fit(X, seed, 3, max_iter=1)
        assert f.best_init_ == r["best_init"]
        for got, want in zip(f.all_init_indices_, r["all_init_indices"]):
            assert np.array_equal(got, want)
        assert np.array_equal(f.init_indices_, r["init_indices"]) and np.array_equal(f.init_inertias_, np.array(r["init_inertias"]))
        assert np.array_equal(f.init_centers_, X[r["init_indices"]])


def test_trajectory_without_early_stopping():
    X, r = ref_fit(TRAJECTORY_SEED, 1000)
    assert r["margins"]["assign"] > 1e-3 and r["n_steps"] == r["total_steps"] == 160
    f, c = dev_fit(X, TRAJECTORY_SEED, 1000)
    assert f.n_steps_ == 160 and f.n_iter_ == r["n_iter"] and np.array_equal(f.counts_, r["counts"].astype(np.float32))
    gate = trajectory_gate(X, r)
    err = np.abs(c.astype(np.float64) - r["centers"]).max()
    print(f"trajectory: centre max abs err {err:.3e} after 160 steps, gate {gate:.3e} (4 x numpy float32)")
    assert c.dtype == np.float32 and c.shape == (16, 64) and err <= gate
    assert abs(f.inertia_ - r["inertia"]) <= 1e-5 * r["inertia"]
    # random init and an array init run the same loop
    r2 = KR.fit(X, 16, seed=5, init="random", max_no_improvement=1000, p_dtype=np.float32, **ARGS)
    f2 = kmeans_fit.MiniBatchKMeansFit(16, init="random", max_no_improvement=1000, seed=5, **ARGS)
    c2 = f2.fit(torch.from_numpy(X).cuda())                   # a device tensor
    # (its integer init centres meet exact distance ties, which float64 and the device both give to the lower index; the later
    # trajectory is not gated here because the restatement's margin cannot tell such a tie from a near-tie)
    assert np.array_equal(f2.init_indices_, r2["init_indices"]) and f2.best_init_ == r2["best_init"] and f2.n_steps_ == 160
    assert np.array_equal(f2.init_centers_, X[r2["init_indices"]]) and np.isfinite(c2).all()
    r3 = KR.fit(X, 16, seed=6, init=r["init_centers"], max_no_improvement=1000, p_dtype=np.float32, **ARGS)
    f3 = kmeans_fit.MiniBatchKMeansFit(16, init=r["init_centers"], max_no_improvement=1000, seed=6, **ARGS)
    assert f3.fit(X) is f3.cluster_centers_ and f3.init_indices_ is None and f3.n_steps_ == 160
    assert r3["margins"]["assign"] > 1e-3
    assert np.abs(f3.cluster_centers_ - r3["centers"]).max() <= trajectory_gate(X, r3)


def test_early_stopping_replays_to_the_stopping_step():
    X, r = ref_fit(STOP_SEED, 3)
    assert r["margins"]["ewa"] > 1e-4 and r["margins"]["assign"] > 1e-3 and 2 < r["n_steps"] < r["total_steps"]
    assert r["n_steps"] % 64 and r["n_steps"] % 8                  # the stop falls inside a chunk of either length
    f, c = dev_fit(X, STOP_SEED, 3)                                  # chunks of 64 steps: overshoots, restores, replays
    f8, c8 = dev_fit(X, STOP_SEED, 3, chunk_steps=8)
    f1, c1 = dev_fit(X, STOP_SEED, 3, chunk_steps=1)                 # synchronises every step: no overshoot to undo
    assert f.n_steps_ == f8.n_steps_ == f1.n_steps_ == r["n_steps"] and f.n_iter_ == r["n_iter"]
    assert np.array_equal(c, c1) and np.array_equal(c8, c1) and np.array_equal(f.counts_, f1.counts_) and f.inertia_ == f1.inertia_
    assert np.array_equal(f.counts_, r["counts"].astype(np.float32))
    assert np.abs(c.astype(np.float64) - r["centers"]).max() <= trajectory_gate(X, dict(r, batches=r["batches"]))


def test_resident_and_host_gathered_features_agree_to_the_bit():
    X, r = ref_fit(STOP_SEED, 3)
    fa, ca = dev_fit(X, STOP_SEED, 3, chunk_steps=8)
    fb, cb = dev_fit(X, STOP_SEED, 3, chunk_steps=8, device_budget_bytes=0)
    assert fa.resident_ and not fb.resident_ and not hasattr(fa, "_features")
    assert np.array_equal(ca, cb) and np.array_equal(fa.counts_, fb.counts_) and fa.n_steps_ == fb.n_steps_ == r["n_steps"]
    assert np.array_equal(fa.init_indices_, fb.init_indices_) and fa.inertia_ == fb.inertia_
    a, b = kmeans_fit.mean_min_distance(X, ca), kmeans_fit.mean_min_distance(X, ca, device_budget_bytes=0)
    assert a == b


def test_cli_from_shards(tmp_path, capsys):
    X = planted_int(11, n=1500)
    rng = np.random.default_rng(12)
    at = 0
    for rnk in range(2):
        lens = rng.integers(40, 70, 13)
        np.save(tmp_path / f"train_{rnk}_2.npy", X[at:at + lens.sum()])
        (tmp_path / f"train_{rnk}_2.len").write_text("".join(f"{n}\n" for n in lens))
        at += lens.sum()
    km = str(tmp_path / "out" / "km.bin")
    argv = [str(tmp_path), "train", "2", km, "16", "--seed", "4", "--percent", "0.5", "--max_iter", "10", "--batch_size", "128", "--n_init", "2",
            "--max_no_improvement", "5"]
    capsys.readouterr()
    fit = learn_kmeans.main(argv)
    out = capsys.readouterr().out
    rs = np.random.RandomState(4)
    feat = learn_kmeans.load_feature(str(tmp_path), "train", 2, 0.5, rs)          # the sampled rows, the stream continued by the fit
    assert 300 < len(feat) < 1000
    direct = kmeans_fit.MiniBatchKMeansFit(16, max_iter=10, batch_size=128, n_init=2, max_no_improvement=5, random_state=rs)
    want = direct.fit(feat)
    assert np.array_equal(fit.cluster_centers_, want) and fit.n_steps_ == direct.n_steps_
    cen = speech_units.load_kmeans(km)
    assert np.array_equal(cen, want)
    np_path = str(tmp_path / "centers.npy")
    learn_kmeans.main(argv[:3] + [np_path] + argv[4:])
    assert np.array_equal(speech_units.load_kmeans(np_path), want)
    # the codebook drives the quantiser: every training row lands on the centre l2s_kmeans_nearest reported
    hub = speech_units.HubertModel(speech_units.HubertConfig(encoder_layers=1, encoder_embed_dim=64, encoder_ffn_embed_dim=128,
                                                             encoder_attention_heads=1))
    ex = speech_units.SpeechUnitExtractor(hub, cen, layer=1)
    xd = torch.from_numpy(feat).cuda()
    ids = ex.assign(xd, None, 1, len(feat))
    mine = torch.empty(len(feat), device="cuda", dtype=torch.int32)
    cd = torch.from_numpy(cen).cuda()
    ops.kmeans_nearest(xd, cd, cd.double().pow(2).sum(1).float(), M=len(feat), D=64, K=16, ids=mine)
    assert torch.equal(ids, mine) and len(torch.unique(ids)) == 16
    line = [ln for ln in out.splitlines() if ln.startswith("total intertia: ")]
    assert len(line) == 1
    ref = KR.assign(feat.astype(np.float64), want.astype(np.float64))[1].mean()
    assert abs(float(line[0].split(": ")[1]) - ref) <= 1e-5 * ref
    assert abs(kmeans_fit.mean_min_distance(feat, want) - ref) <= 1e-5 * ref


def test_cli_from_audio(tmp_path, golden_dir):
    from tests import _mel_reference as mr
    from tests import _units_reference as R
    root = str(tmp_path / "data")
    mr.materialise_audio_dataset(root, golden_dir, with_mel=False)
    layers = 1
    sd = R.init_weights(0, layers=layers)
    ck = str(tmp_path / "hubert.pt")
    torch.save({"model": sd, "cfg": {"model": {"_name": "hubert", "encoder_layers": layers}, "task": {"normalize": False}}}, ck)
    out = str(tmp_path / "centers.npy")
    fit = learn_kmeans.main([out, "8", "--audio_root", os.path.join(root, "audio"), "--hubert", ck, "--layer", "1", "--max_iter", "2",
                             "--batch_size", "128", "--n_init", "2", "--batch", "2"])
    cen = speech_units.load_kmeans(out)
    assert cen.shape == (8, 768) and np.isfinite(cen).all() and len(np.unique(cen, axis=0)) == 8
    assert fit.n_samples_ == 214 + 124 + 63 + 178 + 76 and fit.n_steps_ == (2 * 655) // 128


def test_golden_run_of_the_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "kmeans_fit.npz"))
    arg = {k[4:]: z[k].item() for k in z.files if k.startswith("arg_")}
    X = z["sampled"].astype(np.float32)
    rs = np.random.RandomState(arg["seed"])
    for rnk in range(2):                                              # the `--percent` draws that precede the fit
        rs.choice(len(z[f"lens{rnk}"]), int(np.ceil(len(z[f"lens{rnk}"]) * arg["percent"])), replace=False)
    kw = dict(init=arg["init"], max_iter=arg["max_iter"], batch_size=arg["batch_size"], max_no_improvement=arg["max_no_improvement"],
              n_init=arg["n_init"])
    f = kmeans_fit.MiniBatchKMeansFit(arg["n_clusters"], tol=arg["tol"], reassignment_ratio=arg["reassignment_ratio"], random_state=rs, **kw)
    c = f.fit(X)
    assert f.n_steps_ == int(z["n_steps"]) and f.n_iter_ == int(z["n_iter"])
    for i in range(arg["n_init"]):
        assert np.array_equal(X[f.all_init_indices_[i]], z["init_centers"][i].astype(np.float32)), i
    assert np.array_equal(f.counts_, z["counts"])
    rs2 = np.random.RandomState(arg["seed"])
    for rnk in range(2):
        rs2.choice(len(z[f"lens{rnk}"]), int(np.ceil(len(z[f"lens{rnk}"]) * arg["percent"])), replace=False)
    r = KR.fit(X, arg["n_clusters"], random_state=rs2, p_dtype=np.float32, **kw)
    gate = trajectory_gate(X, r)
    err, ref_err = np.abs(c.astype(np.float64) - r["centers"]).max(), np.abs(c - z["centers"]).max()
    print(f"golden: centre max abs err against float64 {err:.3e} (gate {gate:.3e}), against the reference's float32 centres {ref_err:.3e}")
    assert err <= gate
    got = kmeans_fit.mean_min_distance(X, c)
    assert abs(got - float(z["printed_inertia"])) <= 1e-5 * float(z["printed_inertia"])
