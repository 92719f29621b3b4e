"""Mini-batch k-means fit, the parts that need no GPU: the float64 restatement against scikit-learn and against a recorded run of
the reference's own learn_kmeans, the shard reader, the CLI's errors, the ABI's rejections, the operator twins and km.bin."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

from tests import _kmeans_fit_reference as KR

# tests/golden/kmeans_fit.npz (tools/make_kmeans_golden.py): the float64 restatement's centres deviate from the reference's float32
# run by 3.33e-6 at most (6.5e-7 of the centre RMS 5.15); the gate is 4x that, and never above 1e-4 of the RMS
GOLDEN_OBSERVED_DEV = 3.33e-6


def planted(seed, n=2048, D=64, K=16):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((K, D)) * 3
    return cen[rng.integers(0, K, n)] + rng.standard_normal((n, D))


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("max_no_improvement", [3, 1000])
@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_restatement_equals_sklearn_in_float64(seed, max_no_improvement, init):
    cluster = pytest.importorskip("sklearn.cluster")
    X = planted(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = cluster.MiniBatchKMeans(n_clusters=16, init=init, max_iter=20, batch_size=256, compute_labels=False, tol=0.0,
                                     max_no_improvement=max_no_improvement, init_size=None, n_init=3, reassignment_ratio=0.0,
                                     random_state=seed).fit(X)
    r = KR.fit(X, 16, seed=seed, init=init, max_iter=20, batch_size=256, max_no_improvement=max_no_improvement, n_init=3)
    assert r["n_steps"] == km.n_steps_ and r["n_iter"] == km.n_iter_
    assert (r["n_steps"] < r["total_steps"]) == (max_no_improvement == 3)            # the early stop fires, or the fit runs out
    assert np.abs(r["centers"] - km.cluster_centers_).max() <= 1e-12
    assert abs(r["inertia"] - km.inertia_) <= 1e-9 * km.inertia_ and np.array_equal(r["counts"], km._counts)


def test_explicit_batches_equal_partial_fit_with_an_array_init():
    cluster = pytest.importorskip("sklearn.cluster")
    X = planted(5, n=600, D=32, K=6)
    rng = np.random.default_rng(6)
    init = X[rng.permutation(600)[:6]].copy()
    batches = [rng.integers(0, 600, 100) for _ in range(7)]
    km = cluster.MiniBatchKMeans(n_clusters=6, init=init, n_init=1, batch_size=100, reassignment_ratio=0.0, compute_labels=False, random_state=0)
    for b in batches:
        km.partial_fit(X[b])
    c, counts, steps, _ = KR.step_loop(X, init, batches, None)
    assert steps == 7 and np.abs(c - km.cluster_centers_).max() <= 1e-12 and np.array_equal(counts, km._counts)
    # an array init through fit(): one init, the same draw order
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km2 = cluster.MiniBatchKMeans(n_clusters=6, init=init, n_init=1, max_iter=5, batch_size=100, reassignment_ratio=0.0,
                                      compute_labels=False, max_no_improvement=None, random_state=3).fit(X)
    r = KR.fit(X, 6, seed=3, init=init, max_iter=5, batch_size=100, max_no_improvement=None, n_init=1)
    assert r["n_steps"] == km2.n_steps_ == 30 and np.abs(r["centers"] - km2.cluster_centers_).max() <= 1e-12 and r["init_indices"] is None


def _write_shards(z, root):
    for r in range(2):
        np.save(os.path.join(root, f"train_{r}_2.npy"), z[f"shard{r}"].astype(np.float32))
        with open(os.path.join(root, f"train_{r}_2.len"), "w") as f:
            f.write("".join(f"{int(n)}\n" for n in z[f"lens{r}"]))


def test_restatement_and_shard_reader_equal_the_references_recorded_run(golden_dir, tmp_path):
    from lip2speech_unit_amd import learn_kmeans
    path = os.path.join(golden_dir, "kmeans_fit.npz")
    assert os.path.getsize(path) < 200 * 1024
    z = np.load(path)
    arg = {k[4:]: z[k].item() for k in z.files if k.startswith("arg_")}
    _write_shards(z, str(tmp_path))
    rs = np.random.RandomState(arg["seed"])
    feat = learn_kmeans.load_feature(str(tmp_path), "train", 2, arg["percent"], rs)
    assert feat.dtype == np.float32 and np.array_equal(feat, z["sampled"])           # the reference's `--percent` row selection
    X = feat.astype(np.float64)
    # the fixture decides its init without rounding: integer features, every squared distance and potential below 2^24
    K, isz = arg["n_clusters"], min(3 * arg["batch_size"], len(X))
    assert np.array_equal(X, np.round(X)) and isz * KR.sq_dists(X, X).max() < 2 ** 24
    r = KR.fit(X, K, random_state=rs, init=arg["init"], max_iter=arg["max_iter"], batch_size=arg["batch_size"],
               max_no_improvement=arg["max_no_improvement"], n_init=arg["n_init"], p_dtype=np.float32)   # rs: continued after the sampling
    assert r["n_steps"] == int(z["n_steps"]) and r["n_iter"] == int(z["n_iter"]) and r["n_steps"] < r["total_steps"]
    for i in range(arg["n_init"]):                                                      # every init the reference tried, row for row
        assert np.array_equal(X[r["all_init_indices"][i]], z["init_centers"][i].astype(np.float64)), i
    assert np.array_equal(r["counts"], z["counts"].astype(np.float64))
    dev = np.abs(r["centers"] - z["centers"]).max()
    rms = np.sqrt((z["centers"].astype(np.float64) ** 2).mean())
    print(f"centre deviation from the reference's float32 run {dev:.3e} ({dev / rms:.2e} of the centre RMS {rms:.3f}); margins {r['margins']}")
    assert dev <= min(4.0 * GOLDEN_OBSERVED_DEV, 1e-4 * rms)
    assert abs(KR.assign(X, z["centers"].astype(np.float64))[1].mean() - float(z["printed_inertia"])) <= 1e-5 * float(z["printed_inertia"])
    # all shards (percent < 0): read in rank order, nothing drawn
    rs2 = np.random.RandomState(1)
    full = learn_kmeans.load_feature(str(tmp_path), "train", 2, -1, rs2)
    assert np.array_equal(full, np.concatenate([z["shard0"], z["shard1"]]).astype(np.float32))
    assert rs2.randint(0, 1 << 30) == np.random.RandomState(1).randint(0, 1 << 30)


def test_early_stopping_rule_is_a_host_function_of_the_inertias():
    from lip2speech_unit_amd.kmeans_fit import EarlyStopping, init_size_of
    rng = np.random.default_rng(0)
    vals = 1000.0 * (1.0 + 0.5 * np.exp(-np.arange(200) / 10.0) + 0.01 * rng.standard_normal(200))
    for n, batch, mni in ((2048, 256, 3), (2048, 256, 10), (100, 256, 2), (5000, 100, None)):
        a, b = EarlyStopping(n, batch, mni), KR.EarlyStop(n, batch, mni)
        got = [a.feed(i, v) for i, v in enumerate(vals)]
        want = [b.feed(i, v) for i, v in enumerate(vals)]
        assert got == want and a.ewa == b.ewa and a.ewa_min == b.ewa_min
        assert (True in got) == (mni is not None)
    s = EarlyStopping(1000, 100, 2)
    assert [s.feed(i, v) for i, v in enumerate([1e3, 3e3, 4e3, 4e3])] == [False, False, False, True]
    assert s.ewa_min == 30.0                                     # step 0 never enters the average; two steps above the minimum stop
    assert s.ewa == pytest.approx((30.0 * (1 - 200 / 1001) + 40.0 * 200 / 1001) * (1 - 200 / 1001) + 40.0 * 200 / 1001)
    assert init_size_of(2048, 16, 256) == 768 and init_size_of(500, 16, 256) == 500 and init_size_of(5000, 100, 10) == 300


def test_options_that_are_not_built_raise_by_name():
    from lip2speech_unit_amd.kmeans_fit import L2SError, MiniBatchKMeansFit
    for kw, word in ((dict(reassignment_ratio=0.01), "reassignment_ratio"), (dict(tol=1e-3), "tol"), (dict(init=lambda *a: None), "callable")):
        with pytest.raises(NotImplementedError, match=word):
            MiniBatchKMeansFit(8, **kw)
    with pytest.raises(NotImplementedError, match="sample_weight"):
        MiniBatchKMeansFit(8).fit(np.zeros((64, 32), np.float32), sample_weight=np.ones(64))
    with pytest.raises(ValueError):
        MiniBatchKMeansFit(8, init="kmeans")
    with pytest.raises(L2SError):
        MiniBatchKMeansFit(1)
    with pytest.raises(L2SError):                                # a host tensor: there is no CPU path
        MiniBatchKMeansFit(8).fit(torch.zeros(64, 32))
    if not torch.cuda.is_available():
        with pytest.raises(L2SError, match="no CPU path"):
            MiniBatchKMeansFit(8).fit(np.zeros((64, 32), np.float32))


def test_cli_argument_and_path_errors(tmp_path, capsys):
    from lip2speech_unit_amd import learn_kmeans
    d = str(tmp_path)
    np.save(tmp_path / "train_0_1.npy", np.zeros((4, 32), np.float32))
    (tmp_path / "train_0_1.len").write_text("4\n")
    (tmp_path / "h.pt").write_bytes(b"x")
    bad = (["feat", "train", "1"], [d, "train", "1", "km.bin"], [d, "train", "x", "km.bin", "8"], [d, "train", "1", "km.bin", "1"],
           [d, "train", "1", "km.bin", "2000"], [str(tmp_path / "missing"), "train", "1", "km.bin", "8"], [d, "valid", "1", "km.bin", "8"],
           [d, "train", "2", "km.bin", "8"], [d, "train", "0", "km.bin", "8"], [d, "train", "1", "km.bin", "8", "--percent", "1.5"],
           [d, "train", "1", "km.bin", "8", "--init", "zeros"], [d, "train", "1", "km.bin", "8", "--tol", "0.1"],
           [d, "train", "1", "km.bin", "8", "--reassignment_ratio", "0.01"], [d, "train", "1", "km.bin", "8", "--batch_size", "0"],
           [d, "train", "1", "km.bin", "8", "--hubert", str(tmp_path / "h.pt")],
           ["km.bin", "8", "--audio_root", d], ["km.bin", "8", "--audio_root", str(tmp_path / "missing"), "--hubert", str(tmp_path / "h.pt")],
           ["km.bin", "8", "--audio_root", d, "--hubert", str(tmp_path / "none.pt")],
           ["km.bin", "8", "--audio_root", d, "--hubert", str(tmp_path / "h.pt"), "--layer", "0"],
           ["km.bin", "8", "--audio_root", d, "--hubert", str(tmp_path / "h.pt"), "--dtype", "f64"],
           [d, "train", "1", "km.bin", "8", "--audio_root", d, "--hubert", str(tmp_path / "h.pt")])
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            learn_kmeans.main(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        learn_kmeans.main([d, "train", "1", "km.bin", "8", "--reassignment_ratio", "0.01"])
    assert "reassignment_ratio" in capsys.readouterr().err
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit) as e:
            learn_kmeans.main([d, "train", "1", str(tmp_path / "c.npy"), "2"])
        assert "no CPU path" in str(e.value.code)


def test_abi_entries_reject_bad_arguments_without_a_gpu():
    from lip2speech_unit_amd import _lib
    lib = _lib.load()
    assert lib.l2s_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.l2s_kmeans_nearest_workspace(10000) == 313 * 8 and lib.l2s_kmeans_nearest_workspace(0) == 0
    assert lib.l2s_kmeans_update_workspace(10000, 200) == (40 * 200 + 201 + 10000) * 4
    assert lib.l2s_kmeans_update_workspace(0, 200) == 0 == lib.l2s_kmeans_update_workspace(10, 1) == lib.l2s_kmeans_update_workspace((1 << 24) + 1, 8)
    assert lib.l2s_kmeans_pp_workspace(30000) == 469 * 16 * 8 and lib.l2s_kmeans_pp_workspace(0) == 0
    ok = dict(x=0x10000, ldx=768, N=100000, rows=0x20000, M=10000, cen=0x30000, cn=0x40000, D=768, K=200, ids=0x50000, dmin=0x60000,
              inertia=0x70000, ws=0x80000, wsb=313 * 8, stream=None)

    def near(**kw):
        a = dict(ok, **kw)
        return lib.l2s_kmeans_nearest(a["x"], a["ldx"], a["N"], a["rows"], a["M"], a["cen"], a["cn"], a["D"], a["K"], a["ids"], a["dmin"],
                                      a["inertia"], a["ws"], a["wsb"], a["stream"])
    for name in ("x", "cen", "cn", "ws"):
        assert near(**{name: None}) == -1, name
    assert near(ids=None, dmin=None, inertia=None) == -1
    assert near(M=0) == -2 and near(N=0) == -2 and near(ldx=767) == -2 and near(K=0) == -2 and near(wsb=8) == -2
    assert near(rows=None, N=9999) == -2
    assert near(D=40, ldx=40) == -4 and near(D=1056, ldx=1056) == -4 and near(K=1) == -4 and near(K=1025) == -4 and near(N=1 << 31) == -4
    assert near(x=0x10004) == -3 and near(cen=0x30008) == -3 and near(ldx=770) == -3 and near(ids=0x50002) == -3 and near(rows=0x20001) == -3
    assert near(inertia=0x70004) == -3 and near(ws=0x80004) == -3
    oku = dict(x=0x10000, ldx=768, N=100000, rows=0x20000, M=10000, ids=0x50000, cen=0x30000, w=0x40000, D=768, K=200, co=0x30000, wo=0x40000,
               cn=0x60000, ws=0x80000, wsb=(40 * 200 + 201 + 10000) * 4, stream=None)

    def upd(**kw):
        a = dict(oku, **kw)
        return lib.l2s_kmeans_update(a["x"], a["ldx"], a["N"], a["rows"], a["M"], a["ids"], a["cen"], a["w"], a["D"], a["K"], a["co"], a["wo"],
                                     a["cn"], a["ws"], a["wsb"], a["stream"])
    for name in ("x", "ids", "cen", "w", "co", "wo", "cn", "ws"):
        assert upd(**{name: None}) == -1, name
    assert upd(M=0) == -2 and upd(ldx=700) == -2 and upd(wsb=100) == -2 and upd(rows=None, N=5000) == -2
    assert upd(D=48, ldx=48) == -4 and upd(K=1) == -4 and upd(K=2048) == -4 and upd(M=(1 << 24) + 1, wsb=1 << 40) == -4
    assert upd(x=0x10008) == -3 and upd(co=0x30004) == -3 and upd(ids=0x50001) == -3 and upd(ws=0x80002) == -3
    okp = dict(x=0x10000, ldx=768, N=100000, rows=0x20000, m=30000, D=768, cand=0x30000, t=7, cl=0x40000, sel=None, pot=0x50000, out=None,
               chosen=None, ws=0x80000, wsb=469 * 16 * 8, stream=None)

    def pot(**kw):
        a = dict(okp, **kw)
        return lib.l2s_kmeans_pp_pot(a["x"], a["ldx"], a["N"], a["rows"], a["m"], a["D"], a["cand"], a["t"], a["cl"], a["sel"], a["pot"], a["out"],
                                     a["chosen"], a["ws"], a["wsb"], a["stream"])
    for name in ("x", "cand", "ws", "pot"):
        assert pot(**{name: None}) == -1, name
    assert pot(sel=0x90000) == -1                                # a selection without a closest_out to write
    assert pot(m=0) == -2 and pot(t=0) == -2 and pot(ldx=100) == -2 and pot(wsb=64) == -2 and pot(out=0x40000) == -2    # t = 7 and no select
    assert pot(t=17) == -4 and pot(D=100, ldx=100) == -4 and pot(D=2048, ldx=2048) == -4
    assert pot(x=0x10004) == -3 and pot(pot=0x50004) == -3 and pot(cl=0x40002) == -3 and pot(out=0x40002, sel=0x90000) == -3
    okk = dict(cl=0x40000, m=30000, u=0x50000, t=7, scale=0x60000, idx=0x70000, total=0x80000, stream=None)

    def pick(**kw):
        a = dict(okk, **kw)
        return lib.l2s_kmeans_pp_pick(a["cl"], a["m"], a["u"], a["t"], a["scale"], a["idx"], a["total"], a["stream"])
    for name in ("cl", "u", "idx"):
        assert pick(**{name: None}) == -1, name
    assert pick(m=0) == -2 and pick(t=-1) == -2 and pick(t=17) == -4 and pick(m=(1 << 24) + 1) == -4
    assert pick(cl=0x40002) == -3 and pick(u=0x50004) == -3 and pick(scale=0x60004) == -3 and pick(idx=0x70002) == -3 and pick(total=0x80004) == -3


def test_ops_schemas_and_fakes_exist():
    from lip2speech_unit_amd import ops
    for name in ("kmeans_nearest", "kmeans_update", "kmeans_pp_pot", "kmeans_pp_pick"):
        assert ops.ENTRY_OF[name] == "l2s_" + name and hasattr(torch.ops.lip2speech, name)
        schema = str(getattr(torch.ops.lip2speech, name).default._schema)
        assert schema.rstrip().endswith("-> ()") and "!" in schema
    for q in ("l2s_kmeans_nearest_workspace", "l2s_kmeans_update_workspace", "l2s_kmeans_pp_workspace"):
        assert q in ops.HOST_QUERIES
    assert ops.kmeans_nearest_workspace_bytes(64) == 16 and ops.kmeans_pp_workspace_bytes(65) == 256
    with pytest.raises(ops.L2SError):
        ops.kmeans_update_workspace_bytes(10, 1)
    with pytest.raises(ops.L2SError):                            # host tensors: there is no CPU path
        ops.kmeans_nearest(torch.zeros(4, 32), torch.zeros(2, 32), torch.zeros(2), M=4, D=32, K=2, ids=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ops.L2SError):
        ops.kmeans_pp_pick(torch.zeros(4), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), m=4, t=2)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x, c = torch.empty(64, 32, device="cuda"), torch.empty(4, 32, device="cuda")
        ids = torch.empty(64, device="cuda", dtype=torch.int32)
        w = torch.empty(4, device="cuda")
        ws = torch.empty(4096, device="cuda", dtype=torch.uint8)
        assert torch.ops.lip2speech.kmeans_nearest(x, c, w, M=64, D=32, K=4, ids=ids) is None
        assert torch.ops.lip2speech.kmeans_update(x, ids, c, w, c, w, torch.empty(4, device="cuda"), ws, M=64, D=32, K=4) is None
        assert torch.ops.lip2speech.kmeans_pp_pot(x, ids, ws, m=64, D=32, t=2, pot=torch.empty(2, device="cuda", dtype=torch.float64)) is None
        assert torch.ops.lip2speech.kmeans_pp_pick(torch.empty(64, device="cuda"), torch.empty(2, device="cuda", dtype=torch.float64), ids,
                                                   m=64, t=2) is None


def test_km_bin_round_trips(tmp_path):
    from lip2speech_unit_amd import kmeans_fit, speech_units
    rng = np.random.default_rng(0)
    cen = rng.standard_normal((9, 64)).astype(np.float32)
    fit = kmeans_fit.MiniBatchKMeansFit(9, max_iter=7, batch_size=50, n_init=2, max_no_improvement=5)
    fit.cluster_centers_, fit.n_steps_, fit.n_iter_, fit.counts_, fit.inertia_ = cen, 11, 3, np.arange(9, dtype=np.float32), 12.5
    kmeans_fit.save_kmeans(str(tmp_path / "centers.npy"), fit)
    assert np.array_equal(speech_units.load_kmeans(str(tmp_path / "centers.npy")), cen)
    pytest.importorskip("sklearn")
    joblib = pytest.importorskip("joblib")
    kmeans_fit.save_kmeans(str(tmp_path / "km.bin"), fit)
    got = speech_units.load_kmeans(str(tmp_path / "km.bin"))
    assert got.dtype == np.float32 and np.array_equal(got, cen)
    km = joblib.load(tmp_path / "km.bin")
    assert type(km).__name__ == "MiniBatchKMeans" and km.n_features_in_ == 64 and km.n_steps_ == 11 and km.n_iter_ == 3 and km._n_threads >= 1
    p = km.get_params()
    assert (p["n_clusters"], p["max_iter"], p["batch_size"], p["n_init"], p["max_no_improvement"], p["init"], p["compute_labels"],
            p["reassignment_ratio"], p["tol"], p["init_size"]) == (9, 7, 50, 2, 5, "k-means++", False, 0.0, 0.0, None)
    feat = rng.standard_normal((40, 64)).astype(np.float32)
    want = KR.assign(feat.astype(np.float64), cen.astype(np.float64))
    assert -km.score(feat) == pytest.approx(want[1].sum(), rel=1e-5) and np.array_equal(km.predict(feat), want[0])


def test_km_bin_without_sklearn_says_so(tmp_path, monkeypatch):
    import builtins
    from lip2speech_unit_amd import kmeans_fit
    real = builtins.__import__

    def no_sklearn(name, *a, **k):
        if name.split(".")[0] == "sklearn":
            raise ImportError("No module named 'sklearn'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_sklearn)
    fit = types.SimpleNamespace(cluster_centers_=np.zeros((2, 32), np.float32))
    with pytest.raises(kmeans_fit.L2SError, match="scikit-learn"):
        kmeans_fit.save_kmeans(str(tmp_path / "km.bin"), fit)
    kmeans_fit.save_kmeans(str(tmp_path / "c.npy"), fit)          # the centres alone need nothing
    assert np.load(tmp_path / "c.npy").shape == (2, 32)
