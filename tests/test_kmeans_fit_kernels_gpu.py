"""The four device entries of the mini-batch k-means fit (csrc/kmeans_fit.hip) against float64 on the GPU:
l2s_kmeans_nearest, l2s_kmeans_update, l2s_kmeans_pp_pot, l2s_kmeans_pp_pick."""
import numpy as np
import pytest
import torch

from tests import _kmeans_fit_reference as KR
from tests import _units_reference as R
from lip2speech_unit_amd import ops

pytestmark = pytest.mark.gpu


def _bytes(n):
    return torch.empty(max(int(n), 8), device="cuda", dtype=torch.uint8)


def _cnorm(c):
    return torch.from_numpy(c).double().pow(2).sum(1).float()


def _case(D, K, M, seed=0, noise=0.25):
    """kmeans_case-style inputs in which EVERY row is a centre plus noise, so that float64 decides each row by a wide margin
    (kmeans_case's rows without a centre of their own see their two nearest centres at almost the same distance)."""
    rng = np.random.default_rng(1000 * D + K + seed)
    c = rng.standard_normal((K, D)).astype(np.float32)
    x = (c[rng.integers(0, K, M)] + noise * rng.standard_normal((M, D))).astype(np.float32)
    return x, c


def _nearest(x, c, rows=None, M=None):
    M = M if M is not None else (len(rows) if rows is not None else x.shape[0])
    D, K = c.shape[1], c.shape[0]
    cn = _cnorm(c)
    ids = torch.full((M,), -7, device="cuda", dtype=torch.int32)
    dmin = torch.full((M,), float("nan"), device="cuda")
    inertia = torch.full((1,), float("nan"), device="cuda", dtype=torch.float64)
    ops.kmeans_nearest(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda(), cn.cuda(), M=M, D=D, K=K,
                       rows=None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda(), ids=ids, dmin=dmin, inertia=inertia,
                       workspace=_bytes(ops.kmeans_nearest_workspace_bytes(M)))
    torch.cuda.synchronize()
    return ids.cpu(), dmin.cpu(), inertia.cpu(), cn


def _check_nearest(x, c, rows, tag):
    xb = x if rows is None else x[rows]
    M, K = xb.shape[0], c.shape[0]
    ids, dmin, inertia, cn = _nearest(x, c, rows)
    # float64 on the fp32 |c|^2 the kernel is handed
    xd = torch.from_numpy(xb).double()
    d = xd.pow(2).sum(1, keepdim=True) + cn.double()[None, :] - 2 * xd @ torch.from_numpy(c).double().t()
    two = d.topk(2, dim=1, largest=False)
    margin = (two.values[:, 1] - two.values[:, 0]) / (xd.pow(2).sum(1) + torch.from_numpy(c).double().pow(2).sum(1)[two.indices[:, 0]])
    mask = margin > 1e-4
    assert bool(mask.all()), f"{tag}: the float64 reference excuses {int((~mask).sum())} rows; choose other inputs"
    assert torch.equal(ids.long(), two.indices[:, 0])
    rel = ((dmin.double() - two.values[:, 0]).abs() / two.values[:, 0]).max().item()
    own = dmin.double().sum().item()
    irel = abs(inertia.item() - own) / own
    iref = abs(inertia.item() - two.values[:, 0].sum().item()) / own
    print(f"{tag}: {M} rows agree, dmin max rel err {rel:.2e}, inertia rel err against the float64 sum of dmin {irel:.1e}, "
          f"against the float64 distances {iref:.2e}")
    assert rel <= 1e-4
    # 1e-6 is the reduction's bound: the inertia is the fp64 sum of the fp32 dmin values the kernel wrote.  Against float64
    # distances it can be no closer than dmin itself (at M = 1 it is one dmin), so that comparison carries dmin's gate.
    assert irel <= 1e-6
    assert iref <= 1e-4
    ids2, dmin2, inertia2, _ = _nearest(x, c, rows)
    assert torch.equal(ids, ids2) and torch.equal(dmin, dmin2) and inertia.item() == inertia2.item()   # bit-identical


@pytest.mark.parametrize("D,K,M", [(32, 2, 1), (32, 2, 70), (768, 37, 130), (1024, 1000, 97)])
def test_nearest_against_float64(D, K, M):
    x, c = _case(D, K, M)
    _check_nearest(x, c, None, f"D={D} K={K} M={M}")


def test_nearest_through_rows_with_repeats_and_out_of_order_indices():
    x, c = _case(64, 200, 130)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 130, 300)                       # repeats, any order
    rows[:4] = (129, 0, 129, 7)
    assert len(np.unique(rows)) < 300 and bool((np.diff(rows) < 0).any())
    _check_nearest(x, c, rows, "D=64 K=200 M=300 via rows")
    # only the inertia, and only the ids
    cn = _cnorm(c).cuda()
    xd, cd, rd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(rows.astype(np.int32)).cuda()
    full = _nearest(x, c, rows)
    inertia = torch.zeros(1, device="cuda", dtype=torch.float64)
    ops.kmeans_nearest(xd, cd, cn, M=300, D=64, K=200, rows=rd, inertia=inertia, workspace=_bytes(ops.kmeans_nearest_workspace_bytes(300)))
    ids = torch.empty(300, device="cuda", dtype=torch.int32)
    ops.kmeans_nearest(xd, cd, cn, M=300, D=64, K=200, rows=rd, ids=ids)
    assert inertia.item() == full[2].item() and torch.equal(ids.cpu(), full[0])


def test_nearest_exact_tie_goes_to_the_lower_index():
    x, c = R.kmeans_case(64, 40)
    c[7], c[38] = c[3], c[3]                               # three identical centres, in two different waves' tiles
    ids, _, _, _ = _nearest(x, c)
    ref = R.kmeans_ids(x, c)
    near = ref == 3
    assert int(near.sum()) >= 1 and not bool(((ids == 7) | (ids == 38)).any())
    assert torch.equal(ids.long()[near], ref[near])
    x2, c2 = R.kmeans_case(32, 2)
    c2[1] = c2[0]
    assert bool((_nearest(x2, c2)[0] == 0).all())


# ---- update -----------------------------------------------------------------------------------------------------------------
def _update_case(name):
    rng = np.random.default_rng({"skew": 11, "wide_k": 12, "wide_d": 13}[name])
    if name == "skew":                                       # one centre holds 600 of 700 batch rows, one holds none; repeated rows
        D, K, N = 64, 16, 400
        c = (4.0 * rng.standard_normal((K, D))).astype(np.float32)
        c[5] = 60.0                                          # far from every row: stays empty
        x = np.empty((N, D), np.float32)
        x[:300] = c[3] + 0.5 * rng.standard_normal((300, D))
        lab = rng.permutation(np.r_[np.arange(K)[np.arange(K) != 5], rng.integers(0, 5, 100 - (K - 1))])
        x[300:] = c[lab] + 0.5 * rng.standard_normal((100, D))
        rows = np.r_[rng.integers(0, 300, 600), rng.integers(300, 400, 100)]
        rows = rows[rng.permutation(700)]
        counts = rng.integers(0, 50, K).astype(np.float32)
    elif name == "wide_k":
        D, K, N = 32, 1024, 1500
        x = rng.standard_normal((N, D)).astype(np.float32)
        c = (x[rng.permutation(N)[:K]] + 0.1 * rng.standard_normal((K, D))).astype(np.float32)
        rows = rng.integers(0, N, 2000)
        counts = rng.integers(0, 9, K).astype(np.float32)
    else:
        D, K, N = 1024, 2, 300
        x = rng.standard_normal((N, D)).astype(np.float32)
        c = (x[:2] + 0.1 * rng.standard_normal((2, D))).astype(np.float32)
        rows = None
        counts = np.array([3.0, 0.0], np.float32)
    return x, c, rows, counts


def _run_update(x, c, rows, counts, ids, in_place):
    M = len(rows) if rows is not None else x.shape[0]
    K, D = c.shape
    cd, wd = torch.from_numpy(c).cuda(), torch.from_numpy(counts).cuda()
    co, wo = (cd, wd) if in_place else (torch.full_like(cd, float("nan")), torch.full_like(wd, float("nan")))
    cn = torch.full((K,), float("nan"), device="cuda")
    ops.kmeans_update(torch.from_numpy(x).cuda(), ids.cuda(), cd, wd, co, wo, cn, _bytes(ops.kmeans_update_workspace_bytes(M, K)), M=M, D=D,
                      K=K, rows=None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    return co.cpu().numpy(), wo.cpu().numpy(), cn.cpu().numpy()


@pytest.mark.parametrize("name", ["skew", "wide_k", "wide_d"])
def test_update_against_float64_fed_the_devices_ids(name):
    x, c, rows, counts = _update_case(name)
    ids = _nearest(x, c, rows)[0]
    lab = ids.numpy().astype(np.int64)
    xb = x if rows is None else x[rows]
    K = c.shape[0]
    cnt = np.bincount(lab, minlength=K)
    if name == "skew":
        assert cnt.max() >= 600 and cnt[5] == 0 and len(np.unique(rows)) < len(rows) and counts.max() > 0
    new, w, cn = _run_update(x, c, rows, counts, ids, in_place=False)
    ref_c, ref_w = c.astype(np.float64), counts.astype(np.float64)
    KR.update(ref_c, ref_w, xb.astype(np.float64), lab)
    f32_c, f32_w = c.copy(), counts.copy()
    KR.update(f32_c, f32_w, xb, lab)                         # the same update in numpy float32: the yardstick
    err, yard = np.abs(new - ref_c).max(), np.abs(f32_c.astype(np.float64) - ref_c).max()
    print(f"{name}: centre max abs err {err:.3e}, numpy float32 {yard:.3e}, {int((cnt == 0).sum())} empty, largest cluster {cnt.max()}")
    assert err <= 4.0 * yard
    assert np.array_equal(w, (counts.astype(np.float64) + cnt).astype(np.float32))
    empty = cnt == 0
    assert np.array_equal(new[empty], c[empty]) and np.array_equal(w[empty], counts[empty])       # untouched, to the bit
    cn_ref = (new.astype(np.float64) ** 2).sum(1)
    assert (np.abs(cn - cn_ref) / cn_ref).max() <= 1.2e-7    # |c|^2 of the NEW centres, summed in fp64 and rounded once (2 ulp)
    again = _run_update(x, c, rows, counts, ids, in_place=True)  # in place, and bit-identical from run to run
    assert all(np.array_equal(a, b) for a, b in zip(again, (new, w, cn)))


# ---- k-means++ --------------------------------------------------------------------------------------------------------------
def _pp(x, cand, closest, rows=None, select=None, write=False):
    m = len(rows) if rows is not None else x.shape[0]
    D, t = x.shape[1], len(cand)
    ws = _bytes(ops.kmeans_pp_workspace_bytes(m))
    xd = torch.from_numpy(x).cuda()
    rd = None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda()
    cd = torch.from_numpy(np.asarray(cand, dtype=np.int32)).cuda()
    cl = None if closest is None else torch.from_numpy(closest).cuda()
    if not write:
        pot = torch.full((t,), float("nan"), device="cuda", dtype=torch.float64)
        ops.kmeans_pp_pot(xd, cd, ws, m=m, D=D, t=t, rows=rd, closest=cl, pot=pot)
        return pot.cpu().numpy()
    out = torch.full((m,), float("nan"), device="cuda")
    pot = torch.full((1,), float("nan"), device="cuda", dtype=torch.float64)
    chosen = torch.full((1,), -1, device="cuda", dtype=torch.int32)
    ops.kmeans_pp_pot(xd, cd, ws, m=m, D=D, t=t, rows=rd, closest=cl, select=None if select is None else torch.from_numpy(select).cuda(),
                      closest_out=out, pot=pot, chosen=chosen if select is not None else None)
    return out.cpu().numpy(), pot.item(), chosen.item()


def test_pp_pot_real_valued_against_float64():
    rng = np.random.default_rng(21)
    N, D, m, t = 400, 96, 300, 7
    x = rng.standard_normal((N, D)).astype(np.float32)
    rows = rng.integers(0, N, m)
    cand = rng.integers(0, m, t)
    closest = (4.0 * D * rng.random(m)).astype(np.float32)   # uniform about E|a - b|^2 = 2 D of two normal rows: about half fall below it
    xs = x[rows]
    d64 = KR.sq_dists(xs.astype(np.float64), xs[cand].astype(np.float64))
    d32 = KR.sq_dists(xs, xs[cand])                          # numpy float32 throughout: the yardstick
    ref = np.minimum(closest.astype(np.float64)[:, None], d64)
    y32 = np.minimum(closest[:, None], d32)
    assert 0.2 < (d64 < closest[:, None]).mean() < 0.8       # both arms of the min are taken
    pot = _pp(x, cand, closest, rows)
    err = (np.abs(pot - ref.sum(0)) / ref.sum(0)).max()
    yard = (np.abs(y32.sum(0, dtype=np.float32).astype(np.float64) - ref.sum(0)) / ref.sum(0)).max()
    print(f"pp_pot: potentials max rel err {err:.2e}, numpy float32 {yard:.2e}")
    assert err <= 4.0 * yard
    assert np.array_equal(pot, _pp(x, cand, closest, rows))  # bit-identical
    # second mode: the new closest of the candidate with the lowest potential, picked on the device
    out, p1, chosen = _pp(x, cand, closest, rows, select=pot, write=True)
    best = int(np.argmin(pot))
    assert chosen == cand[best] and p1 == pot[best]
    rb, pos = ref[:, best], ref[:, best] > 0                  # the candidate's own row (and its repeats in rows) is at distance 0
    e2, y2 = (np.abs(out - rb)[pos] / rb[pos]).max(), (np.abs(y32[:, best].astype(np.float64) - rb)[pos] / rb[pos]).max()
    print(f"pp_pot: closest_out max rel err {e2:.2e}, numpy float32 {y2:.2e}")
    assert e2 <= 4.0 * y2
    assert not pos.all() and np.array_equal(out[~pos], np.zeros((~pos).sum(), np.float32))      # differences of equal rows: exactly 0
    # one candidate against closest = +inf: the first centre's distances
    first, p0, _ = _pp(x, cand[:1], None, rows, write=True)
    assert (np.abs(first - d64[:, 0]) / np.maximum(d64[:, 0], 1e-30))[d64[:, 0] > 0].max() <= 4.0 * \
        (np.abs(d32[:, 0].astype(np.float64) - d64[:, 0]) / np.maximum(d64[:, 0], 1e-30))[d64[:, 0] > 0].max()
    assert first[cand[0]] == 0.0 and abs(p0 - first.astype(np.float64).sum()) <= 1e-12 * p0


@pytest.mark.parametrize("D,t,m,lim", [(64, 7, 333, 8), (1024, 16, 200, 3)])
def test_pp_pot_is_exact_on_integer_valued_data(D, t, m, lim):
    rng = np.random.default_rng(22 + D)
    x = rng.integers(-lim, lim + 1, (m, D)).astype(np.float32)
    cand = rng.integers(0, m, t)
    cand[-1] = cand[0]                                        # a repeated candidate
    d = KR.sq_dists(x.astype(np.float64), x[cand].astype(np.float64))
    closest = rng.integers(0, int(d.max()) + 1, m).astype(np.float32)
    ref = np.minimum(closest.astype(np.float64)[:, None], d)
    assert ref.sum(0).max() < 2 ** 24
    pot = _pp(x, cand, closest)
    assert np.array_equal(pot, ref.sum(0))
    out, p1, chosen = _pp(x, cand, closest, select=pot, write=True)
    best = int(np.argmin(ref.sum(0)))                          # the first of equal potentials
    assert chosen == cand[best] and p1 == ref.sum(0)[best] and np.array_equal(out, ref[:, best].astype(np.float32))
    first, p0, _ = _pp(x, cand[2:3], None, write=True)
    assert np.array_equal(first, d[:, 2].astype(np.float32)) and p0 == d[:, 2].sum()


@pytest.mark.parametrize("m", [1, 1023, 1024, 1025, 30000])
def test_pp_pick_is_searchsorted_left_on_the_float64_prefix(m):
    rng = np.random.default_rng(m)
    closest = rng.integers(0, 100, m).astype(np.float32)
    closest[rng.random(m) < 0.2] = 0.0                       # runs of equal prefixes: side = left picks the first
    if m > 1:
        closest[0] = 3.0
    else:
        closest[0] = 5.0
    prefix = np.cumsum(closest.astype(np.float64))
    total = prefix[-1]
    at = rng.integers(0, m, 5)
    thr = np.r_[prefix[at], prefix[at] + 0.5, 0.0, total, total + 1.0, 0.25]          # on a prefix, just above, 0, the total, beyond
    want = np.clip(np.searchsorted(prefix, thr, side="left"), None, m - 1)
    cd = torch.from_numpy(closest).cuda()
    got, tot = [], torch.zeros(1, device="cuda", dtype=torch.float64)
    for a in range(0, len(thr), 16):
        part = thr[a:a + 16]
        idx = torch.full((len(part),), -1, device="cuda", dtype=torch.int32)
        ops.kmeans_pp_pick(cd, torch.from_numpy(part).cuda(), idx, m=m, t=len(part), total=tot)
        got.append(idx.cpu().numpy())
    assert np.array_equal(np.concatenate(got), want), (np.concatenate(got), want)
    assert tot.item() == total
    # thresholds as fractions of a potential held on the device
    idx = torch.full((6,), -1, device="cuda", dtype=torch.int32)
    ops.kmeans_pp_pick(cd, torch.from_numpy(thr[:6] / 4.0).cuda(), idx, m=m, t=6, scale=torch.tensor([4.0], device="cuda", dtype=torch.float64))
    assert np.array_equal(idx.cpu().numpy(), want[:6])
