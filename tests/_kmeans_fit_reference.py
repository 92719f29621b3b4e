"""Float64 restatement of scikit-learn's MiniBatchKMeans.fit as avhubert/clustering/learn_kmeans.py:25-47,88-121 uses it
(compute_labels=False, init_size=None, reassignment_ratio=0, tol=0, unit sample weights), written from scikit-learn's observable
behaviour: one numpy RandomState consumed in scikit-learn's order.  Besides the result it reports the smallest margins any
decision of the run was taken by, so that a test can tell whether a lower-precision run is bound to decide alike.

  validation rows  randint(0, n, init_size);  init_size = 3 batch (3 K if that is under K), at most n
  per init         randint(0, n, init_size) (only if init_size < n), greedy k-means++ on that subset, inertia on the validation rows
  per step         randint(0, n, batch);  assign;  c <- (c w + sum x) / (w + cnt);  EWA early stopping from the second step on
"""
import numpy as np

INF = float("inf")


def sq_dists(a, b):
    """|a_i - b_j|^2 [len(a), len(b)] by direct differences (no cancellation), in the arrays' own precision."""
    out = np.empty((a.shape[0], b.shape[0]), dtype=a.dtype)
    for j in range(b.shape[0]):
        d = a - b[j]
        out[:, j] = np.einsum("ij,ij->i", d, d)
    return out


def assign(x, centers):
    """(labels, dmin, relative gap between the best and the second-best distance of the closest call)."""
    d = sq_dists(x, centers)
    lab = d.argmin(1)
    two = np.partition(d, 1, axis=1)[:, :2]
    scale = np.maximum(two[:, 1], np.finfo(d.dtype).tiny)
    return lab, d[np.arange(len(x)), lab], float(((two[:, 1] - two[:, 0]) / scale).min())


class Margins:
    def __init__(self):
        self.assign = INF        # (second - best) / second of any assignment
        self.draw = INF          # distance of a k-means++ draw from a prefix boundary, relative to the potential
        self.candidate = INF     # (second - best) / second over the distinct candidate potentials of a k-means++ round
        self.init = INF          # (second - best) / second over the init inertias
        self.ewa = INF           # |ewa - ewa_min| / ewa_min at any comparison of the two

    def as_dict(self):
        return dict(vars(self))


def unit_p(m, dtype):
    """sample_weight / sample_weight.sum() of unit weights held in the features' dtype, as scikit-learn forms it."""
    sw = np.ones(m, dtype=dtype)
    return sw / sw.sum()


def kmeans_pp(x, K, rs, mg, p_dtype):
    """Greedy k-means++ on x [m, D]: returns the chosen positions [K]."""
    m = x.shape[0]
    trials = 2 + int(np.log(K))
    idx = np.empty(K, dtype=np.int64)
    idx[0] = rs.choice(m, p=unit_p(m, p_dtype))
    closest = sq_dists(x, x[idx[:1]])[:, 0]
    pot = closest.sum()
    for c in range(1, K):
        draws = rs.uniform(size=trials) * pot
        prefix = np.cumsum(closest.astype(np.float64))
        cand = np.searchsorted(prefix, draws)
        np.clip(cand, None, m - 1, out=cand)
        if pot > 0:
            mg.draw = min(mg.draw, float(np.abs(prefix[None, :] - draws[:, None]).min() / pot))
        dist = np.minimum(closest[:, None], sq_dists(x, x[cand]))
        pots = dist.sum(0)
        best = int(np.argmin(pots))
        distinct = np.unique(pots[np.unique(cand, return_index=True)[1]])
        if len(distinct) > 1 and distinct[1] > 0:
            mg.candidate = min(mg.candidate, float((distinct[1] - distinct[0]) / distinct[1]))
        idx[c], closest, pot = cand[best], dist[:, best], pots[best]
    return idx


def update(centers, counts, xb, lab):
    """One centre update in place, in the arrays' own precision: members added in ascending batch position."""
    for k in np.unique(lab):
        rows = xb[lab == k]
        acc = centers[k] * counts[k]
        for r in rows:
            acc = acc + r
        counts[k] = counts[k] + centers.dtype.type(len(rows))
        centers[k] = acc * (centers.dtype.type(1) / counts[k])


class EarlyStop:
    """The EWA rule of a fit: feed(step, batch_inertia) -> True when the fit stops after that step (steps count from 0)."""

    def __init__(self, n, batch, max_no_improvement, mg=None):
        self.n, self.batch, self.max_no_improvement = n, batch, max_no_improvement
        self.ewa = self.ewa_min = None
        self.no_improvement = 0
        self.mg = mg

    def feed(self, step, batch_inertia):
        v = batch_inertia / self.batch
        if step == 0:
            return False
        if self.ewa is None:
            self.ewa = v
        else:
            alpha = min(self.batch * 2.0 / (self.n + 1), 1)
            self.ewa = self.ewa * (1 - alpha) + v * alpha
        if self.ewa_min is not None and self.mg is not None and self.ewa_min > 0:
            self.mg.ewa = min(self.mg.ewa, abs(self.ewa - self.ewa_min) / self.ewa_min)
        if self.ewa_min is None or self.ewa < self.ewa_min:
            self.no_improvement = 0
            self.ewa_min = self.ewa
        else:
            self.no_improvement += 1
        return self.max_no_improvement is not None and self.no_improvement >= self.max_no_improvement


def step_loop(X, centers, batches, max_no_improvement, dtype=np.float64, mg=None, batch_size=None):
    """The step loop over explicit batches (index arrays) in `dtype`; returns (centers, counts, n_steps, ewa)."""
    X = np.asarray(X)
    c = np.array(centers, dtype=dtype)
    counts = np.zeros(len(c), dtype=dtype)
    stop = EarlyStop(X.shape[0], batch_size or len(batches[0]), max_no_improvement, mg)
    done = 0
    for i, b in enumerate(batches):
        xb = X[b].astype(dtype)
        lab, dmin, gap = assign(xb, c)
        if mg is not None:
            mg.assign = min(mg.assign, gap)
        update(c, counts, xb, lab)
        done = i + 1
        if stop.feed(i, float(dmin.astype(np.float64).sum())):
            break
    return c, counts, done, stop.ewa


def fit(X, n_clusters, *, seed=0, random_state=None, init="k-means++", max_iter=100, batch_size=1024, max_no_improvement=10, n_init=3,
        p_dtype=None):
    """Returns a dict: centers float64 [K, D], init_indices (rows of X, None for an array init), best_init, init_inertias, batches,
    n_steps, n_iter, counts, inertia (EWA * n), init_centers, margins."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    rs = random_state if random_state is not None else np.random.RandomState(seed)
    p_dtype = p_dtype or np.float64
    mg = Margins()
    K = n_clusters
    batch = min(batch_size, n)
    init_size = 3 * batch
    if init_size < K:
        init_size = 3 * K
    init_size = min(init_size, n)
    array_init = not isinstance(init, str)
    if array_init:
        n_init = 1
    valid = rs.randint(0, n, init_size)
    best = None
    inertias, all_idx = [], []
    for it in range(n_init):
        sub = rs.randint(0, n, init_size) if init_size < n else np.arange(n)     # drawn whatever the init is
        if array_init:
            cen, rows = np.array(init, dtype=np.float64), None
        else:
            xs = X[sub]
            if init == "k-means++":
                pos = kmeans_pp(xs, K, rs, mg, p_dtype)
            elif init == "random":
                pos = rs.choice(len(xs), size=K, replace=False, p=unit_p(len(xs), p_dtype))
            else:
                raise ValueError(init)
            rows = sub[pos]
            cen = X[rows].copy()
        lab, dmin, gap = assign(X[valid], cen)
        mg.assign = min(mg.assign, gap)
        inertias.append(float(dmin.sum()))
        all_idx.append(rows)
        if best is None or inertias[-1] < inertias[best]:
            best = it
            best_cen = cen
    if len(inertias) > 1:
        s = np.unique(inertias)
        if len(s) > 1:
            mg.init = float((s[1] - s[0]) / s[1])
    n_steps = (max_iter * n) // batch
    c = best_cen.copy()
    counts = np.zeros(K)
    stop = EarlyStop(n, batch, max_no_improvement, mg)
    batches = []
    done = 0
    for i in range(n_steps):
        b = rs.randint(0, n, batch)
        batches.append(b)
        lab, dmin, gap = assign(X[b], c)
        mg.assign = min(mg.assign, gap)
        update(c, counts, X[b], lab)
        done = i + 1
        if stop.feed(i, float(dmin.sum())):
            break
    return {"centers": c, "init_indices": all_idx[best], "all_init_indices": all_idx, "best_init": best, "init_inertias": inertias,
            "init_centers": best_cen, "batches": batches, "n_steps": done, "n_iter": int(np.ceil(done * batch / n)), "counts": counts,
            "inertia": (stop.ewa * n) if stop.ewa is not None else None, "margins": mg.as_dict(), "total_steps": n_steps}
