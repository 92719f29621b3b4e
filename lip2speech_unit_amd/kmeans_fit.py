"""Learn the speech-unit codebook on the device: scikit-learn's MiniBatchKMeans.fit as avhubert/clustering/learn_kmeans.py:25-47,
88-121 runs it (compute_labels=False, init_size=None, unit sample weights), on the kernels of csrc/kmeans_fit.hip.

All random numbers come from ONE host numpy RandomState, in scikit-learn's order, so a run is a function of (features, arguments,
seed) and consumes the stream exactly as the reference's fit does after its `--percent` draws:

  1. validation rows  randint(0, n, init_size);  init_size = 3 batch (3 K if that is under K), at most n
  2. per init         randint(0, n, init_size) if init_size < n (also for an array init);  greedy k-means++ on that subset: first centre choice(m, p=uniform),
                      then per centre uniform(size=2 + int(log K)) * pot -> searchsorted on cumsum(closest) -> the candidate of the
                      lowest potential;  the init of the lowest inertia on the validation rows wins (the first of equal ones)
  3. per step         randint(0, n, batch);  nearest centre;  c <- (c w + sum x) / (w + cnt), w += cnt for centres with members;
                      from the second step on the EWA of batch_inertia / batch (alpha = min(2 batch / (n + 1), 1)) stops the fit
                      after max_no_improvement steps without a new minimum
None of these draws depends on the data, so an init is queued without a host synchronisation (the candidate of the lowest
potential is picked on the device) and the step loop synchronises once per chunk of steps: indices are drawn and inertias read
back a chunk at a time, the EWA rule runs on the host, and a stop inside a chunk restores the chunk's starting centres and
replays to the stopping step - the kernels are deterministic, so that equals having stopped there.

Features that fit `device_budget_bytes` live on the device and batches are gathered inside the kernels (`rows`); larger sets
stay on the host (ndarray or memmap), batches are gathered into pinned memory and uploaded per step, through the same kernels
with rows = None.  There is no CPU path.
"""
import numpy as np
import torch

from . import ops
from ._lib import L2SError

DEVICE_BUDGET_BYTES = 32 << 30     # features up to this size are kept on the device
CHUNK_STEPS = 64                   # steps queued between two host synchronisations
MAX_BATCH = (1 << 24) // 3         # init_size = 3 batch rows go through one l2s_kmeans_pp_pick block (m <= 2^24)
SCORE_ROWS = 1 << 20               # rows per l2s_kmeans_nearest call of mean_min_distance


class EarlyStopping:
    """scikit-learn's mini-batch convergence rule (tol = 0) as a pure host function of the batch inertias:
    feed(step, batch_inertia) -> True when the fit ends after `step` (counted from 0)."""

    def __init__(self, n_samples, batch_size, max_no_improvement):
        self.n_samples, self.batch_size, self.max_no_improvement = int(n_samples), int(batch_size), max_no_improvement
        self.ewa = None
        self.ewa_min = None
        self.no_improvement = 0

    def feed(self, step, batch_inertia):
        v = float(batch_inertia) / self.batch_size
        if step == 0:
            return False
        if self.ewa is None:
            self.ewa = v
        else:
            alpha = min(self.batch_size * 2.0 / (self.n_samples + 1), 1)
            self.ewa = self.ewa * (1 - alpha) + v * alpha
        if self.ewa_min is None or self.ewa < self.ewa_min:
            self.no_improvement = 0
            self.ewa_min = self.ewa
        else:
            self.no_improvement += 1
        return self.max_no_improvement is not None and self.no_improvement >= self.max_no_improvement


def init_size_of(n, n_clusters, batch_size):
    s = 3 * min(batch_size, n)
    if s < n_clusters:
        s = 3 * n_clusters
    return min(s, n)


def _unit_p(m):
    """sample_weight / sample_weight.sum() for unit weights in the features' dtype (float32), as scikit-learn hands it to choice."""
    sw = np.ones(m, dtype=np.float32)
    return sw / sw.sum()


def _dev_bytes(n, dev):
    return torch.empty(max(int(n), 8), device=dev, dtype=torch.uint8)


class Features:
    """The feature matrix behind one interface: batch(idx) -> (x, rows, M) for the kernels.  fit() and mean_min_distance() build
    one from an array; a caller that needs both (learn_kmeans) builds it once and passes it to each, and owns its lifetime."""

    def __init__(self, feat, budget=DEVICE_BUDGET_BYTES):
        if isinstance(feat, torch.Tensor):
            if not feat.is_cuda:
                raise L2SError("kmeans_fit: a torch tensor must live on the device (host features are numpy arrays; there is no CPU path)")
            if feat.dtype != torch.float32 or feat.dim() != 2:
                raise ValueError("features: float32 [N, D]")
            self.dev, self.host = feat.contiguous(), None
        else:
            if not isinstance(feat, np.ndarray) or feat.ndim != 2 or feat.dtype != np.float32:
                raise ValueError("features: float32 [N, D] (ndarray, memmap or a device tensor)")
            if not torch.cuda.is_available():
                raise L2SError("kmeans_fit runs on the device only (there is no CPU path)")
            self.host, self.dev = feat, None
        self.n, self.D = (self.dev if self.dev is not None else self.host).shape
        self.device = self.dev.device if self.dev is not None else torch.device("cuda", torch.cuda.current_device())
        if self.dev is None and self.n * self.D * 4 <= budget and self.n < (1 << 31):
            self.dev = torch.empty(self.n, self.D, device=self.device, dtype=torch.float32)
            step = max(1, (256 << 20) // (4 * self.D))
            for a in range(0, self.n, step):
                self.dev[a:a + step].copy_(torch.from_numpy(np.ascontiguousarray(self.host[a:a + step])))
        if self.dev is not None and self.n >= (1 << 31):
            raise L2SError("kmeans_fit: device-resident features are indexed by int32 rows (N < 2^31)")
        self.resident = self.dev is not None
        self._pin, self._ev, self._turn, self._stage = None, None, 0, {}

    def rows_tensor(self, idx):
        """Row indices (host int array, any shape) -> int32 device tensor."""
        return torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)

    def gather(self, idx, tag):
        """Host-resident features: rows idx -> a device buffer (one per tag, reused), through two pinned staging buffers."""
        M = len(idx)
        if self._pin is None or self._pin[0].shape[0] < M:
            self._pin = [torch.empty(M, self.D, dtype=torch.float32).pin_memory() for _ in range(2)]
            self._ev = [None, None]
        t = self._turn
        self._turn ^= 1
        if self._ev[t] is not None:
            self._ev[t].synchronize()          # the upload that last used this staging buffer (not the kernels behind it)
        np.take(self.host, np.asarray(idx), axis=0, out=self._pin[t].numpy()[:M])
        buf = self._stage.get(tag)
        if buf is None or buf.shape[0] < M:
            buf = self._stage[tag] = torch.empty(M, self.D, device=self.device, dtype=torch.float32)
        buf[:M].copy_(self._pin[t][:M], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ev[t] = ev
        return buf

    def batch(self, idx, dev_rows=None, tag="batch"):
        """(x, rows, M) naming the rows idx: in place when resident (dev_rows: idx already on the device), else uploaded."""
        if self.resident:
            return self.dev, (dev_rows if dev_rows is not None else self.rows_tensor(idx)), len(idx)
        return self.gather(idx, tag), None, len(idx)

    def take(self, idx):
        """Rows idx as a new float32 device tensor (the init centres: K rows)."""
        if self.resident:
            return self.dev.index_select(0, torch.from_numpy(np.asarray(idx, dtype=np.int64)).to(self.device)).contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.take(self.host, np.asarray(idx), axis=0))).to(self.device)


def _cnorm(centers):
    return centers.double().pow(2).sum(1).float()       # |c|^2 rounded once, as speech_units.SpeechUnitExtractor holds it


def mean_min_distance(feat, centers, device_budget_bytes=DEVICE_BUDGET_BYTES):
    """-score(feat) / len(feat) of learn_kmeans.py:119: the mean squared distance to the nearest centre, through l2s_kmeans_nearest
    in blocks of rows (each block's sum is fixed-order fp64 on the device; the blocks are added in float64 on the host)."""
    F = feat if isinstance(feat, Features) else Features(feat, device_budget_bytes)
    cen = torch.as_tensor(np.asarray(centers, dtype=np.float32)).to(F.device).contiguous() if not isinstance(centers, torch.Tensor) else centers
    K, D = cen.shape
    cn = _cnorm(cen)
    nblk = (F.n + SCORE_ROWS - 1) // SCORE_ROWS
    out = torch.zeros(nblk, device=F.device, dtype=torch.float64)
    ws = _dev_bytes(ops.kmeans_nearest_workspace_bytes(min(SCORE_ROWS, F.n)), F.device)
    for b in range(nblk):
        a, e = b * SCORE_ROWS, min((b + 1) * SCORE_ROWS, F.n)
        x = F.dev[a:e] if F.resident else F.gather(np.arange(a, e), "score")
        ops.kmeans_nearest(x, cen, cn, M=e - a, D=D, K=K, inertia=out[b:b + 1], workspace=ws)
    return float(out.cpu().numpy().sum()) / F.n


class MiniBatchKMeansFit:
    """MiniBatchKMeans(...).fit(feat).cluster_centers_ on the device.  fit() returns the centres float32 [K, D] and sets n_steps_,
    n_iter_, counts_, inertia_ (EWA * n, as scikit-learn with compute_labels=False), init_indices_ (rows of feat the winning
    init chose; None for an array init), best_init_ and init_inertias_, n_samples_ and resident_ (whether the features lived on the
    device).  all_init_indices_ (the rows every init chose) and init_centers_ are kept as the record of the init phase: n_init * K
    indices and one [K, D] array."""

    def __init__(self, n_clusters, init="k-means++", max_iter=100, batch_size=10000, tol=0.0, max_no_improvement=100, n_init=20,
                 reassignment_ratio=0.0, seed=0, random_state=None, device_budget_bytes=DEVICE_BUDGET_BYTES, chunk_steps=CHUNK_STEPS):
        if reassignment_ratio > 0:
            raise NotImplementedError("reassignment_ratio > 0 (random reassignment of small clusters) is not built; the reference's default is 0")
        if tol > 0:
            raise NotImplementedError("tol > 0 (stopping on the centre movement) is not built; the reference's default is 0")
        if callable(init):
            raise NotImplementedError("a callable init is not built: pass 'k-means++', 'random' or a [K, D] array")
        if isinstance(init, str) and init not in ("k-means++", "random"):
            raise ValueError(f"init={init!r}: 'k-means++', 'random' or a [K, D] array")
        if reassignment_ratio < 0 or tol < 0 or max_iter < 1 or batch_size < 1 or n_init < 1 or chunk_steps < 1:
            raise ValueError("max_iter, batch_size, n_init, chunk_steps >= 1; tol, reassignment_ratio >= 0")
        if not 2 <= n_clusters <= 1024:
            raise L2SError(f"n_clusters={n_clusters}: the kernels serve 2 <= K <= 1024")
        self.n_clusters, self.init, self.max_iter, self.batch_size = int(n_clusters), init, int(max_iter), int(batch_size)
        self.tol, self.max_no_improvement, self.n_init, self.reassignment_ratio = tol, max_no_improvement, int(n_init), reassignment_ratio
        self.random_state = random_state if random_state is not None else np.random.RandomState(seed)
        self.device_budget_bytes, self.chunk_steps = device_budget_bytes, int(chunk_steps)

    # ---- init ------------------------------------------------------------------------------------------------------------
    def _kmeans_pp(self, F, sub, rs):
        """Queues one greedy k-means++ on the subset `sub` (host row indices); returns the chosen positions, int32 [K] on the device."""
        K, D, m, dev = self.n_clusters, F.D, len(sub), F.device
        trials = 2 + int(np.log(K))
        first = int(rs.choice(m, p=_unit_p(m)))
        u = torch.from_numpy(np.stack([rs.uniform(size=trials) for _ in range(K - 1)])).to(dev)          # float64 [K - 1, trials]
        x, rows, _ = F.batch(sub, tag="init")
        ws = _dev_bytes(ops.kmeans_pp_workspace_bytes(m), dev)
        closest = torch.empty(m, device=dev, dtype=torch.float32)
        chosen = torch.empty(K, device=dev, dtype=torch.int32)
        chosen[:1] = first
        cand = torch.empty(trials, device=dev, dtype=torch.int32)
        pots = torch.empty(trials, device=dev, dtype=torch.float64)
        pot = torch.empty(1, device=dev, dtype=torch.float64)
        ops.kmeans_pp_pot(x, chosen, ws, m=m, D=D, t=1, rows=rows, closest_out=closest, pot=pot)
        for c in range(1, K):
            ops.kmeans_pp_pick(closest, u[c - 1], cand, m=m, t=trials, scale=pot)
            ops.kmeans_pp_pot(x, cand, ws, m=m, D=D, t=trials, rows=rows, closest=closest, pot=pots)
            ops.kmeans_pp_pot(x, cand, ws, m=m, D=D, t=trials, rows=rows, closest=closest, select=pots, closest_out=closest, pot=pot,
                              chosen=chosen[c:c + 1])
        return chosen, (x, rows)

    def _inits(self, F, rs):
        K, D, n, dev = self.n_clusters, F.D, F.n, F.device
        isz = init_size_of(n, K, self.batch_size)
        valid = rs.randint(0, n, isz)
        array_init = not isinstance(self.init, str)
        n_init = 1 if array_init else self.n_init
        xv, rv, _ = F.batch(valid, tag="valid")
        inert = torch.zeros(n_init, device=dev, dtype=torch.float64)
        ws = _dev_bytes(ops.kmeans_nearest_workspace_bytes(isz), dev)
        cens, picks, subs = [], [], []
        for it in range(n_init):
            sub = rs.randint(0, n, isz) if isz < n else np.arange(n)       # scikit-learn draws the subset whatever the init is
            if array_init:
                c = np.ascontiguousarray(np.asarray(self.init), dtype=np.float32)
                if c.shape != (K, D):
                    raise ValueError(f"init: expected [{K}, {D}], got {c.shape}")
                cen, pos = torch.from_numpy(c).to(dev), None
            else:
                if self.init == "k-means++":
                    pos, (x, rows) = self._kmeans_pp(F, sub, rs)
                    at = pos.long() if rows is None else rows.index_select(0, pos.long()).long()
                    cen = x.index_select(0, at).contiguous()
                else:
                    pos = rs.choice(len(sub), size=K, replace=False, p=_unit_p(len(sub)))
                    cen = F.take(sub[pos])
            ops.kmeans_nearest(xv, cen, _cnorm(cen), M=isz, D=D, K=K, rows=rv, inertia=inert[it:it + 1], workspace=ws)
            cens.append(cen), picks.append(pos), subs.append(sub)
        inertias = inert.cpu().numpy()                   # the one synchronisation of the init phase
        best = int(np.argmin(inertias))                  # the first of equal ones, as a strict "<" keeps it
        pos = picks[best]
        if pos is not None:
            pos = pos.cpu().numpy().astype(np.int64) if isinstance(pos, torch.Tensor) else np.asarray(pos, dtype=np.int64)
        self.best_init_, self.init_inertias_ = best, inertias
        self.init_indices_ = None if pos is None else np.asarray(subs[best])[pos]
        self.all_init_indices_ = [None if p is None else np.asarray(s)[p.cpu().numpy().astype(np.int64) if isinstance(p, torch.Tensor) else p]
                                  for p, s in zip(picks, subs)]
        return cens[best].clone()

    # ---- steps -----------------------------------------------------------------------------------------------------------
    def fit(self, feat, sample_weight=None):
        if sample_weight is not None:
            raise NotImplementedError("sample_weight is not built: every frame weighs 1, as in the reference")
        F = feat if isinstance(feat, Features) else Features(feat, self.device_budget_bytes)
        K, D, n, dev = self.n_clusters, F.D, F.n, F.device
        if D % 32 or D > 1024:
            raise L2SError(f"kmeans_fit: D={D}; the kernels serve D a multiple of 32 up to 1024")
        if n < K:
            raise ValueError(f"n_samples={n} should be >= n_clusters={K}")
        batch = min(self.batch_size, n)
        if batch > MAX_BATCH:
            raise L2SError(f"kmeans_fit: batch_size={batch} is above {MAX_BATCH}")
        rs = self.random_state
        with torch.cuda.device(dev):
            cen = self._inits(F, rs)
            self.init_centers_ = cen.cpu().numpy()
            counts = torch.zeros(K, device=dev, dtype=torch.float32)
            cn = _cnorm(cen)
            n_steps = (self.max_iter * n) // batch
            stop = EarlyStopping(n, batch, self.max_no_improvement)
            ids = torch.empty(batch, device=dev, dtype=torch.int32)
            ws_n = _dev_bytes(ops.kmeans_nearest_workspace_bytes(batch), dev)
            ws_u = _dev_bytes(ops.kmeans_update_workspace_bytes(batch, K), dev)

            def run(idx_chunk, inert):
                dev_idx = F.rows_tensor(np.stack(idx_chunk)) if F.resident else None
                for s, idx in enumerate(idx_chunk):
                    x, rows, M = F.batch(idx, dev_rows=None if dev_idx is None else dev_idx[s])
                    ops.kmeans_nearest(x, cen, cn, M=M, D=D, K=K, rows=rows, ids=ids, inertia=inert[s:s + 1], workspace=ws_n)
                    ops.kmeans_update(x, ids, cen, counts, cen, counts, cn, ws_u, M=M, D=D, K=K, rows=rows)

            done, stopped = 0, False
            while done < n_steps and not stopped:
                S = min(self.chunk_steps, n_steps - done)
                idx_chunk = [rs.randint(0, n, batch) for _ in range(S)]
                saved = (cen.clone(), counts.clone(), cn.clone())
                inert = torch.zeros(S, device=dev, dtype=torch.float64)
                run(idx_chunk, inert)
                vals = inert.cpu().numpy()               # the chunk's one synchronisation
                for s in range(S):
                    if stop.feed(done + s, vals[s]):
                        stopped = True
                        if s + 1 < S:                    # overshot: back to the chunk's start, replay to the stopping step
                            cen.copy_(saved[0]), counts.copy_(saved[1]), cn.copy_(saved[2])
                            run(idx_chunk[:s + 1], torch.zeros(s + 1, device=dev, dtype=torch.float64))
                        done += s + 1
                        break
                else:
                    done += S
            self.cluster_centers_ = cen.cpu().numpy()
            self.counts_ = counts.cpu().numpy()
        self.n_steps_ = done
        self.n_iter_ = int(np.ceil((done * batch) / n))
        self.inertia_ = None if stop.ewa is None else stop.ewa * n
        self.n_features_in_ = D
        self.n_samples_, self.resident_ = n, F.resident        # the features themselves are not kept
        return self.cluster_centers_


def to_sklearn(fit, centers=None):
    """A scikit-learn MiniBatchKMeans carrying the fitted state, as learn_kmeans.py:117 dumps it (what ApplyKmeans.__init__ loads)."""
    try:
        from sklearn.cluster import MiniBatchKMeans
    except ImportError as e:
        raise L2SError("writing km.bin as a scikit-learn model needs scikit-learn, which is not importable here; "
                       "give a km_path ending in .npy to write the centres alone") from e
    init = fit.init if isinstance(fit.init, str) else np.asarray(fit.init)
    km = MiniBatchKMeans(n_clusters=fit.n_clusters, init=init, max_iter=fit.max_iter, batch_size=fit.batch_size, verbose=1,
                         compute_labels=False, tol=fit.tol, max_no_improvement=fit.max_no_improvement, init_size=None, n_init=fit.n_init,
                         reassignment_ratio=fit.reassignment_ratio)
    c = np.ascontiguousarray(fit.cluster_centers_ if centers is None else centers, dtype=np.float32)
    km.cluster_centers_ = c
    km.n_features_in_ = int(c.shape[1])
    km._n_features_out = int(c.shape[0])
    km.n_steps_ = int(getattr(fit, "n_steps_", 0))
    km.n_iter_ = int(getattr(fit, "n_iter_", 0))
    km._n_threads = 1
    if getattr(fit, "counts_", None) is not None:
        km._counts = np.asarray(fit.counts_, dtype=np.float32)
    if getattr(fit, "inertia_", None) is not None:
        km.inertia_ = float(fit.inertia_)
    return km


def save_kmeans(path, fit, centers=None):
    """km_path ending in .npy: the centres; anything else: a joblib dump of the scikit-learn model (learn_kmeans.py:117)."""
    c = np.ascontiguousarray(fit.cluster_centers_ if centers is None else centers, dtype=np.float32)
    if str(path).endswith(".npy"):
        np.save(path, c)
        return
    km = to_sklearn(fit, c)
    import joblib
    joblib.dump(km, path)
