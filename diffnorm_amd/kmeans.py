"""Learning the unit quantizer on the device: sklearn.cluster.MiniBatchKMeans as the reference's
examples/textless_nlp/gslm/speech2unit/clustering/cluster_kmeans.py (and examples/hubert/simple_kmeans/learn_kmeans.py) runs it.

One mini-batch step is dn_kmeans_assign -> dn_kmeans_accumulate -> dn_kmeans_update (csrc/kmeans.hip); k-means++ seeding takes its
distances and potentials from dn_kmeans_min_dist.  What stays on the host is bookkeeping: the seeded generators (batch indices,
k-means++ draws, reassignment rows), the early-stop rule and the reassignment decision (MiniBatchSchedule, reassign_decision: plain
numpy, testable without a device).

Equal to scikit-learn: the update rule (in double, rounded once, where scikit-learn runs it in the data's fp32), the loop's step
count, its early-stop rule and its reassignment rule.  Not equal: the trajectory of fit() from a seed -- scikit-learn consumes its
generator in ways that are internal to it (n_init trials on a validation subset among them); sparse input and sample weights are
not taken."""
import math
import random
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, data
from .hubert import KMeansQuantizer, kmeans_scores_tables

__all__ = ["KMeansTrainer", "MiniBatchSchedule", "reassign_decision", "sample_manifest", "learn_kmeans", "accumulate", "update", "min_dist"]

MAX_CANDIDATES = 16
SCORE_CHUNK = 65536


# ---------------------------------------------------------------- host bookkeeping (no device)
class MiniBatchSchedule:
    """The loop of MiniBatchKMeans.fit around its step: n_steps = max_iter * n_samples // batch_size, batch indices from a seeded
    generator, the exponentially weighted average of the batch inertia with max_no_improvement (_mini_batch_convergence) and the
    steps at which low-count centres are reassigned (_random_reassign)."""

    def __init__(self, n_samples: int, n_clusters: int, batch_size: int = 10000, max_iter: int = 150, seed: int = 1369, tol: float = 0.0,
                 max_no_improvement: Optional[int] = 100):
        if n_samples < n_clusters:
            raise ValueError(f"n_samples={n_samples} should be >= n_clusters={n_clusters}")
        self.n_samples, self.n_clusters = int(n_samples), int(n_clusters)
        self.batch_size = min(int(batch_size), self.n_samples)
        self.n_steps = (int(max_iter) * self.n_samples) // self.batch_size
        self.rng = np.random.RandomState(seed)
        self.tol, self.max_no_improvement = float(tol), max_no_improvement
        self.ewa_inertia = self.ewa_inertia_min = None
        self.no_improvement = 0
        self.n_since_last_reassign = 0

    @property
    def monitors(self) -> bool:
        """Whether converged() can ever say yes (else the loop never needs the batch inertia on the host)."""
        return self.tol > 0.0 or self.max_no_improvement is not None

    def next_batch(self) -> np.ndarray:
        return self.rng.randint(0, self.n_samples, self.batch_size)

    def random_reassign(self, any_zero_count: bool) -> bool:
        self.n_since_last_reassign += self.batch_size
        if any_zero_count or self.n_since_last_reassign >= 10 * self.n_clusters:
            self.n_since_last_reassign = 0
            return True
        return False

    def reassign_due(self) -> bool:
        """Whether the next random_reassign() says yes whatever the counts are (so they need not be looked at to know)."""
        return self.n_since_last_reassign + self.batch_size >= 10 * self.n_clusters

    def converged(self, step: int, batch_inertia: float, centers_squared_diff: float = 0.0) -> bool:
        """step: 0-based index of the step that just ran; batch_inertia: its summed inertia."""
        batch_inertia = batch_inertia / self.batch_size
        if step + 1 == 1:  # the first step's inertia comes from the initial centres: ignored
            return False
        if self.ewa_inertia is None:
            self.ewa_inertia = batch_inertia
        else:
            alpha = min(self.batch_size * 2.0 / (self.n_samples + 1), 1.0)
            self.ewa_inertia = self.ewa_inertia * (1 - alpha) + batch_inertia * alpha
        if self.tol > 0.0 and centers_squared_diff <= self.tol:
            return True
        if self.ewa_inertia_min is None or self.ewa_inertia < self.ewa_inertia_min:
            self.no_improvement = 0
            self.ewa_inertia_min = self.ewa_inertia
        else:
            self.no_improvement += 1
        return self.max_no_improvement is not None and self.no_improvement >= self.max_no_improvement


def reassign_decision(weight_sums: np.ndarray, reassignment_ratio: float, batch_rows: int, rng: np.random.RandomState):
    """scikit-learn's low-count reassignment (_mini_batch_step): clusters whose weight is under ratio * max, at most half the batch
    of them (the lowest weights first); -> (cluster indices, batch rows that replace them, the weight they all get) or None."""
    weight_sums = np.asarray(weight_sums, dtype=np.float64)
    to_reassign = weight_sums < reassignment_ratio * weight_sums.max()
    if to_reassign.sum() > 0.5 * batch_rows:
        keep = np.argsort(weight_sums)[int(0.5 * batch_rows):]
        to_reassign[keep] = False
    n = int(to_reassign.sum())
    if n == 0:
        return None
    rows = rng.choice(batch_rows, replace=False, size=n)
    return np.flatnonzero(to_reassign), rows, float(weight_sums[~to_reassign].min())


def sample_manifest(manifest_path: str, sample_pct: float = 1.0, seed: int = 0) -> List[str]:
    """The feature files of a manifest dump_features wrote, sampled as gslm/speech2unit/pretrained/utils.py samples its utterances:
    random.sample(paths, int(sample_pct * len(paths))) when sample_pct < 1, from a generator of its own seeded here."""
    paths = [p for p, _ in data.read_feature_manifest(manifest_path).values()]
    if sample_pct < 1.0:
        paths = random.Random(seed).sample(paths, int(sample_pct * len(paths)))
    return paths


class _HostRows:
    """Rows of a host array, or of the [T_i, D] arrays of a list of .npy paths laid end to end (memory-mapped), gathered by index."""

    def __init__(self, source):
        if isinstance(source, (list, tuple)):
            self.parts = [np.load(p, mmap_mode="r") if isinstance(p, str) else np.asarray(p) for p in source]
        else:
            self.parts = [np.asarray(source)]
        if not self.parts or any(p.ndim != 2 or p.shape[1] != self.parts[0].shape[1] for p in self.parts):
            raise ValueError("features must be [M, D] arrays of one width")
        self.offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in self.parts])]).astype(np.int64)
        self.shape = (int(self.offsets[-1]), int(self.parts[0].shape[1]))

    def gather(self, idx: np.ndarray, out: np.ndarray) -> None:
        if len(self.parts) == 1:
            out[:] = self.parts[0][idx]
            return
        part = np.searchsorted(self.offsets, idx, side="right") - 1
        for p in np.unique(part):
            sel = np.flatnonzero(part == p)
            out[sel] = self.parts[p][idx[sel] - self.offsets[p]]


# ---------------------------------------------------------------- bindings of the three kernels
def _check_feats(feats: torch.Tensor, who: str) -> Tuple[int, int]:
    if feats.dim() != 2 or feats.dtype != torch.float32 or not feats.is_contiguous() or not feats.is_cuda:
        raise ValueError(f"{who}: feats must be a contiguous fp32 [M, D] device tensor")
    M, D = feats.shape
    if D % 32:
        raise ValueError(f"{who}: feature width {D} must be a multiple of 32")
    return M, D


def workspace_bytes(M: int, n: int) -> int:
    return int(_lib.load().dn_kmeans_workspace_bytes_train(M, n))


def accumulate(feats: torch.Tensor, labels: torch.Tensor, centers: torch.Tensor, n: int, workspace: Optional[torch.Tensor] = None,
               check_labels: bool = True, out=None):
    """dn_kmeans_accumulate: -> (sums double [n, D], counts int32 [n], inertia double [1]).  centers: the packed fp32 matrix of
    kmeans_scores_tables.  check_labels: refuse labels outside [0, n) here, on the host (one synchronisation; partial_fit, whose
    labels come from dn_kmeans_assign, skips it)."""
    lib = _lib.load()
    M, D = _check_feats(feats, "accumulate")
    if labels.dtype != torch.int32 or labels.shape != (M,) or not labels.is_contiguous():
        raise ValueError("accumulate: labels must be a contiguous int32 [M] tensor")
    if check_labels and M and bool(((labels < 0) | (labels >= n)).any().item()):
        raise ValueError(f"accumulate: a label lies outside [0, {n})")
    dev = feats.device
    sums, counts, inertia = out or (torch.empty(n, D, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                                    torch.empty(1, dtype=torch.float64, device=dev))
    if workspace is None:
        workspace = _lib.alloc_workspace(workspace_bytes(M, n), dev)
    wp, nb = _lib.aligned(workspace)
    with torch.cuda.device(dev):
        _lib.check(lib.dn_kmeans_accumulate(feats.data_ptr(), labels.data_ptr(), centers.data_ptr(), M, D, n, sums.data_ptr(), counts.data_ptr(),
                                            inertia.data_ptr(), wp, nb, _lib.current_stream()), "dn_kmeans_accumulate")
    return sums, counts, inertia


def update(centers: torch.Tensor, half_norm: torch.Tensor, weight_sums: torch.Tensor, sums: torch.Tensor, counts: torch.Tensor, n: int) -> None:
    """dn_kmeans_update, in place on centers (packed, [n -> 128, D]), half_norm [n -> 4] and weight_sums double [n]."""
    D = centers.shape[1]
    assert centers.dtype == torch.float32 and half_norm.dtype == torch.float32 and weight_sums.dtype == torch.float64 and sums.dtype == torch.float64
    assert counts.dtype == torch.int32 and centers.shape[0] >= n and half_norm.numel() >= n and weight_sums.numel() >= n and sums.shape == (n, D)
    with torch.cuda.device(centers.device):
        _lib.check(_lib.load().dn_kmeans_update(centers.data_ptr(), half_norm.data_ptr(), weight_sums.data_ptr(), sums.data_ptr(), counts.data_ptr(), n, D,
                                                _lib.current_stream()), "dn_kmeans_update")


def min_dist(feats: torch.Tensor, cands: torch.Tensor, mind2: torch.Tensor, commit: int = -1, pot: Optional[torch.Tensor] = None,
             workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dn_kmeans_min_dist: -> pot double [k], pot[j] = sum_m min(mind2[m], |x_m - cands[j]|^2); commit >= 0 also lowers mind2 by
    that candidate's distances."""
    M, D = _check_feats(feats, "min_dist")
    k = cands.shape[0]
    if cands.dtype != torch.float32 or cands.shape != (k, D) or not cands.is_contiguous() or not 1 <= k <= MAX_CANDIDATES:
        raise ValueError(f"min_dist: cands must be a contiguous fp32 [k <= {MAX_CANDIDATES}, {D}] tensor")
    assert mind2.dtype == torch.float32 and mind2.shape == (M,) and mind2.is_contiguous()
    dev = feats.device
    pot = torch.empty(k, dtype=torch.float64, device=dev) if pot is None else pot
    if workspace is None:
        workspace = _lib.alloc_workspace(workspace_bytes(M, 1), dev)
    wp, nb = _lib.aligned(workspace)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().dn_kmeans_min_dist(feats.data_ptr(), M, D, cands.data_ptr(), k, commit, mind2.data_ptr(), pot.data_ptr(), wp, nb,
                                                  _lib.current_stream()), "dn_kmeans_min_dist")
    return pot


# ---------------------------------------------------------------- the trainer
class KMeansTrainer:
    """Centres (the packed matrix and -|c|^2 / 2 table dn_kmeans_assign reads), weight_sums and the workspaces of one codebook."""

    def __init__(self, n_clusters: int, dim: int, device="cuda:0", reassignment_ratio: float = 0.0):
        from .engine import _require_cuda

        if dim % 32:
            raise ValueError(f"KMeansTrainer: feature width {dim} must be a multiple of 32")
        if n_clusters < 1:
            raise ValueError("KMeansTrainer: n_clusters must be positive")
        self.device = _require_cuda(device)
        self.lib = _lib.load()
        self.n, self.D, self.reassignment_ratio = int(n_clusters), int(dim), float(reassignment_ratio)
        self.centers = self.half = None
        dev = self.device
        self.weight_sums = torch.zeros(self.n, dtype=torch.float64, device=dev)
        self.sums = torch.empty(self.n, self.D, dtype=torch.float64, device=dev)
        self.counts = torch.empty(self.n, dtype=torch.int32, device=dev)
        self.inertia = torch.empty(1, dtype=torch.float64, device=dev)
        self._rows = 0
        self._labels = self._assign_ws = self._train_ws = None
        self.init_indices_ = None
        self._reassign_rng, self._clock = np.random.RandomState(0), _ReassignClock(self.n)  # (partial_fit's reassignments)

    # -- centres
    def init_centers(self, centers) -> "KMeansTrainer":
        c = np.asarray(centers.detach().cpu() if isinstance(centers, torch.Tensor) else centers, dtype=np.float32)
        if c.shape != (self.n, self.D):
            raise ValueError(f"init_centers: expected [{self.n}, {self.D}], got {list(c.shape)}")
        C_, h = kmeans_scores_tables(c)
        self.centers, self.half = C_.to(self.device).contiguous(), h.to(self.device).contiguous()
        self.weight_sums.zero_()
        return self

    def centers_array(self) -> np.ndarray:
        self._need_centers()
        return self.centers[: self.n].cpu().numpy()

    def _need_centers(self):
        if self.centers is None:
            raise RuntimeError("KMeansTrainer: no centres yet (init_centers, init_plus_plus or fit first)")

    def _reserve(self, rows: int):
        if rows > self._rows:
            self._labels = torch.empty(rows, dtype=torch.int32, device=self.device)
            self._assign_ws = _lib.alloc_workspace(self.lib.dn_kmeans_workspace_bytes(rows, self.n), self.device)
            self._train_ws = _lib.alloc_workspace(workspace_bytes(rows, self.n), self.device)
            self._rows = rows

    def _device_feats(self, feats) -> torch.Tensor:
        x = torch.as_tensor(feats).to(self.device, torch.float32).contiguous()
        if x.dim() != 2 or x.shape[1] != self.D:
            raise ValueError(f"expected [M, {self.D}] features, got {list(x.shape)}")
        return x

    def init_plus_plus(self, feats, seed: int, n_local_trials: Optional[int] = None) -> "KMeansTrainer":
        """scikit-learn's greedy k-means++ (_kmeans_plusplus): the first centre uniform, every further one the best of
        2 + int(log n) candidates drawn proportional to the squared distance to the nearest centre so far.  The picked rows are
        kept in init_indices_ (device int64 [n]); nothing is copied back to the host."""
        x = self._device_feats(feats)
        M = x.shape[0]
        if self.n > M:
            raise ValueError(f"init_plus_plus: n_clusters={self.n} exceeds the {M} rows given")
        trials = int(n_local_trials) if n_local_trials else 2 + int(math.log(self.n))
        if not 1 <= trials <= MAX_CANDIDATES:
            raise ValueError(f"init_plus_plus: {trials} local trials (1 .. {MAX_CANDIDATES})")
        rng = np.random.RandomState(seed)
        first = int(rng.randint(M))
        draws = torch.from_numpy(rng.uniform(size=(max(self.n - 1, 1), trials))).to(self.device)
        ws = _lib.alloc_workspace(workspace_bytes(M, 1), self.device)
        mind2 = torch.full((M,), float("inf"), dtype=torch.float32, device=self.device)
        pot, pot1 = torch.empty(trials, dtype=torch.float64, device=self.device), torch.empty(1, dtype=torch.float64, device=self.device)
        picks = torch.empty(self.n, dtype=torch.int64, device=self.device)
        picks[0] = first
        min_dist(x, x[first: first + 1], mind2, commit=0, pot=pot1, workspace=ws)
        for c in range(1, self.n):
            cum = torch.cumsum(mind2.double(), 0)
            ids = torch.searchsorted(cum, draws[c - 1] * pot1).clamp_(max=M - 1)
            min_dist(x, x.index_select(0, ids), mind2, commit=-1, pot=pot, workspace=ws)
            pick = ids.index_select(0, pot.argmin().view(1))
            min_dist(x, x.index_select(0, pick), mind2, commit=0, pot=pot1, workspace=ws)
            picks[c: c + 1] = pick
        self.init_indices_ = picks
        C_ = torch.zeros((self.n + 127) // 128 * 128, self.D, dtype=torch.float32, device=self.device)
        C_[: self.n] = x.index_select(0, picks)
        self.centers = C_
        self.half = torch.zeros((self.n + 3) // 4 * 4, dtype=torch.float32, device=self.device)
        self.half[: self.n] = (-0.5 * C_[: self.n].double().pow(2).sum(1)).float()
        self.weight_sums.zero_()
        return self

    # -- steps
    def _assign(self, x: torch.Tensor) -> torch.Tensor:
        M = x.shape[0]
        self._reserve(M)
        wp, nb = _lib.aligned(self._assign_ws)
        _lib.check(self.lib.dn_kmeans_assign(x.data_ptr(), self.centers.data_ptr(), self.half.data_ptr(), M, self.D, self.n, self._labels.data_ptr(), wp, nb,
                                             _lib.current_stream()), "dn_kmeans_assign")
        return self._labels[:M]

    def _accumulate(self, x: torch.Tensor):
        labels = self._assign(x)
        return accumulate(x, labels, self.centers, self.n, workspace=self._train_ws, check_labels=False, out=(self.sums, self.counts, self.inertia))

    def _step(self, x: torch.Tensor):
        with torch.cuda.device(self.device):
            self._accumulate(x)
            update(self.centers, self.half, self.weight_sums, self.sums, self.counts, self.n)

    def partial_fit(self, batch) -> Tuple[torch.Tensor, torch.Tensor]:
        """One step on `batch` [B, D]: assign -> accumulate -> update.  -> (the batch's inertia against the centres it was assigned
        with, double [1]; the clusters' member counts, int32 [n]), both on the device.  With reassignment_ratio == 0 nothing is
        synchronised; otherwise weight_sums are read back at the steps where scikit-learn reassigns."""
        self._need_centers()
        x = self._device_feats(batch)
        if x.shape[0] == 0:
            raise ValueError("partial_fit: empty batch")
        reassign = self.reassignment_ratio > 0 and self._clock.tick(x.shape[0], self.weight_sums)
        self._step(x)
        if reassign:
            self._reassign(x, self._reassign_rng)
        return self.inertia.clone(), self.counts.clone()

    def _reassign(self, x: torch.Tensor, rng: np.random.RandomState) -> int:
        """After a step: low-count centres take rows of the batch (the host decides from weight_sums, the device scatters)."""
        dec = reassign_decision(self.weight_sums.cpu().numpy(), self.reassignment_ratio, x.shape[0], rng)
        if dec is None:
            return 0
        clusters, rows, weight = dec
        cl = torch.from_numpy(clusters).to(self.device)
        new = x.index_select(0, torch.from_numpy(rows.astype(np.int64)).to(self.device))
        self.centers.index_copy_(0, cl, new)
        self.half.index_copy_(0, cl, (-0.5 * new.double().pow(2).sum(1)).float())
        self.weight_sums.index_fill_(0, cl, weight)
        return len(clusters)

    def fit(self, feats, batch_size: int = 10000, max_iter: int = 150, seed: int = 1369, tol: float = 0.0, max_no_improvement: Optional[int] = 100,
            init: Union[str, np.ndarray, torch.Tensor] = "k-means++", init_size: Optional[int] = None) -> "KMeansTrainer":
        """MiniBatchKMeans.fit's loop.  feats: a device tensor [M, D] (batches by index_select), or a host array / a list of .npy
        paths (batches gathered on the host into one pinned buffer, one asynchronous copy per step).  tol is relative, as
        scikit-learn's (scaled by the mean column variance of the features, which must then be one array).  The batch inertia is read
        back once per step only while the early stop can fire (tol > 0 or max_no_improvement set).  Sets n_steps_ and inertia_trace_."""
        on_device = isinstance(feats, torch.Tensor) and feats.is_cuda
        src = self._device_feats(feats) if on_device else _HostRows(feats.cpu().numpy() if isinstance(feats, torch.Tensor) else feats)
        M, D = src.shape
        if D != self.D:
            raise ValueError(f"fit: expected width {self.D}, got {D}")
        sched = MiniBatchSchedule(M, self.n, batch_size, max_iter, seed, 0.0, max_no_improvement)
        B = sched.batch_size
        if tol > 0.0:
            if not on_device and len(src.parts) > 1:
                raise ValueError("fit: tol > 0 needs the features as one array")
            var = src.double().var(0, unbiased=False).mean().item() if on_device else float(np.var(np.asarray(src.parts[0], dtype=np.float64), axis=0).mean())
            sched.tol = tol * var
        pinned = stage = copied = None
        if not on_device:
            pinned = torch.empty(B, D, dtype=torch.float32).pin_memory()
            stage = torch.empty(B, D, dtype=torch.float32, device=self.device)
            copied = torch.cuda.Event()

        def batch_of(idx: np.ndarray, out: Optional[torch.Tensor] = None) -> torch.Tensor:
            if on_device:
                return src.index_select(0, torch.from_numpy(idx).to(self.device))
            if out is None:
                rows = np.empty((len(idx), D), dtype=np.float32)
                src.gather(idx, rows)
                return torch.from_numpy(rows).to(self.device)
            src.gather(idx, pinned.numpy())
            with torch.cuda.device(self.device):
                out.copy_(pinned, non_blocking=True)
                copied.record()
            copied.synchronize()  # the pinned buffer is free for the next gather; the step itself is not waited for
            return out

        if isinstance(init, str):
            if init != "k-means++":
                raise ValueError(f"fit: init {init!r} (\"k-means++\" or an array of centres)")
            size = init_size or 3 * B
            size = min(3 * self.n if size < self.n else size, M)
            self.init_plus_plus(batch_of(sched.rng.randint(0, M, size)), seed=int(sched.rng.randint(2 ** 31 - 1)))
        else:
            self.init_centers(init)
        self.inertia_trace_ = []
        self.n_steps_ = 0
        nonzero = False  # once every weight is positive none returns to zero (a reassigned centre takes a positive weight)
        for step in range(sched.n_steps):
            x = batch_of(sched.next_batch(), stage)
            reassign = False
            if self.reassignment_ratio > 0:
                if not nonzero and not sched.reassign_due():
                    nonzero = not bool((self.weight_sums == 0).any().item())
                reassign = sched.random_reassign(not nonzero)
            prev = self.centers[: self.n].clone() if sched.tol > 0.0 else None
            self._step(x)
            if reassign:
                self._reassign(x, sched.rng)
            self.n_steps_ = step + 1
            if sched.monitors:
                inertia = float(self.inertia.item())
                self.inertia_trace_.append(inertia)
                diff = float((self.centers[: self.n].double() - prev.double()).pow(2).sum().item()) if prev is not None else 0.0
                if sched.converged(step, inertia, diff):
                    break
        torch.cuda.synchronize(self.device)
        return self

    # -- results
    def score(self, feats) -> float:
        """Mean inertia sum_m |x_m - c(x_m)|^2 / M, what the reference script logs after training; assign + accumulate in chunks."""
        self._need_centers()
        rows = feats if isinstance(feats, torch.Tensor) else _HostRows(feats)
        M = rows.shape[0]
        total = torch.zeros(1, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            for s in range(0, M, SCORE_CHUNK):
                e = min(M, s + SCORE_CHUNK)
                if isinstance(rows, torch.Tensor):
                    x = self._device_feats(rows[s:e])
                else:
                    buf = np.empty((e - s, self.D), dtype=np.float32)
                    rows.gather(np.arange(s, e), buf)
                    x = torch.from_numpy(buf).to(self.device)
                self._accumulate(x)
                total += self.inertia
        return float(total.item()) / M

    def quantizer(self) -> KMeansQuantizer:
        return KMeansQuantizer(self.centers_array(), device=self.device)

    def save_centers(self, path: str) -> None:
        """The .npy [n, D] that KMeansQuantizer and the recipe's quantize step load."""
        with open(path, "wb") as fh:
            np.save(fh, self.centers_array())

    def to_sklearn(self):
        """A fitted sklearn.cluster.MiniBatchKMeans carrying the learned centres (what the reference's joblib.dump stores)."""
        try:
            from sklearn.cluster import MiniBatchKMeans
        except ImportError as e:
            raise ImportError("to_sklearn() needs scikit-learn, which is not importable here; save_centers() writes the same centres as .npy") from e
        return sklearn_model(self.centers_array(), self.weight_sums.cpu().numpy())


def sklearn_model(centers: np.ndarray, weight_sums: Optional[np.ndarray] = None):
    """MiniBatchKMeans with cluster_centers_ = centers: one partial_fit on the centres themselves sets every fitted attribute in the
    way the installed version wants them, then the centres (and counts) are put in."""
    from sklearn.cluster import MiniBatchKMeans

    centers = np.ascontiguousarray(centers, dtype=np.float32)
    km = MiniBatchKMeans(n_clusters=len(centers), init=centers.copy(), n_init=1, reassignment_ratio=0.0)
    km.partial_fit(centers)
    km.cluster_centers_ = centers.copy()
    if weight_sums is not None:
        km._counts = np.asarray(weight_sums, dtype=np.float32)
    return km


class _ReassignClock:
    """_random_reassign for a sequence of partial_fit calls."""

    def __init__(self, n_clusters: int):
        self.n, self.since, self.nonzero = n_clusters, 0, False

    def tick(self, rows: int, weight_sums: torch.Tensor) -> bool:
        self.since += rows
        if not self.nonzero and self.since < 10 * self.n:
            self.nonzero = not bool((weight_sums == 0).any().item())
        if not self.nonzero or self.since >= 10 * self.n:
            self.since = 0
            return True
        return False


def learn_kmeans(manifest_path: str, n_clusters: int, sample_pct: float = 0.1, seed: int = 1369, device="cuda:0", out_path: Optional[str] = None,
                 reassignment_ratio: float = 0.0, **fit_args) -> KMeansTrainer:
    """cluster_kmeans.py's main on the device: the manifest dump_features wrote, sample_pct of its utterances, fit, the mean inertia
    (logged by the script; kept in final_inertia_), and optionally the centres as .npy."""
    paths = sample_manifest(manifest_path, sample_pct, seed)
    if not paths:
        raise ValueError(f"learn_kmeans: no feature files sampled from {manifest_path} (sample_pct={sample_pct})")
    dim = int(np.load(paths[0], mmap_mode="r").shape[1])
    trainer = KMeansTrainer(n_clusters, dim, device=device, reassignment_ratio=reassignment_ratio)
    trainer.fit(paths, seed=seed, **fit_args)
    trainer.final_inertia_ = trainer.score(paths)
    if out_path:
        trainer.save_centers(out_path)
    return trainer
