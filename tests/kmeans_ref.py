"""Float64 restatement of mini-batch k-means training (scikit-learn's dense rule and greedy k-means++), and the seeded data of
tests/golden/kmeans_train.npz.  Shared by tools/gen_golden_kmeans.py, tests/test_kmeans_host.py and tests/test_hip_kmeans_train.py."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_train.npz")
MARGIN = 1e-4          # float64 top-2 margin of |x - c|^2 under which an assignment is not compared
N_STEPS, BATCH = 20, 256
FAR = 100.0            # every coordinate of data set (a)'s ninth initial centre: it never wins a row

# name: (data seed, M, D, blobs, scale of the blob centres, noise sigma, seed of the batch stream and of C0's rows)
SETS = {"a": (101, 2000, 32, 8, 1.0, 0.2, 201), "b": (102, 1037, 768, 50, 0.25, 0.1, 202)}
PP_SEED = 7            # init_plus_plus on (a) with n = 8: one pick per blob (checked where the fixture is made and in the host test)


def blobs(name):
    """-> (X fp32 [M, D], the blob of every row)."""
    seed, M, D, k, scale, sigma, _ = SETS[name]
    rng = np.random.RandomState(seed)
    mu = rng.standard_normal((k, D)) * scale
    which = rng.randint(0, k, M)
    return (mu[which] + sigma * rng.standard_normal((M, D))).astype(np.float32), which


def batches_and_c0(name, X):
    """-> (20 batch index arrays of 256 rows, the rows of X that start the centres)."""
    _, M, D, k, _, _, seed = SETS[name]
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, M, (N_STEPS, BATCH)).astype(np.int32)
    rows = rng.choice(M, size=k, replace=False)
    return idx, rows


def initial_centers(name, X, rows):
    c0 = X[rows].astype(np.float32)
    if name == "a":
        c0 = np.concatenate([c0, np.full((1, X.shape[1]), FAR, np.float32)])
    return c0


def sq_dists(X, C):
    """|x - c|^2 in float64, from the differences."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty((len(X), len(C)))
    for j in range(len(C)):
        d = X - C[j]
        out[:, j] = np.einsum("md,md->m", d, d)
    return out


def assign(X, C):
    """-> (labels: the first minimum, the top-2 margin of every row (inf with one centre), the summed inertia)."""
    d = sq_dists(X, C)
    labels = d.argmin(1)
    best = d[np.arange(len(X)), labels]
    if d.shape[1] > 1:
        d2 = d.copy()
        d2[np.arange(len(X)), labels] = np.inf
        margin = d2.min(1) - best
    else:
        margin = np.full(len(X), np.inf)
    return labels, margin, float(best.sum())


def update(C, w, X, labels):
    """scikit-learn's dense mini-batch rule in float64: c <- (c w + sum) / (w + count), w += count; rows added in ascending index.
    C, w are float64 arrays changed in place; clusters without a row are untouched."""
    X = np.asarray(X, np.float64)
    sums = np.zeros_like(C)
    np.add.at(sums, labels, X)
    counts = np.bincount(labels, minlength=len(C))
    on = counts > 0
    C[on] = (C[on] * w[on, None] + sums[on]) / (w[on] + counts[on])[:, None]
    w[on] += counts[on]
    return counts


def step(C32, w, X):
    """One step as the kernels state it: from fp32 centres, arithmetic in float64, ONE rounding to fp32.
    -> (new centres fp32, labels, margins, inertia, counts); w (float64) is changed in place."""
    labels, margin, inertia = assign(X, C32)
    C = np.asarray(C32, np.float64).copy()
    counts = update(C, w, X, labels)
    return C.astype(np.float32), labels, margin, inertia, counts


def trajectory(X, idx, c0):
    """-> (centres after every step [steps, n, D] fp32, margins [steps, B], labels [steps, B])."""
    C, w = c0.astype(np.float32), np.zeros(len(c0))
    out, margins, labels = [], [], []
    for b in idx:
        C, l, m, _, _ = step(C, w, X[b])
        out.append(C)
        margins.append(m)
        labels.append(l)
    return np.stack(out), np.stack(margins), np.stack(labels)


def half_norm(C32):
    return (-0.5 * (np.asarray(C32, np.float64) ** 2).sum(1)).astype(np.float32)


def plus_plus(X, n, seed, n_local_trials=None):
    """Greedy k-means++ in float64 with KMeansTrainer.init_plus_plus's draws.  -> (picked rows, for every pick after the first
    the smallest distance of one of its draws to a boundary of the cumulative sum, as a share of the total potential)."""
    X64 = np.asarray(X, np.float64)
    M = len(X)
    trials = int(n_local_trials) if n_local_trials else 2 + int(math.log(n))
    rng = np.random.RandomState(seed)
    first = int(rng.randint(M))
    draws = rng.uniform(size=(max(n - 1, 1), trials))
    picks, slack = [first], []
    mind2 = sq_dists(X64, X64[first: first + 1])[:, 0]
    pot = mind2.sum()
    for c in range(1, n):
        cum = np.cumsum(mind2)
        vals = draws[c - 1] * pot
        ids = np.minimum(np.searchsorted(cum, vals), M - 1)
        slack.append(float(np.abs(cum[None, :] - vals[:, None]).min() / pot))
        cand = np.minimum(mind2[None, :], sq_dists(X64, X64[ids]).T)
        best = int(cand.sum(1).argmin())
        mind2, pot = cand[best], cand[best].sum()
        picks.append(int(ids[best]))
    return np.array(picks), np.array(slack)


def fit(X, n, init, batch_size, max_iter, seed, max_no_improvement=100, schedule_cls=None):
    """KMeansTrainer.fit's loop (the package's MiniBatchSchedule) around the float64 step.  -> (centres fp32, steps run, the batch
    index arrays it drew)."""
    from diffnorm_amd.kmeans import MiniBatchSchedule

    sched = (schedule_cls or MiniBatchSchedule)(len(X), n, batch_size, max_iter, seed, 0.0, max_no_improvement)
    if isinstance(init, str):
        size = min(3 * n if 3 * sched.batch_size < n else 3 * sched.batch_size, len(X))
        sub = X[sched.rng.randint(0, len(X), size)]
        picks, _ = plus_plus(sub, n, int(sched.rng.randint(2 ** 31 - 1)))
        C = sub[picks].astype(np.float32)
    else:
        C = np.asarray(init, np.float32).copy()
    w, drawn, steps = np.zeros(n), [], 0
    for s in range(sched.n_steps):
        b = sched.next_batch()
        drawn.append(b)
        C, _, _, inertia, _ = step(C, w, X[b])
        steps = s + 1
        if sched.monitors and sched.converged(s, inertia):
            break
    return C, steps, drawn


def mean_inertia(X, C):
    return assign(X, C)[2] / len(X)
