"""Times quantizer learning at the recipe's size: n = 1000 clusters, D = 768, batches of 10 000 rows out of 10^6 synthetic frames.

  python tools/kmeans_bench.py [--frames 1000000] [--steps 100] [--blocks 3] [--sklearn]

Measured, each behind a warm-up, in `--blocks` alternating blocks (device, plain torch, device, ...), reported as the median with
(min - max): one step (assign -> accumulate -> update; device events around 20 steps), its per-kernel split, and a `--steps`-step
fit from given centres (host clock around a run that ends in a synchronise).  The comparison is the same step written in plain
torch on the same device (cdist / argmin / index_add_), and with --sklearn scikit-learn's MiniBatchKMeans.partial_fit on the host's
cores where it is importable.  Prints one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffnorm_amd import kmeans  # noqa: E402


def torch_step(x, C, w):
    """The same step in plain torch: fp32 distances, fp32 sums."""
    labels = torch.cdist(x, C).argmin(1)
    sums = torch.zeros_like(C).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=C.shape[0]).to(C.dtype)
    on = counts > 0
    Cn = torch.where(on[:, None], (C * w[:, None] + sums) / (w + counts).clamp_min(1)[:, None], C)
    C.copy_(Cn)
    w += counts


def events_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--clusters", type=int, default=1000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, D, B = a.clusters, a.dim, a.batch
    g = torch.Generator(device=dev).manual_seed(0)
    mu = torch.randn(n, D, device=dev, generator=g)
    X = torch.empty(a.frames, D, device=dev)
    for s in range(0, a.frames, 100000):  # blobs around n centres, built in slices
        e = min(a.frames, s + 100000)
        X[s:e] = mu[torch.randint(0, n, (e - s,), device=dev, generator=g)] + 0.5 * torch.randn(e - s, D, device=dev, generator=g)
    C0 = X[torch.randperm(a.frames, device=dev, generator=g)[:n]].clone()
    x = X[:B].contiguous()
    t = kmeans.KMeansTrainer(n, D, device=dev).init_centers(C0)
    Ct, wt = C0.clone(), torch.zeros(n, device=dev)

    def fit_once():
        t.init_centers(C0)
        t0 = time.perf_counter()
        t.fit(X, batch_size=B, max_iter=1, seed=1, max_no_improvement=None, init=C0)
        return (time.perf_counter() - t0) * 1e3 * a.steps / t.n_steps_

    # a fit of exactly --steps steps: max_iter is whole passes, so time a pass-limited run scaled to --steps when they differ
    sched_steps = a.frames // B
    if sched_steps != a.steps:
        print(f"note: one pass over {a.frames} frames is {sched_steps} steps; the fit time is scaled to {a.steps} steps")

    def torch_fit():
        Ct.copy_(C0)
        wt.zero_()
        rng = np.random.RandomState(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            torch_step(X.index_select(0, torch.from_numpy(rng.randint(0, a.frames, B)).to(dev)), Ct, wt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    split = {"assign": lambda: t._assign(x), "accumulate": lambda: kmeans.accumulate(x, t._labels[:B], t.centers, n, workspace=t._train_ws, check_labels=False,
                                                                                      out=(t.sums, t.counts, t.inertia)),
             "update": lambda: kmeans.update(t.centers, t.half, t.weight_sums, t.sums, t.counts, n)}
    for _ in range(3):  # warm-up of every shape timed below
        t._step(x)
        torch_step(x, Ct, wt)
    torch.cuda.synchronize()
    res = {k: [] for k in ("step_ms", "torch_step_ms", "fit_ms", "torch_fit_ms", "assign_ms", "accumulate_ms", "update_ms")}
    for _ in range(a.blocks):
        res["step_ms"].append(events_ms(lambda: t._step(x), 20))
        res["torch_step_ms"].append(events_ms(lambda: torch_step(x, Ct, wt), 20))
        for k, fn in split.items():
            res[k + "_ms"].append(events_ms(fn, 20))
        res["fit_ms"].append(fit_once())
        res["torch_fit_ms"].append(torch_fit())
    out = {"n": n, "D": D, "batch": B, "frames": a.frames, "fit_steps": a.steps, "blocks": a.blocks}
    for k, v in res.items():
        out[k] = summary(v)
        print(f"{k:16s} median {out[k]['median']:9.3f}  ({out[k]['min']:.3f} - {out[k]['max']:.3f})")
    if a.sklearn:
        try:
            from sklearn.cluster import MiniBatchKMeans
        except ImportError:
            print("scikit-learn is not importable here: no host comparison")
        else:
            xh, c0 = x.cpu().numpy(), C0.cpu().numpy()
            km = MiniBatchKMeans(n_clusters=n, init=c0, n_init=1, reassignment_ratio=0)
            km.partial_fit(xh)
            ts = []
            for _ in range(a.blocks):
                t0 = time.perf_counter()
                km.partial_fit(xh)
                ts.append((time.perf_counter() - t0) * 1e3)
            out["sklearn_step_ms"] = summary(ts)
            print(f"sklearn_step_ms  median {out['sklearn_step_ms']['median']:9.3f}  ({min(ts):.3f} - {max(ts):.3f})  on {os.cpu_count()} visible cores")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
