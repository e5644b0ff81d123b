#!/usr/bin/env python3
"""Times what `engine()` costs after an update of a model in training, at the recipe size (the 260.6 M-parameter eps-predictor and
the 138.6 M-parameter VAE): the rebuild (state_dict() of the training engine -> pack_eps / pack_vae on the host -> a new inference
engine: what the module layer did before refresh_from existed; the destruction of the old engine is not in the figure) against
EpsEngine / VaeEngine.refresh_from (dn_repack_weights on the device into the existing tensors).

Every repetition is a child process of its own under its own `timeout`: it builds the training engine and a live inference engine,
moves the master buffer (an update), times one rebuild and one refresh (host clock around work that ends in a device synchronise),
compares the refreshed tensors with the rebuilt engine's byte for byte, and then times the refresh alone back to back (device events)
for its bytes read + written over its time.  The parent reports the medians over the repetitions beside the HBM peak (MI355X: 8.0
TB/s spec, about 6.3 TB/s achievable for a float4 copy).  A child that fails ends the run: nothing more is started on the device.

    python tools/refresh_bench.py [--train-dtype bf16] [--sample-dtype f16] [--repeats 5] [--timeout 300]
One JSON line per model."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3  # spec, measured float4 copy


def child(model: str, train_dtype: str, sample_dtype: str, seed: int):
    """One repetition: prints one JSON line."""
    import torch

    from diffnorm_amd import engine, synthetic, training

    dev = "cuda:0"
    if model == "eps":
        cfg = synthetic.eps_config()
        train = training.EpsTrainEngine(synthetic.random_eps_state_dict(cfg, seed), cfg, None, timesteps=200, dtype=train_dtype, device=dev,
                                        multitask=False)
        build = lambda: engine.EpsEngine(train.state_dict(), cfg, dtype=sample_dtype, device=dev)
    else:
        train = training.VaeTrainEngine(synthetic.random_vae_state_dict(768, 128, seed=seed + 1), dim=768, latent_dim=128, dtype=train_dtype,
                                        device=dev)
        build = lambda: engine.VaeEngine(train.state_dict(), dim=768, latent_dim=128, dtype=sample_dtype, device=dev)
    live = build()
    live.refresh_from(train)  # warm-up: builds and uploads the descriptors (once per layout), loads the kernel
    train.master.mul_(1.001)  # an update: the master buffer moves
    train.sync_work()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rebuild_ms, fresh = timed(build)
    refresh_ms, _ = timed(lambda: live.refresh_from(train))
    same = all(a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(live.tensors, fresh.tensors))
    del fresh
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(20):
        live.refresh_from(train)
    ev[1].record()
    torch.cuda.synchronize()
    print(json.dumps({"params": int(train.n_params), "rebuild_ms": rebuild_ms, "refresh_ms": refresh_ms, "same": bool(same),
                      "bytes": live.refresh_bytes(), "descriptors": live._repack[2], "back_to_back_ms": ev[0].elapsed_time(ev[1]) / 20}), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-dtype", default="bf16")
    ap.add_argument("--sample-dtype", default="f16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per repetition")
    ap.add_argument("--models", default="eps,vae")
    ap.add_argument("--child", default=None)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.train_dtype, a.sample_dtype, a.seed)
    for model in a.models.split(","):
        runs = []
        for rep in range(a.repeats):
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", model, "--seed", str(rep),
                                "--train-dtype", a.train_dtype, "--sample-dtype", a.sample_dtype], stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:  # a fault, a time limit or a mismatch: nothing more is started on the device
                print(f"refresh_bench: {model} repetition {rep} ended with status {r.returncode}\n{r.stdout}", file=sys.stderr)
                return r.returncode
            runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(f"refresh_bench: {model} repetition {rep}: {runs[-1]}", file=sys.stderr, flush=True)
        med = lambda k: statistics.median(v[k] for v in runs)
        b2b, moved = med("back_to_back_ms"), runs[0]["bytes"]
        print(json.dumps({"model": model, "params": runs[0]["params"], "train_dtype": a.train_dtype, "sample_dtype": a.sample_dtype,
                          "repeats": len(runs), "rebuild_ms_median": round(med("rebuild_ms"), 1), "refresh_ms_median": round(med("refresh_ms"), 3),
                          "rebuild_ms": [round(v["rebuild_ms"], 1) for v in runs], "refresh_ms": [round(v["refresh_ms"], 3) for v in runs],
                          "refresh_equals_rebuild": all(v["same"] for v in runs), "descriptors": runs[0]["descriptors"], "refresh_bytes": moved,
                          "refresh_back_to_back_ms_median": round(b2b, 3), "refresh_TBps": round(moved / (b2b * 1e-3) / 1e12, 2),
                          "hbm_peak_TBps": HBM_PEAK_TBS, "hbm_float4_copy_TBps": HBM_COPY_TBS}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
