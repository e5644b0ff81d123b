"""Times the DDIM chain over a timestep schedule (EpsEngine.ddim_schedule_loop) on the full-size model: f16, [32,512],
timesteps = 1000, start_step = 999, N in {998, 100, 50, 20} evaluations.

Per N: the chain's wall time (synchronised host clock around one call, after a warm-up call that pays capture and workspace growth),
split into set-up (the conditioning table of N rows) and the steps, and ms per evaluation.  The set-up is measured on the same code
(eps_cond_rows over N rows) through `ddim_loop(start_step=N, max_evals=1)` = set-up + one evaluation, solved with the chain's own
time for the evaluation: setup = (w1 - wall / N) / (1 - 1 / N).  For N = 998 the chain is also timed against `ddim_loop`: three
alternating pairs in this process.  The unit agreement of each N with the 998-evaluation chain (VAE decode of the final latents) is
reported without a bar: the weights are random, the logits flat.  Prints one JSON line.

    python tools/ddim_schedule_bench.py [--dtype f16] [--batch 32] [--frames 512] [--steps 998 100 50 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffnorm_amd import engine, ops, scheduler, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, nargs="+", default=[998, 100, 50, 20])
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, start = a.batch, a.frames, a.timesteps - 1
    cfg = synthetic.eps_config()
    eng = engine.EpsEngine(synthetic.random_eps_state_dict(cfg, seed=0), cfg, dtype=a.dtype, device=dev)
    vae = engine.VaeEngine(synthetic.random_vae_state_dict(768, 128, seed=1), dtype=a.dtype, device=dev)
    sched = scheduler.DDPMScheduler(a.timesteps)
    coef = sched.ddim_coef_table(dev)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    feat = torch.randn(B, T, 768, generator=torch.Generator().manual_seed(0)).to(dev)
    z = vae.encode(feat, ops.randn((B, T, 128), seed=99, device=dev))
    t_start = torch.full((B,), start, dtype=torch.int32, device=dev)
    x0 = ops.q_sample(z, ops.randn((B, T, 128), seed=98, device=dev), sched.f32("sqrt_alphas_cumprod", dev),
                      sched.f32("sqrt_one_minus_alphas_cumprod", dev), t_start, T)
    x = torch.empty_like(x0)
    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream

    def timed(fn):
        x.copy_(x0)
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, n

    def units_of():
        return vae.decode(x, lengths, want_logits=False)[2].clone()

    out = {"dtype": a.dtype, "B": B, "T": T, "timesteps": a.timesteps, "start_step": start, "chains": {}}
    full_units = None
    for n in a.steps:
        st, rows = sched.ddim_schedule(start, sampling_steps=n, device=dev)
        chain = lambda: eng.ddim_schedule_loop(x, lengths, st, rows, timesteps=a.timesteps)  # noqa: E731
        timed(chain)  # warm-up: capture, workspace
        wall, got = timed(chain)
        assert got == n
        units = units_of()
        if n == start - 1:
            full_units = units
        one = lambda: eng.ddim_loop(x, lengths, n, coef, max_evals=1)  # noqa: E731
        timed(one)
        w1 = statistics.median(timed(one)[0] for _ in range(3))
        setup = (w1 - wall / n) / (1 - 1 / n) if n > 1 else float("nan")
        row = {"wall_ms": wall, "setup_ms": setup, "steps_ms": wall - setup, "ms_per_eval": (wall - setup) / n,
               "workspace_bytes": int(eng.lib.dn_ddim_sched_workspace_bytes(eng.handle, B, T, n))}
        out["chains"][str(n)] = row
        print(f"N = {n:4d}: chain {wall:9.2f} ms = set-up {setup:7.2f} + steps {wall - setup:9.2f}  ({row['ms_per_eval']:.3f} ms / evaluation)", flush=True)
        if n == start - 1:  # against the every-timestep loop: alternating pairs
            base = lambda: eng.ddim_loop(x, lengths, start, coef)  # noqa: E731
            timed(base)
            pairs = []
            for _ in range(a.pairs):
                wb, nb = timed(base)
                ub = units_of()
                ws, _ = timed(chain)
                pairs.append({"ddim_loop_ms": wb, "schedule_ms": ws, "ratio": ws / wb})
                assert nb == n and torch.equal(ub, units_of()), "the every-timestep schedule is dn_ddim_loop's chain"
                print(f"  pair: ddim_loop {wb:9.2f} ms   schedule {ws:9.2f} ms   ratio {ws / wb:.4f}", flush=True)
            row["pairs_vs_ddim_loop"] = pairs
            row["ddim_loop_ms_per_eval"] = statistics.median(p["ddim_loop_ms"] for p in pairs) / n
        row["_units"] = units
    for n, row in out["chains"].items():
        u = row.pop("_units")
        if full_units is not None:
            row["unit_agreement_vs_full_chain"] = (u == full_units).float().mean().item()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
