"""Times stochastic chains with keyed per-step noise (`keys=`: dn_ddim_sched_loop_keyed, dn_ddpm_loop_keyed) against the same chains
drawing from a seed (dn_ddim_sched_loop, dn_ddpm_loop) on the full-size model: f16, [32,512], timesteps = 1000, start_step = 50,
N = 49 evaluations, eta = 0.5 for the scheduled DDIM chain.

The keyed update pays one 64-bit division and one 8-byte load per quad of an update that is well under 1 % of a step, so the
expectation is "no measurable difference".  Per loop, in a fresh child process with a time limit of its own: both chains are warmed
up (capture, workspace) and timed in alternating blocks of `--pairs` calls (synchronised host clock around one call), `--rounds` blocks
each; the medians are reported in ms per evaluation with their ratio, and the spread of a leg as (max - min) / median of its calls.
`--seed-only` times the seed-drawn legs alone (an engine without `keys=`).  The first loop that fails or runs out of time ends the
run.  Prints one JSON line.

    python tools/keyed_steps_bench.py [--dtype f16] [--batch 32] [--frames 512] [--evals 49] [--eta 0.5] [--pairs 5] [--rounds 2]
                                      [--loops ddim ddpm] [--seed-only] [--limit 240]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a, loop):
    import torch

    from diffnorm_amd import engine, ops, scheduler, sharding, synthetic

    dev = torch.device("cuda:0")
    B, T, start, n = a.batch, a.frames, a.start_step, a.evals
    cfg = synthetic.eps_config()
    eng = engine.EpsEngine(synthetic.random_eps_state_dict(cfg, seed=0), cfg, dtype=a.dtype, device=dev)
    sched = scheduler.DDPMScheduler(a.timesteps)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    z = ops.randn((B, T, cfg.latent_dim), seed=99, device=dev)
    t_start = torch.full((B,), start, dtype=torch.int32, device=dev)
    x0 = ops.q_sample(z, ops.randn((B, T, cfg.latent_dim), seed=98, device=dev), sched.f32("sqrt_alphas_cumprod", dev),
                      sched.f32("sqrt_one_minus_alphas_cumprod", dev), t_start, T)
    x = torch.empty_like(x0)
    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream
    keys = sharding.utterance_keys(5, range(B)).to(dev)  # on the device once: its address is part of the graph key
    if loop == "ddim":
        steps, coef = sched.ddim_schedule(start, sampling_steps=n, eta=a.eta, device=dev)
        run = lambda **noise: eng.ddim_schedule_loop(x, lengths, steps, coef, eta=a.eta, timesteps=a.timesteps, **noise)  # noqa: E731
    else:
        table = sched.gaussian_table(dev)
        run = lambda **noise: eng.ddpm_loop(x, lengths, start, table, max_evals=n, **noise)  # noqa: E731
    legs = [("seed", dict(seed=7))] + ([] if a.seed_only else [("keyed", dict(keys=keys))])

    def timed(noise):
        x.copy_(x0)
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = run(**noise)
            torch.cuda.synchronize()
        assert got == n, (got, n)
        return (time.perf_counter() - t0) * 1e3

    # the two chains share one graph slot and evict each other's captured step: alternate BLOCKS, each behind a warm-up call of its own
    # that pays the capture, so every timed call replays a cached graph
    walls = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, noise in legs:
            timed(noise)
            walls[name] += [timed(noise) for _ in range(a.pairs)]
    row = {"loop": loop, "n": n, "walls_ms": walls}
    for name, w in walls.items():
        row[f"{name}_ms_per_eval"] = statistics.median(w) / n
        row[f"{name}_spread"] = (max(w) - min(w)) / statistics.median(w)
    if "keyed" in walls:
        row["ratio"] = row["keyed_ms_per_eval"] / row["seed_ms_per_eval"]
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--start-step", type=int, default=50)
    ap.add_argument("--evals", type=int, default=49)
    ap.add_argument("--eta", type=float, default=0.5)
    ap.add_argument("--loops", nargs="+", default=["ddim", "ddpm"], choices=["ddim", "ddpm"])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed-only", action="store_true")
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per loop")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    out = {"dtype": a.dtype, "B": a.batch, "T": a.frames, "timesteps": a.timesteps, "start_step": a.start_step, "eta": a.eta, "loops": {}}
    passed = [f"--{k}={getattr(a, k.replace('-', '_'))}" for k in ("dtype", "batch", "frames", "timesteps", "start-step", "evals", "eta", "pairs",
                                                                  "rounds")] + (["--seed-only"] if a.seed_only else [])
    for loop in a.loops:  # a fresh process per loop; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--child={loop}"] + passed, capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{loop}: no result within {a.limit:.0f} s: stopping", file=sys.stderr)
            out["failed"] = {"loop": loop, "why": "time limit"}
            break
        if r.returncode != 0:
            print(f"{loop}: exit status {r.returncode}: stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            out["failed"] = {"loop": loop, "why": f"exit status {r.returncode}"}
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["loops"][loop] = row
        keyed = f"  keyed {row['keyed_ms_per_eval']:.3f} (spread {row['keyed_spread']:.2%}, ratio {row['ratio']:.4f})" if "ratio" in row else ""
        print(f"{loop}: seed {row['seed_ms_per_eval']:.3f} ms / evaluation (spread {row['seed_spread']:.2%}){keyed}", flush=True)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
