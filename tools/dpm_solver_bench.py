"""Times the DPM-Solver++(2M) chain (EpsEngine.dpm_schedule_loop, dn_dpm_loop) against the DDIM chain over the same schedule
(EpsEngine.ddim_schedule_loop, dn_ddim_sched_loop) on the full-size model: f16, [32,512], timesteps = 1000, start_step = 50,
N in {49, 20, 10} evaluations (49 is every timestep below start_step = 50).

The update kernel adds one read and one write of the latent (2 x 8 MB at [32,512]) to a step that moves about 12 GB, so the
expectation is "no measurable difference".  Per N, in a fresh child process with a time limit of its own: both chains are warmed up
(capture, workspace) and timed in alternating blocks of `--pairs` calls (synchronised host clock around one call), `--rounds` blocks
each; the medians are reported in ms per evaluation, with their ratio.  The first configuration that fails or runs out of time ends the run.  Prints one JSON line.

    python tools/dpm_solver_bench.py [--dtype f16] [--batch 32] [--frames 512] [--steps 49 20 10] [--pairs 5] [--rounds 2] [--limit 240]
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


def child(a, n):
    import torch

    from diffnorm_amd import engine, ops, scheduler, synthetic

    dev = torch.device("cuda:0")
    B, T, start = a.batch, a.frames, a.start_step
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
    sd, cd = sched.ddim_schedule(start, sampling_steps=n, device=dev)
    sp, cp = sched.dpm_schedule(start, sampling_steps=n, device=dev)
    eng._workspace(int(eng.lib.dn_dpm_workspace_bytes(eng.handle, B, T, n)))  # one workspace for both: no growth inside a timing
    ddim = lambda: eng.ddim_schedule_loop(x, lengths, sd, cd, timesteps=a.timesteps)  # noqa: E731
    dpm = lambda: eng.dpm_schedule_loop(x, lengths, sp, cp, timesteps=a.timesteps)  # noqa: E731

    def timed(fn):
        x.copy_(x0)
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
        assert got == n
        return (time.perf_counter() - t0) * 1e3

    # the two loops share one graph slot and evict each other's captured step: alternate BLOCKS, each behind a warm-up call of its own
    # that pays the capture, so every timed call replays a cached graph
    wd, wp = [], []
    for _ in range(a.rounds):
        for fn, walls in ((ddim, wd), (dpm, wp)):
            timed(fn)
            walls += [timed(fn) for _ in range(a.pairs)]
    md, mp = statistics.median(wd) / n, statistics.median(wp) / n
    print(json.dumps({"n": n, "ddim_ms_per_eval": md, "dpm_ms_per_eval": mp, "ratio": mp / md, "walls_ms": {"ddim": wd, "dpm": wp},
                      "workspace_bytes": {"ddim": int(eng.lib.dn_ddim_sched_workspace_bytes(eng.handle, B, T, n)),
                                          "dpm": int(eng.lib.dn_dpm_workspace_bytes(eng.handle, B, T, n))}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--start-step", type=int, default=50)
    ap.add_argument("--steps", type=int, nargs="+", default=[49, 20, 10])
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per configuration")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    out = {"dtype": a.dtype, "B": a.batch, "T": a.frames, "timesteps": a.timesteps, "start_step": a.start_step, "chains": {}}
    passed = [f"--{k}={getattr(a, k.replace('-', '_'))}" for k in ("dtype", "batch", "frames", "timesteps", "start-step", "pairs", "rounds")]
    for n in a.steps:  # a fresh process per configuration; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--child={n}"] + passed, capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"N = {n}: no result within {a.limit:.0f} s: stopping", file=sys.stderr)
            out["failed"] = {"n": n, "why": "time limit"}
            break
        if r.returncode != 0:
            print(f"N = {n}: exit status {r.returncode}: stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            out["failed"] = {"n": n, "why": f"exit status {r.returncode}"}
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["chains"][str(n)] = row
        print(f"N = {n:3d}: ddim {row['ddim_ms_per_eval']:.3f}  dpm 2M {row['dpm_ms_per_eval']:.3f} ms / evaluation  (ratio {row['ratio']:.4f})",
              flush=True)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
