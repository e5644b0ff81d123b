"""Times the prompted, guided DDIM chain as a device loop over a timestep schedule (EpsEngine.guided_ddim_schedule_loop,
dn_guided_ddim_loop) on the full-size conditional model as tools/cond_ab.py builds it: f16, [32,512], Tp = 512, cond_scale 2,
timesteps = 1000, start_step = 999.

(a) the host-driven chain `guided_ddim_chain` against the new loop on the every-timestep schedule (998 evaluations each): alternating
    pairs in this process, median and range of ms per evaluation (whole-chain wall time / evaluations, set-up included on both sides);
    the two final latents must be bit-identical.
(b) the new loop at N in {998, 100, 50, 20} evaluations: whole-chain wall time (after a warm-up call that pays capture and workspace
    growth), set-up = the time table of N rows (`cond_time_table_steps`, timed alone) + the prompt-only work (a 2B-row pass without
    minus one with DN_COND_REUSE_PROMPT), and ms per evaluation = (wall - set-up) / N.

(c) `--solver dpmpp_2m`, instead of (a) and (b): the guided DPM-Solver++(2M) loop (EpsEngine.guided_dpm_schedule_loop, dn_guided_dpm_loop)
    against dn_guided_ddim_loop on the same schedule from `--solver-start` (50) at N in `--solver-steps` (49 20 10) evaluations: a warm-up
    call of each (capture, workspace), then alternating pairs in this process; median and range of whole-chain ms per evaluation and of
    the pair's ratio.  dn_guided_ddim_loop is the baseline: the update adds one latent-sized read and one write to a step.

One process; `--only a` / `--only b` and `--steps` let a caller put each part under a time limit of its own.  Prints one JSON line.

    python tools/guided_schedule_bench.py [--dtype f16] [--batch 32] [--frames 512] [--prompt-frames 512] [--scale 2.0] [--only a|b]
    python tools/guided_schedule_bench.py --solver dpmpp_2m [--solver-steps 49 20 10] [--pairs 3]
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
    ap.add_argument("--prompt-frames", type=int, default=512)
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--steps", type=int, nargs="+", default=[998, 100, 50, 20])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--solver", choices=["dpmpp_2m"], default=None)
    ap.add_argument("--solver-start", type=int, default=50)
    ap.add_argument("--solver-steps", type=int, nargs="+", default=[49, 20, 10])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, Tp, start = a.batch, a.frames, a.prompt_frames, a.timesteps - 1
    cfg = synthetic.eps_config(dim_prompt=768, num_latents_m=64)
    eng = engine.EpsEngine(synthetic.random_eps_state_dict(cfg, seed=2), cfg, dtype=a.dtype, device=dev)
    sched = scheduler.DDPMScheduler(a.timesteps)
    coef = sched.ddim_coef_table(dev)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    plens = torch.full((B,), Tp, dtype=torch.int32, device=dev)
    x0 = ops.randn((B, T, cfg.latent_dim), seed=77, device=dev)
    prompt = ops.randn((B, Tp, 768), seed=78, device=dev)
    x = torch.empty_like(x0)
    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream

    def timed(fn, reset=True):
        if reset:
            x.copy_(x0)
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, n

    def loop_of(n):
        st, rows = sched.ddim_schedule(start, sampling_steps=n, device=dev)
        return st, lambda: eng.guided_ddim_schedule_loop(x, lengths, prompt, plens, st, rows, cond_scale=a.scale, timesteps=a.timesteps)

    out = {"dtype": a.dtype, "B": B, "T": T, "Tp": Tp, "scale": a.scale, "timesteps": a.timesteps, "start_step": start}
    if a.solver is not None:
        assert a.pairs >= 3, "at least three alternating pairs"
        out["start_step"], out["solver"], out["solver_chains"] = a.solver_start, a.solver, {}
        for n in a.solver_steps:
            sd, cd = sched.ddim_schedule(a.solver_start, sampling_steps=n, device=dev)
            sp, cp = sched.dpm_schedule(a.solver_start, sampling_steps=n, device=dev)
            ddim = lambda: eng.guided_ddim_schedule_loop(x, lengths, prompt, plens, sd, cd, cond_scale=a.scale, timesteps=a.timesteps)  # noqa: E731
            dpm = lambda: eng.guided_dpm_schedule_loop(x, lengths, prompt, plens, sp, cp, cond_scale=a.scale, timesteps=a.timesteps)  # noqa: E731
            timed(ddim)
            timed(dpm)  # warm-up of each: capture, workspace growth
            pairs = []
            for _ in range(a.pairs):
                wd, nd = timed(ddim)
                wp, np_ = timed(dpm)
                assert nd == np_ == n and bool(torch.isfinite(x).all())
                pairs.append({"ddim_ms_per_eval": wd / n, "dpm_ms_per_eval": wp / n, "ratio": wp / wd})
                print(f"  N = {n:3d} pair: dn_guided_ddim_loop {wd / n:7.3f} ms / evaluation   dn_guided_dpm_loop {wp / n:7.3f}   ratio {wp / wd:.4f}", flush=True)
            row = {"pairs": pairs}
            for k in ("ddim_ms_per_eval", "dpm_ms_per_eval", "ratio"):
                v = [p[k] for p in pairs]
                row[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            row["workspace_bytes"] = {"ddim": int(eng.lib.dn_guided_ddim_workspace_bytes(eng.handle, B, T, Tp, n, int(a.scale != 1.0))),
                                      "dpm": int(eng.lib.dn_guided_dpm_workspace_bytes(eng.handle, B, T, Tp, n, int(a.scale != 1.0)))}
            out["solver_chains"][str(n)] = row
        print(json.dumps(out))
        return
    if a.only in (None, "a"):
        n = start - 1
        _, loop = loop_of(n)
        chain = lambda: eng.guided_ddim_chain(x, lengths, prompt, plens, start, coef, cond_scale=a.scale)  # noqa: E731
        timed(lambda: eng.guided_ddim_chain(x, lengths, prompt, plens, 5, coef, cond_scale=a.scale))  # warm-up: workspaces, kernel attributes
        timed(lambda: loop_of(4)[1]())
        pairs = []
        for _ in range(a.pairs):
            wc, nc = timed(chain)
            xc = x.clone()
            wl, nl = timed(loop)
            assert nc == nl == n and torch.equal(xc, x), "the every-timestep schedule is guided_ddim_chain's chain"
            pairs.append({"chain_ms_per_eval": wc / n, "loop_ms_per_eval": wl / n, "ratio": wl / wc})
            print(f"  pair: guided_ddim_chain {wc / n:7.3f} ms / evaluation   dn_guided_ddim_loop {wl / n:7.3f}   ratio {wl / wc:.4f}", flush=True)
        out["every_timestep"] = {"evaluations": n, "pairs": pairs}
        for k in ("chain_ms_per_eval", "loop_ms_per_eval"):
            v = [p[k] for p in pairs]
            out["every_timestep"][k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    if a.only in (None, "b"):
        out["chains"] = {}
        l2, p2, pl2, drop2 = eng._guided_inputs(lengths, prompt, plens)
        t2 = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        xin, both = torch.cat([x0, x0]).contiguous(), torch.empty(2 * B, T, cfg.latent_dim, device=dev)
        for n in a.steps:
            st, loop = loop_of(n)
            timed(loop)  # warm-up: capture, workspace
            wall, got = timed(loop)
            assert got == n
            table_ms = statistics.median(timed(lambda: eng.cond_time_table_steps(st), reset=False)[0] for _ in range(3))
            table = eng.cond_time_table_steps(st)
            fwd = lambda reuse: timed(lambda: eng.forward_cond(xin, t2, l2, p2, pl2, drop2, out=both, reuse_prompt=reuse, time_table=table), reset=False)[0]  # noqa: E731
            fwd(False)
            prompt_ms = statistics.median(fwd(False) for _ in range(3)) - statistics.median(fwd(True) for _ in range(3))
            setup = table_ms + prompt_ms
            row = {"wall_ms": wall, "table_ms": table_ms, "prompt_only_ms": prompt_ms, "setup_ms": setup, "ms_per_eval": (wall - setup) / n,
                   "workspace_bytes": int(eng.lib.dn_guided_ddim_workspace_bytes(eng.handle, B, T, Tp, n, int(a.scale != 1.0))),
                   "time_table_bytes": int(table.numel() * 4)}
            out["chains"][str(n)] = row
            print(f"N = {n:4d}: chain {wall:9.2f} ms = set-up {setup:7.2f} (table {table_ms:.2f} + prompt-only {prompt_ms:.2f}) + steps "
                  f"{wall - setup:9.2f}  ({row['ms_per_eval']:.3f} ms / evaluation)", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
