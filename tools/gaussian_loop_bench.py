"""Times the generic Gaussian scheduler's device loop (GaussianDiffusion.*_sample_loop_device, EpsEngine.gaussian_loop,
dn_gaussian_loop: hipGraph replay + two half-batch streams) against the host loop the scheduler has always had (ddim_sample_loop /
p_sample: per step a timestep tensor, an eager evaluation of the engine through a small callable, torch.randn_like,
dn_gaussian_step) on the full-size model: f16, [32,512], create_diffusion(..., noise_schedule="cosine", learn_sigma=False,
diffusion_steps=1000) for

    "ddim50"   the 50 respaced steps, ddim_sample at eta = 0
    ""         the 50-step tail of the un-respaced diffusion (start_index = 50), p_sample

Per configuration, in a fresh child process with a time limit of its own: both loops are warmed up (capture, workspace), then
timed in `--rounds` alternating blocks of `--calls` calls (synchronised host clock around one call); the medians and the spread
(min .. max) are reported in ms per evaluation, with their ratio.  The first configuration that fails or runs out of time ends the
run.  Prints one JSON line.

    python tools/gaussian_loop_bench.py [--dtype f16] [--batch 32] [--frames 512] [--calls 5] [--rounds 3] [--limit 300]
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

CONFIGS = {"ddim50": ("ddim50", "ddim", None), "tail50": ("", "p_sample", 50)}


def child(a, name):
    import torch

    from diffnorm_amd import engine, ops, synthetic
    from diffnorm_amd.diffusion import create_diffusion

    respacing, sampler, start = CONFIGS[name]
    dev = torch.device("cuda:0")
    B, T = a.batch, a.frames
    cfg = synthetic.eps_config()
    eng = engine.EpsEngine(synthetic.random_eps_state_dict(cfg, seed=0), cfg, dtype=a.dtype, device=dev)
    diff = create_diffusion(respacing, noise_schedule="cosine", learn_sigma=False, diffusion_steps=1000)
    n = diff.num_timesteps if start is None else start
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    x0 = ops.randn((B, T, cfg.latent_dim), seed=99, device=dev)
    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream
    model = lambda x, t: eng.forward(x, t, lengths)  # noqa: E731  (elementwise scheduler: the [B,T,z] layout is fine)
    step = diff.ddim_sample if sampler == "ddim" else diff.p_sample

    def host():
        x = x0
        for i in range(n - 1, -1, -1):  # ddim_sample_loop_progressive / p_sample_loop_progressive (:145-188), entered at index n-1
            x = step(model, x, torch.tensor([i] * B, device=dev), clip_denoised=False)["sample"]
        return x

    def device():
        fn = diff.ddim_sample_loop_device if sampler == "ddim" else diff.p_sample_loop_device
        return fn(eng, x0, lengths, clip_denoised=False, start_index=start, seed=7)

    def timed(fn):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        return (time.perf_counter() - t0) * 1e3

    eng._workspace(int(eng.lib.dn_gaussian_workspace_bytes(eng.handle, B, T, n)))  # one workspace for both: no growth inside a timing
    wh, wd = [], []
    for _ in range(a.rounds):  # alternating blocks, each behind a warm-up call of its own (the device loop's pays the capture once)
        for fn, walls in ((host, wh), (device, wd)):
            timed(fn)
            walls += [timed(fn) for _ in range(a.calls)]
    per = lambda w: {"median": statistics.median(w) / n, "min": min(w) / n, "max": max(w) / n}  # noqa: E731
    h, d = per(wh), per(wd)
    print(json.dumps({"config": name, "respacing": respacing, "sampler": sampler, "evaluations": n, "host_ms_per_eval": h, "device_ms_per_eval": d,
                      "ratio": d["median"] / h["median"], "walls_ms": {"host": wh, "device": wd}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--configs", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per configuration")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    out = {"dtype": a.dtype, "B": a.batch, "T": a.frames, "chains": {}}
    passed = [f"--{k}={getattr(a, k)}" for k in ("dtype", "batch", "frames", "calls", "rounds")]
    for name in a.configs:  # a fresh process per configuration; the first failure ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--child={name}"] + passed, capture_output=True, text=True,
                               timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {a.limit:.0f} s: stopping", file=sys.stderr)
            out["failed"] = {"config": name, "why": "time limit"}
            break
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}: stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            out["failed"] = {"config": name, "why": f"exit status {r.returncode}"}
            break
        row = json.loads(r.stdout.strip().splitlines()[-1])
        out["chains"][name] = row
        h, d = row["host_ms_per_eval"], row["device_ms_per_eval"]
        print(f"{name:7s} ({row['sampler']}, {row['evaluations']} evaluations): host {h['median']:.3f} ({h['min']:.3f} .. {h['max']:.3f})  "
              f"device {d['median']:.3f} ({d['min']:.3f} .. {d['max']:.3f}) ms / evaluation  (ratio {row['ratio']:.4f})", flush=True)
    print(json.dumps(out))
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
