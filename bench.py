#!/usr/bin/env python3
"""Benchmark of the DiffNorm denoising hot path on MI355X (driver contract: one JSON line on rank 0).

A "step" = one denoising step: eps-predictor forward (`Model.forward`, reference latent_module.py:828-876)
+ DDIM eta=0 scheduler update (:1419-1442) on a batch of B x T latent frames.  Workload at N=1 =
BASELINE.json configs[2]: [B=32, T=512] latents (z=128, hidden 512) on the 1000-step cosine schedule,
IEEE-half MFMA operands with fp32 accumulation by default (--dtype f16: the 2-byte mode whose outputs are inside north_star's
1e-2 budget on every golden; bf16 / bf16x3 / f32 selectable), synthetic N(0,1) latents and random-init weights of the recipe architecture.
With N > 1 every rank runs its own [32,512] batch (utterances are independent: weak scaling, no
data-path collective); value = N*K steps / max-over-ranks time.

Sequence per rank: an untimed 3-step set-up call (builds the chain's conditioning table for all remaining timesteps and
captures the step graph), W untimed warm-up steps, barrier, EXACTLY K timed steps of the same chain, barrier.  When the
set-up, warm-up and timed steps together outrun the chain (998 steps at 1000 timesteps), a new chain starts from t = 998 on
the latents as they stand, its conditioning table rebuilt as at the start of any chain.

A plain run does only that and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step and the workload's
description).  --dump-outputs DIR then writes what the timed path computed -- the latents after the last timed step -- as
DIR/latents.npy (fp32; other ranks' as latents_rank<r>.npy; --mode train: the last update's loss statistics and gradient
norm and a fixed sample of the parameters it left); inputs and weights are seeded, so two builds compare output for output.

--full adds the secondary figures of the same line (rank 0): "chain_setup_ms" (the once-per-chain table build, ~4 ms
against a 998-step chain of ~5.7 s), "roofline" (dominant kernel = the FFN causal-conv contraction, timed live with HIP
events), the committed PMC step traffic, the ancestral (DDPM) chain, and at N = 1 the other-precision, full-chain,
conditional, refinement and training legs and "cpu_baseline" (the CPU oracle timed on the host cores on a bounded sample);
the --no-* options below leave single legs out of a --full run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "f32": 157.3, "bf16x3": 2500.0 / 3}  # dense peaks, /opt/skills/guides/MI355X_MICROARCH.md; bf16x3 = three bf16 MFMAs per product


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--mode", default="sample", choices=["sample", "train"],
                    help="sample = BASELINE configs[2] (denoising-steps/s, the headline metric); train = configs[3] "
                         "(speech_vae_decoder_loss training step, samples/s + all-reduce ms)")
    ap.add_argument("--max-tokens", type=int, default=15000, help="train: per-GPU token budget of a batch (scripts/vae/train.sh:8)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--timesteps", type=int, default=1000)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "bf16x3", "f32"],
                    help="arithmetic of the contractions; f16 (default) = IEEE-half MFMA operands, the 2-byte mode inside north_star's 1e-2 budget")
    ap.add_argument("--full", action="store_true",
                    help="also measure the secondary figures (chain set-up, roofline, profiles' traffic, DDPM chain, other precisions, full "
                         "chain, conditional / refinement / training legs, CPU baseline); a plain run times the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed as DIR/<name>.npy (fp32)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-split", action="store_true", help="one stream per chain instead of two forked half-batches")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-batch", type=int, default=0, help="CPU baseline on a slice of this many sequences (0 = the whole batch)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="cap on host threads of the CPU baseline (0 = every core this process may use)")
    ap.add_argument("--no-full-chain", action="store_true", help="skip the end-to-end 998-evaluation chain leg")
    ap.add_argument("--no-x3", action="store_true", help="skip the split-operand (bf16x3) leg")
    ap.add_argument("--no-train", action="store_true", help="skip the two training legs of the --full line")
    ap.add_argument("--no-refine", action="store_true", help="skip the mask-predict refinement leg (SURVEY 8 f4)")
    ap.add_argument("--no-cond", action="store_true", help="skip the conditional-variant (guided chain) leg (SURVEY 8 f3)")
    ap.add_argument("--train-loss", default="vae", choices=["vae", "diffusion"], help="--mode train: which loss's update is the step")
    ap.add_argument("--no-f32", action="store_true", help="skip the exact-fp32 legs (20 steps + the full chain for the unit agreement)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


DUMP_LIMIT = 64 << 20  # bytes of --dump-outputs in all


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each array (torch tensor or numpy) as out_dir/<name>.npy, fp32 (fp64 stays fp64)."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        if hasattr(a, "detach"):
            a = a.detach().cpu()
            a = (a.double() if a.dtype == torch.float64 else a.float()).numpy()
        a = np.asarray(a, dtype=np.float64 if np.asarray(a).dtype == np.float64 else np.float32)
        total += a.nbytes
        assert total <= DUMP_LIMIT, f"--dump-outputs: more than {DUMP_LIMIT >> 20} MB"
        np.save(os.path.join(out_dir, name + ".npy"), a)


def time_dominant_kernel(ops, _lib, packing, dev, B, T, dtype, iters=20):
    """FFN CausalConv1d(1365,1365,3) as one dn_conv_gemm launch: M = B*T rows, K = 3 x 1408 (padded), N = 1408.
    Returns (avg seconds per launch, algorithmic FLOPs per launch)."""
    import torch

    inner, ip = 1365, packing.padk(1365)
    M = B * T
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16 if dtype == "f16" else torch.float32
    a = torch.randn(M, ip, device=dev)
    a[:, inner:] = 0
    w = torch.randn(3, packing.padn(inner), ip, device=dev) * 0.02
    x3 = dtype == "bf16x3"
    if x3:  # split rows: (hi, lo) bf16 pairs, twice the bf16 count per row
        a, w = packing.split_rows(a.cpu()).to(dev), packing.split_rows(w.cpu(), weight=True).to(dev)
        out = torch.empty(M, 2 * ip, device=dev, dtype=torch.bfloat16)
    else:
        a, w = a.to(tdt), w.to(tdt)
        out = torch.empty(M, ip, device=dev, dtype=tdt)
    bias = torch.zeros(ip, device=dev)
    terms = [(a, w[j], 2 - j) for j in range(3)]
    for _ in range(3):
        ops.conv_gemm(terms, out, T, ip, bias=bias, x3=x3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.conv_gemm(terms, out, T, ip, bias=bias, x3=x3)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters, 2.0 * M * (3 * inner) * inner


def _build_id():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_id import build_id

    return build_id()


def _latest_profile(pattern):
    """(contents, belongs to this build?) of the newest committed profile JSON matching `pattern`; (None, None) when there is none.  The
    counters are collected in separate rocprofv3 --pmc passes (tools/collect_profiles_r03.sh) and committed under profiles/ with the hash
    of the kernel sources they were measured on: a pass that no longer belongs to the kernels being run is flagged, not silently quoted."""
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    if not files:
        return None, None
    try:
        d = json.load(open(files[-1]))
    except (OSError, ValueError):
        return None, None
    return d, (d.get("build_id") == _build_id()) if "build_id" in d else None


def traffic_from_profiles(dtype="bf16"):
    """Fabric-side bytes per launch of the dominant kernel, (2 * FETCH_SIZE + WRITE_SIZE) * 1024 with the gfx950 x2 read correction
    -> (bytes or None, profile matches this build?)."""
    d, ok = _latest_profile("r*_x3_pmc_traffic_ffn_conv*.json" if dtype == "bf16x3" else "r[0-9][0-9]_pmc_traffic_ffn_conv*.json")
    return (d.get("hbm_bytes_per_launch") if d else None), ok


def train_traffic_from_profiles():
    """Fabric-side bytes per launch of the training leg's roofline kernel from the committed PMC passes
    (profiles/*pmc_train_wgrad*.json); None when absent."""
    d, ok = _latest_profile("*pmc_train_wgrad*.json")
    return d.get("hbm_bytes_per_launch") if (d and ok) else None  # (only a measurement of THIS build's kernel: round 2's was the transposed-copies form)


def step_traffic_from_profiles(dtype="bf16"):
    """Fabric-side bytes of one denoising step at [32,512] from the committed PMC passes -> (bytes or None, matches this build?)."""
    d, ok = _latest_profile("r*_x3_pmc_step_traffic.json" if dtype == "bf16x3" else "r[0-9][0-9]_pmc_step_traffic.json")
    return (d.get("bytes_per_step") if d else None), ok


def usable_cores(cap):
    """Threads the CPU leg may use: affinity mask, cgroup CPU quota, and the per-GPU host share (`cap`)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:  # cgroup v2
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:  # cgroup v1
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // per))
        except (OSError, ValueError):
            pass
    return max(1, min(n, cap))


def host_cpu_info():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return model, os.cpu_count() or 1


def cpu_baseline(sd, cfg, B, T, timesteps, sample_b, max_threads):
    """The CPU oracle (a port of the reference's algorithm, pinned to it by tests/golden) on the node's own host cores: every core
    this process may use (affinity mask / cgroup quota; `max_threads` <= 0 = no further cap), un-sliced [B, T] steps of the same
    workload -- one warm-up step, then steps until ~10 s have passed (at least one).  `sample_b` < B times a slice instead."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch

    import diffnorm_oracle as O

    cores = usable_cores(max_threads if max_threads > 0 else 1 << 30)
    torch.set_num_threads(cores)
    ocfg = O.EpsConfig(dim=cfg.dim, latent_dim=cfg.latent_dim, depth=cfg.depth, heads=cfg.heads, dim_head=cfg.dim_head,
                       wavenet_layers=cfg.wavenet_layers, wavenet_stacks=cfg.wavenet_stacks, dim_cond_mult=cfg.dim_cond_mult)
    tab = O.ddpm_tables(timesteps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(sample_b, T, cfg.latent_dim, generator=g)
    mask = torch.ones(sample_b, T, dtype=torch.bool)

    def step(xx, tval):
        t = torch.full((xx.shape[0],), tval, dtype=torch.long)
        return O.ddim_update(tab, xx, O.eps_forward(sd, ocfg, xx, t, mask[: xx.shape[0], : xx.shape[1]]), t)

    with torch.no_grad():
        step(x[:1, :64], 500)  # warm-up (thread pool, allocator)
        n, t0 = 0, time.perf_counter()
        while True:
            x = step(x, timesteps - 2 - n)
            n += 1
            dt = time.perf_counter() - t0
            if dt > 10.0 or n >= 64:
                break
    steps_per_s = n / dt * (sample_b / B)  # sequences are independent: a B-sequence step costs B/sample_b as much
    model, total = host_cpu_info()
    sliced = "" if sample_b == B else f" (a {sample_b}/{B} slice of the batch; rate scaled by {sample_b}/{B})"
    return {"value": steps_per_s, "unit": "denoising-steps/s", "cores": cores, "kind": "port", "host_cores_total": total,
            "cpu_model": model,
            "sample": f"{n} un-sliced step(s) of [{sample_b},{T},{cfg.latent_dim}]{sliced} in {dt:.1f} s, torch {torch.__version__} fp32, "
                      f"{cores} of the host's {total} logical cores (affinity / cgroup limit of this process)"}


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: this parent (which has made NO GPU call) starts N ranks through
    torch.distributed.run on 127.0.0.1 and relays their output; rank 0's JSON line is the result.  Returns the exit code."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def full_chain_legs(args, eng, sd, cfg, dev, stream, B, T, coef, sched):
    """Secondary figures of the same workload (rank 0, N = 1): the config AS STATED end to end -- feats [B,T,768] -> VAE encode ->
    noise at start_step 999 -> 998 evaluations -> VAE decode -> units, wall clock including the per-chain set-up -- in the headline
    dtype, and (unless --no-f32) the exact-fp32 mode: 20 mid-chain steps and the same full chain for the unit agreement."""
    import torch

    from diffnorm_amd import engine, ops, synthetic

    out = {}
    vsd = synthetic.random_vae_state_dict(768, 128, seed=1)
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(B, T, 768, generator=g).to(dev)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    post = ops.randn((B, T, 128), seed=99, device=dev)
    start_noise = ops.randn((B, T, 128), seed=98, device=dev)
    start = args.timesteps - 1
    t_start = torch.full((B,), start, dtype=torch.int32, device=dev)
    sa, s1 = sched.f32("sqrt_alphas_cumprod", dev), sched.f32("sqrt_one_minus_alphas_cumprod", dev)

    def chain(eps_eng, vae_eng):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            z = vae_eng.encode(feat, post)
            x = ops.q_sample(z, start_noise, sa, s1, t_start, T)
            n = eps_eng.ddim_loop(x, lengths, start, coef, use_graph=not args.no_graph, split=not args.no_split)
            recon, _, units = vae_eng.decode(x, lengths, want_logits=False)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, n, x, units

    vae = engine.VaeEngine(vsd, dtype=args.dtype, device=dev)
    chain(eng, vae)  # first call pays graph capture / workspace growth: the timed call below is a steady-state chain
    wall, n, x_main, units_main = chain(eng, vae)
    out["full_chain"] = {"dtype": args.dtype, "evaluations": n, "wall_s": wall, "steps_per_s_incl_setup_and_vae": n / wall,
                         "what": f"feats [{B},{T},768] -> VAE encode -> start_step {start} -> {n} eps-predictor evaluations + DDIM updates "
                                 f"-> VAE decode -> units (conditioning table, graph launch and both VAE ends inside the clock)"}
    del vae
    if args.no_f32 or args.dtype == "f32":
        return out
    eng32 = engine.EpsEngine(sd, cfg, dtype="f32", device=dev)
    vae32 = engine.VaeEngine(vsd, dtype="f32", device=dev)
    with torch.cuda.stream(stream):
        x = ops.randn((B, T, cfg.latent_dim), seed=1234, device=dev)
        eng32.ddim_loop(x, lengths, start, coef, use_graph=not args.no_graph, max_evals=3, split=not args.no_split)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng32.ddim_loop(x, lengths, start - 3, coef, use_graph=not args.no_graph, max_evals=20, split=not args.no_split, keep_table=True)
        torch.cuda.synchronize()
        out["f32_steps_per_s"] = 20 / (time.perf_counter() - t0)
    wall32, n32, x32, units32 = chain(eng32, vae32)
    valid = torch.ones_like(units_main, dtype=torch.bool)
    out["f32_full_chain_wall_s"] = wall32
    out[f"{args.dtype}_vs_f32_after_full_chain"] = {
        "unit_agreement": float((units_main == units32)[valid].float().mean()),
        "latent_rel_rms_diff": float((x_main - x32).pow(2).mean().sqrt() / x32.pow(2).mean().sqrt()),
        "what": f"same features, posterior and start noise through all {n32} evaluations in {args.dtype} and in exact fp32"}
    del eng32, vae32
    if not args.no_x3:  # the split-operand mode through the same full chain (one call: graph capture inside the clock)
        engx, vaex = engine.EpsEngine(sd, cfg, dtype="bf16x3", device=dev), engine.VaeEngine(vsd, dtype="bf16x3", device=dev)
        wallx, nx, xx, unitsx = chain(engx, vaex)
        out["bf16x3_full_chain"] = {"evaluations": nx, "wall_s": wallx, "steps_per_s_incl_setup_and_vae": nx / wallx}
        out["bf16x3_vs_f32_after_full_chain"] = {
            "unit_agreement": float((unitsx == units32)[valid].float().mean()),
            "latent_rel_rms_diff": float((xx - x32).pow(2).mean().sqrt() / x32.pow(2).mean().sqrt()),
            "what": f"the same chain in split-operand bf16x3 and in exact fp32, after all {nx} evaluations"}
    return out


def other_mode_leg(args, dtype, sd, cfg, dev, stream, B, T, coef, lengths):
    """The same chain on the OTHER 2-byte operand type (bf16 when the headline is f16 and vice versa): 20 mid-chain steps after the
    same 3 + 3-step set-up, so the default line carries both rates from one box."""
    import torch

    from diffnorm_amd import engine, ops

    eng = engine.EpsEngine(sd, cfg, dtype=dtype, device=dev)
    start, n_steps = args.timesteps - 1, 20
    with torch.cuda.stream(stream):
        x = ops.randn((B, T, cfg.latent_dim), seed=1234, device=dev)
        eng.ddim_loop(x, lengths, start, coef, use_graph=not args.no_graph, max_evals=3, split=not args.no_split)
        eng.ddim_loop(x, lengths, start - 3, coef, use_graph=not args.no_graph, max_evals=3, split=not args.no_split, keep_table=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ddim_loop(x, lengths, start - 6, coef, use_graph=not args.no_graph, max_evals=n_steps, split=not args.no_split, keep_table=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(x).all().item()
    del eng
    return {f"{dtype}_steps_per_s": n_steps / dt}


def x3_legs(args, sd, cfg, dev, stream, B, T, coef, lengths):
    """The same chain in the split-operand mode (dtype bf16x3: contraction operands as (hi, lo) bf16 pairs, three bf16 MFMAs per
    product, fp32 everywhere else) -- the mode that meets north_star's fp32-column tolerance (1e-3) at matrix-pipe speed: 20
    mid-chain steps after the same 3-step set-up, and its FFN causal-conv contraction timed in the chain with HIP events."""
    import ctypes

    import torch

    from diffnorm_amd import _lib, engine, ops, synthetic

    eng = engine.EpsEngine(sd, cfg, dtype="bf16x3", device=dev)
    start = args.timesteps - 1
    n_steps = 20
    with torch.cuda.stream(stream):
        x = ops.randn((B, T, cfg.latent_dim), seed=1234, device=dev)
        eng.ddim_loop(x, lengths, start, coef, use_graph=not args.no_graph, max_evals=3, split=not args.no_split)
        eng.ddim_loop(x, lengths, start - 3, coef, use_graph=not args.no_graph, max_evals=3, split=not args.no_split, keep_table=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.ddim_loop(x, lengths, start - 6, coef, use_graph=not args.no_graph, max_evals=n_steps, split=not args.no_split, keep_table=True)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert torch.isfinite(x).all().item()
        lib = _lib.load()
        _lib.check(lib.dn_profile_start(_lib.TAG_FFN_CONV, 12 * 3), "dn_profile_start")
        eng.ddim_loop(x, lengths, start - 6 - n_steps, coef, use_graph=False, max_evals=3, split=False)
        avg_ms, n_l = ctypes.c_float(), ctypes.c_int32()
        _lib.check(lib.dn_profile_stop(ctypes.byref(avg_ms), ctypes.byref(n_l)), "dn_profile_stop")
    peak = MFMA_PEAK_TFLOPS["bf16x3"]
    kflops = 2.0 * B * T * (3 * 1365) * 1365
    ach = kflops / (avg_ms.value * 1e-3) / 1e12
    sf = synthetic.eps_step_flops(B, T)
    del eng
    return {"bf16x3_steps_per_s": n_steps / dt,
            "bf16x3": {"steps_per_s": n_steps / dt, "ms_per_step": dt / n_steps * 1e3, "steps": n_steps,
                       "step_tflops_per_gpu": sf * n_steps / dt / 1e12, "step_mfma_frac": sf * n_steps / dt / 1e12 / peak,
                       "what": "same chain, same set-up, contraction operands as (hi, lo) bf16 pairs: a_hi.b_hi + a_lo.b_hi + a_hi.b_lo into one fp32 "
                               "accumulator; peak = dense bf16 MFMA peak / 3 (algorithmic FLOPs, three MFMAs each)",
                       "roofline": {"bound": "mfma", "kernel": f"conv_gemm_big_kernel<bf16x3, BIAS> FFN causal conv k=3 [{B * T} x 4095] x [4095 x 1365]",
                                    "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "flops_per_launch": kflops,
                                    "avg_launch_ms": avg_ms.value, "launches_timed": n_l.value, "traffic": traffic_from_profiles("bf16x3")[0],
                                    "traffic_profile_matches_build": traffic_from_profiles("bf16x3")[1]},
                       "hbm_bytes_per_step": step_traffic_from_profiles("bf16x3")[0]}}


def refine_leg(args, dev, stream):
    """The loop downstream of the normalised units: mask-predict iterative refinement of the NAR S2UT decoder
    (research/TranSpeech/nar_transformer.py: embed 512, FFN 2048, 6 layers, 8 heads, 1004 units) on the HIP engine -- B = 32
    hypotheses of T = 256 target frames against S = 128 encoder frames, 10 refinement iterations (one decoder pass + the CMLM update
    each; the encoder-attention keys / values of all layers computed once per batch), random-init weights, the encoder output a
    given tensor."""
    import torch

    from diffnorm_amd import nar_decoder, synthetic
    from diffnorm_amd.iterative_refinement import DecoderOut

    B, T, S, iters = 32, 256, 128, 10
    sd = synthetic.random_nar_decoder_state_dict(seed=3)
    model = nar_decoder.NARS2UTDecoderModel(sd, dtype=args.dtype if args.dtype != "bf16x3" else "bf16x3", device=dev)
    g = torch.Generator().manual_seed(5)
    enc = {"encoder_out": [torch.randn(S, B, 512, generator=g).to(dev)], "encoder_padding_mask": [], "encoder_embedding": [], "encoder_states": [],
           "src_tokens": [], "src_lengths": []}
    lengths = torch.full((B,), T, dtype=torch.long, device=dev)

    def chain(host_stepped=False):
        state = model.initialize_output_tokens(enc, None, true_length=lengths)
        if not host_stepped:  # one captured iteration (decoder pass + dn_cmlm_step_dev + counter) replayed: no host work between iterations
            return model.refine(state._replace(step=0, max_step=iters), enc, iters)
        for step in range(iters):  # the generator's own stepping: forward_decoder per iteration (each one graph launch + its copies)
            state = model.forward_decoder(state._replace(step=step, max_step=iters), enc)
        return state

    def timed(host_stepped):
        chain(host_stepped)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 5
        for _ in range(reps):
            st = chain(host_stepped)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, st

    with torch.cuda.stream(stream):
        dt_host, st_host = timed(True)
        dt, st = timed(False)
    assert torch.equal(st.output_tokens, st_host.output_tokens)  # the replayed iterations are the host-stepped ones
    # the speech encoder in front of the loop (one pass per utterance batch): [B, 512, 80] fbank frames -> [B, 128, 512]
    enc_eng = nar_decoder.NarEncoderEngine(synthetic.random_nar_encoder_state_dict(seed=4), dtype=args.dtype, device=dev)
    fb = torch.randn(B, 4 * S, 80, generator=g).to(dev)
    fl = torch.full((B,), 4 * S, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        enc_eng.forward(fb, fl)
        torch.cuda.synchronize()
        passes = []
        for _ in range(3):  # the median of three groups of five passes (a single stall of the box once put 15 ms on a 1.2 ms pass)
            t0 = time.perf_counter()
            for _ in range(5):
                eo, _ = enc_eng.forward(fb, fl)
            torch.cuda.synchronize()
            passes.append((time.perf_counter() - t0) / 5 * 1e3)
        enc_ms = sorted(passes)[1]
    assert eo.shape == (B, S, 512) and torch.isfinite(eo).all().item()
    del enc_eng
    assert int(st.output_tokens.ne(3).sum()) == B * T  # every position decided after the last iteration
    flops = B * T * 2.0 * 6 * (4 * 512 * 512 + 2 * 512 * 512 + 2 * 512 * 2048 + 2 * 512 * (T + S)) + B * T * 2.0 * 512 * 1004
    return {"refine": {"iterations_per_s": iters / dt, "ms_per_iteration": dt / iters * 1e3, "ms_per_iteration_host_stepped": dt_host / iters * 1e3, "speech_encoder_ms_per_batch": enc_ms,
                       "hypothesis_frames_per_s": B * T * iters / dt,
                       "dtype": args.dtype, "tflops": flops * iters / dt / 1e12,
                       "what": f"NAR S2UT decoder (512 / 2048 / 6 layers / 8 heads / 1004 units) inside mask-predict refinement: B = {B}, T = {T}, "
                               f"S = {S} encoder frames, {iters} iterations (decoder pass + dn_cmlm_step each): one iteration captured into a hipGraph "
                               f"with the iteration index on the device and replayed; host_stepped = forward_decoder per iteration as the reference's generator calls it"}}


def cond_leg(args, dev, stream, B, T):
    """The conditional variant (use_cond=True: pooled-prompt condition, PerceiverResampler, a cross-attention block per
    layer, classifier-free guidance at scale 2 = conditioned + null rows in ONE 2B-row pass) at the recipe's sizes: guided denoising
    steps per second of the prompted chain, one step captured into a hipGraph and replayed."""
    import torch

    from diffnorm_amd import engine, ops, scheduler, synthetic

    cfg = synthetic.eps_config(dim_prompt=768, num_latents_m=64)
    eng = engine.EpsEngine(synthetic.random_eps_state_dict(cfg, seed=2), cfg, dtype=args.dtype, device=dev)
    Tp = 256
    coef = scheduler.DDPMScheduler(args.timesteps).ddim_coef_table(dev)
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
    plens = torch.full((B,), Tp, dtype=torch.int32, device=dev)
    n = 21
    with torch.cuda.stream(stream):
        x = ops.randn((B, T, cfg.latent_dim), seed=77, device=dev)
        prompt = ops.randn((B, Tp, 768), seed=78, device=dev)
        eng.guided_ddim_chain(x, lengths, prompt, plens, 5, coef, cond_scale=2.0)  # warm-up: workspaces, attributes
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evals = eng.guided_ddim_chain(x, lengths, prompt, plens, n + 1, coef, cond_scale=2.0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # a chain's fixed cost (the time table of its steps, the prompt-only stage, the graph capture) amortises over its length: a
        # second, 4x longer chain separates the per-step time from it
        t0 = time.perf_counter()
        evals4 = eng.guided_ddim_chain(x, lengths, prompt, plens, 4 * n + 1, coef, cond_scale=2.0)
        torch.cuda.synchronize()
        dt4 = time.perf_counter() - t0
        assert torch.isfinite(x).all().item()
    per_step = (dt4 - dt) / (evals4 - evals)
    return {"cond": {"guided_steps_per_s": 1.0 / per_step, "ms_per_guided_step": per_step * 1e3, "chain_fixed_ms": max(0.0, dt - evals * per_step) * 1e3,
                     "ms_per_guided_step_of_a_21_step_chain_incl_fixed": dt / evals * 1e3, "dtype": args.dtype, "cond_scale": 2.0,
                     "what": f"prompted + guided chain of the conditional eps-predictor (dim 512, prompt 768 x {Tp} frames, 64 resampler latents) on [B={B},T={T}] "
                             f"latents: every step = one pass over 2B rows (conditioned ; null) + guidance + DDIM update; per-step time from the difference of a "
                             f"{evals4}- and a {evals}-step chain (the prompt-only stage, the chain's time table and the graph capture are once per chain)"}}


# Which arithmetic mode meets which of north_star's budgets ("1e-3 fp32 / 1e-2 bf16", max-abs vs the reference's fp32 outputs),
# as measured by the -m gpu tests on the reference-generated goldens (tests/test_hip_engine.py; BASELINE config 2 = eps_full_cfg2).
TOLERANCE = {
    "f32": {"budget": 1e-3, "config2_max_abs": 4.8e-6, "meets": True, "arithmetic": "exact fp32 MFMA"},
    "bf16x3": {"budget": 1e-3, "config2_max_abs": 2.9e-5, "meets": True, "arithmetic": "split-operand bf16, 3 MFMAs per product, fp32 accumulate"},
    "f16": {"budget": 1e-2, "config2_max_abs": 1.91e-3, "config2_eps_mse": 1.50e-7, "meets": True,
            "arithmetic": "IEEE-half MFMA operands (v_mfma_f32_16x16x32_f16: the bf16 rate, 11 significand bits), fp32 accumulate; every golden "
                          "asserted at 1e-2 flat (tests/test_hip_engine.py, test_hip_fullsize.py, test_hip_refine.py), no overflow at t in {3, 500, 999} "
                          "(profiles/r04_f16_model_distances.txt), results beyond 65504 saturate"},
    "bf16": {"budget": 1e-2, "config2_max_abs": 1.41e-2, "config2_eps_mse": 1.08e-5, "meets": "eps-MSE yes (config 2's stated criterion); max-abs misses by 1.4x at t = 500",
             "arithmetic": "bf16 MFMA operands, fp32 accumulate"},
    "note": "value (the headline) is quoted in --dtype (default f16: inside the 2-byte budget); bf16_steps_per_s is the same chain on bf16 operands, "
            "bf16x3_steps_per_s the rate of the fastest mode that meets the fp32-column budget (1e-3) on every golden",
}


def run_sampling(args, ctx):
    """BASELINE configs[2]: the DDIM reverse chain (denoising-steps/s)."""
    import torch

    rank, world, dev, rccl_ranks, dist = ctx["rank"], ctx["world"], ctx["dev"], ctx["rccl_ranks"], ctx["dist"]
    from diffnorm_amd import _lib, engine, ops, packing, scheduler, synthetic

    cfg = synthetic.eps_config()
    sd = synthetic.random_eps_state_dict(cfg, seed=0)
    eng = engine.EpsEngine(sd, cfg, dtype=args.dtype, device=dev)
    B, T, K, W = args.batch, args.frames, args.steps, args.warmup
    sched = scheduler.DDPMScheduler(args.timesteps)
    coef = sched.ddim_coef_table(dev)
    start = args.timesteps - 1  # "full 1000-step" chain: t = 998 ... 1 (last bullet)
    if args.full:  # (the secondary legs below continue the chain for 7 more steps)
        assert W + K + 10 <= start - 1, "--full: steps + warmup exceed the chain length"
    x = ops.randn((B, T, cfg.latent_dim), seed=1234 + rank, device=dev)  # x_T ~ N(0, I): the build's Philox
    lengths = torch.full((B,), T, dtype=torch.int32, device=dev)

    stream = torch.cuda.Stream(device=dev)  # graphs cannot be captured on the null stream

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def chain_steps(n, pos, new_chain=False):
        """n more steps of the chain whose next call starts at `pos`; -> the position after them.  A chain keeps its conditioning
        table (built once per chain, for all its steps); one that has run out (its t = 1 update done) is followed by a new chain
        from `start` on the latents as they stand, which builds its table again."""
        while n > 0:
            if pos <= 1:
                pos, new_chain = start, True
            k = min(n, pos - 1)
            got = eng.ddim_loop(x, lengths, pos, coef, use_graph=not args.no_graph, max_evals=k, split=not args.no_split, keep_table=not new_chain)
            assert got == k, (got, k)
            n, pos, new_chain = n - k, pos - k, False
        return pos

    SETUP = 3  # untimed: builds the chain's conditioning table and captures the step graph (the analogue of loading / compiling)
    with torch.cuda.stream(stream):
        pos = chain_steps(SETUP, start, new_chain=True)
        pos = chain_steps(W, pos)
        barrier()
        t0 = time.perf_counter()
        # the timed K steps continue the same chain: its conditioning table (built once per chain, for all 998 steps) is
        # kept, as it would be for the rest of a real chain
        pos = chain_steps(K, pos)
        barrier()
        dt = time.perf_counter() - t0
        assert torch.isfinite(x).all().item(), "state diverged"
    if args.dump_outputs:  # (before the --full legs, which continue the chain)
        dump_outputs(args.dump_outputs, {"latents" if rank == 0 else f"latents_rank{rank}": x})
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = tmax.item()

    if rank == 0:
        step_flops = synthetic.eps_step_flops(B, T)
        peak = MFMA_PEAK_TFLOPS[args.dtype]
        result = {
            "metric": "denoising-steps/sec (BxT latents)", "value": world * K / dt, "unit": "denoising-steps/s",
            "n_gpus": world, "backend": ctx["backend"], "rccl_ranks": rccl_ranks, "process_group_ranks": ctx["group_ranks"], "steps": K, "warmup": W,
            "ms_per_step": dt / K * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"configs[2]: DDIM/DDPM-schedule reverse chain, eps-predictor Model(512, z=128) on "
                                   f"[B={B},T={T}] latents per GPU, {args.timesteps}-step cosine schedule, random-init weights",
                       "batch_per_gpu": B, "frames": T, "latent_dim": cfg.latent_dim, "timesteps": args.timesteps,
                       "hip_graph": not args.no_graph, "half_batch_streams": 1 if args.no_split else 2, "parallelism": f"batch-sharded x{world} (no collective)"},
            "frame_steps_per_s": world * K * B * T / dt,
            "step_tflops_per_gpu": step_flops * K / dt / 1e12,
            "step_mfma_frac": step_flops * K / dt / 1e12 / peak,
        }
        if not args.full:
            print(json.dumps(result), flush=True)
            return
        # once-per-chain work that the timed window (which continues the warm-up's chain) does not contain: the conditioning
        # table for all remaining timesteps.  Timed here: one call that rebuilds it and runs 2 steps, minus 2 steps.
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eng.ddim_loop(x, lengths, pos, coef, use_graph=not args.no_graph, max_evals=2, split=not args.no_split)
            torch.cuda.synchronize()
            chain_setup_ms = max(0.0, (time.perf_counter() - t1) * 1e3 - 2 * dt / K * 1e3)
        with torch.cuda.stream(stream):
            ksec_iso, kflops = time_dominant_kernel(ops, _lib, packing, dev, B, T, args.dtype)
            # the same contraction timed where it runs: HIP events around its launches inside 5 eager chain steps
            import ctypes
            lib = _lib.load()
            _lib.check(lib.dn_profile_start(_lib.TAG_FFN_CONV, 12 * 5), "dn_profile_start")
            eng.ddim_loop(x, lengths, pos - 2, coef, use_graph=False, max_evals=5, split=False)
            avg_ms, n_l = ctypes.c_float(), ctypes.c_int32()
            _lib.check(lib.dn_profile_stop(ctypes.byref(avg_ms), ctypes.byref(n_l)), "dn_profile_stop")
            ksec = avg_ms.value * 1e-3
        achieved = kflops / ksec / 1e12
        result.update({
            "chain_setup_ms": chain_setup_ms,  # conditioning table of a whole chain, built once per chain (not per step)
            "roofline": {"bound": "mfma", "kernel": f"{'conv_gemm_fat_kernel' if args.dtype in ('bf16', 'f16') else 'conv_gemm_big_kernel'}<{args.dtype}, BIAS> FFN causal conv k=3 "
                                                    f"[{B * T} x 4095] x [4095 x 1365]",
                         "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                         "flops_per_launch": kflops, "avg_launch_ms": ksec * 1e3, "launches_timed": n_l.value,
                         "avg_launch_ms_isolated_back_to_back": ksec_iso * 1e3, "traffic": traffic_from_profiles(args.dtype)[0],
                         "traffic_profile_matches_build": traffic_from_profiles(args.dtype)[1]},
        })
        # BASELINE config 2 asks for an HBM rate beside steps/s: the measured fabric-side bytes of one step (PMC, committed under
        # profiles/; an upper bound on HBM bytes, Infinity-Cache hits included) x the measured step rate.  Only for the shape and
        # dtype the passes were collected on.
        sb, sb_ok = step_traffic_from_profiles(args.dtype)
        if sb is not None and (B, T) == (32, 512) and args.dtype in ("f16", "bf16", "bf16x3"):
            result["hbm_bytes_per_step"] = sb
            result["hbm_gbps_per_gpu"] = sb * K / dt / 1e9
            result["hbm_profile_matches_build"] = sb_ok
        # BASELINE configs[2] read literally ("DDPM reverse sampling"): the same chain with the ancestral update of
        # GaussianDiffusion.p_sample, noise drawn in the update kernel (dn_ddpm_loop) -- 20 steps after a 3-step set-up
        if world == 1:
            with torch.cuda.stream(stream):
                gtab = sched.gaussian_table(dev)
                xd = ops.randn((B, T, cfg.latent_dim), seed=4321, device=dev)
                eng.ddpm_loop(xd, lengths, args.timesteps, gtab, seed=11, use_graph=not args.no_graph, max_evals=3, split=not args.no_split)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                eng.ddpm_loop(xd, lengths, args.timesteps - 3, gtab, seed=11, use_graph=not args.no_graph, max_evals=20, split=not args.no_split, keep_table=True)
                torch.cuda.synchronize()
                result["ddpm_steps_per_s"] = 20 / (time.perf_counter() - t1)
                assert torch.isfinite(xd).all().item()
        result["tolerance"] = TOLERANCE
        if world == 1 and not args.no_x3 and args.dtype in ("bf16", "f16"):
            result.update(other_mode_leg(args, "bf16" if args.dtype == "f16" else "f16", sd, cfg, dev, stream, B, T, coef, lengths))
            result.update(x3_legs(args, sd, cfg, dev, stream, B, T, coef, lengths))
        if world == 1 and not args.no_full_chain:
            result.update(full_chain_legs(args, eng, sd, cfg, dev, stream, B, T, coef, sched))
        if world == 1 and not args.no_cond:
            result.update(cond_leg(args, dev, stream, B, T))
        if world == 1 and not args.no_refine:
            result.update(refine_leg(args, dev, stream))
        if world == 1 and not args.no_train:
            del eng
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            result.update(train_legs(args, ctx, stream))
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(sd, cfg, B, T, args.timesteps, min(args.cpu_sample_batch, B) if args.cpu_sample_batch > 0 else B,
                                                  args.cpu_threads)
            result["gpu_over_cpu"] = result["value"] / result["cpu_baseline"]["value"]
        print(json.dumps(result), flush=True)


def make_train_batches(n, max_tokens, dim, vocab, seed, dev):
    """Synthetic (feat, unit) batches of BASELINE configs[3] / SURVEY 8(d) config 4: lengths U[64, 512], feat ~ N(0,1), units
    U{4..1003}; a batch = the longest-first prefix of 64 drawn utterances that fits `max_tokens` padded frames, its size rounded
    down to a multiple of 8 (fairseq's required_batch_size_multiple).  Everything is resident on the device."""
    import torch

    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        lens = torch.randint(64, 513, (64,), generator=g).sort(descending=True).values
        T = int(lens[0])
        B = max(8, min(64, max_tokens // T) // 8 * 8)
        lens = lens[:B]
        mask = torch.arange(T).view(1, -1) < lens.view(-1, 1)
        feat = torch.randn(B, T, dim, generator=g) * mask.unsqueeze(-1)
        unit = torch.randint(4, vocab, (B, T), generator=g) * mask
        out.append({"reduce_target": feat.to(dev), "reduce_target_unit": unit.to(dev, torch.int32),
                    "reduce_target_lengths": lens.to(dev, torch.int32), "ntokens": int(lens.sum()), "n_units": int((unit != 0).sum()),
                    "nsentences": B, "frames": B * T})
    return out


def vae_train_flops(B, T, ntokens):
    """Algorithmic FLOPs of one speech_vae_decoder_loss update on a [B, T] batch (MAC = 2): forward = encode + decode
    (4,849,664 and 272,271,360 + 18,432 T per frame) + the LM head; backward = 2x the contraction work of the
    forward (data + weight gradient), the attention backward 2.5x its forward."""
    M = B * T
    fwd_lin = M * (4849664 + 272271360)  # per-frame contraction work without the T-dependent attention part
    attn = M * 18432 * T
    return 3.0 * fwd_lin + 3.5 * attn


def eps_train_flops(B, T):
    """Algorithmic FLOPs of one ddpm_discrete_loss update on a [B, T] batch (MAC = 2): the eps-predictor forward + backward (3x its
    contraction work, 3.5x its attention), the frozen VAE's encode (forward only) and decode (forward + data gradients: 2x its
    contractions, 3.5x its attention; no weight gradients, diff_discrete.py:79-82)."""
    M = B * T
    eps_lin, eps_attn = M * 283824136.0 + B * 236982272.0, M * 24576.0 * T
    dec_lin, dec_attn = M * 272271360.0, M * 18432.0 * T
    return 3.0 * eps_lin + 3.5 * eps_attn + 2.0 * dec_lin + 3.5 * dec_attn + M * 4849664.0


def measure_training(kind, dtype, max_tokens, K, W, ctx, stream, dump=None):
    """K timed updates of one of the two training losses on this rank's `max_tokens` batches (4 batch shapes cycled, lengths
    U[64,512]); one update = forward, backward, bucketed gradient all-reduce (RCCL when world > 1), clip + Adam, refresh, attention
    dropout on as in the reference's train mode.  kind = "vae": speech_vae_decoder_loss (BASELINE configs[3]); "diffusion":
    ddpm_discrete_loss with the frozen VAE (scripts/diffusion/train.sh).  -> dict of this rank's raw figures."""
    import ctypes
    import types

    import torch

    from diffnorm_amd import _lib, synthetic, training

    rank, world, dev, dist = ctx["rank"], ctx["world"], ctx["dev"], ctx["dist"]
    sd = synthetic.random_vae_state_dict(768, 128, seed=1)
    if kind == "vae":
        eng = training.VaeTrainEngine(sd, dim=768, latent_dim=128, dtype=dtype, device=dev)
        tr = training.VaeTrainer(eng, lr=5e-4, betas=(0.9, 0.98), clip_norm=2.0, warmup_updates=10000, warmup_init_lr=1e-7)
        inner = 2048
    else:
        from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

        vae = SpeechVAEEncoderDecoder(dim=768, latent_dim=128, dtype=dtype).to(dev)
        vae.load_state_dict(sd, strict=True)
        ldm = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 512, 128, timesteps=200, dtype=dtype).to(dev)
        tr = training.DiffusionTrainer(ldm, lr=1e-4, betas=(0.9, 0.98), clip_norm=2.0, warmup_updates=10000, warmup_init_lr=1e-7)
        eng = tr.engine
        inner = 1365
    batches = make_train_batches(4, max_tokens, 768, 1004, 100 + rank, dev)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def step(i):
        b = batches[i % len(batches)]
        if kind == "vae":
            return tr.train_step([b], noises=[("philox", 7 + rank, i << 24)])
        return tr.train_step([b])

    with torch.cuda.stream(stream):
        for i in range(max(W, len(batches))):  # warm-up visits every batch shape once (workspace growth, kernel attributes)
            logged, norm = step(i)
        barrier()
        if os.environ.get("DN_SYNC_DEBUG"):  # diagnostic: warn on every host-synchronising call inside the timed updates
            torch.cuda.set_sync_debug_mode("warn")
        t0 = time.perf_counter()
        for i in range(K):
            logged, norm = step(i)
        if os.environ.get("DN_SYNC_DEBUG"):
            torch.cuda.set_sync_debug_mode("default")
        dt_enqueue = time.perf_counter() - t0  # the host's share: all K updates are enqueued (nothing in an update waits for the GPU)
        barrier()
        dt = time.perf_counter() - t0
        used = [batches[i % len(batches)] for i in range(K)]
        sent, toks, frames = (sum(b[k] for b in used) for k in ("nsentences", "ntokens", "frames"))
        fl = vae_train_flops if kind == "vae" else (lambda B, T, _n: eps_train_flops(B, T))
        flops = sum(fl(b["nsentences"], b["frames"] // b["nsentences"], b["ntokens"]) for b in used)
        assert torch.isfinite(logged).all().item() and torch.isfinite(norm).item(), "training diverged"
        if dump:  # what the last timed update returned, and a fixed sample of the parameters it left (before the kernel timing below)
            idx = torch.randint(0, eng.n_params, (1 << 20,), generator=torch.Generator().manual_seed(0)).sort().values.to(dev)
            sfx = "" if rank == 0 else f"_rank{rank}"
            dump_outputs(dump, {"loss_stats" + sfx: logged, "grad_norm" + sfx: norm.reshape(1), "params_sample" + sfx: eng.master[idx]})
        # the dominant backward kernel, timed where it runs: HIP events around the FFN causal conv's weight-gradient contraction
        # (one per transformer layer of the trained model) inside two more updates of the first batch shape
        # Twice: as the updates above ran it (on the second stream beside the data-gradient chain -- train_engine.hip: WgSide -- so
        # the events also span the launches it shares the GPU with), and alone on the caller's stream (option wgrad_stream = 0): the
        # kernel's own rate, which is what the roofline object quotes.
        lib = _lib.load()
        timed = {}
        for mode in ("overlapped", "alone"):
            with _lib.option("wgrad_stream", 0 if mode == "alone" else _lib.get_option("wgrad_stream")):
                _lib.check(lib.dn_profile_start(_lib.TAG_FFN_CONV_WGRAD, 24), "dn_profile_start")
                for _ in range(2):
                    if kind == "vae":
                        tr.train_step([batches[0]], noises=[("philox", 7 + rank, 1 << 40)])
                    else:
                        tr.train_step([batches[0]])
                k_ms, k_n = ctypes.c_float(), ctypes.c_int32()
                _lib.check(lib.dn_profile_stop(ctypes.byref(k_ms), ctypes.byref(k_n)), "dn_profile_stop")
                timed[mode] = k_ms.value
        ar_ms = 0.0
        if world > 1:  # all-reduce time of one update (buckets timed with events on the side stream)
            tr.reducer.measure = True
            step(0)
            ar_ms = tr.reducer.all_reduce_ms()
            tr.reducer.measure = False
    ip = (inner + 63) // 64 * 64
    return {"dt": dt, "dt_enqueue": dt_enqueue, "sent": float(sent), "toks": float(toks), "frames": float(frames), "flops": flops, "ar_ms": ar_ms,
            "k_flops": 2.0 * ip * (3 * ip) * batches[0]["frames"], "k_ms": timed["alone"], "k_ms_overlapped": timed["overlapped"], "k_n": k_n.value, "k_frames": batches[0]["frames"], "inner": ip,
            "loss": float(logged[0]), "grad_norm": float(norm), "buckets": len(tr.reducer.buckets), "gradient_bytes": eng.n_params * 4}


def train_summary(kind, dtype, max_tokens, K, m, world):
    """The figures of `measure_training` as a JSON object (m: aggregated over ranks)."""
    peak = MFMA_PEAK_TFLOPS[dtype]
    ach = m["k_flops"] / (m["k_ms"] * 1e-3) / 1e12 if m["k_ms"] > 0 else 0.0
    what = ("speech_vae_decoder_loss update of SpeechVAEEncoderDecoder(768, latent 128)" if kind == "vae" else
            "ddpm_discrete_loss update of the eps-predictor Model(512, z=128) through the frozen VAE (260.6 M trained parameters)")
    return {"loss": kind, "workload": f"{what}, synthetic (feat, unit) pairs, lengths U[64,512], --max-tokens {max_tokens} per GPU, Adam(0.9,0.98) "
                                      f"clip 2.0, attention dropout 0.1, random-init weights", "dtype": dtype, "updates": K,
            "samples_per_s": m["sent"] / m["dt"], "tokens_per_s": m["toks"] / m["dt"], "ms_per_update": m["dt"] / K * 1e3, "host_enqueue_ms_per_update": m.get("dt_enqueue", 0.0) / K * 1e3,
            "step_tflops_per_gpu": m["flops"] / m["dt"] / 1e12 / world, "step_mfma_frac": m["flops"] / m["dt"] / 1e12 / world / peak,
            "all_reduce_ms_per_update": m["ar_ms"], "gradient_bytes": m["gradient_bytes"], "buckets": m["buckets"],
            "final_loss": m["loss"], "grad_norm": m["grad_norm"],
            "roofline": {"bound": "mfma", "kernel": f"weight gradient of the FFN causal conv k=3 (inner {m['inner']}): [{m['inner']} x {m['k_frames']}] x "
                                                    f"[{m['k_frames']} x {3 * m['inner']}] over the frames, straight from the row-major operands (wgrad_tn_kernel: "
                                                    f"transposing LDS reads; DN_WGRAD_TN=0: transposed copies + dn_conv_gemm)",
                         "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "flops_per_launch": m["k_flops"],
                         "avg_launch_ms": m["k_ms"], "launches_timed": m["k_n"],
                         "avg_launch_ms_beside_the_data_gradient_chain": m.get("k_ms_overlapped"),
                         "timed": "alone on the caller's stream (option wgrad_stream = 0); in the measured updates it runs on a second stream beside the "
                                  "data-gradient chain and its events span the launches it shares the GPU with",
                         "traffic": train_traffic_from_profiles() if kind == "vae" else None}}


def train_legs(args, ctx, stream):
    """Both training losses inside the DEFAULT line (rank 0, N = 1): 10 VAE updates at --max-tokens 15000 and 5 diffusion updates at
    --max-tokens 12000 (scripts/vae/train.sh:8, scripts/diffusion/train.sh:5-9), so the driver's run observes them."""
    out = {}
    for kind, mt, K in (("vae", 15000, 10), ("diffusion", 12000, 5)):
        tdt = args.dtype if args.dtype in ("bf16", "f32") else "bf16"  # the training engines run bf16 / f32 (the reference trains in fp32)
        m = measure_training(kind, tdt, mt, K, 2, ctx, stream)
        out[kind] = train_summary(kind, tdt, mt, K, m, 1)
        import gc

        import torch
        gc.collect()
        torch.cuda.empty_cache()
    return {"train": out}


def run_training(args, ctx):
    """BASELINE configs[3]: speech_vae_decoder_loss training (or, with --train-loss diffusion, ddpm_discrete_loss), one update per
    step: forward, backward, bucketed gradient all-reduce (RCCL), clip + Adam, refresh.  value = sentences / s over all ranks (weak
    scaling: every rank has its own `--max-tokens` batch)."""
    import torch

    rank, world, dev, rccl_ranks, dist = ctx["rank"], ctx["world"], ctx["dev"], ctx["rccl_ranks"], ctx["dist"]
    K, W = args.steps, args.warmup
    stream = torch.cuda.Stream(device=dev)
    if args.dtype not in ("bf16", "f32"):
        args.dtype = "bf16"  # the training engines run bf16 / f32 (the reference trains in fp32); the line's dtype says which ran
    torch.manual_seed(rank)  # (the diffusion loss draws its timesteps with torch's generator)
    m = measure_training(args.train_loss, args.dtype, args.max_tokens, K, W, ctx, stream, dump=args.dump_outputs)
    keys = ["dt", "sent", "toks", "frames", "flops", "ar_ms"]
    vals = torch.tensor([m[k] for k in keys], dtype=torch.float64, device=dev if world > 1 and dist.get_backend() == "nccl" else "cpu")
    if world > 1:
        tmax = vals[:1].clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(vals)
        vals[0] = tmax[0]
        vals[5] /= world
    m.update({k: float(v) for k, v in zip(keys, vals)})
    if rank == 0:
        t = train_summary(args.train_loss, args.dtype, args.max_tokens, K, m, world)
        result = {
            "metric": f"training samples/sec ({'speech_vae_decoder_loss' if args.train_loss == 'vae' else 'ddpm_discrete_loss'})",
            "value": t["samples_per_s"], "unit": "samples/s", "n_gpus": world,
            "backend": ctx["backend"], "rccl_ranks": rccl_ranks, "process_group_ranks": ctx["group_ranks"], "steps": K, "warmup": W,
            "ms_per_step": t["ms_per_update"], "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("configs[3]: " if args.train_loss == "vae" else "") + t["workload"], "max_tokens_per_gpu": args.max_tokens,
                       "parallelism": f"dp{world} ({'RCCL' if ctx['backend'] == 'rccl' else ctx['backend']} gradient all-reduce, {t['buckets']} buckets)"},
            "tokens_per_s": t["tokens_per_s"], "padded_frames_per_s": m["frames"] / m["dt"], "all_reduce_ms_per_update": t["all_reduce_ms_per_update"],
            "gradient_bytes": t["gradient_bytes"], "step_tflops_per_gpu": t["step_tflops_per_gpu"], "step_mfma_frac": t["step_mfma_frac"],
            "host_enqueue_ms_per_update": t["host_enqueue_ms_per_update"],
            "loss": t["final_loss"], "grad_norm": t["grad_norm"], "roofline": t["roofline"],
        }
        print(json.dumps(result), flush=True)


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args))
    if int(env_world or "1") != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={env_world}: launch with "
                 f"`python -m torch.distributed.run --nproc-per-node {args.gpus} bench.py --gpus {args.gpus} ...` or plain `python bench.py --gpus N`")
    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the product path has no CPU fallback)"
    dev_index = local_rank % torch.cuda.device_count()  # == local_rank on a node with one GPU per rank
    if world > 1:
        # RCCL ("nccl") is the contract; DN_BENCH_BACKEND=gloo only rehearses the N > 1 control flow with several ranks
        # sharing one GPU (RCCL refuses duplicate devices).  The data path has no collective either way.
        backend = os.environ.get("DN_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend=backend)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    # `backend`: what carried the collectives of this run ("none" for one rank).  `rccl_ranks` is a statement about RCCL and is
    # null under any other backend: a gloo rehearsal on one GPU must not read as an RCCL run.
    backend_name, group_ranks = "none", 1
    if world > 1:  # the ranks the collective backend actually connected: must be the N that was asked for
        backend_name = dist.get_backend()
        ones = torch.ones(1, device=dev if backend_name == "nccl" else "cpu")
        dist.all_reduce(ones)
        group_ranks = int(ones.item())
        if group_ranks != args.gpus:
            sys.exit(f"bench.py: {group_ranks} ranks joined the process group, --gpus {args.gpus} expected")
    rccl_ranks = group_ranks if (world == 1 or backend_name == "nccl") else None

    ctx = dict(rank=rank, world=world, dev=dev, rccl_ranks=rccl_ranks, dist=dist if world > 1 else None,
               backend="rccl" if backend_name == "nccl" else backend_name, group_ranks=group_ranks)
    if args.mode == "train":
        run_training(args, ctx)
    else:
        run_sampling(args, ctx)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
