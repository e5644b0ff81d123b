"""Times the optimizer step with and without the EMA of the parameters at the two models' real parameter counts:

  adam        dn_adam_step                      (30 B per parameter + 2 B for the bf16 copy)
  fused       dn_adam_step_ema                  (+ 8 B: the EMA read and written in the same pass)
  separate    dn_adam_step + dn_ema_update      (+ 12 B and a launch)

Five alternating repetitions (adam, fused, separate, adam, ...), each the mean of `--iters` back-to-back launches between two
events after a warm-up; prints median and range per variant and one JSON line.  `--lib PATH` loads another build of the library
(e.g. the parent commit's) for the `adam` row: run it alternately with this build's on one machine to compare the unchanged path.

    python tools/ema_bench.py [--n 138000000 260000000] [--iters 100] [--reps 5] [--lib path/to/libdiffnorm_hip.so]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffnorm_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[138_000_000, 260_000_000], help="parameter counts (the VAE's and the diffusion model's)")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None, help="another build of libdiffnorm_hip.so (only the rows it exports are timed)")
    ap.add_argument("--no-bf16-copy", action="store_true")
    a = ap.parse_args()
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
        if not hasattr(C.CDLL(_lib.LIB_PATH), "dn_adam_step_ema"):
            for name in ("dn_adam_step_ema", "dn_ema_update"):
                _lib.SYMBOLS.pop(name)
    lib = _lib.load()
    have_ema = "dn_ema_update" in _lib.SYMBOLS
    dev = torch.device("cuda:0")
    stream = _lib.current_stream()
    out = {"lib": _lib.LIB_PATH, "iters": a.iters, "reps": a.reps, "sizes": {}}
    for n in a.n:
        p, g, m, v, e = (torch.randn(n, device=dev) * s for s in (1.0, 1e-2, 1e-3, 1e-6, 1.0))
        v.abs_()
        bf = None if a.no_bf16_copy else torch.empty(n, dtype=torch.bfloat16, device=dev)
        scratch = torch.empty(1025, device=dev)
        _lib.check(lib.dn_grad_sumsq(g.data_ptr(), n, scratch.data_ptr(), scratch[1024:].data_ptr(), 0, stream), "dn_grad_sumsq")
        hp = _lib.AdamParams(lr=1e-6, beta1=0.9, beta2=0.98, eps=1e-8, max_norm=2.0, step=100, grad_scale=1.0)
        head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, C.byref(hp), scratch[1024:].data_ptr(), _lib.ptr(bf))
        adam = lambda: _lib.check(lib.dn_adam_step(*head, stream), "dn_adam_step")
        variants = {"adam": adam}
        if have_ema:
            variants["fused"] = lambda: _lib.check(lib.dn_adam_step_ema(*head, e.data_ptr(), 0.9999, stream), "dn_adam_step_ema")
            variants["separate"] = lambda: (adam(), _lib.check(lib.dn_ema_update(e.data_ptr(), p.data_ptr(), n, 0.9999, stream), "dn_ema_update"))
        times = {k: [] for k in variants}
        for fn in variants.values():  # warm-up: code objects loaded, clocks up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) / a.iters)
        row = {}
        for k, ts in times.items():
            row[k] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
            print(f"n = {n:>11,d}  {k:<9s} median {row[k]['median_ms']:.4f} ms   range [{min(ts):.4f}, {max(ts):.4f}]")
        if have_ema:
            print(f"n = {n:>11,d}  fused / adam = {row['fused']['median_ms'] / row['adam']['median_ms']:.3f} (bytes: 38/30 = 1.267, 40/32 = 1.25 with the "
                  f"bf16 copy)   separate / fused = {row['separate']['median_ms'] / row['fused']['median_ms']:.3f}")
        out["sizes"][str(n)] = row
        del p, g, m, v, e, bf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
