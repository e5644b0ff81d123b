#!/usr/bin/env python3
"""Times the VAE training update (bench.py's measure_training: the recipe-sized SpeechVAEEncoderDecoder at --max-tokens 15000,
attention dropout on) in one arithmetic mode and prints one JSON line with ms per update.  bench.py --mode train coerces its
dtype to bf16; this is how the split-operand training mode (bf16x3) and the exact-fp32 one are put side by side.
    python tools/train_x3_bench.py --dtype bf16x3 [--steps 20] [--warmup 4] [--max-tokens 15000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16x3", choices=["bf16x3", "f32", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--max-tokens", type=int, default=15000)
    a = ap.parse_args()
    import torch

    import bench

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ctx = {"rank": 0, "world": 1, "dev": dev, "dist": None}
    m = bench.measure_training("vae", a.dtype, a.max_tokens, a.steps, a.warmup, ctx, torch.cuda.Stream(device=dev))
    print(json.dumps({"kind": "vae", "dtype": a.dtype, "max_tokens": a.max_tokens, "steps": a.steps,
                      "ms_per_update": m["dt"] / a.steps * 1e3, "loss": m["loss"], "grad_norm": m["grad_norm"]}))


if __name__ == "__main__":
    main()
