#!/usr/bin/env python3
"""Times the HuBERT front end: 16 utterances of 10 s at the recipe's size (mHuBERT base), output layer 11, in f16 and f32,
against the plain-torch restatement (tests/hubert_ref.py) through torch-ROCm one utterance at a time -- the reference reader's shape.
Three alternating blocks behind a warm-up; prints the median and the spread of each, the times-real-time of the median, and the
engine's per-stage split (dn_hubert_set_profile).
Usage: python tools/hubert_bench.py [--utts 16] [--seconds 10] [--layer 11] [--iters 5]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hubert_ref as R  # noqa: E402

from diffnorm_amd import hubert, synthetic  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--layer", type=int, default=11)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    cfg, dev = hubert.MHUBERT_BASE, "cuda:0"
    sd = synthetic.random_hubert_state_dict(cfg, 0)
    n = int(a.seconds * 16000)
    waves = torch.stack([R.make_wave(n, 10 + i) for i in range(a.utts)])
    lens = torch.full((a.utts,), n, dtype=torch.int32)
    audio_s = a.utts * a.seconds
    for dtype, tdt in (("f16", torch.float16), ("f32", torch.float32)):
        eng = hubert.HubertEngine(sd, cfg, dtype=dtype, device=dev)
        wd, ld = waves.to(dev), lens.to(dev)
        sd_dev = {k: v.to(dev, tdt) for k, v in sd.items()}

        def ours():
            eng.forward(wd, ld, a.layer)

        def torch_ref():
            with torch.no_grad():
                for i in range(a.utts):
                    R.extract_features(sd_dev, cfg, wd[i], a.layer, tdt)

        ours(); torch_ref()  # warm-up: allocations, kernel loading
        blocks = {"engine": [], "torch": []}
        for _ in range(3):
            blocks["engine"].append(timed(ours, a.iters))
            blocks["torch"].append(timed(torch_ref, max(1, a.iters // 2)))
        eng.set_profile(True)
        ours()
        split = eng.stage_times()
        eng.set_profile(False)
        print(f"{dtype} stages (ms): " + ", ".join(f"{n} {t:.2f}" for n, t in zip(eng.STAGES, split)))
        for name, v in blocks.items():
            med = statistics.median(v)
            print(f"{dtype} {name}: {med:.2f} ms per batch of {audio_s:.0f} s (min {min(v):.2f}, max {max(v):.2f}) = {audio_s * 1e3 / med:.0f} x real time")


if __name__ == "__main__":
    main()
