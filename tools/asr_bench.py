#!/usr/bin/env python3
"""Times the wav2vec 2.0 CTC recogniser: 16 utterances of 10 s on the full-size configuration (wav2vec 2.0 large: 24
pre-norm layers, LayerNorm extractor, 32 letters; seeded synthetic weights), in f16 and f32, against the plain-torch restatement
(tests/wav2vec_ref.py) through torch-ROCm one utterance at a time -- the shape of the reference's transcribe loop.  Three
alternating blocks behind a warm-up; prints the median and the spread of each, the times-real-time of the median, the engine's
per-stage split (dn_hubert_set_profile; its fifth stage is final norm + head) and the decode launch timed by events of its own.
Usage: python tools/asr_bench.py [--utts 16] [--seconds 10] [--layers 24] [--iters 3]"""
import argparse
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wav2vec_ref as W  # noqa: E402

from diffnorm_amd import asr, hubert  # noqa: E402


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
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    cfg, dev = types.SimpleNamespace(**dict(vars(hubert.WAV2VEC2_LARGE), encoder_layers=a.layers)), "cuda:0"
    sd = W.make_state_dict(cfg, 0)
    n = int(a.seconds * 16000)
    waves = torch.stack([W.R.make_wave(n, 10 + i) for i in range(a.utts)])
    lens = torch.full((a.utts,), n, dtype=torch.int32)
    audio_s = a.utts * a.seconds
    for dtype, tdt in (("f16", torch.float16), ("f32", torch.float32)):
        eng = asr.Wav2VecCtcEngine(sd, cfg, W.TOKENS, dtype=dtype, device=dev)
        wd, ld = waves.to(dev), lens.to(dev)
        sd_dev = {k: v.to(dev, tdt) for k, v in sd.items()}

        def ours():
            eng.forward(wd, ld)

        def torch_ref():
            with torch.no_grad():
                for i in range(a.utts):
                    W.emissions(sd_dev, cfg, wd[i], tdt).argmax(-1)

        ours(); torch_ref()  # warm-up: allocations, kernel loading
        blocks = {"engine": [], "torch": []}
        for _ in range(3):
            blocks["engine"].append(timed(ours, a.iters))
            blocks["torch"].append(timed(torch_ref, max(1, a.iters // 2)))
        eng.set_profile(True)
        em, olens = eng.emissions(wd, ld)
        split = eng.stage_times()
        eng.set_profile(False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.decode(em, olens)
        e1.record()
        torch.cuda.synchronize()
        print(f"{dtype} stages (ms): " + ", ".join(f"{s} {t:.2f}" for s, t in zip(eng.STAGES, split)) + f", CTC decode (fill + launch) {e0.elapsed_time(e1):.3f}")
        for name, v in blocks.items():
            med = statistics.median(v)
            print(f"{dtype} {name}: {med:.2f} ms per batch of {audio_s:.0f} s (min {min(v):.2f}, max {max(v):.2f}) = {audio_s * 1e3 / med:.0f} x real time")
        del eng, sd_dev


if __name__ == "__main__":
    main()
