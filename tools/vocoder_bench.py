"""Times the CodeHiFiGAN unit vocoder at the full-size configuration (tests/vocoder_ref.FULL_CFG, generated weights): 16 utterances
of 150-250 units, duration prediction on (the durations are what the generated predictor gives; the sample count is printed):
  a  the HIP engine, f16 (half operands, fp32 accumulation)      b  the HIP engine, f32
  c  tests/vocoder_ref.py on the GPU through torch-ROCm's own convs, one utterance at a time like the reference, the whole
     generator in torch.float16: half weights, half STORAGE of activations, residuals and bias adds -- less traffic and less
     precision than (a), which stores fp32 and rounds only the conv operands (the duration predictor is fp32 in both)
  d  the same in f32
(c) / (d) are the only baseline there is: the library had no vocoder before.  Protocol (README "how numbers are taken"): every leg
warmed up, then alternating blocks of calls per leg, a synchronised host clock around each call; the median in ms per batch, the
spread (max - min) / median, samples / s and x real time at 16 kHz.  For (a) and (b) also the per-stage times of one profiled pass
(events between the stages: dn_voc_set_profile).  Prints one JSON line.

    python tools/vocoder_bench.py [--utts 16] [--blocks 3] [--calls 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import torch

    import vocoder_ref as R
    from diffnorm_amd import vocoder as V

    dev = torch.device("cuda:0")
    cfg = R.FULL_CFG
    sd = R.make_state_dict(cfg, R.FULL_SEED)
    g = torch.Generator().manual_seed(7)
    units = [torch.randint(0, cfg["num_embeddings"], (int(torch.randint(150, 251, (1,), generator=g)),), generator=g) for _ in range(a.utts)]
    engines = {dt: V.CodeHiFiGANVocoder(sd, cfg, dtype=dt, device=dev) for dt in ("f16", "f32")}
    folded = {dt: {k: v.to(dev) for k, v in R.fold(sd, dt).items()} for dt in (torch.float16, torch.float32)}

    def torch_leg(dt):
        # the duration predictor in fp32 in both (the engine's rule), the generator in `dt`
        with torch.no_grad():
            out = []
            for u in units:
                dur = R.durations_from_log(R.log_durations(folded[torch.float32], cfg, folded[torch.float32]["dict.weight"][u.to(dev)][None]))
                out.append(R.vocode(sd, cfg, u, True, dtype=dt, device=dev, folded=folded[dt], durations=dur)[0])
            return out

    legs = {"a_engine_f16": lambda: engines["f16"].generate(units, True), "b_engine_f32": lambda: engines["f32"].generate(units, True),
            "c_torch_f16": lambda: torch_leg(torch.float16), "d_torch_f32": lambda: torch_leg(torch.float32)}
    samples = {}
    for name, fn in legs.items():  # warm-up (allocations, kernel selection)
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        samples[name] = int(sum(w.numel() for w in out))
    times = {k: [] for k in legs}
    for _ in range(a.blocks):
        for name, fn in legs.items():
            for _ in range(a.calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
    res = {"utterances": a.utts, "units": int(sum(u.numel() for u in units)), "calls_per_leg": a.blocks * a.calls}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"ms_per_batch": round(med, 3), "spread": round((max(ts) - min(ts)) / med, 3), "samples": samples[name],
                     "samples_per_s": round(samples[name] / med * 1e3), "x_real_time_16k": round(samples[name] / 16000 / (med * 1e-3), 1)}
    for dt in ("f16", "f32"):
        eng = engines[dt].engine
        eng.set_profile(True)
        engines[dt].generate(units, True)
        stages = eng.stage_times()
        eng.set_profile(False)
        res["stages_ms_" + dt] = {"embed+conv_pre": round(stages[0], 3), **{f"stage{i + 1}": round(t, 3) for i, t in enumerate(stages[1:-1])},
                                  "conv_post": round(stages[-1], 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
