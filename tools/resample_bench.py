#!/usr/bin/env python3
"""Times the device resampler: 16 utterances of 10 s at 48 kHz, 24 kHz and 44.1 kHz to 16 kHz, fp32 mono and int16
stereo, against the plain float32 torch restatement of the same steps (tests/resample_ref.py: F.conv1d at stride `orig` over the
padded batch) through torch-ROCm, and, in the same alternating blocks, the two consumers on the resampled batch: Kaldi fbank + CMVN
and the mHuBERT base front end (random weights, f16).  Three alternating blocks of five calls behind a warm-up; prints the median and
the spread of each and the share of `resample + fbank` and of `resample + HuBERT` the resampler takes.
Usage: python tools/resample_bench.py [--utts 16] [--seconds 10] [--iters 5] [--no-consumers]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_ref as R  # noqa: E402

from diffnorm_amd import fbank, hubert, resample, synthetic  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def report(name, v, audio_s):
    med = statistics.median(v)
    print(f"{name}: {med:.3f} ms per batch of {audio_s:.0f} s (min {min(v):.3f}, max {max(v):.3f}) = {audio_s * 1e3 / med:.0f} x real time")
    return med


def conv1d_restatement(batch, orig, new, bank):
    """The restatement's steps on a [B, L] device batch of full-length rows: pad (width, width + orig), conv1d at stride orig,
    interleave the phases, cut."""
    o, n, _, width, K = R.geometry(orig, new)
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(batch[:, None, :], (width, width + o)), bank.view(n, 1, K), stride=o)
    return y.transpose(1, 2).reshape(batch.shape[0], -1)[:, : R.out_length(o, n, batch.shape[1])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-consumers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench: no GPU visible: a time is measured on the device or not at all")
    dev, audio_s = "cuda:0", a.utts * a.seconds
    consumers = {}
    if not a.no_consumers:
        n16 = int(a.seconds * 16000)
        w16 = torch.stack([R.noise_wave(n16, 90 + i) for i in range(a.utts)]).to(dev)
        l16 = torch.full((a.utts,), n16, dtype=torch.int32, device=dev)
        fb = fbank.FbankEngine(fbank.FbankConfig(input_scale=32768.0), device=dev)
        hb = hubert.HubertEngine(synthetic.random_hubert_state_dict(hubert.MHUBERT_BASE, 0), hubert.MHUBERT_BASE, dtype="f16", device=dev)
        consumers = {"fbank + CMVN at 16 kHz": lambda: fb.forward(w16, l16), "mHuBERT base, layer 11, f16 at 16 kHz": lambda: hb.forward(w16, l16, 11)}
    for rate in (48000, 24000, 44100):
        n = int(a.seconds * rate)
        rs = resample.Resampler(rate, 16000, device=dev)
        orig, new = rs.cfg.reduced
        mono = torch.stack([R.noise_wave(n, 10 + i) for i in range(a.utts)])
        stereo = (torch.stack([mono, mono.flip(0)], 2) * 32767.0).round().to(torch.int16)
        lens = torch.full((a.utts,), n, dtype=torch.int32, device=dev)
        md, sd, bank = mono.to(dev), stereo.to(dev), rs.tensors[0]
        cases = {"engine, fp32 mono": lambda: rs.forward(md, lens),
                 "engine, int16 stereo": lambda: rs.forward(sd, lens),
                 "torch-ROCm float32 conv1d, fp32 mono": lambda: conv1d_restatement(md, orig, new, bank),
                 "torch-ROCm float32 conv1d, int16 stereo": lambda: conv1d_restatement((sd.float() * 2.0 ** -15).mean(2), orig, new, bank)}
        cases.update(consumers)
        for fn in cases.values():
            fn()  # warm-up: allocations, kernel loading, the convolution's plan
        blocks = {k: [] for k in cases}
        for _ in range(3):
            for k, fn in cases.items():
                blocks[k].append(timed(fn, a.iters))
        head = f"{rate} -> 16000 ({orig} : {new}, K = {rs.cfg.taps}, bank in {'LDS' if rs.table_in_lds else 'global memory'}, tile {rs.tile})"
        med = {k: report(k if k in consumers else f"{head}, {k}", v, audio_s) for k, v in blocks.items()}
        for k in consumers:
            print(f"{rate} -> 16000: the resampler (fp32 mono) is {med['engine, fp32 mono'] / (med['engine, fp32 mono'] + med[k]):.1%} of resample + {k.split(',')[0].split(' at')[0]}")


if __name__ == "__main__":
    main()
