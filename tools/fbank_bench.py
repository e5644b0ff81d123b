#!/usr/bin/env python3
"""Times the Kaldi fbank + utterance CMVN front end: 16 utterances of 10 s at 16 kHz, with and without CMVN, against
(a) the plain float32 torch restatement (tests/fbank_ref.py) through torch-ROCm, batched, and (b) the same restatement on the CPU one
utterance at a time -- the shape of the reference's loader -- and, in the same alternating blocks, both speech encoders at the recipe's
sizes (random weights, f16) on the features.  Three alternating blocks of five calls behind a warm-up; prints the median and the
spread of each and the share of `fbank + encoder` the front end takes.
Usage: python tools/fbank_bench.py [--utts 16] [--seconds 10] [--iters 5] [--no-encoders]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fbank_ref as R  # noqa: E402

from diffnorm_amd import _lib, fbank, nar_decoder, synthetic  # noqa: E402


def timed(fn, iters, sync=True):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def report(name, v, audio_s):
    med = statistics.median(v)
    print(f"{name}: {med:.3f} ms per batch of {audio_s:.0f} s (min {min(v):.3f}, max {max(v):.3f}) = {audio_s * 1e3 / med:.0f} x real time")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--no-encoders", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fbank_bench: no GPU visible: a time is measured on the device or not at all")
    dev, n = "cuda:0", int(a.seconds * 16000)
    waves = torch.stack([torch.from_numpy(R.parity_wave(n, 10 + i)).float() for i in range(a.utts)])
    lens = torch.full((a.utts,), n, dtype=torch.int32)
    wd, ld = waves.to(dev), lens.to(dev)
    audio_s = a.utts * a.seconds
    encoders = {}
    if not a.no_encoders:  # both speech encoders at the recipe's sizes, timed in the same alternating blocks as the front end
        import conformer_ref as CR

        ccfg = CR.RECIPE2.__class__(**{**vars(CR.RECIPE2), "layers": 12})
        feats, flens = fbank.FbankEngine(device=dev).forward(wd, ld)
        tenc = nar_decoder.NarEncoderEngine(synthetic.random_nar_encoder_state_dict(seed=4), dtype="f16", device=dev)
        cenc = nar_decoder.ConformerEncoderEngine(CR.make_state_dict(ccfg, 31), dtype="f16", device=dev)
        encoders = {"transformer encoder (12 layers, f16)": (lambda: tenc.forward(feats, flens), True, a.iters),
                    "conformer encoder (12 layers, f16)": (lambda: cenc.forward(feats, flens), True, a.iters)}
    for cmvn in (False, True):
        eng = fbank.FbankEngine(fbank.FbankConfig(cmvn=cmvn), device=dev)
        post32 = (lambda x: R.cmvn32_torch(x)) if cmvn else (lambda x: x)
        # "engine" is FbankEngine.forward as a caller sees it: the launches plus its host work (two output allocations, the
        # workspace query); "C entry" is dn_fbank_forward alone into preallocated buffers
        B, L = wd.shape
        out = torch.empty(B, eng.out_frames(L), eng.n_mels, device=dev)
        ol = torch.empty(B, dtype=torch.int32, device=dev)
        wp, wn = eng._aligned(eng._workspace(int(eng.lib.dn_fbank_workspace_bytes(eng.handle, B, L))))
        stream = _lib.current_stream()
        c_entry = lambda: _lib.check(eng.lib.dn_fbank_forward(eng.handle, wd.data_ptr(), ld.data_ptr(), B, L, out.data_ptr(), ol.data_ptr(), wp, wn, stream))
        cases = {"engine": (lambda: eng.forward(wd, ld), True, a.iters),
                 "C entry": (c_entry, True, a.iters),
                 "torch-ROCm float32, batched": (lambda: post32(R.fbank32_torch(wd)), True, a.iters),
                 "torch CPU float32, one utterance at a time": (lambda: [post32(R.fbank32_torch(w)) for w in waves], False, 1)}
        if cmvn:
            cases.update(encoders)
        for fn, _, _ in cases.values():
            fn()  # warm-up: allocations, kernel loading, FFT plans
        blocks = {k: [] for k in cases}
        for _ in range(3):
            for k, (fn, sync, iters) in cases.items():
                blocks[k].append(timed(fn, iters, sync))
        med = {}
        for k, v in blocks.items():
            name = k if k in encoders else f"{'fbank + CMVN' if cmvn else 'fbank (raw log-mel)'}, {k}"
            med[k] = report(name, v, audio_s)
        for k in encoders if cmvn else ():
            print(f"fbank + CMVN is {med['engine'] / (med['engine'] + med[k]):.1%} of fbank + {k.split(' (')[0]}")

if __name__ == "__main__":
    main()
