"""Device BLEU statistics against their host restatement, in one process; prints one JSON line.

Corpora (those of tools/edit_distance_bench.py):
  a  400 pairs with the synthetic length distribution of tools/normalize_bench.py (log-normal, clipped to [58, 1024], seeds 1 / 2), alphabet 1000
  b  32 pairs of 8192 x 8192, alphabet 1000
Legs, timed in alternating blocks behind a warm-up; per leg the median and (max - min) / median of its blocks:
  kernel  dn_bleu_stats alone on device tensors (one launch per call, events around `--iters` calls)
  lists   metrics.bleu_stats from host lists, upload through the pinned staging buffer and the copy back of [B, 10] included
          (host clock around a call that ends in the copy)
  host    the collections.Counter restatement tests/bleu_ref.py over the same lists
Reported: host / lists and host / kernel, and whether host / lists exceeds the legs' spread.  There is no threshold to meet and no
torch baseline: torch has no comparable operator."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)


def summary(xs):
    med = statistics.median(xs)
    return {"median_ms": 1e3 * med, "spread": (max(xs) - min(xs)) / med, "blocks": len(xs)}


def host_time(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="device launches per timed block of the kernel leg")
    a = ap.parse_args()
    import torch

    import bleu_ref as R
    from diffnorm_amd import _lib
    from diffnorm_amd import metrics as M
    from normalize_bench import corpus_lengths

    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    lib = _lib.load()
    out = {"tool": "bleu_bench", "blocks": a.blocks, "iters": a.iters}

    def leg(lens_h, lens_r, alphabet):
        hyp = [rng.randint(0, alphabet, n).tolist() for n in lens_h]
        ref = [rng.randint(0, alphabet, n).tolist() for n in lens_r]
        for h, r in zip(hyp, ref):  # a shared stretch, so that every order has matches
            k = min(len(h), len(r)) // 2
            h[:k] = r[:k]
        B = len(hyp)
        (th, hl, tr, rl), _ = M._sides([("hyp", hyp, None), ("ref", ref, None)], dev)
        stats = torch.empty(B, _lib.BLEU_STATS, dtype=torch.int32, device=dev)
        ws = torch.empty(16, dtype=torch.int32, device=dev)
        stream = _lib.current_stream()

        def kernel():
            _lib.check(lib.dn_bleu_stats(th.data_ptr(), th.shape[1], hl.data_ptr(), tr.data_ptr(), tr.shape[1], rl.data_ptr(), B, stats.data_ptr(),
                                         ws.data_ptr(), ws.numel() * 4, stream), "dn_bleu_stats")

        def kernel_time():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.iters):
                kernel()
            stop.record()
            stop.synchronize()
            return start.elapsed_time(stop) / 1e3 / a.iters

        lists = lambda: M.bleu_stats(hyp, ref).cpu()
        host = lambda: [R.stats(h, r) for h, r in zip(hyp, ref)]
        want = host()
        assert lists().tolist() == want, "the device and the restatement disagree"
        kernel()
        assert stats.cpu().tolist() == want
        for _ in range(3):  # warm-up: allocations, code load
            kernel()
            lists()
        torch.cuda.synchronize()
        times = {"kernel": [], "lists": [], "host": []}
        order = ["kernel", "lists", "host"]
        for k in range(a.blocks):
            for name in order[k % 3:] + order[: k % 3]:
                times[name].append(kernel_time() if name == "kernel" else host_time(lists if name == "lists" else host))
        res = {name: summary(xs) for name, xs in times.items()}
        res["tokens"] = int(sum(lens_h) + sum(lens_r))
        res["host_over_lists"] = res["host"]["median_ms"] / res["lists"]["median_ms"]
        res["host_over_kernel"] = res["host"]["median_ms"] / res["kernel"]["median_ms"]
        worst = max(res["host"]["spread"], res["lists"]["spread"])
        res["lists_faster_than_host_beyond_spread"] = bool(res["host_over_lists"] > 1 + worst)
        return res

    out["a_400_pairs_58_1024"] = leg(corpus_lengths(400, 1), corpus_lengths(400, 2), 1000)
    out["b_32_pairs_8192"] = leg([8192] * 32, [8192] * 32, 1000)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
