"""Device edit distance and unit reduction against their host restatements, in one process; prints one JSON line.

Legs (each timed in alternating blocks behind a warm-up; per side the median and the min-max spread of the blocks):
  a  400 pairs with the synthetic length distribution of tools/normalize_bench.py (log-normal, clipped to [58, 1024], seed 1), alphabet 1000:
     dn_edit_distance (one launch, events around it) against the numpy row-wise restatement tests/edit_distance_ref.py
  b  32 pairs of 8192 x 8192: the same; the host side is timed on `--host-pairs` (2) pairs and scaled to 32
  r  dn_reduce_units on [100, 1024] (alphabet 3) against the normalize.reduce_token loop over .tolist() rows
There is no torch baseline: torch has no comparable operator.

`--normalize`: additionally normalize() over normalize_bench's corpus and plan max_tokens = 16384, with and without
`unit_changes=`, alternating in the same session: the medians, their spreads and the difference."""
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
    return {"median_ms": 1e3 * statistics.median(xs), "min_ms": 1e3 * min(xs), "max_ms": 1e3 * max(xs), "blocks": len(xs)}


def device_time(fn, iters):
    import torch

    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / 1e3 / iters


def host_time(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def alternate(dev_fn, host_fn, blocks, iters, host_scale=1.0):
    for _ in range(3):
        dev_fn()  # warm-up: allocations, code load
    dev, host = [], []
    for k in range(blocks):
        for side in (("d", "h") if k % 2 == 0 else ("h", "d")):
            if side == "d":
                dev.append(device_time(dev_fn, iters))
            else:
                host.append(host_time(host_fn) * host_scale)
    d, h = summary(dev), summary(host)
    return {"device": d, "host": h, "host_over_device": h["median_ms"] / d["median_ms"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10, help="device launches per timed block")
    ap.add_argument("--host-pairs", type=int, default=2, help="pairs of leg b the host restatement is timed on")
    ap.add_argument("--normalize", action="store_true")
    ap.add_argument("--reps", type=int, default=3, help="rounds of the normalize leg")
    a = ap.parse_args()
    import torch

    import edit_distance_ref as R
    from diffnorm_amd import metrics as M
    from diffnorm_amd.normalize import reduce_token
    from normalize_bench import corpus_lengths

    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    out = {"tool": "edit_distance_bench", "blocks": a.blocks, "iters": a.iters}

    def pairs_of(lens_a, lens_b, alphabet):
        A = np.zeros((len(lens_a), max(lens_a)), dtype=np.int32)
        Bm = np.zeros((len(lens_b), max(lens_b)), dtype=np.int32)
        for i, (na, nb) in enumerate(zip(lens_a, lens_b)):
            A[i, :na], Bm[i, :nb] = rng.randint(0, alphabet, na), rng.randint(0, alphabet, nb)
        return A, Bm

    def leg(lens_a, lens_b, alphabet, host_pairs=None):
        A, Bm = pairs_of(lens_a, lens_b, alphabet)
        ta, tb = torch.from_numpy(A).to(dev), torch.from_numpy(Bm).to(dev)
        la, lb = torch.tensor(lens_a, dtype=torch.int32, device=dev), torch.tensor(lens_b, dtype=torch.int32, device=dev)
        n = len(lens_a) if host_pairs is None else host_pairs
        host = lambda: [R.edit_distance(A[i, : lens_a[i]], Bm[i, : lens_b[i]]) for i in range(n)]
        got = M.edit_distance(ta, tb, la, lb).cpu().tolist()
        assert got[:n] == host(), "the device and the restatement disagree"
        res = alternate(lambda: M.edit_distance(ta, tb, la, lb), host, a.blocks, a.iters, len(lens_a) / n)
        res["cells"] = int(sum(x * y for x, y in zip(lens_a, lens_b)))
        res["device_gcells_per_s"] = res["cells"] / res["device"]["median_ms"] / 1e6
        return res

    lens = corpus_lengths(400, 1)
    out["a_400_pairs_58_1024"] = leg(lens, corpus_lengths(400, 2), 1000)
    out["b_32_pairs_8192"] = leg([8192] * 32, [8192] * 32, 1000, host_pairs=a.host_pairs)
    units = rng.randint(0, 3, size=(100, 1024)).astype(np.int32)
    tu, tl = torch.from_numpy(units).to(dev), torch.full((100,), 1024, dtype=torch.int32, device=dev)
    out["r_reduce_100x1024"] = alternate(lambda: M.reduce_units(tu, tl), lambda: [reduce_token(r) for r in units.tolist()], a.blocks, a.iters)
    if a.normalize:
        out["normalize_max_tokens_16384"] = normalize_leg(a.reps)
    print(json.dumps(out))


def normalize_leg(reps):
    import types

    import torch

    from diffnorm_amd import normalize as N
    from diffnorm_amd import synthetic
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder
    from normalize_bench import PAD, corpus_lengths

    dev = torch.device("cuda", 0)
    cfg = synthetic.eps_config()
    vae = SpeechVAEEncoderDecoder(dim=768, latent_dim=128, dtype="f16")
    vae.load_state_dict(synthetic.random_vae_state_dict(768, 128, seed=1), strict=True)
    ldm = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 512, 128, timesteps=1000, dtype="f16")
    ldm.model.load_state_dict(dict(synthetic.random_eps_state_dict(cfg, seed=0), **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    ldm = ldm.to(dev).eval()
    lengths = corpus_lengths(400, 1)
    g = torch.Generator().manual_seed(1)
    rng = np.random.RandomState(2)
    utts = []
    for i, n in enumerate(lengths):
        units = (rng.randint(0, 500, size=n) * 2 + np.arange(n) % 2).tolist()
        utts.append(N.Utterance(f"utt{i}", f"src{i}.wav", n, torch.randn(n, 768, generator=g), units, units))
    kw = dict(start_step=50, device=dev, noise_seed=1, max_tokens=16384, pad_multiple=PAD)

    def one(report):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lines = N.normalize(ldm.ddim_sample, utts, unit_changes=[] if report else None, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lines

    _, want = one(False)  # first pass: captures and allocations
    one(True)
    times = {False: [], True: []}
    for r in range(reps):
        for report in ((False, True) if r % 2 == 0 else (True, False)):
            t, lines = one(report)
            assert lines == want
            times[report].append(t)
    off, on = summary(times[False]), summary(times[True])
    return {"without": off, "with_unit_changes": on, "difference_ms": on["median_ms"] - off["median_ms"],
            "spread_without_ms": off["max_ms"] - off["min_ms"], "spread_with_ms": on["max_ms"] - on["min_ms"]}


if __name__ == "__main__":
    main()
