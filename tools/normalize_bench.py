"""Wall time of normalize() under different batch plans on ONE synthetic corpus, in one process.

The corpus: `--n` utterances (400) with log-normal lengths clipped to [58, 1024] frames (seeded; the seed and the length statistics
are printed), random features, units without repeats.  It is a synthetic length distribution, not a speech corpus.

Plans:
  consecutive-100, torch noise     today's path: 100 consecutive utterances padded to the longest, noise from torch's generators
  consecutive-100, noise_seed      the same batches, keyed noise drawn on the device (dn_chain_start)
  max_tokens 16384 / 32768 / 49152 length-sorted batches under a frame budget, pad_multiple 32, keyed noise

`--plan-only` (no GPU): per plan the batch count, the frame-rows computed and the padding fraction 1 - valid frames / frame-rows.

On a GPU: recipe-size synthetic engines (synthetic.eps_config()), f16, start_step 50 (49 evaluations per chain).  One first pass
over all plans (it includes graph captures and allocations; reported on its own), then `--reps` (3) timed rounds in which the plans
alternate; per plan the median: seconds, utterances/s, valid-frame-steps/s, the number of distinct (B, T) batch shapes (a proxy for
graph re-captures) and the ratio against consecutive-100 with torch noise of the same process."""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffnorm_amd import sharding  # noqa: E402

BUDGETS = (16384, 32768, 49152)
PAD = 32


def corpus_lengths(n, seed):
    rng = np.random.RandomState(seed)
    return np.clip(np.round(rng.lognormal(5.54, 0.55, n)), 58, 1024).astype(int).tolist()


def plans():
    """name -> normalize() keywords"""
    out = {"consecutive-100, torch noise": dict(batch_size=100), "consecutive-100, noise_seed": dict(batch_size=100, noise_seed=1)}
    for b in BUDGETS:
        out[f"max_tokens {b}, pad {PAD}"] = dict(noise_seed=1, max_tokens=b, pad_multiple=PAD)
    return out


def batches_of(lengths, kw):
    if "max_tokens" in kw:
        return sharding.plan_batches(lengths, kw["max_tokens"], kw.get("max_sentences"), kw.get("pad_multiple", 1))
    return [list(r) for r in sharding.batch_indices(len(lengths), kw["batch_size"])]


def plan_stats(lengths, kw):
    bs = batches_of(lengths, kw)
    shapes = [(len(b), sharding.padded_length(max(lengths[i] for i in b), kw.get("pad_multiple", 1))) for b in bs]
    rows = sum(B * T for B, T in shapes)
    return len(bs), rows, 1.0 - sum(lengths) / rows, len(set(shapes))


def print_plans(lengths):
    valid = sum(lengths)
    table = dict(plans())
    for b in BUDGETS:  # the budget alone, without rounding T up
        table[f"max_tokens {b}, pad 1"] = dict(noise_seed=1, max_tokens=b)
    print(f"{'plan':<34} {'batches':>7} {'frame-rows':>10} {'padding':>8} {'(B,T) shapes':>12}")
    for name, kw in table.items():
        if "torch" in name:
            continue
        n, rows, pad, shapes = plan_stats(lengths, kw)
        print(f"{name.replace(', noise_seed', ''):<34} {n:>7} {rows:>10} {100 * pad:>7.1f}% {shapes:>12}")
    print(f"valid frames: {valid}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=400, help="utterances in the corpus")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--start-step", type=int, default=50)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--plan-only", action="store_true")
    a = ap.parse_args()
    lengths = corpus_lengths(a.n, a.seed)
    L = np.array(lengths)
    print(f"synthetic corpus: seed {a.seed}, {a.n} utterances, lengths log-normal(5.54, 0.55) clipped to [58, 1024]: min {L.min()} "
          f"median {int(np.median(L))} mean {L.mean():.1f} max {L.max()}, {L.sum()} valid frames")
    print_plans(lengths)
    if a.plan_only:
        return
    import torch

    from diffnorm_amd import normalize as N
    from diffnorm_amd import synthetic
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    assert torch.cuda.is_available(), "the timed part needs a GPU (use --plan-only without one)"
    dev = torch.device("cuda", 0)
    cfg = synthetic.eps_config()
    vae = SpeechVAEEncoderDecoder(dim=768, latent_dim=128, dtype=a.dtype)
    vae.load_state_dict(synthetic.random_vae_state_dict(768, 128, seed=1), strict=True)
    ldm = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 512, 128, timesteps=1000, dtype=a.dtype)
    ldm.model.load_state_dict(dict(synthetic.random_eps_state_dict(cfg, seed=0), **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    ldm = ldm.to(dev).eval()
    g = torch.Generator().manual_seed(a.seed)
    rng = np.random.RandomState(a.seed + 1)
    utts = []
    for i, n in enumerate(lengths):
        units = (rng.randint(0, 500, size=n) * 2 + np.arange(n) % 2).tolist()  # neighbours differ: frame-level == de-duplicated
        utts.append(N.Utterance(f"utt{i}", f"src{i}.wav", n, torch.randn(n, 768, generator=g), units, units))
    shapes = set()

    def sample(feat, **kw):
        shapes.add(tuple(feat.shape[:2]))
        return ldm.ddim_sample(feat, **kw)

    def one(kw):
        shapes.clear()
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lines = N.normalize(sample, utts, start_step=a.start_step, device=dev, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, lines, len(shapes)

    table = plans()
    names = list(table)
    evals, valid = a.start_step - 1, sum(lengths)
    first, times, lines, nshapes = {}, {n: [] for n in names}, {}, {}
    for n in names:
        first[n], lines[n], nshapes[n] = one(table[n])
        print(f"first pass  {n:<34} {first[n]:8.2f} s  ({nshapes[n]} batch shapes)", flush=True)
    for r in range(a.reps):
        for n in (names if r % 2 == 0 else names[::-1]):  # alternate, and turn the order round every other round
            t, got, _ = one(table[n])
            times[n].append(t)
            assert "torch" in n or got == lines[n], f"{n}: a keyed plan did not reproduce its own lines"
            print(f"round {r}     {n:<34} {t:8.2f} s", flush=True)
    keyed = [n for n in names if "torch" not in n]
    agree = {n: float(np.mean([x == y for x, y in zip(lines[n], lines[keyed[0]])])) for n in keyed[1:]}
    base = statistics.median(times[names[0]])
    print(f"\n{a.dtype}, start_step {a.start_step} ({evals} evaluations), {a.n} utterances, {valid} valid frames; median of {a.reps} alternating rounds")
    print(f"{'plan':<34} {'s':>7} {'range':>13} {'utt/s':>7} {'valid-frame-steps/s':>19} {'shapes':>6} {'vs today':>8} {'first pass s':>12}")
    for n in names:
        m = statistics.median(times[n])
        print(f"{n:<34} {m:>7.2f} {min(times[n]):>6.2f}-{max(times[n]):<6.2f} {a.n / m:>7.1f} {valid * evals / m:>19.3e} {nshapes[n]:>6} "
              f"{base / m:>7.2f}x {first[n]:>12.2f}")
    for n, f in agree.items():
        print(f"TSV lines of '{n}' identical to '{keyed[0]}': {100 * f:.1f}% of the utterances")


if __name__ == "__main__":
    main()
