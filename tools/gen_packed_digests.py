#!/usr/bin/env python3
"""Writes tests/golden/packed_digests.npz: shape, torch dtype and SHA-256 of every tensor diffnorm_amd/packing.py builds from a
seeded synthetic state dict -- the ordered lists of `pack_eps` / `pack_vae` in all four arithmetic dtypes, and the flat fp32
training buffer of `pack_flat` over `*_train_entries` (with the sorted key list `unpack_flat` gives back).
tests/test_packing.py asserts that packing.py reproduces the table, so a change of packing.py that is not meant to move a packed
byte can be checked without a GPU.

Only packing.py's public functions are used (pack_eps, pack_vae, vae_mults, *_train_entries, pack_flat, unpack_flat).  The flat
buffer is laid out contiguously from the entries' shapes; the library's real offsets are pinned by tests/test_train_layout.py.
No GPU and no library.
    python tools/gen_packed_digests.py [out.npz]"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from diffnorm_amd import _lib, packing, synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "packed_digests.npz")
DTYPES = (("f32", _lib.DN_F32), ("bf16", _lib.DN_BF16), ("f16", _lib.DN_F16), ("bf16x3", _lib.DN_BF16X3))
MAX_POS = 100  # of the small eps cases (the recipe case packs the default table)

# eps-predictor cases: name -> (config, seed).  dn_eps_create wants dim % 4 == 0, heads * dim_head % 64 == 0, dim * dim_cond_mult % 64 == 0.
EPS = {
    "eps_even": (dict(dim=64, latent_dim=16, depth=2, heads=4, dim_head=16, wavenet_layers=3, wavenet_stacks=2), 11),
    # dim and inner = 213 are no multiples of 64: pad rows and columns, and -1 rows in the GEGLU interleave
    "eps_odd": (dict(dim=80, latent_dim=12, depth=2, heads=2, dim_head=32, wavenet_layers=3, wavenet_stacks=2), 12),
    # the prompt-conditioned model: three norms per layer, 2C conditioning columns, the resampler and cross-attention tensors
    "eps_prompt": (dict(dim=64, latent_dim=16, depth=2, heads=4, dim_head=16, wavenet_layers=3, wavenet_stacks=2, dim_prompt=32,
                        num_latents_m=4, resampler_depth=1), 13),
}
EPS_RECIPE = ("eps_recipe", dict(), 14)  # bf16 only
# VAE cases: one per latent flag (3, 2 and 1 cascaded WaveNets each way); stacks and layers > 1 and unequal
VAE = {f"vae_{flag}": (dict(dim=192, latent_dim=flag, depth=2, heads=2, dim_head=32, stacks=2, layers=3, vocab=100), 20 + n)
       for n, flag in enumerate((16, 32, 128))}
FLAT = ("eps_even", "eps_odd", "vae_16", "vae_32", "vae_128")  # the prompt-conditioned model has no training path


def _random_gammas(sd, seed):
    """synthetic's gammas are all 1 and would hide two norms swapped: seeded random values instead"""
    g = torch.Generator().manual_seed(1000 + seed)
    for k in sorted(sd):
        if k.endswith(".gamma"):
            sd[k] = 1.0 + 0.25 * torch.randn(sd[k].shape, generator=g)
    return sd


def state_dict(name):
    if name in VAE:
        kw, seed = VAE[name]
        return _random_gammas(synthetic.random_vae_state_dict(seed=seed, **kw), seed)
    kw, seed = EPS_RECIPE[1:] if name == EPS_RECIPE[0] else EPS[name]
    return _random_gammas(synthetic.random_eps_state_dict(synthetic.eps_config(**kw), seed=seed), seed)


def pack(name, dtype):
    """The inference list of one case in one arithmetic dtype."""
    sd = state_dict(name)
    if name in VAE:
        kw = VAE[name][0]
        return packing.pack_vae(sd, kw["dim"], packing.vae_mults(kw["latent_dim"]), kw["depth"], kw["heads"], kw["dim_head"],
                                kw["stacks"], kw["layers"], kw["vocab"], dtype)
    if name == EPS_RECIPE[0]:
        return packing.pack_eps(sd, synthetic.eps_config(), dtype)
    return packing.pack_eps(sd, synthetic.eps_config(**EPS[name][0]), dtype, MAX_POS)


def inference_cases():
    """(key, case name, dtype code) of every stored inference list"""
    out = [(f"{name}.{tag}", name, code) for name in list(EPS) + list(VAE) for tag, code in DTYPES]
    return out + [(EPS_RECIPE[0] + ".bf16", EPS_RECIPE[0], _lib.DN_BF16)]


def entries(name):
    if name in VAE:
        kw = VAE[name][0]
        return packing.vae_train_entries(kw["dim"], packing.vae_mults(kw["latent_dim"]), kw["depth"], kw["heads"], kw["dim_head"],
                                         kw["stacks"], kw["layers"], kw["vocab"])
    return packing.eps_train_entries(synthetic.eps_config(**EPS[name][0]))


def contiguous_offsets(ents):
    """-> (offsets, total) of the entries laid end to end"""
    offs, total = [], 0
    for e in ents:
        offs.append(total)
        total += int(np.prod(e.shape))
    return offs, total


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def describe(t: torch.Tensor) -> str:
    return f"{'x'.join(str(s) for s in t.shape)} {t.dtype} {sha(t)}"


def build():
    """-> {key: array of strings}: `list/<case>.<dtype>` one line per tensor; `flat/<case>` the buffer's digest; `keys/<case>`"""
    table = {}
    for key, name, code in inference_cases():
        table["list/" + key] = np.array([describe(t) for t in pack(name, code)])
    for name in FLAT:
        ents = entries(name)
        offs, total = contiguous_offsets(ents)
        flat = packing.pack_flat(state_dict(name), ents, offs, total)
        table["flat/" + name] = np.array([describe(flat)])
        table["keys/" + name] = np.array(sorted(packing.unpack_flat(flat, ents, offs)))
    return table


def main(out=OUT):
    table = build()
    np.savez_compressed(out, **table)
    n = sum(len(v) for k, v in table.items() if k.startswith("list/"))
    print(f"{out}: {len(table)} arrays, {n} list tensors, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
