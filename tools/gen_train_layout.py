#!/usr/bin/env python3
"""Writes tests/golden/train_layout.npz: the flat-buffer layout of the two training engines (csrc/train_engine.hip) -- parameter
count, aux bytes, the offsets of every packed tensor, the gradient range of every backward stage, and the workspace size at a
handful of batch shapes -- one row per (model, config, dtype in {f32, bf16}).  tests/test_train_layout.py asserts that the library
reproduces the table.

The configs are stored beside the answers (CFG: one row of COLS per case); `measure` asks the library for the numbers of one row.
No GPU: create / param_count / aux_bytes / offsets / stage_range / workspace_bytes are host logic.
    python tools/gen_train_layout.py [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from diffnorm_amd import _lib, packing, synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "train_layout.npz")
VAE, EPS = 0, 1
# VAE rows: a = latent flag (16 / 32 / 128), b = stacks, c = layers, d = vocab, e unused; `pair` = -1
# eps rows: a = latent width, b = WaveNet stacks, c = WaveNet layers, d = dim_cond_mult, e = max_pos; `pair` = the row of the frozen
#           VAE (same dtype, z == latent) whose decoder the multitask loss runs through
COLS = ("model", "dtype", "dim", "depth", "heads", "dim_head", "a", "b", "c", "d", "e", "pair")
SHAPES = ((2, 40), (4, 256), (16, 512), (24, 512), (8, 1024))  # (B, T) of the stored workspace sizes
# plan_wgrad reads these once per process; they change workspace_bytes.  The table is their defaults.
WGRAD_ENV = ("DN_WGRAD_FILL", "DN_WGRAD_UNSLICED")


def configs():
    """(name, COLS row without dtype and with `pair` as a name) -- the tiny configs of the training tests, the smoke VAE, the recipe
    VAE at every latent flag (1, 2 and 3 cascaded WaveNets each way), the recipe eps-predictor and one odd shape of each."""
    vae = lambda dim, flag, depth=6, heads=8, dim_head=96, stacks=2, layers=3, vocab=1004: (VAE, dim, depth, heads, dim_head, flag, stacks, layers, vocab, 0)
    eps = lambda dim, latent, depth=12, heads=8, dim_head=64, layers=8, stacks=4, cond_mult=4, max_pos=2048: (EPS, dim, depth, heads, dim_head, latent, stacks, layers, cond_mult, max_pos)
    return [
        ("vae_smoke_192_32", vae(192, 32), None),     # z = 8: also the training tests' CHAIN_VAE
        ("vae_tiny_192_16", vae(192, 16), None),      # z = 4, three WaveNets each way
        ("vae_recipe_768_16", vae(768, 16), None),    # z = 16
        ("vae_recipe_768_32", vae(768, 32), None),    # z = 32
        ("vae_recipe_768_128", vae(768, 128), None),  # z = 128: the recipe
        ("vae_odd_384_32", vae(384, 32, depth=3, heads=4, dim_head=64, stacks=3, layers=2, vocab=500), None),  # z = 16
        ("eps_tiny", eps(64, 16, depth=2, heads=4, dim_head=16, layers=3, stacks=2), "vae_recipe_768_16"),
        ("eps_chain", eps(64, 8), "vae_smoke_192_32"),
        ("eps_recipe", eps(512, 128), "vae_recipe_768_128"),
        ("eps_odd_256", eps(256, 32, depth=3, heads=4, dim_head=64, layers=5, stacks=3, cond_mult=2, max_pos=1500), "vae_recipe_768_32"),
    ]


def build():
    """-> (names, CFG int64 [rows, len(COLS)])"""
    names, rows = [], []
    for dtype, tag in ((_lib.DN_F32, "f32"), (_lib.DN_BF16, "bf16")):
        index = {}
        for name, (model, *rest), pair in configs():
            index[name] = len(rows)
            names.append(f"{name}.{tag}")
            rows.append([model, dtype] + rest + [-1 if pair is None else index[pair]])
    return names, np.array(rows, dtype=np.int64)


def entries(row):
    """The Python side's table of packed tensors (diffnorm_amd/packing.py) for one row."""
    r = dict(zip(COLS, (int(v) for v in row)))
    if r["model"] == VAE:
        return packing.vae_train_entries(r["dim"], packing.vae_mults(r["a"]), r["depth"], r["heads"], r["dim_head"], r["b"], r["c"], r["d"])
    return packing.eps_train_entries(synthetic.eps_config(r["dim"], r["a"], r["depth"], r["heads"], r["dim_head"], r["c"], r["b"], r["d"]))


class Handle:
    """A training engine of one row (created without touching a device), destroyed on exit."""

    def __init__(self, lib, row):
        r = dict(zip(COLS, (int(v) for v in row)))
        self.lib, self.depth = lib, r["depth"]
        self.prefix = "dn_vae_train_" if r["model"] == VAE else "dn_eps_train_"
        if r["model"] == VAE:
            mults = packing.vae_mults(r["a"])
            z = r["dim"]
            for m in mults:
                z //= m
            cfg = _lib.VaeConfig(r["dim"], z // 2, r["depth"], r["heads"], r["dim_head"], r["b"], r["c"], r["d"], len(mults),
                                 (C.c_int32 * 4)(*(mults + [0] * (4 - len(mults)))), r["dtype"])
        else:
            cfg = _lib.EpsConfig(r["dim"], r["a"], r["depth"], r["heads"], r["dim_head"], r["c"], r["b"], r["d"], r["dtype"], r["e"])
        self.h = C.c_void_p()
        _lib.check(self.fn("create")(C.byref(cfg), C.byref(self.h)), self.prefix + "create")

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fn("destroy")(self.h)


def measure(lib, CFG, i):
    """The library's numbers for row i: head = (param_count, aux_bytes, number of offsets), offsets, stages [depth + 3, 2] =
    (offset, count), ws [len(SHAPES)] (VAE) or [len(SHAPES), 2] (eps: without, with the frozen VAE's handle)."""
    with Handle(lib, CFG[i]) as m:
        cap = 4096
        offs = (C.c_int64 * cap)()
        n = _lib.check(m.fn("offsets")(m.h, offs, cap), m.prefix + "offsets")
        head = [int(m.fn("param_count")(m.h)), int(m.fn("aux_bytes")(m.h)), n]
        stages, off, cnt = [], C.c_int64(), C.c_int64()
        for st in range(m.depth + 3):
            _lib.check(m.fn("stage_range")(m.h, st, C.byref(off), C.byref(cnt)), m.prefix + "stage_range")
            stages.append((off.value, cnt.value))
        if int(CFG[i][0]) == VAE:
            ws = [int(m.fn("workspace_bytes")(m.h, B, T)) for B, T in SHAPES]
        else:
            with Handle(lib, CFG[int(CFG[i][-1])]) as vae:
                ws = [[int(m.fn("workspace_bytes")(m.h, v, B, T)) for v in (None, vae.h)] for B, T in SHAPES]
    return {"head": np.array(head, dtype=np.int64), "offsets": np.array(offs[:n], dtype=np.int64),
            "stages": np.array(stages, dtype=np.int64), "ws": np.array(ws, dtype=np.int64)}


def main(out=OUT):
    assert not [v for v in WGRAD_ENV if v in os.environ], "the table is written at the default weight-gradient plan"
    lib = _lib.load()
    names, CFG = build()
    table = {"names": np.array(names), "CFG": CFG, "shapes": np.array(SHAPES, dtype=np.int64)}
    for i in range(len(CFG)):
        for k, v in measure(lib, CFG, i).items():
            table[f"{k}_{i}"] = v
    np.savez_compressed(out, **table)
    print(f"{out}: {len(CFG)} rows, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
