"""Fixture of the EMA of the parameters (tests/golden/ema.npz) from the REAL reference class, fairseq/models/ema/ema.py:32-209.

The file is leaf-loaded where it lies (oracle/ref_loader.py's loader): it imports copy, logging, torch and
`from fairseq import checkpoint_utils`, which only a seed model (--ema-seed-model, not supported here) uses, so an empty stand-in
module is enough.  The real `EMA` (ema_fp32=True) then follows a three-tensor module -- shapes [5,7], [9], [2,3,4] -- through 7
updates of seeded parameters (a random walk, like training), stepped the way the reference's trainer steps it: `ema.step(model,
updates)` with the number of updates after the increment (fairseq/trainer.py:1018-1025).  Three configurations of (decay,
start_update, update_freq): (0.999, 0, 1), (0.9, 3, 1), (0.9, 2, 3).

Written (flat = the three tensors concatenated in state-dict order, 68 values):
  configs [3,3]        (decay, start_update, update_freq)
  shapes  [3,3]        the tensors' shapes, zero-padded
  params  [8,68]       row 0: the parameters the EMA is created from; row u: after update u
  c{i}/decay   [7]     EMA.get_decay() after step u
  c{i}/applied [7]     whether _step_internal ran in step u
  c{i}/ema     [7,68]  the EMA's fp32 state after step u

Run in the build container (the reference must be present): python tools/gen_golden_ema.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_loader  # noqa: E402

SHAPES = [(5, 7), (9,), (2, 3, 4)]
CONFIGS = [(0.999, 0, 1), (0.9, 3, 1), (0.9, 2, 3)]
UPDATES = 7


def load_ema_class():
    if not ref_loader.available():
        raise RuntimeError("reference checkout not present at %s" % ref_loader.REF)
    sys.dont_write_bytecode = True  # the reference mount is read-only
    if "fairseq" not in sys.modules:
        ref_loader._pkg("fairseq")
    if not hasattr(sys.modules["fairseq"], "checkpoint_utils"):
        stub = types.ModuleType("fairseq.checkpoint_utils")  # used by ema_seed_model only
        sys.modules["fairseq.checkpoint_utils"] = stub
        sys.modules["fairseq"].checkpoint_utils = stub
    for name in ("fairseq.models", "fairseq.models.ema"):
        if name not in sys.modules:
            ref_loader._pkg(name)
    return ref_loader._load("fairseq.models.ema.ema", "fairseq/models/ema/ema.py").EMA


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.zeros(SHAPES[0]))
        self.b = torch.nn.Parameter(torch.zeros(SHAPES[1]))
        self.c = torch.nn.Parameter(torch.zeros(SHAPES[2]))


def flat(sd):
    return torch.cat([sd[k].detach().float().reshape(-1) for k in ("a", "b", "c")]).numpy()


def trajectory():
    g = torch.Generator().manual_seed(2024)
    rows = [torch.randn(sum(int(np.prod(s)) for s in SHAPES), generator=g)]
    for _ in range(UPDATES):
        rows.append(rows[-1] + 0.1 * torch.randn(rows[0].shape, generator=g))
    return torch.stack(rows)


def set_params(model, row):
    off = 0
    with torch.no_grad():
        for p in (model.a, model.b, model.c):
            p.copy_(row[off: off + p.numel()].view(p.shape))
            off += p.numel()


def main():
    EMA = load_ema_class()
    params = trajectory()
    out = {"configs": np.array(CONFIGS, dtype=np.float64), "params": params.numpy(),
           "shapes": np.array([list(s) + [0] * (3 - len(s)) for s in SHAPES], dtype=np.int64)}
    for i, (decay, start, freq) in enumerate(CONFIGS):
        model = Toy()
        set_params(model, params[0])
        cfg = types.SimpleNamespace(ema_decay=decay, ema_start_update=start, ema_update_freq=freq, ema_fp32=True, ema_seed_model=None)
        ema = EMA(model, cfg)
        calls = [0]
        inner = ema._step_internal

        def counted(new_model, updates=None, inner=inner, calls=calls):
            calls[0] += 1
            return inner(new_model, updates)

        ema._step_internal = counted
        decays, applied, states = [], [], []
        for u in range(1, UPDATES + 1):
            set_params(model, params[u])
            before = calls[0]
            ema.step(model, u)
            decays.append(float(ema.get_decay()))
            applied.append(calls[0] > before)
            states.append(flat(ema.fp32_params))
        out[f"c{i}/decay"] = np.array(decays, dtype=np.float64)
        out[f"c{i}/applied"] = np.array(applied, dtype=np.bool_)
        out[f"c{i}/ema"] = np.stack(states).astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "ema.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
