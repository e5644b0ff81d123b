"""TEST INFRASTRUCTURE ONLY.  Golden vectors for the attention operator, produced in the build container by the REAL reference
code: Attend.forward's non-flash branch (fairseq/models/text_to_speech/latent_module.py:299-343), run on CPU in float64 in eval
mode on seeded q / k / v in the [b, h, n, d] layout it takes, with the key-padding mask the callers build from lengths.
Cases: self-attention with ragged lengths (full, inside, 1, 0 = an all-masked row) with the autograd gradients of q / k / v for
a seeded dO; cross-attention Tk < T and Tk > T, without and with a key mask (incl. an all-masked row).
oracle/attention_ref.py restates the branch for every parity test; tests/test_attention_ref.py holds it to these vectors.
Usage:  python oracle/gen_golden_attention.py    ->  tests/golden/attention_ref.npz
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_loader  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "attention_ref.npz")
# name: (B, T, Tk, heads, dim_head, key lengths or None)
CASES = {
    "self_ragged": (3, 20, 20, 2, 8, [20, 13, 1]),
    "self_dead": (3, 17, 17, 2, 16, [0, 17, 6]),
    "self_nomask": (2, 9, 9, 2, 4, None),
    "cross_short": (2, 20, 7, 2, 8, None),
    "cross_short_masked": (3, 20, 7, 2, 8, [7, 3, 0]),
    "cross_long": (2, 5, 33, 2, 8, None),
    "cross_long_masked": (3, 5, 33, 2, 8, [33, 1, 0]),
}


def main():
    lm, _ = ref_loader.load_reference()
    attend = lm.Attend(dropout=0.1, causal=False, use_flash=False).eval()
    out = {"names": np.array(sorted(CASES))}
    for i, name in enumerate(sorted(CASES)):
        B, T, Tk, heads, d, lens = CASES[name]
        g = torch.Generator().manual_seed(1000 + i)
        q = torch.randn(B, T, heads * d, generator=g, dtype=torch.float64).requires_grad_(True)
        k = torch.randn(B, Tk, heads * d, generator=g, dtype=torch.float64).requires_grad_(True)
        v = torch.randn(B, Tk, heads * d, generator=g, dtype=torch.float64).requires_grad_(True)
        do = torch.randn(B, T, heads * d, generator=g, dtype=torch.float64)
        heads_of = lambda t: t.view(B, -1, heads, d).transpose(1, 2)
        mask = None if lens is None else torch.arange(Tk).unsqueeze(0) < torch.tensor(lens).unsqueeze(1)
        o = attend(heads_of(q), heads_of(k), heads_of(v), mask=mask).transpose(1, 2).reshape(B, T, heads * d)
        out[name + ".meta"] = np.array([B, T, Tk, heads, d], dtype=np.int64)
        out[name + ".lens"] = np.array(lens if lens is not None else [-1], dtype=np.int64)
        for key, t in (("q", q), ("k", k), ("v", v), ("out", o)):
            out[f"{name}.{key}"] = t.detach().numpy()
        if name.startswith("self"):
            o.backward(do)
            for key, t in (("do", do), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
                out[f"{name}.{key}"] = t.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
