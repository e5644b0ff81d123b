"""oracle/attention_ref.py, the float64 reference of every attention parity test, against the REAL Attend.forward
(tests/golden/attention_ref.npz, recipe oracle/gen_golden_attention.py) and against its own definitions.  CPU only."""
import math

import numpy as np
import pytest
import torch

from attention_ref import attention_grads_stored_out, attention_ref, key_mask, mode_rounders, round_to
from dropout_mask import dropout_keep_mask

RTOL = 1e-12  # the same operations in the same precision: round-off only


def relerr(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def case(g, name):
    B, T, Tk, heads, d = (int(x) for x in g[name + ".meta"])
    lens = g[name + ".lens"]
    lens = None if lens[0] < 0 else torch.from_numpy(lens)
    t = lambda key: torch.from_numpy(g[f"{name}.{key}"])
    return (B, T, Tk, heads, d), lens, t


def test_golden_covers_the_masked_and_cross_cases(golden):
    g = golden("attention_ref")
    names = [str(n) for n in g["names"]]
    shapes = {n: case(g, n) for n in names}
    assert any(l is not None and 0 in l.tolist() and s[1] == s[2] for s, l, _ in shapes.values())      # self, all-masked row
    assert any(l is not None and 1 in l.tolist() for s, l, _ in shapes.values())                        # one key
    assert any(l is not None and 0 in l.tolist() and s[2] < s[1] for s, l, _ in shapes.values())        # cross Tk < T, all-masked row
    assert any(l is not None and 0 in l.tolist() and s[2] > s[1] for s, l, _ in shapes.values())        # cross Tk > T, all-masked row
    assert any(l is None and s[2] != s[1] for s, l, _ in shapes.values())


def test_attention_ref_reproduces_the_real_module(golden):
    g = golden("attention_ref")
    for name in (str(n) for n in g["names"]):
        (B, T, Tk, heads, d), lens, t = case(g, name)
        q, k, v = (t(x).clone().requires_grad_(True) for x in "qkv")
        out, _ = attention_ref(q, k, v, heads, lens)
        assert out.dtype == torch.float64 and relerr(out.detach(), t("out")) < RTOL, name
        if name.startswith("self"):
            out.backward(t("do"))
            for x, grad in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
                assert relerr(grad, t(x)) < RTOL, (name, x)


def test_all_masked_row_is_uniform_over_every_key(golden):
    g = golden("attention_ref")
    for name in ("self_dead", "cross_short_masked", "cross_long_masked"):
        (B, T, Tk, heads, d), lens, t = case(g, name)
        b = lens.tolist().index(0)
        want = t("v")[b].mean(dim=0, keepdim=True).expand(T, heads * d)  # mean over ALL Tk keys, not the valid ones
        assert relerr(t("out")[b], want) < RTOL
        out, lse = attention_ref(t("q"), t("k"), t("v"), heads, lens)
        assert relerr(out[b], want) < RTOL
        assert torch.all(lse[b] == math.log2(Tk))  # the kernels' convention: scores 0, not -finfo.max


def test_lengths_above_tk_mean_tk():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, n, 16, generator=g, dtype=torch.float64) for n in (6, 11, 11))
    a, la = attention_ref(q, k, v, 2, torch.tensor([11, 4]))
    b, lb = attention_ref(q, k, v, 2, torch.tensor([500, 4]))
    assert torch.equal(a, b) and torch.equal(la, lb)
    c, lc = attention_ref(q, k, v, 2, None)
    assert torch.equal(a[0], c[0]) and torch.equal(la[0], lc[0])


@pytest.mark.parametrize("T,Tk,lens", [(13, 13, [13, 5, 1]), (9, 21, [21, 20, 2]), (21, 9, None)])
def test_lse_is_the_log2_logsumexp_of_the_masked_scores(T, Tk, lens):
    B, heads, d = 3, 2, 8
    g = torch.Generator().manual_seed(T)
    q, k, v = (torch.randn(B, n, heads * d, generator=g, dtype=torch.float64) * 3 for n in (T, Tk, Tk))
    lens_t = None if lens is None else torch.tensor(lens)
    _, lse = attention_ref(q, k, v, heads, lens_t)
    sim = torch.einsum("bihd,bjhd->bhij", q.view(B, T, heads, d), k.view(B, Tk, heads, d)) * d ** -0.5
    if lens is not None:
        sim = sim.masked_fill(~key_mask(lens_t, Tk).view(B, 1, 1, Tk), -math.inf)
    want = torch.logsumexp(sim, dim=-1) / math.log(2.0)
    assert lse.shape == (B, heads, T) and relerr(lse, want) < RTOL
    # P = 2^(s log2(e) - lse) is the softmax (what dn_attention_backward recomputes)
    P = torch.exp2(sim / math.log(2.0) - lse.unsqueeze(-1))
    assert (P.sum(-1) - 1).abs().max().item() < 1e-12


def test_keep_is_a_mask_multiply_after_the_softmax():
    B, T, Tk, heads, d, p = 2, 19, 19, 2, 8, 0.25
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(B, T, heads * d, generator=g, dtype=torch.float64) for _ in range(3))
    lens = torch.tensor([19, 7])
    keep = dropout_keep_mask(B, heads, T, Tk, p, 0xABCDEF0123456789)
    out, lse = attention_ref(q, k, v, heads, lens, keep=keep, p=p)
    _, lse0 = attention_ref(q, k, v, heads, lens)
    assert torch.equal(lse, lse0)  # of the undropped softmax
    split = lambda t: t.view(B, T, heads, d).transpose(1, 2)
    sim = torch.einsum("bhid,bhjd->bhij", split(q), split(k)) * d ** -0.5
    sim = sim.masked_fill(~key_mask(lens, Tk).view(B, 1, 1, Tk), -torch.finfo(sim.dtype).max)
    attn = sim.softmax(-1) * keep.double() / (1.0 - p)
    want = torch.einsum("bhij,bhjd->bhid", attn, split(v)).transpose(1, 2).reshape(B, T, heads * d)
    assert relerr(out, want) < RTOL and 0.15 < 1 - keep.double().mean().item() < 0.35


def test_mode_rounders_cost_what_the_format_costs():
    """The emulated format error (exact minus rounded, no kernel involved) is of the order of the format's epsilon."""
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(2, 70, 64, generator=g, dtype=torch.float64) for _ in range(3))
    exact, _ = attention_ref(q, k, v, 2, torch.tensor([70, 33]))
    err = {}
    for mode in ("f32", "bf16", "f16", "x3"):
        src = (lambda t: t) if mode in ("f32", "x3") else mode_rounders(mode)["operand"]
        want, _ = attention_ref(src(q), src(k), src(v), 2, torch.tensor([70, 33]))
        got, _ = attention_ref(src(q), src(k), src(v), 2, torch.tensor([70, 33]), rounders=mode_rounders(mode))
        err[mode] = relerr(got, want)
    assert err["f32"] < 2.0 ** -22 and err["x3"] < 2.0 ** -14 and err["f16"] < 2.0 ** -9 and err["bf16"] < 2.0 ** -6
    assert err["f32"] < err["x3"] < err["f16"] < err["bf16"]
    assert np.isfinite(list(err.values())).all() and relerr(exact, exact) == 0


def test_flash_gradient_formulas_equal_autograd_and_show_the_cost_of_a_stored_output():
    B, T, heads, d, p = 3, 23, 2, 8, 0.1
    g = torch.Generator().manual_seed(17)
    q, k, v, do = (torch.randn(B, T, heads * d, generator=g, dtype=torch.float64) for _ in range(4))
    lens = torch.tensor([23, 14, 1])
    keep = dropout_keep_mask(B, heads, T, T, p, 99)
    qd, kd, vd = (t.clone().requires_grad_(True) for t in (q, k, v))
    attention_ref(qd, kd, vd, heads, lens, keep=keep, p=p)[0].backward(do)
    exact = attention_grads_stored_out(q, k, v, do, heads, lens, keep, p, lambda t: t)
    for a, b in zip(exact, (qd.grad, kd.grad, vd.grad)):
        assert relerr(a, b) < 1e-12
    rounded = attention_grads_stored_out(q, k, v, do, heads, lens, keep, p, round_to(torch.bfloat16))
    assert torch.equal(rounded[2], exact[2])                      # dv does not read O
    assert 0 < relerr(rounded[0], exact[0]) < 2.0 ** -5            # dq / dk carry the rounding of O through delta
    o, _ = attention_ref(q, k, v, heads, lens, keep=keep, p=p)
    given = attention_grads_stored_out(q, k, v, do, heads, lens, keep, p, out=round_to(torch.bfloat16)(o))
    assert all(torch.equal(a, b) for a, b in zip(given, rounded))  # the same thing when handed the stored O
