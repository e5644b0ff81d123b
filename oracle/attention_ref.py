"""TEST INFRASTRUCTURE ONLY -- never imported by the product path (diffnorm_amd/).

The one float64 statement of what dn_attention / dn_attention_backward compute: Attend.forward's non-flash branch (reference
latent_module.py:299-343) on the kernels' [B, T, heads*dim_head] layout.  tests/golden/attention_ref.npz (recipe:
oracle/gen_golden_attention.py) pins it to the real module; every attention parity test compares a kernel with it.

`rounders` lets the same function state what a storage FORMAT costs, without any kernel: each entry is applied in float64
arithmetic where a kernel of that mode rounds (operands, the probabilities before the PV product, the stored output), so
attention_ref(exact) - attention_ref(rounded) is the error the format alone accounts for (tests/test_hip_attention_grid.py derives
its bounds for long and peaked softmaxes from it).  bf16_emulation.py has the same idiom for the whole model."""
import math

import torch

LOG2E = 1.0 / math.log(2.0)


def round_to(dtype):
    """float64 -> nearest value of `dtype` (round to nearest even), kept in float64."""
    return lambda t: t.to(dtype).to(torch.float64)


def hi_lo(t):
    """float64 -> (hi, lo), the DN_BF16X3 split of the fp32 value: hi = bf16(x), lo = bf16(x - hi) (16 mantissa bits in all)."""
    x = t.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64), lo.to(torch.float64)


def split_bf16(t):
    hi, lo = hi_lo(t)
    return hi + lo


def mode_rounders(mode):
    """Where a kernel of arithmetic mode `mode` rounds: {"operand", "score", "p", "out", "split"} (absent = exact).
    Every mode keeps the scores and the probabilities in fp32 accumulators ("score").  f32: nothing else below fp32.  bf16 / f16:
    q, k, v, P before the PV product and the stored output.  x3 (attn_x3_kernel): q, k, v and P (before the dropout mask) are each split into
    two bf16 halves and both products keep three of the four partial products, lo x lo is dropped ("split"); the output is stored
    as a split pair."""
    f32 = round_to(torch.float32)
    if mode == "f32":
        return {"operand": f32, "score": f32, "out": f32}
    if mode in ("bf16", "f16"):
        r = round_to(torch.bfloat16 if mode == "bf16" else torch.float16)
        return {"operand": r, "score": f32, "p": r, "out": r}
    if mode == "x3":
        return {"operand": f32, "score": f32, "p": f32, "out": split_bf16, "split": True}
    raise ValueError(mode)


def key_mask(key_lengths, Tk):
    """[B] valid-key counts -> bool [B, Tk]; a count above Tk means Tk."""
    return torch.arange(Tk).unsqueeze(0) < torch.as_tensor(key_lengths).long().clamp(max=Tk).unsqueeze(1)


def attention_ref(q, k, v, heads, key_lengths=None, keep=None, p=0.0, rounders=None):
    """q [B, T, h*d], k / v [B, Tk, h*d] -> (out float64 [B, T, h*d], lse float64 [B, h, T]).

    sim = q k^T d^-0.5; keys j >= key_lengths[b] are masked_fill'ed with -finfo.max, so a row with every key masked is uniform over
    all Tk keys; attn = softmax(sim); train mode: attn * keep / (1 - p) with keep bool [B, h, T, Tk] (oracle/dropout_mask.py);
    out = attn v.  lse is DnAttnParams.lse: the log2-domain log-sum-exp of the scaled, masked scores (of the undropped softmax).
    In an all-masked row the kernels' scores are all 0 (the scale is dropped with the mask): lse = log2(Tk) there.
    Plain differentiable torch ops: gradients come from autograd."""
    B, T, hd = q.shape
    Tk, d = k.shape[1], hd // heads
    rd = rounders or {}
    ident = lambda t: t
    r_op, r_s, r_p, r_out = rd.get("operand", ident), rd.get("score", ident), rd.get("p", ident), rd.get("out", ident)

    def prod(eq, a, b):
        if not rd.get("split"):
            return torch.einsum(eq, a, b)
        (ah, al), (bh, bl) = hi_lo(a), hi_lo(b)
        return torch.einsum(eq, al, bh) + torch.einsum(eq, ah, bl) + torch.einsum(eq, ah, bh)

    heads_of = lambda t, n: r_op(t.to(torch.float64)).view(B, n, heads, d).transpose(1, 2)
    qh, kh, vh = heads_of(q, T), heads_of(k, Tk), heads_of(v, Tk)
    sim = r_s(prod("bhid,bhjd->bhij", qh, kh) * d ** -0.5)
    if key_lengths is not None:
        mask = key_mask(key_lengths, Tk).view(B, 1, 1, Tk)
        sim = sim.masked_fill(~mask, -torch.finfo(sim.dtype).max)
    attn = sim.softmax(dim=-1)
    lse = torch.logsumexp(sim.detach(), dim=-1) * LOG2E
    if key_lengths is not None:
        dead = ~mask.view(B, Tk).any(dim=1)
        lse = torch.where(dead.view(B, 1, 1), torch.full_like(lse, math.log2(Tk)), lse)
    attn = r_p(attn)  # the kernels round (split) P itself; the mask zeroes entries and 1 / (1 - p) scales the fp32 accumulator
    if keep is not None:
        attn = attn * keep.to(torch.float64)
    out = prod("bhij,bhjd->bhid", attn, vh)
    if keep is not None:
        out = out / (1.0 - p)
    return r_out(out.transpose(1, 2).reshape(B, T, hd)), lse


def attention_grads_stored_out(q, k, v, do, heads, key_lengths, keep, p, r_out=None, out=None):
    """(dq, dk, dv) in float64 by the formulas dn_attention_backward uses (csrc/attention_bwd.hip), with delta = sum_d dO * O taken
    from the STORED output: dS = P o (dP o M / (1 - p) - delta).  `out` [B, T, h*d]: the O the backward is handed (then this is what
    the operator must return for ITS inputs); else O is computed here and passed through r_out: with the identity this is the exact
    gradient, with a 2-byte rounder the difference to it is what storing O in that format costs the gradients (it does not cancel
    where the true dS is zero, e.g. a one-key sequence under dropout).  Sequences with at least one valid key only."""
    B, T, hd = q.shape
    d = hd // heads
    sp = lambda t: t.to(torch.float64).view(B, T, heads, d).transpose(1, 2)
    qh, kh, vh, doh = sp(q), sp(k), sp(v), sp(do)
    sim = torch.einsum("bhid,bhjd->bhij", qh, kh) * d ** -0.5
    sim = sim.masked_fill(~key_mask(key_lengths, T).view(B, 1, 1, T), -torch.finfo(sim.dtype).max)
    P = sim.softmax(dim=-1)
    md = keep.to(torch.float64) / (1.0 - p) if keep is not None else torch.ones_like(P)
    stored = sp(out) if out is not None else r_out(torch.einsum("bhij,bhjd->bhid", P * md, vh))
    delta = (doh * stored).sum(-1, keepdim=True)
    dS = P * (torch.einsum("bhid,bhjd->bhij", doh, vh) * md - delta)
    back = lambda t: t.transpose(1, 2).reshape(B, T, hd)
    return (back(torch.einsum("bhij,bhjd->bhid", dS, kh)) * d ** -0.5, back(torch.einsum("bhij,bhid->bhjd", dS, qh)) * d ** -0.5,
            back(torch.einsum("bhij,bhid->bhjd", P * md, doh)))
