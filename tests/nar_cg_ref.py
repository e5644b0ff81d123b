"""TEST INFRASTRUCTURE ONLY.  CPU restatement (plain torch) of the reference's classifier-free-guided mask-predict decoding
(research/TranSpeech/nat_gen.py:192-236 with TransformerUnitDecoder.cg_forward, nar_transformer.py:123-183) on top of
oracle/nar_oracle.py: `decoder_logits` for both halves (null half: the encoder output replaced by copies of
embed_tokens.weight[bos], no padding mask) and `skeptical_unmasking`.  Pinned by tests/golden/nar_cg.npz, which the REAL classes
wrote (tools/gen_golden_nar_cg.py)."""
import torch

import nar_oracle as N

MARGIN = 1e-3  # the fixtures' and the kernel tests' inputs keep every decision this far from a tie


def null_logits(sd, cfg, tokens, S, null_token=None):
    """cg_forward: every source position of every row is e_null = embed_tokens.weight[bos] (raw: no scale, no position), mask cleared."""
    e = sd["embed_tokens.weight"][cfg.bos if null_token is None else null_token]
    mem = e[None, None, :].expand(S, tokens.size(0), -1).contiguous()
    return N.decoder_logits(sd, cfg, tokens, mem, None, normalize=False)


def null_rows(sd, cfg, dtype=torch.float64):
    """c_l = W_o (W_v e_null + b_v) + b_o, the formula, in `dtype`."""
    e = sd["embed_tokens.weight"][cfg.bos].to(dtype)
    rows = []
    for l in range(cfg.layers):
        p = f"layers.{l}.encoder_attn."
        v = sd[p + "v_proj.weight"].to(dtype) @ e + sd[p + "v_proj.bias"].to(dtype)
        rows.append(sd[p + "out_proj.weight"].to(dtype) @ v + sd[p + "out_proj.bias"].to(dtype))
    return torch.stack(rows)


def guided_logits(sd, cfg, tokens, enc_out, enc_pad, cg_scale, null_token=None):
    """-> (cond, null, cond + cg_scale * (cond - null)) (nat_gen.py:209-223); enc_out [S, B, D]."""
    cond = N.decoder_logits(sd, cfg, tokens, enc_out, enc_pad, normalize=False)
    null = null_logits(sd, cfg, tokens, enc_out.size(0), null_token)
    return cond, null, cond + cg_scale * (cond - null)


def guided_update(logits, tokens, step, n_iters, unk, pad):
    """One iteration's update (nat_gen.py:197-236) on the logits the arg-max is taken of (scaled, or the conditioned ones without
    guidance): scores start from zero.  -> (tokens, scores, predicted) -- `predicted`: the tokens before the re-masking."""
    tokens = tokens.clone()
    scores = torch.zeros(tokens.shape, dtype=torch.float32)
    masks = tokens.eq(unk)
    sc, tk = torch.log_softmax(logits.float(), -1).max(-1)
    tokens = torch.where(masks, tk.to(tokens.dtype), tokens)
    scores = torch.where(masks, sc, scores)
    predicted = tokens.clone()
    if step < n_iters - 1:
        sk = N.skeptical_unmasking(scores, tokens.ne(pad), 1 - (step + 1) / n_iters)
        tokens = tokens.masked_fill(sk, unk)
        scores = scores.masked_fill(sk, 0.0)
    return tokens, scores, predicted


def _boundary(n_nonpad, step, n_iters):
    """trunc(fp32(n_nonpad - 2) p), p the Python float cast to the scores' fp32 (cmlm_transformer.py:19-25)."""
    return int((torch.tensor(float(n_nonpad - 2), dtype=torch.float32) * (1 - (step + 1) / n_iters)).long())


def kept_update(logits, tokens, scores, step, n_iters, unk, pad):
    """forward_decoder's update (nar_transformer.py:791-842), the one that does NOT reset: the positions that are not masked keep
    the scores of the earlier iterations, and the re-mask ranking runs over old scores, new scores and the zeros of pad / bos / eos.
    The sort is stable: equal scores are ordered by position.  -> (tokens, scores, predicted)."""
    masks = tokens.eq(unk)
    sc, tk = torch.log_softmax(logits.float(), -1).max(-1)
    tokens = torch.where(masks, tk.to(tokens.dtype), tokens)
    scores = torch.where(masks, sc, scores.float())
    predicted = tokens.clone()
    if step < n_iters - 1:
        order = torch.sort(scores, dim=-1, stable=True)[1]
        boundary = torch.tensor([[_boundary(int(n), step, n_iters)] for n in tokens.ne(pad).sum(1)])
        cut = torch.arange(scores.size(1))[None, :] < boundary
        sk = torch.zeros_like(cut).scatter(1, order, cut)
        tokens = tokens.masked_fill(sk, unk)
        scores = scores.masked_fill(sk, 0.0)
    return tokens, scores, predicted


def kept_margins(logits, tokens, scores, step, n_iters, unk, pad):
    """`margins` for `kept_update`.  -> (arg-max margin, boundary gap, new scores equal to 0.0, rows whose boundary falls inside a
    group of equal scores).  Equal scores may straddle a boundary only if every one of them is an INPUT (a kept position's score
    or a pad / bos / eos zero: the same fp32 value on both sides, the position order decides); the gap of such a row is the distance
    from the group to the nearest other score.  Any other pair across a boundary counts with its own difference."""
    masks = tokens.eq(unk)
    lp = torch.log_softmax(logits.double(), -1)
    top = lp.topk(2, -1)[0]
    m_arg = float((top[..., 0] - top[..., 1])[masks].min()) if bool(masks.any()) else float("inf")
    sc = torch.where(masks, top[..., 0], scores.double())
    zeros = int((sc[masks] == 0).sum())
    gap, straddled = float("inf"), 0
    if step < n_iters - 1:
        nonpad = torch.where(masks, lp.argmax(-1), tokens).ne(pad)
        for b in range(tokens.size(0)):
            k = _boundary(int(nonpad[b].sum()), step, n_iters)
            s = sc[b].sort()[0]
            if not 0 < k < s.numel():
                continue
            if s[k] != s[k - 1]:
                gap = min(gap, float(s[k] - s[k - 1]))
                continue
            group = sc[b] == s[k]
            if bool((group & masks[b]).any()):
                gap = 0.0  # a computed score inside the group: not reproducible
                continue
            straddled += 1
            gap = min(gap, float((sc[b][~group] - s[k]).abs().min()) if bool((~group).any()) else float("inf"))
    return m_arg, gap, zeros, straddled


def margins(logits, tokens, step, n_iters, unk, pad):
    """The three conditions a fixture / a kernel input must meet for its decisions to be reproducible across arithmetic:
    -> (smallest top-2 margin of an arg-max at a masked position, smallest score gap across a re-mask boundary, number of new
    scores that equal 0.0)."""
    masks = tokens.eq(unk)
    lp = torch.log_softmax(logits.double(), -1)
    top = lp.topk(2, -1)[0]
    m_arg = float((top[..., 0] - top[..., 1])[masks].min()) if bool(masks.any()) else float("inf")
    sc = torch.where(masks, top[..., 0], torch.zeros_like(top[..., 0]))
    zeros = int((sc[masks] == 0).sum())
    gap = float("inf")
    if step < n_iters - 1:
        nonpad = torch.where(masks, lp.argmax(-1), tokens).ne(pad)
        for b in range(tokens.size(0)):
            boundary = int(float(torch.tensor(float(nonpad[b].sum() - 2), dtype=torch.float32) * (1 - (step + 1) / n_iters)))
            s = sc[b].sort()[0]
            if 0 < boundary < s.numel():
                gap = min(gap, float(s[boundary] - s[boundary - 1]))
    return m_arg, gap, zeros


def initial_tokens(lengths, cfg):
    """prepare_batch (nat_gen.py:109-113): `unk` at lengths[b] positions, then `eos`, then `pad`."""
    T = int(lengths.max()) + 1
    idx = torch.arange(T)[None, :]
    tok = torch.full((lengths.numel(), T), cfg.pad, dtype=torch.long)
    return tok.masked_fill(idx < lengths[:, None], cfg.unk).masked_fill(idx == lengths[:, None], cfg.eos)


def guided_mask_predict(sd, cfg, enc_out, enc_pad, lengths, n_iters, cg_scale, null_token=None):
    """The loop.  -> list over iterations of (tokens, scores, predicted); the first iteration's (cond, null) logits."""
    tokens = initial_tokens(lengths, cfg)
    hist, first = [], None
    for step in range(n_iters):
        if cg_scale is not None and cg_scale > 0:
            cond, null, use = guided_logits(sd, cfg, tokens, enc_out, enc_pad, cg_scale, null_token)
        else:
            cond = null = use = N.decoder_logits(sd, cfg, tokens, enc_out, enc_pad, normalize=False)
        first = first or (cond, null)
        tokens, scores, predicted = guided_update(use, tokens, step, n_iters, cfg.unk, cfg.pad)
        hist.append((tokens, scores, predicted))
    return hist, first
