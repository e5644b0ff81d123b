"""State-dict -> packed tensors for libdiffnorm_hip.so: ONE table of packed tensors behind inference and training.

Input: tensors in the reference's state-dict layout (conv weights [Cout,Cin,k], linear weights [out,in]).  Each
network piece (`_wavenet_entries`, `_tf_layer_entries`, the models' own tensors in `_eps_entries` / `_vae_entries`) is a table of
`_Entry` rows: name, packed fp32 shape, how to build the packed fp32 tensor from a state dict, how to write it back.  Two walks
over the tables:

* training (`*_train_entries`, `pack_flat` / `unpack_flat`): the flat fp32 master / gradient buffers of csrc/train_engine.hip hold
  the entries one after the other, the transformer's layer by layer;
* inference (`pack_eps` / `pack_vae`: the ordered lists `dn_eps_create` / `dn_vae_create` expect, documented in csrc/engine.h):
  the same entries, weights converted to the arithmetic dtype, the transformer's stacked per tensor, plus the few tensors derived
  for inference only (summed skip bias, K-blocked copies, placeholders, the sinusoidal table).

A third walk (`repack_plan`) describes the inference lists as a device pass over the training engine's flat master buffer
(dn_repack_weights); `repack_emulate` is that pass in torch.

Packing rules:

* every weight becomes [rows padded to 128][K padded to 64] with K contiguous; pads are zeros, so padded channels stay exactly zero
  through the network.  Arithmetic dtypes (`_arith`): bf16, f16, fp32, or DN_BF16X3 split rows (`split_rows`);
* a k-tap causal conv becomes k matrices, tap j multiplying the frame t-(k-1-j)*dilation (`_conv`);
* Linear(D, 2*inner) of the GEGLU is interleaved per 16-row MFMA tile = [8 value rows ; 8 gate rows of the same output columns], so
  every tile is self-contained and one wave holds value and gate of a column (epilogue DN_EPI_GEGLU; `_geglu_pack` / `_geglu_unpack`);
* the 2*S*L FiLM and 2 (3 with a prompt branch) * depth adaptive-RMSNorm projections (`eps_cond_modules`) are stacked into one
  [n_cond, C] matrix, each as [gamma(Dp) ; beta(Dp)] (`_cond_stack` / `_cond_unstack`);
* biases, norm gammas, the conditioning path, the Fourier frequencies and the sinusoidal table stay fp32.
"""
import math
import re
from typing import Dict, List, NamedTuple

import torch

from . import _lib

SD = Dict[str, torch.Tensor]


def padk(c: int) -> int:
    return (c + 63) // 64 * 64


def padn(c: int) -> int:
    return (c + 127) // 128 * 128


def _act_dtype(dtype: int):
    return torch.bfloat16 if dtype == _lib.DN_BF16 else torch.float16 if dtype == _lib.DN_F16 else torch.float32


def _is16(dtype: int) -> bool:
    """the two 2-byte arithmetic modes share every packed layout (K-blocked copies included)"""
    return dtype in (_lib.DN_BF16, _lib.DN_F16)


def split_rows(t: torch.Tensor, weight: bool = False) -> torch.Tensor:
    """fp32 [..., K] (K a multiple of 32) -> DN_BF16X3 "split rows" (include/diffnorm_hip.h): a bf16 tensor [..., 2 K] of the same
    byte size as the fp32 one, every group of 32 elements stored as two 64-byte halves: hi = bf16(x) and lo = bf16(x - hi) (the
    difference is exact in fp32), so x = hi + lo to 16 mantissa bits.  Activations store [hi | lo], weights [lo | hi]: a
    contraction that walks a row in 64-byte K-tiles then meets (w_lo, a_hi) and (w_hi, a_lo) and has to keep only the
    activations' hi fragments across the pair for its three products w_lo a_hi + w_hi a_lo + w_hi a_hi."""
    t = t.float()
    assert t.shape[-1] % 32 == 0, t.shape
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    halves = [lo, hi] if weight else [hi, lo]
    g = torch.stack([h.reshape(*t.shape[:-1], -1, 32) for h in halves], dim=-2)  # [..., K/32, 2, 32]
    return g.reshape(*t.shape[:-1], 2 * t.shape[-1]).contiguous()


def unsplit_rows(t: torch.Tensor) -> torch.Tensor:
    """Inverse of split_rows (either order; tests): bf16 [..., 2 K] -> fp32 [..., K] = hi + lo."""
    g = t.reshape(*t.shape[:-1], -1, 2, 32).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*t.shape[:-1], t.shape[-1] // 2)


def _arith(t: torch.Tensor, dtype: int, weight: bool = True) -> torch.Tensor:
    """fp32 tensor (last dim = K, padded) -> the arithmetic dtype's storage (weight: a packed weight matrix, else activation rows)."""
    if dtype == _lib.DN_BF16X3:
        return split_rows(t, weight=weight)
    if dtype == _lib.DN_F16:  # the format ends at 65504: saturate, as the kernels do (FP16_OVFL), instead of inf
        return t.float().clamp(-65504.0, 65504.0).to(torch.float16)
    return t.to(_act_dtype(dtype))


def _mat(w: torch.Tensor, dtype: int, rows: int = None, cols: int = None) -> torch.Tensor:
    """[N,K] -> zero-padded [rows or padn(N), cols or padk(K)] in the arithmetic dtype."""
    n, k = w.shape
    out = torch.zeros(rows or padn(n), cols or padk(k), dtype=torch.float32)
    out[:n, :k] = w.float()
    return _arith(out, dtype)


def _vec(b: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=torch.float32)
    out[: b.numel()] = b.float().flatten()
    return out


def _conv(w: torch.Tensor, dtype: int) -> torch.Tensor:
    """[Cout,Cin,k] -> [k, padn(Cout), padk(Cin)], tap j = w[:, :, j]."""
    return torch.stack([_mat(w[:, :, j], dtype) for j in range(w.shape[2])])


def sinusoidal_table(num: int, dim: int, ld: int) -> torch.Tensor:
    """fairseq SinusoidalPositionalEmbedding table with padding_idx 0
    (reference fairseq/modules/sinusoidal_positional_embedding.py:36-58): rows
    [sin(p f_j) | cos(p f_j)], f_j = exp(-j ln(1e4)/(dim/2-1)), row 0 = 0; built in fp32 like upstream."""
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(num, dtype=torch.float).unsqueeze(1) * f.unsqueeze(0)
    tab = torch.zeros(num, ld, dtype=torch.float32)
    tab[:, :half] = torch.sin(ang)
    tab[:, half:2 * half] = torch.cos(ang)
    tab[0] = 0
    return tab


def _geglu_rows(inner: int) -> torch.Tensor:
    """Source row in Linear(D,2*inner).weight for every packed row (or -1 for a zero row)."""
    ip = padk(inner)
    p = torch.arange(2 * ip)
    # every 16-row MFMA tile is self-contained: 8 value rows then the 8 gate rows of the same output columns, so a kernel
    # may cut the packed matrix at any multiple of 16 rows (the 256 x 352 tile gives a wave 176 of them)
    col = (p // 16) * 8 + (p % 8)
    is_gate = (p % 16) >= 8
    src = torch.where(is_gate, col + inner, col)
    return torch.where(col < inner, src, torch.full_like(src, -1))


def kblock(t: torch.Tensor) -> torch.Tensor:
    """[.., rows, K] -> the K-blocked layout [.., K/32, rows, 32] (include/diffnorm_hip.h, DN_LAYOUT_*): the 64 bytes a
    32-deep K-tile takes from a row sit next to the neighbouring rows' 64 bytes of the same K-tile."""
    *lead, rows, K = t.shape
    assert K % 32 == 0
    return t.reshape(*lead, rows, K // 32, 32).transpose(-3, -2).contiguous()


def unkblock(t: torch.Tensor) -> torch.Tensor:
    """Inverse of kblock: [.., K/32, rows, 32] -> [.., rows, K]."""
    *lead, kb, rows, _ = t.shape
    return t.transpose(-3, -2).reshape(*lead, rows, kb * 32).contiguous()


# ------------------------------------------------------------------------------------------ layout rules, each beside its inverse
def _geglu_pack(w: torch.Tensor, inner: int, cols: int = None) -> torch.Tensor:
    """Linear(D, 2*inner) weight [2*inner, D] -> [2*padk(inner), cols], or its bias [2*inner] -> [2*padk(inner)], rows as _geglu_rows says."""
    rows = _geglu_rows(inner)
    keep = rows >= 0
    w2 = w.float().reshape(2 * inner, -1)
    out = torch.zeros(len(rows), cols or 1)
    out[keep, :w2.shape[1]] = w2[rows[keep]]
    return out if w.dim() == 2 else out[:, 0].contiguous()


def _geglu_unpack(p: torch.Tensor, inner: int, cols: int = None) -> torch.Tensor:
    """Inverse of _geglu_pack: the packed matrix -> [2*inner, cols], the packed bias -> [2*inner]."""
    rows = _geglu_rows(inner)
    keep = rows >= 0
    w = torch.zeros(2 * inner, cols or 1)
    w[rows[keep]] = p.reshape(len(rows), -1)[keep, :w.shape[1]]
    return w if p.dim() == 2 else w[:, 0].contiguous()


def _cond_stack(sd: SD, mods: List[str], leaf: str, D: int, Dp: int, rows: int = None) -> torch.Tensor:
    """The `leaf` ("weight" [2D, cols] / "bias" [2D], each [gamma ; beta]) of the conditioning projections `mods`, stacked as one
    [gamma (Dp) ; beta (Dp)] block per module: [rows or len(mods) * 2 Dp (, cols)]."""
    tail = sd[mods[0] + leaf].shape[1:]
    out = torch.zeros(rows or len(mods) * 2 * Dp, *tail)
    for m, blk in zip(mods, out[: len(mods) * 2 * Dp].view(len(mods), 2, Dp, *tail)):
        blk[:, :D] = sd[m + leaf].float().reshape(2, D, *tail)
    return out


def _cond_unstack(p: torch.Tensor, sd: SD, mods: List[str], leaf: str, D: int, Dp: int):
    """Inverse of _cond_stack: every module's [2D (, cols)] back under its key."""
    for m, blk in zip(mods, p[: len(mods) * 2 * Dp].view(len(mods), 2, Dp, *p.shape[1:])):
        sd[m + leaf] = blk[:, :D].reshape(2 * D, *p.shape[1:]).clone()


def eps_cond_modules(cfg) -> List[str]:
    """Key prefixes of the eps model's conditioning projections in the order of the stacked conditioning matrix: the FiLM of every
    WaveNet block, then per transformer layer the attention norm, [the cross-attention norm of the prompt-conditioned model,] the
    feed-forward norm.  A conditioning row has 2 * padk(dim) columns for each."""
    norms = (0, 2, 4) if getattr(cfg, "dim_prompt", 0) > 0 else (0, 4)
    return ([f"wavenet.stacks.{s}.blocks.{i}.to_time_cond." for s in range(cfg.wavenet_stacks) for i in range(cfg.wavenet_layers)]
            + [f"transformer.layers.{l}.{j}.to_gamma_beta." for l in range(cfg.depth) for j in norms])


def vae_mults(latent_flag: int) -> List[int]:
    """chan_mults of SpeechVAEEncoderDecoder (reference latent_module.py:1044-1051)."""
    return {16: [4, 3, 2], 32: [4, 3], 128: [3]}[latent_flag]


def vae_chain(dim: int, mults: List[int]):
    """(key prefix, cin, cout) of the VAE's cascaded WaveNets (reference latent_module.py:1053-1081): the encoder divides the width by
    every chan_mult, the decoder multiplies it back; its first WaveNet reads the posterior sample, half the encoder's [mean ; logvar]."""
    cur = dim
    for n, m in enumerate(mults):
        yield f"encoder_wave.{n}.", cur, cur // m
        cur //= m
    cin = cur // 2
    for n, m in enumerate(reversed(mults)):
        cur *= m
        yield f"decoder_wave.{n}.", cin, cur
        cin = cur


# ------------------------------------------------------------------------------------------ the table of packed tensors
class _Entry:
    """One packed tensor: `pack(sd)` builds it in fp32, of `shape`, from a state dict in the reference layout; `unpack(p, sd)` writes
    it (or its gradient) back under the reference's keys and shapes.  `arith`: "weight" = a contraction's weight, which the inference
    lists hold in the arithmetic dtype; "act" = activation rows in it; None = fp32 in every mode (biases, gammas, conditioning).
    `unpack` is None where nothing is trained: the prompt tokens and `lat_pos` (positions folded into the latents: no inverse)."""

    def __init__(self, name, shape, pack, unpack=None, arith=None):
        self.name, self.shape, self.pack, self.unpack, self.arith = name, tuple(shape), pack, unpack, arith


def _set(key: str, fn):
    return lambda p, sd: sd.__setitem__(key, fn(p))


def _raw(name, key, shape) -> _Entry:
    return _Entry(name, shape, lambda sd: sd[key].float().clone(), _set(key, torch.clone))


def _bias(name, key, n, n_pad) -> _Entry:
    return _Entry(name, (n_pad,), lambda sd: _vec(sd[key], n_pad), _set(key, lambda p: p[:n].clone()))


def _lin(name, key, n, k, k1=False, arith="weight") -> _Entry:
    """Linear weight [n, k], or (k1) the [n, k, 1] of a 1 x 1 conv."""
    return _Entry(name, (padn(n), padk(k)), lambda sd: _mat(sd[key][:, :, 0] if k1 else sd[key], _lib.DN_F32),
                  _set(key, lambda p: p[:n, :k].clone().unsqueeze(-1) if k1 else p[:n, :k].clone()), arith)


def _conv3(name, key, n, k) -> _Entry:
    return _Entry(name, (3, padn(n), padk(k)), lambda sd: _conv(sd[key], _lib.DN_F32),
                  _set(key, lambda p: p[:, :n, :k].permute(1, 2, 0).contiguous()), "weight")


def _stacked(name, ents: List[_Entry]) -> _Entry:
    """Entries of one shape as one [len(ents), ...] entry: one tensor of every block of a WaveNet."""
    return _Entry(name, (len(ents),) + ents[0].shape, lambda sd: torch.stack([e.pack(sd) for e in ents]),
                  lambda p, sd: [e.unpack(p[n], sd) for n, e in enumerate(ents)], ents[0].arith)


def _attn_entries(name, key, dim, hd, fused) -> List[_Entry]:
    """Projections of the attention block under `key`: [q, kv, out], or [qkv, out] where q and kv read the same rows (self-attention)."""
    q, kv, out = (_lin(f"{name}{n}_W", f"{key}to_{n}.weight", r, c) for n, r, c in (("q", hd, dim), ("kv", 2 * hd, dim), ("out", dim, hd)))
    if not fused:
        return [q, kv, out]
    qkv = _Entry(name + "qkv_W", (padn(3 * hd), padk(dim)), lambda sd: _mat(torch.cat([q.pack(sd)[:hd], kv.pack(sd)[: 2 * hd]]), _lib.DN_F32),
                 lambda p, sd: (q.unpack(p[:hd], sd), kv.unpack(p[hd:], sd)), "weight")
    return [qkv, out]


def _geglu_entries(name, key, dim, inner) -> List[_Entry]:
    return [_Entry(name + "_W", (2 * padk(inner), padk(dim)), lambda sd: _geglu_pack(sd[key + "weight"], inner, padk(dim)),
                   _set(key + "weight", lambda p: _geglu_unpack(p, inner, dim)), "weight"),
            _Entry(name + "_b", (2 * padk(inner),), lambda sd: _geglu_pack(sd[key + "bias"], inner), _set(key + "bias", lambda p: _geglu_unpack(p, inner)))]


def _wavenet_entries(prefix: str, cin: int, cout: int, S: int, L: int) -> List[_Entry]:
    cp = padk(cout)
    blocks = [f"{prefix}stacks.{s}.blocks.{i}." for s in range(S) for i in range(L)]
    return [
        _conv3(prefix + "init_W", prefix + "init_conv.weight", cout, cin), _bias(prefix + "init_b", prefix + "init_conv.bias", cout, cp),
        _stacked(prefix + "conv_W", [_conv3("", b + "conv.weight", cout, cout) for b in blocks]),
        _stacked(prefix + "conv_b", [_bias("", b + "conv.bias", cout, cp) for b in blocks]),
        _stacked(prefix + "res_W", [_lin("", b + "res_conv.weight", cout, cout, k1=True) for b in blocks]),
        _stacked(prefix + "res_b", [_bias("", b + "res_conv.bias", cout, cp) for b in blocks]),
        # only the last stack's blocks feed the skip sum
        _stacked(prefix + "skip_W", [_lin("", b + "skip_conv.weight", cout, cout, k1=True) for b in blocks[-L:]]),
        _stacked(prefix + "skip_b", [_bias("", b + "skip_conv.bias", cout, cp) for b in blocks[-L:]]),
        _lin(prefix + "final_W", prefix + "final_conv.weight", cout, cout, k1=True), _bias(prefix + "final_b", prefix + "final_conv.bias", cout, cp),
    ]


def _tf_layer_entries(prefix: str, l: int, dim: int, heads: int, dim_head: int, gammas: bool = True) -> List[_Entry]:
    """One transformer layer.  gammas: its two RMSNorms' learned gammas (the VAE's decoder); the eps model's norms are adaptive, their
    scale and shift are rows of the conditioning stack.  (The prompt-conditioned model's cross-attention block: _eps_prompt_entries.)"""
    inner = int(dim * 4 * 2 / 3)
    p_ = f"{prefix}layers.{l}."
    ents = _attn_entries(p_, p_ + "1.", dim, heads * dim_head, fused=True) + _geglu_entries(p_ + "ffin", p_ + "5.0.", dim, inner) + [
        _conv3(p_ + "ffconv_W", p_ + "5.2.1.weight", inner, inner), _bias(p_ + "ffconv_b", p_ + "5.2.1.bias", inner, padk(inner)),
        _lin(p_ + "ffout_W", p_ + "5.3.weight", dim, inner), _bias(p_ + "ffout_b", p_ + "5.3.bias", dim, padk(dim)),
    ]
    if gammas:
        ents += [_raw(p_ + "g1", p_ + "0.gamma", (dim,)), _raw(p_ + "g2", p_ + "4.gamma", (dim,))]
    return ents


def _tf_entries(name: str, prefix: str, dim: int, depth: int, heads: int, dim_head: int, gammas: bool):
    """A transformer as (per-layer tables, [final norm's gamma, to_pred])."""
    return ([_tf_layer_entries(prefix, l, dim, heads, dim_head, gammas) for l in range(depth)],
            [_raw(name + "pred_gamma", prefix + "to_pred.0.gamma", (dim,)), _lin(name + "pred_W", prefix + "to_pred.1.weight", dim, dim)])


def _eps_entries(cfg):
    """The eps model as (head, WaveNet, transformer layers, to_pred, tail).  head = the conditioning path first: to_time_cond, then
    the conditioning projections (eps_cond_modules) stacked as [gamma (Dp) ; beta (Dp)] rows over C (2C: [time | pooled prompt]
    with a prompt branch, reference latent_module.py:784, 852) columns."""
    D, Dp, zl, C = cfg.dim, padk(cfg.dim), cfg.latent_dim, cfg.dim * cfg.dim_cond_mult
    mods = eps_cond_modules(cfg)
    n_cond, C2 = len(mods) * 2 * Dp, 2 * C if getattr(cfg, "dim_prompt", 0) > 0 else C
    head = [
        _raw("w_freq", "to_time_cond.0.weights", (D // 2,)), _raw("tc_W", "to_time_cond.1.weight", (C, D + 1)), _raw("tc_b", "to_time_cond.1.bias", (C,)),
        _Entry("cond_W", (padn(n_cond), C2), lambda sd: _cond_stack(sd, mods, "weight", D, Dp, padn(n_cond)),
               lambda p, sd: _cond_unstack(p, sd, mods, "weight", D, Dp)),
        _Entry("cond_b", (n_cond,), lambda sd: _cond_stack(sd, mods, "bias", D, Dp), lambda p, sd: _cond_unstack(p, sd, mods, "bias", D, Dp)),
        _lin("init_W", "init_conv.weight", D, zl, k1=True), _bias("init_b", "init_conv.bias", D, Dp),
    ]
    tail = [_lin("final_W", "final_proj.weight", zl, D), _bias("final_b", "final_proj.bias", zl, padk(zl))]
    return (head, _wavenet_entries("wavenet.", D, D, cfg.wavenet_stacks, cfg.wavenet_layers),
            *_tf_entries("", "transformer.", D, cfg.depth, cfg.heads, cfg.dim_head, gammas=False), tail)


def _eps_prompt_entries(cfg):
    """The prompt branch (reference latent_module.py:416-471, 752-773) as (head, resampler layers, resampler norm, cross-attention
    layers).  head = prompt-condition MLP and null condition (fp32), null prompt tokens, the PerceiverResampler's input projection and
    its latents with their sinusoidal positions 1..m folded in (a constant); then the resampler's layers and, per transformer layer,
    the cross-attention projections."""
    D, Dp, C, P, m = cfg.dim, padk(cfg.dim), cfg.dim * cfg.dim_cond_mult, cfg.dim_prompt, cfg.num_latents_m
    inner, hd, r = int(D * 4 * 2 / 3), cfg.heads * cfg.dim_head, "perceiver_resampler."
    resampler = [_attn_entries("", f"{r}layers.{l}.0.", D, hd, fused=False) + _geglu_entries("", f"{r}layers.{l}.1.0.", D, inner)
                 + [_lin("", f"{r}layers.{l}.1.2.weight", D, inner), _bias("", f"{r}layers.{l}.1.2.bias", D, Dp)] for l in range(cfg.resampler_depth)]
    cross = [_attn_entries("", f"transformer.layers.{l}.3.", D, hd, fused=False) for l in range(cfg.depth)]
    head = [
        _lin("tpc_W", "to_prompt_cond.1.weight", C, P, arith=None), _raw("tpc_b", "to_prompt_cond.1.bias", (C,)), _raw("null_pc", "null_prompt_cond", (C,)),
        _Entry("null_tok", (m, Dp), lambda sd: _mat(sd["null_prompt_tokens"], _lib.DN_F32, rows=m), arith="act"),
        _lin("proj_W", r + "proj_context.weight", D, P), _bias("proj_b", r + "proj_context.bias", D, Dp),
        _Entry("lat_pos", (m, Dp), lambda sd: _mat(sd[r + "latents"].float() + sinusoidal_table(m + 1, D, D)[1: m + 1], _lib.DN_F32, rows=m)),
    ]
    return head, resampler, [_raw("rnorm_g", r + "norm.gamma", (D,))], cross


def _vae_entries(dim: int, mults: List[int], depth: int, heads: int, dim_head: int, stacks: int, layers: int, vocab: int):
    """The VAE as (its WaveNets' tables, transformer layers, to_pred, tail)."""
    tail = [_lin("decoder_lm.W", "decoder_lm.weight", vocab, dim), _bias("decoder_lm.b", "decoder_lm.bias", vocab, padn(vocab))]
    return ([_wavenet_entries(prefix, cin, cout, stacks, layers) for prefix, cin, cout in vae_chain(dim, mults)],
            *_tf_entries("decoder_tf.", "decoder_tf.", dim, depth, heads, dim_head, gammas=True), tail)


# ------------------------------------------------------------------------------------------ training: the flat buffers
# The flat fp32 parameter / gradient buffers of the training engines (csrc/train_engine.hip) hold the table's packed tensors one
# after the other, the transformer's layer by layer.  `unpack` is what turns the flat gradient buffer into per-parameter gradients
# under the reference's names, and the flat master buffer into a checkpoint the reference can load.
def vae_train_entries(dim: int, mults: List[int], depth: int, heads: int, dim_head: int, stacks: int, layers: int,
                      vocab: int) -> List[_Entry]:
    """Table of the VAE training engine's packed tensors, in the order of dn_vae_train_offsets."""
    waves, tf_layers, pred, tail = _vae_entries(dim, mults, depth, heads, dim_head, stacks, layers, vocab)
    return sum(waves + tf_layers, []) + pred + tail


def eps_train_entries(cfg) -> List[_Entry]:
    """Table of the diffusion training engine's packed tensors, in the order of dn_eps_train_offsets."""
    head, wave, tf_layers, pred, tail = _eps_entries(cfg)
    return head + wave + sum(tf_layers, []) + pred + tail


def pack_flat(sd: SD, entries: List[_Entry], offsets: List[int], total: int) -> torch.Tensor:
    """State dict (reference layout) -> flat fp32 buffer of `total` elements."""
    flat = torch.zeros(total, dtype=torch.float32)
    for e, off in zip(entries, offsets):
        t = e.pack(sd).float()
        assert tuple(t.shape) == e.shape, (e.name, tuple(t.shape), e.shape)
        flat[off: off + t.numel()] = t.reshape(-1)
    return flat


def unpack_flat(flat: torch.Tensor, entries: List[_Entry], offsets: List[int]) -> SD:
    """Flat buffer (parameters or gradients) -> tensors under the reference's state-dict names and shapes."""
    flat = flat.detach().float().cpu()
    sd: SD = {}
    for e, off in zip(entries, offsets):
        e.unpack(flat[off: off + math.prod(e.shape)].view(e.shape), sd)
    return sd


# ------------------------------------------------------------------------------------------ inference: the ordered lists (csrc/engine.h)
# Each list walks the same tables: the packed fp32 tensor in the arithmetic dtype (_pack), a layered piece's stacked per tensor
# (_per_tensor), plus the tensors derived for inference only, which each function below names where it returns.
def _pack(ents: List[_Entry], sd: SD, dtype: int) -> List[torch.Tensor]:
    return [_arith(e.pack(sd), dtype, weight=e.arith == "weight") if e.arith else e.pack(sd) for e in ents]


def _per_tensor(layers: List[List[_Entry]], sd: SD, dtype: int) -> List[torch.Tensor]:
    """Per-layer tables (the flat buffers are layer-major) -> every tensor stacked over the layers (the inference lists' order)."""
    return [torch.stack(_pack(col, sd, dtype)) for col in zip(*layers)]


def _kb(w: torch.Tensor, dtype: int) -> torch.Tensor:
    """The K-blocked copy of a stacked weight that the 2-byte modes' large tiles read; a placeholder in the other modes."""
    return kblock(w) if _is16(dtype) else torch.zeros(4)


def _wavenet_tensors(ents: List[_Entry], sd: SD, dtype: int) -> List[torch.Tensor]:
    init_W, init_b, conv_W, conv_b, res_W, res_b, skip_W, skip_b, final_W, final_b = _pack(ents, sd, dtype)
    # derived: one bias for the summed skip path; conv_W and res_W K-blocked for the 256 x 256 tile
    return [init_W, init_b, conv_W, conv_b, res_W, res_b, skip_W, sum(skip_b), final_W, final_b, _kb(conv_W, dtype), _kb(res_W, dtype)]


def _tf_tensors(tf_layers: List[List[_Entry]], pred: List[_Entry], sd: SD, dtype: int) -> List[torch.Tensor]:
    qkv, out, ffin, ffin_b, ffc, ffc_b, ffo, ffo_b, *gammas = _per_tensor(tf_layers, sd, dtype)
    # derived: placeholders for the gammas adaptive norms do not have; K-blocked copies of the FFN conv's weights (256 x 352 tile),
    # the GEGLU projection's (its activations arrive K-blocked from the split norm's producer) and the q/kv projection's (layers
    # >= 1 read the attention norm's output K-blocked from the previous layer's last contraction)
    g1, g2 = gammas or (torch.zeros(4), torch.zeros(4))
    return [qkv, out, ffin, ffin_b, ffc, ffc_b, ffo, ffo_b, g1, g2, *_pack(pred, sd, dtype), _kb(ffc, dtype), _kb(ffin, dtype), _kb(qkv, dtype)]


def pack_wavenet(sd: SD, prefix: str, cin: int, cout: int, stacks: int, layers: int, dtype: int) -> List[torch.Tensor]:
    return _wavenet_tensors(_wavenet_entries(prefix, cin, cout, stacks, layers), sd, dtype)


def pack_transformer(sd: SD, prefix: str, dim: int, depth: int, heads: int, dim_head: int, dtype: int,
                     conditioned: bool) -> List[torch.Tensor]:
    return _tf_tensors(*_tf_entries("", prefix, dim, depth, heads, dim_head, gammas=not conditioned), sd, dtype)


def pack_eps(sd: SD, cfg, dtype: int, max_pos: int = 2048) -> List[torch.Tensor]:
    """cfg: object with dim, latent_dim, depth, heads, dim_head, wavenet_layers, wavenet_stacks, dim_cond_mult [, dim_prompt,
    num_latents_m, resampler_depth: the conditional variant, whose extra tensors (csrc/engine.h kEpsCondTensors) follow the table]."""
    head, wave, tf_layers, pred, tail = _eps_entries(cfg)
    tensors = _pack(head, sd, dtype) + _wavenet_tensors(wave, sd, dtype) + _tf_tensors(tf_layers, pred, sd, dtype) + _pack(tail, sd, dtype)
    tensors.append(sinusoidal_table(max_pos + 1, cfg.dim, padk(cfg.dim)))  # derived: the frames' positions
    return tensors + (pack_eps_cond(sd, cfg, dtype) if getattr(cfg, "dim_prompt", 0) > 0 else [])


def pack_eps_cond(sd: SD, cfg, dtype: int) -> List[torch.Tensor]:
    """The conditional variant's extra tensors, in csrc/engine.h's kEpsCondTensors order."""
    head, resampler, norm, cross = _eps_prompt_entries(cfg)
    return _pack(head, sd, dtype) + _per_tensor(resampler, sd, dtype) + _pack(norm, sd, dtype) + _per_tensor(cross, sd, dtype)


def pack_vae(sd: SD, dim: int, mults: List[int], depth: int, heads: int, dim_head: int, stacks: int, layers: int,
             vocab: int, dtype: int) -> List[torch.Tensor]:
    waves, tf_layers, pred, tail = _vae_entries(dim, mults, depth, heads, dim_head, stacks, layers, vocab)
    return sum((_wavenet_tensors(w, sd, dtype) for w in waves), []) + _tf_tensors(tf_layers, pred, sd, dtype) + _pack(tail, sd, dtype)


# ------------------------------------------------------------------------------------------ inference: the folded feed-forward weights
# Beside the lists, not in them (csrc/engine.h TransformerW.fold_W / fold_b): dn_ffn_fold (csrc/repack.hip) forms them on the device
# from the packed fp32 sources below -- here from a state dict, in engine.py from a training engine's flat buffer.
_FOLD_COLS = (4, 5, 6, 7)  # ffconv_W, ffconv_b, ffout_W, ffout_b in _tf_layer_entries' order


def ffn_fold_sources(layer: List[_Entry], sd: SD) -> List[torch.Tensor]:
    """One transformer layer's packed fp32 (conv_W [3][padn(inner)][padk(inner)], conv_b, out_W [padn(dim)][padk(inner)], out_b)."""
    return [layer[j].pack(sd).float().contiguous() for j in _FOLD_COLS]


def ffn_fold_offsets(entries: List[_Entry], offsets: List[int]):
    """Where a training engine's flat buffer holds those four tensors: (layer 0's element offsets, the elements between layers)."""
    per = [[o for e, o in zip(entries, offsets) if re.search(r"(?:^|\.)layers\.\d+\." + n + "$", e.name)] for n in ("ffconv_W", "ffconv_b", "ffout_W", "ffout_b")]
    depth = len(per[0])
    assert depth >= 1 and all(len(p) == depth for p in per)
    strides = [p[1] - p[0] if depth > 1 else 0 for p in per]
    assert all(p[l] == p[0] + l * st for p, st in zip(per, strides) for l in range(depth)), "the layers' tables lie a constant distance apart"
    return [p[0] for p in per], strides


def ffn_fold_storage(dim: int, depth: int, dtype: int):
    """((shape, torch dtype) of fold_W, shape of fold_b) for a transformer of width `dim` in the arithmetic `dtype`."""
    inner = int(dim * 4 * 2 / 3)
    return _w_storage((depth, 3, padn(dim), padk(inner)), dtype), (depth, padk(dim))


def ffn_fold_ref(conv_W: torch.Tensor, conv_b: torch.Tensor, out_W: torch.Tensor, out_b: torch.Tensor):
    """The fold in float64 from the reference's tensors (conv_W [inner, inner, 3], out_W [dim, inner]): (W' [3, dim, inner], b' [dim])."""
    cw, ow = conv_W.double(), out_W.double()
    return torch.stack([ow @ cw[:, :, j] for j in range(3)]), ow @ conv_b.double() + out_b.double()


# ------------------------------------------------------------------------------------------ inference lists from the flat master buffer
# The third walk over the tables: for a training engine's entry table and offsets, the descriptors of dn_repack_weights
# (csrc/repack.hip), which writes the tensors pack_eps / pack_vae return straight from the flat fp32 master buffer on the device.
# The master holds every entry's packed fp32 tensor, so what is left is the conversion to the arithmetic dtype (CONVERT), the
# transformer's per-tensor stacking (one item per layer slice), the K-blocked copies (KBLOCK), fp32 copies (COPY) and the summed
# skip bias (SUM).
class RepackItem(NamedTuple):
    """One DnRepackDesc (include/diffnorm_hip.h): `mats` matrices [rows][K] from element `src` of the master to byte `dst_byte` of
    destination tensor `tensor` (its index in pack_eps / pack_vae's list)."""
    tensor: int
    dst_byte: int
    src: int
    kind: int
    mats: int
    rows: int
    K: int
    count: int = 0
    stride: int = 0


class RepackPlan(NamedTuple):
    """items: the descriptors, in destination order.  shapes: per tensor of pack_eps / pack_vae's list its (shape, torch dtype), or
    None for a tensor that does not depend on the parameters (the sinusoidal table, placeholders): those are not written."""
    items: List[RepackItem]
    shapes: list


def _w_storage(shape, dtype: int):
    """(shape, torch dtype) in which a weight of packed fp32 `shape` is stored in the arithmetic dtype."""
    if dtype == _lib.DN_BF16X3:
        return tuple(shape[:-1]) + (2 * shape[-1],), torch.bfloat16
    return tuple(shape), _act_dtype(dtype)


def repack_plan(entries: List[_Entry], offsets: List[int], dtype: int, kind: str = "eps") -> RepackPlan:
    """entries / offsets: a training engine's table (eps_train_entries / vae_train_entries) and dn_*_train_offsets; dtype: the
    inference engine's arithmetic.  kind "eps": the unconditional eps-predictor's list (pack_eps); "vae": pack_vae's."""
    assert kind in ("eps", "vae") and len(entries) == len(offsets)
    wes = 2 if _is16(dtype) else 4  # bytes per element of a stored weight (split rows: two bf16)
    items, shapes = [], []

    def put(e: _Entry, src: int, tensor: int, layer: int = 0):
        n = math.prod(e.shape)
        if e.arith == "weight":
            *lead, rows, K = e.shape
            items.append(RepackItem(tensor, layer * n * wes, src, _lib.REPACK_CONVERT, math.prod(lead), rows, K))
        elif e.arith is None:
            items.append(RepackItem(tensor, layer * n * 4, src, _lib.REPACK_COPY, 1, 1, n))
        else:
            raise NotImplementedError(f"{e.name}: activation-order entries belong to the prompt-conditioned model, which has no training engine")

    def tensor_of(e: _Entry, lead=()):
        shapes.append(_w_storage(lead + e.shape, dtype) if e.arith == "weight" else (lead + e.shape, torch.float32))
        return len(shapes) - 1

    def plain(e: _Entry, src: int):
        put(e, src, tensor_of(e))

    def kblocked(e: _Entry, srcs: List[int], lead=()):
        """The K-blocked copy of a weight (stacked over len(srcs) layers when lead is given); a placeholder outside the 2-byte modes."""
        if not _is16(dtype):
            shapes.append(None)
            return
        *mid, rows, K = e.shape
        shapes.append((lead + tuple(mid) + (K // 32, rows, 32), _act_dtype(dtype)))
        for l, src in enumerate(srcs):
            items.append(RepackItem(len(shapes) - 1, l * math.prod(e.shape) * wes, src, _lib.REPACK_KBLOCK, math.prod(mid), rows, K))

    def wavenet(ents: List[_Entry], offs: List[int]):
        init_W, init_b, conv_W, conv_b, res_W, res_b, skip_W, skip_b, final_W, final_b = ents
        for e, o in zip(ents[:7], offs[:7]):
            plain(e, o)
        L, cp = skip_b.shape  # one bias for the summed skip path
        shapes.append(((cp,), torch.float32))
        items.append(RepackItem(len(shapes) - 1, 0, offs[7], _lib.REPACK_SUM, 1, 1, cp, L, cp))
        plain(final_W, offs[8])
        plain(final_b, offs[9])
        kblocked(conv_W, [offs[2]])
        kblocked(res_W, [offs[4]])

    def transformer(layers: List[List[_Entry]], layer_offs: List[List[int]], pred: List[_Entry], pred_offs: List[int]):
        depth, cols = len(layers), list(zip(*layers))
        for j, col in enumerate(cols):
            t = tensor_of(col[0], (depth,))
            for l, e in enumerate(col):
                assert e.shape == col[0].shape and e.arith == col[0].arith
                put(e, layer_offs[l][j], t, l)
        if len(cols) == 8:  # adaptive norms: no learned gammas, two placeholders
            shapes.extend([None, None])
        for e, o in zip(pred, pred_offs):
            plain(e, o)
        for j in (4, 2, 0):  # ffconv_W, ffin_W, qkv_W
            kblocked(cols[j][0], [layer_offs[l][j] for l in range(depth)], (depth,))

    layer_of = lambda e: re.search(r"(?:^|\.)layers\.(\d+)\.", e.name)
    i = 0
    while i < len(entries):
        e = entries[i]
        if e.name.endswith(".init_W"):  # a WaveNet's ten tensors
            wavenet(entries[i: i + 10], offsets[i: i + 10])
            i += 10
        elif layer_of(e):  # the transformer: its layers' tables one after the other, then [final norm's gamma, to_pred]
            layers, layer_offs = [], []
            while i < len(entries) and layer_of(entries[i]):
                l = int(layer_of(entries[i]).group(1))
                if l == len(layers):
                    layers.append([])
                    layer_offs.append([])
                layers[l].append(entries[i])
                layer_offs[l].append(offsets[i])
                i += 1
            transformer(layers, layer_offs, entries[i: i + 2], offsets[i: i + 2])
            i += 2
        else:
            plain(e, offsets[i])
            i += 1
    if kind == "eps":
        shapes.append(None)  # the sinusoidal table of the frames' positions
    return RepackPlan(items, shapes)


def repack_emulate(master: torch.Tensor, plan: RepackPlan, dtype: int) -> list:
    """What dn_repack_weights writes for `plan` from the flat fp32 `master`, in torch on the CPU: the list of destination tensors
    (None where the plan leaves a tensor alone).  Bytes no item writes stay 0xFF."""
    master = master.detach().float().cpu()
    esize = lambda dt: torch.empty(0, dtype=dt).element_size()
    bufs = [None if s is None else torch.full((math.prod(s[0]) * esize(s[1]),), 0xFF, dtype=torch.uint8) for s in plan.shapes]
    for it in plan.items:
        src = master[it.src: it.src + it.mats * it.rows * it.K].view(it.mats, it.rows, it.K)
        if it.kind == _lib.REPACK_CONVERT:
            out = _arith(src, dtype, weight=True)
        elif it.kind == _lib.REPACK_KBLOCK:
            out = kblock(_arith(src, dtype, weight=True))
        elif it.kind == _lib.REPACK_COPY:
            out = src
        else:
            out = torch.zeros(it.K)
            for j in range(it.count):
                out = out + master[it.src + j * it.stride: it.src + j * it.stride + it.K]
        b = out.contiguous().view(torch.uint8).reshape(-1)
        bufs[it.tensor][it.dst_byte: it.dst_byte + b.numel()] = b
    return [None if s is None else b.view(s[1]).view(s[0]) for s, b in zip(plan.shapes, bufs)]
