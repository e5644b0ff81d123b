"""TEST INFRASTRUCTURE ONLY.  The Conformer speech encoder of the NAR S2UT recipe restated in plain torch from its equations
(S2TConformerEncoder._forward, fairseq/models/speech_to_text/s2t_conformer.py:91-137; ConformerEncoderLayer.forward,
fairseq/modules/conformer_layer.py:229-284; RelPositionMultiHeadedAttention.forward, fairseq/modules/espnet_multihead_attention.py:
153-196; RelPositionalEncoding, fairseq/modules/positional_encoding.py:94-112), eval mode, parametrised by dtype; a tiny
configuration that plugs into the fixture decoder (oracle/gen_golden_nar_configs.CFG: embed 64, 4 heads); and seeded formula weights
under the reference's state-dict names.  tools/gen_golden_conformer.py checks this file against the real classes and writes
tests/golden/conformer_encoder.npz."""
import math
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

TINY = types.SimpleNamespace(input_dim=80, conv_channels=128, kernel_sizes=(5, 5), embed_dim=64, heads=4, ffn_dim=128, layers=2,
                             depthwise_kernel=31)
RECIPE2 = types.SimpleNamespace(input_dim=80, conv_channels=1024, kernel_sizes=(5, 5), embed_dim=512, heads=8, ffn_dim=2048, layers=2,
                                depthwise_kernel=31)  # the recipe's widths, two layers
TINY_SEED = 20240


def _normal(seed, name, shape, scale):
    """Seeded N(0, scale^2) values, one legacy MT19937 stream per tensor name (stable across numpy / torch versions)."""
    rs = np.random.RandomState((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
    return torch.from_numpy(rs.standard_normal(size=shape) * scale).float()


def make_state_dict(cfg=TINY, seed=TINY_SEED):
    """S2TConformerEncoder.state_dict() names (attn_type espnet, pos_enc_type rel_pos), fp32: O(1) activations, non-trivial BatchNorm
    running statistics, non-zero pos_bias_u / pos_bias_v."""
    D, Fd, H, K = cfg.embed_dim, cfg.ffn_dim, cfg.heads, cfg.depthwise_kernel
    sd = {}
    n = lambda name, shape, scale: _normal(seed, name, shape, scale)

    def lin(name, out, inp, bias=True, gain=1.0):
        sd[name + ".weight"] = n(name + ".weight", (out, inp), gain * inp ** -0.5)
        if bias:
            sd[name + ".bias"] = n(name + ".bias", (out,), 0.1)

    def norm(name):
        sd[name + ".weight"] = 1.0 + n(name + ".weight", (D,), 0.1)
        sd[name + ".bias"] = n(name + ".bias", (D,), 0.1)

    nk = len(cfg.kernel_sizes)
    for i, k in enumerate(cfg.kernel_sizes):
        cin = cfg.input_dim if i == 0 else cfg.conv_channels // 2
        cout = cfg.conv_channels if i < nk - 1 else 2 * D
        sd[f"subsample.conv_layers.{i}.weight"] = n(f"conv{i}.w", (cout, cin, k), 1.7 * (cin * k) ** -0.5)
        sd[f"subsample.conv_layers.{i}.bias"] = n(f"conv{i}.b", (cout,), 0.1)
    lin("linear", D, D, gain=D ** -0.5)  # the input is sqrt(D) * glu(.)
    for l in range(cfg.layers):
        p = f"conformer_layers.{l}."
        for ffn in ("ffn1", "ffn2"):
            norm(p + ffn + ".layer_norm")
            lin(p + ffn + ".w_1", Fd, D)
            lin(p + ffn + ".w_2", D, Fd)
        norm(p + "self_attn_layer_norm")
        for proj in ("linear_q", "linear_k", "linear_v", "linear_out"):
            lin(p + "self_attn." + proj, D, D)
        lin(p + "self_attn.linear_pos", D, D, bias=False)
        sd[p + "self_attn.pos_bias_u"] = n(p + "u", (H, D // H), 0.3)
        sd[p + "self_attn.pos_bias_v"] = n(p + "v", (H, D // H), 0.3)
        cm = p + "conv_module."
        norm(cm + "layer_norm")
        sd[cm + "pointwise_conv1.weight"] = n(cm + "pw1", (2 * D, D, 1), D ** -0.5)
        sd[cm + "depthwise_conv.weight"] = n(cm + "dw", (D, 1, K), 1.5 * K ** -0.5)
        sd[cm + "batch_norm.weight"] = 1.0 + n(cm + "bn.w", (D,), 0.2)
        sd[cm + "batch_norm.bias"] = n(cm + "bn.b", (D,), 0.2)
        sd[cm + "batch_norm.running_mean"] = n(cm + "bn.m", (D,), 0.3)
        sd[cm + "batch_norm.running_var"] = 0.5 + n(cm + "bn.v", (D,), 0.4).abs()
        sd[cm + "pointwise_conv2.weight"] = n(cm + "pw2", (D, D, 1), D ** -0.5)
        norm(p + "final_layer_norm")
    return sd


def make_features(B, L, lengths, input_dim, seed):
    """Zero-padded fbank-like features, as the collater leaves them."""
    lengths = torch.as_tensor(lengths)
    feats = _normal(seed, "feats", (B, L, input_dim), 1.0)
    return feats * (torch.arange(L)[None, :, None] < lengths[:, None, None]), lengths


def rel_pe(S: int, D: int) -> torch.Tensor:
    """RelPositionalEncoding's table for offsets d = -(S-1) .. S-1 (row S - 1 + d), built in FLOAT32 as upstream
    (positional_encoding.py:94-112: position * div_term in float32): pe(d)[2m] = sin(d w_m), pe(d)[2m+1] = cos(d w_m)."""
    d = torch.arange(-(S - 1), S, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, D, 2, dtype=torch.float32) * -(math.log(10000.0) / D))
    pe = torch.zeros(2 * S - 1, D)
    pe[:, 0::2] = torch.sin(d * div)
    pe[:, 1::2] = torch.cos(d * div)
    return pe


def subsampled_lengths(lengths, n=2):
    out = torch.as_tensor(lengths).clone()
    for _ in range(n):
        out = ((out.float() - 1) / 2 + 1).floor().long()
    return out


def rel_attention(q, k, v, pos, u, v_bias, lengths, scale=None):
    """score[i, j] = ((q_i + u) . k_j + (q_i + v) . pos[S - 1 + i - j]) * scale, keys j >= lengths[b] at -inf, softmax, times V.
    q, k, v [B, H, S, dk]; pos [H, 2S-1, dk] (row S - 1 + d); u, v_bias [H, dk] -> [B, H, S, dk].  The [S, S] gather of the positional
    term is the host restatement's; the device kernel never forms it."""
    B, H, S, dk = q.shape
    scale = dk ** -0.5 if scale is None else scale
    ac = torch.matmul(q + u[None, :, None, :], k.transpose(-1, -2))
    bd_all = torch.matmul(q + v_bias[None, :, None, :], pos.transpose(-1, -2)[None])  # [B, H, S, 2S-1]
    t = torch.arange(S, device=q.device)
    idx = (S - 1) + t[:, None] - t[None, :]
    bd = torch.gather(bd_all, 3, idx[None, None].expand(B, H, S, S))
    sc = (ac + bd) * scale
    mask = t[None, :] >= torch.as_tensor(lengths).to(q.device)[:, None]
    sc = sc.masked_fill(mask[:, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(sc, -1), v)


def glu_dwconv(x, w, bn_w, bn_b, bn_mean, bn_var, eps=1e-5):
    """x [B, S, 2C] -> swish(BatchNorm_eval(depthwise_conv(glu(x)))) [B, S, C]; w [C, 1, k]; unmasked, zero 'same' padding."""
    C, k = w.shape[0], w.shape[-1]
    y = F.glu(x, dim=-1).transpose(1, 2)
    y = F.conv1d(y, w, None, 1, (k - 1) // 2, 1, C)
    y = (y - bn_mean[None, :, None]) / torch.sqrt(bn_var[None, :, None] + eps) * bn_w[None, :, None] + bn_b[None, :, None]
    return F.silu(y).transpose(1, 2)


def conformer_layer(x, sd, p, H, lengths, pe):
    """One ConformerEncoderLayer on x [B, S, D] (batch-major)."""
    B, S, D = x.shape
    g = lambda k: sd[p + k]
    ln = lambda t, name: F.layer_norm(t, (D,), g(name + ".weight"), g(name + ".bias"), 1e-5)

    def ffn(t, name):
        return F.linear(F.silu(F.linear(ln(t, name + ".layer_norm"), g(name + ".w_1.weight"), g(name + ".w_1.bias"))), g(name + ".w_2.weight"),
                        g(name + ".w_2.bias"))

    x = x + 0.5 * ffn(x, "ffn1")
    y = ln(x, "self_attn_layer_norm")
    heads = lambda t: t.view(B, S, H, D // H).transpose(1, 2)
    sa = "self_attn."
    q, k, v = (heads(F.linear(y, g(sa + n + ".weight"), g(sa + n + ".bias"))) for n in ("linear_q", "linear_k", "linear_v"))
    pos = F.linear(pe.to(x), g(sa + "linear_pos.weight")).view(2 * S - 1, H, D // H).transpose(0, 1)
    a = rel_attention(q, k, v, pos, g(sa + "pos_bias_u"), g(sa + "pos_bias_v"), lengths)
    x = x + F.linear(a.transpose(1, 2).reshape(B, S, D), g(sa + "linear_out.weight"), g(sa + "linear_out.bias"))
    cm = "conv_module."
    y = F.linear(ln(x, cm + "layer_norm"), g(cm + "pointwise_conv1.weight")[:, :, 0])
    y = glu_dwconv(y, g(cm + "depthwise_conv.weight"), g(cm + "batch_norm.weight"), g(cm + "batch_norm.bias"), g(cm + "batch_norm.running_mean"),
                   g(cm + "batch_norm.running_var"))
    x = x + F.linear(y, g(cm + "pointwise_conv2.weight")[:, :, 0])
    x = x + 0.5 * ffn(x, "ffn2")
    return ln(x, "final_layer_norm")


def subsample(feats, sd, n_conv=2):
    """Conv1dSubsampler (fairseq/models/speech_to_text/modules/convolution.py:13-57) on the whole padded batch -> [B, S, D]."""
    x = feats.transpose(1, 2)
    for i in range(n_conv):
        w = sd[f"subsample.conv_layers.{i}.weight"]
        x = F.glu(F.conv1d(x, w, sd[f"subsample.conv_layers.{i}.bias"], 2, w.shape[-1] // 2), dim=1)
    return x.transpose(1, 2)


def encode(sd, cfg, feats, lengths, dtype=torch.float64):
    """-> (encoder_out [B, S, D] batch-major in `dtype`, subsampled lengths).  Every row of the padded batch is computed; only the
    attention keys are masked."""
    sd = {k: v.to(feats.device, dtype) for k, v in sd.items()}
    D = cfg.embed_dim
    lens = subsampled_lengths(lengths, len(cfg.kernel_sizes))
    x = math.sqrt(D) * subsample(feats.to(dtype), sd, len(cfg.kernel_sizes))
    x = F.linear(x, sd["linear.weight"], sd["linear.bias"])
    pe = rel_pe(x.shape[1], D)
    for l in range(cfg.layers):
        x = conformer_layer(x, sd, f"conformer_layers.{l}.", cfg.heads, lens, pe)
    return x, lens
