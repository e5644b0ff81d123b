"""TEST INFRASTRUCTURE ONLY.  The HuBERT feature reader's forward restated in plain torch from its equations
(HubertModel.forward with features_only, fairseq/models/hubert/hubert.py:429-476; ConvFeatureExtractionModel, fairseq/models/wav2vec/
wav2vec2.py:819-896; make_conv_pos + SamePad, :899-915; TransformerEncoder.extract_features, :1009-1076;
TransformerSentenceEncoderLayer.forward with layer_norm_first False, :1258-1283; MultiheadAttention's scaled q), eval mode, ONE
utterance at a time as the reader runs it (examples/textless_nlp/gslm/speech2unit/pretrained/hubert_feature_reader.py:44-64),
parametrised by dtype; a tiny configuration; seeded formula weights under the reference's state-dict names; and the k-means
assignment (examples/hubert/simple_kmeans/dump_km_label.py:38-53).  tools/gen_golden_hubert.py checks this file against the real
classes and writes tests/golden/hubert.npz."""
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

_COMMON = dict(extractor_mode="default", conv_bias=False, layer_norm_first=False, layer_type="transformer", required_seq_len_multiple=1,
               activation_fn="gelu", normalize=False)
TINY = types.SimpleNamespace(conv_feature_layers="[(64,10,5)] + [(64,3,2)] * 4 + [(64,2,2)] * 2", encoder_embed_dim=64, encoder_ffn_embed_dim=128,
                             encoder_layers=3, encoder_attention_heads=4, conv_pos=8, conv_pos_groups=4, **_COMMON)
RECIPE2 = types.SimpleNamespace(conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", encoder_embed_dim=768,
                                encoder_ffn_embed_dim=3072, encoder_layers=2, encoder_attention_heads=12, conv_pos=128, conv_pos_groups=16,
                                **_COMMON)  # the recipe's widths (mHuBERT base), two layers
TINY_SEED = 31170
GOLDEN_LENGTHS = (3000, 1999, 731)
GOLDEN_LAYERS = (2, 3)
KM_SEED, KM_CENTROIDS = 515, 50


def conv_layers(cfg):
    spec = cfg.conv_feature_layers
    return [tuple(cl) for cl in (eval(spec) if isinstance(spec, str) else spec)]


def _normal(seed, name, shape, scale):
    """Seeded N(0, scale^2) values, one legacy MT19937 stream per tensor name (stable across numpy / torch versions)."""
    rs = np.random.RandomState((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
    return torch.from_numpy(rs.standard_normal(size=shape) * scale).float()


def make_state_dict(cfg=TINY, seed=TINY_SEED):
    """HubertModel.state_dict() names (no label dictionaries: mask_emb and final_proj are the only pre-training leftovers), fp32,
    O(1) activations, non-trivial norms and a non-trivial weight-norm gain."""
    layers = conv_layers(cfg)
    Cw, D, Fd, G, kp = layers[0][0], cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.conv_pos_groups, cfg.conv_pos
    sd = {}
    n = lambda name, shape, scale: _normal(seed, name, shape, scale)

    def lin(name, out, inp, gain=1.0):
        sd[name + ".weight"] = n(name + ".weight", (out, inp), gain * inp ** -0.5)
        sd[name + ".bias"] = n(name + ".bias", (out,), 0.1)

    def norm(name, width):
        sd[name + ".weight"] = 1.0 + n(name + ".weight", (width,), 0.1)
        sd[name + ".bias"] = n(name + ".bias", (width,), 0.1)

    for i, (_, k, _) in enumerate(layers):
        cin = 1 if i == 0 else Cw
        sd[f"feature_extractor.conv_layers.{i}.0.weight"] = n(f"conv{i}.w", (Cw, cin, k), 1.6 * (cin * k) ** -0.5)
    norm("feature_extractor.conv_layers.0.2", Cw)
    norm("layer_norm", Cw)
    if Cw != D:  # (HubertModel has no post_extract_proj when the widths agree, hubert.py:264-268)
        lin("post_extract_proj", D, Cw)
    sd["encoder.pos_conv.0.weight_g"] = 1.0 + n("pos.g", (1, 1, kp), 0.2).abs()
    sd["encoder.pos_conv.0.weight_v"] = n("pos.v", (D, D // G, kp), (kp * D // G) ** -0.5)
    sd["encoder.pos_conv.0.bias"] = n("pos.b", (D,), 0.1)
    norm("encoder.layer_norm", D)
    for l in range(cfg.encoder_layers):
        p = f"encoder.layers.{l}."
        for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(p + "self_attn." + proj, D, D, gain=1.5 if proj in ("q_proj", "k_proj") else 1.0)
        norm(p + "self_attn_layer_norm", D)
        lin(p + "fc1", Fd, D)
        lin(p + "fc2", D, Fd)
        norm(p + "final_layer_norm", D)
    sd["mask_emb"] = n("mask_emb", (D,), 1.0)
    lin("final_proj", D, D)
    return sd


def make_wave(n, seed, dc=0.0, amp=0.3):
    """A seeded waveform: noise plus two slow tones, `amp` in scale, on a DC offset."""
    t = torch.arange(n, dtype=torch.float64)
    w = _normal(seed, "wave", (n,), 1.0).double() * 0.5 + torch.sin(t * 0.031) + 0.5 * torch.sin(t * 0.0047 + 1.0)
    return (dc + amp * w).float()


def out_frames(cfg, L):
    for _, k, s in conv_layers(cfg):
        L = (L - k) // s + 1 if L >= k else 0
    return L


def pos_conv_weight(sd):
    g, v = sd["encoder.pos_conv.0.weight_g"].double(), sd["encoder.pos_conv.0.weight_v"].double()
    return g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()  # weight_norm(dim=2)


def conv_features(sd, cfg, wave, dtype=torch.float64):
    """ConvFeatureExtractionModel on one waveform [n] -> [T, C] (channels last), GroupNorm(C, C) behind the first conv."""
    g = lambda k: sd[k].to(dtype)
    x = wave.to(dtype).view(1, 1, -1)
    for i, (Cw, k, s) in enumerate(conv_layers(cfg)):
        x = F.conv1d(x, g(f"feature_extractor.conv_layers.{i}.0.weight"), None, s)
        if i == 0:
            x = F.group_norm(x, Cw, g("feature_extractor.conv_layers.0.2.weight"), g("feature_extractor.conv_layers.0.2.bias"), 1e-5)
        x = F.gelu(x)
    return x[0].t()


def pos_conv(sd, cfg, x):
    """x [T, D] -> gelu(SamePad(Conv1d(D, D, k, padding k / 2, groups)(x))) [T, D]."""
    k = cfg.conv_pos
    y = F.conv1d(x.t()[None], pos_conv_weight(sd).to(x.dtype), sd["encoder.pos_conv.0.bias"].to(x.dtype), 1, k // 2, 1, cfg.conv_pos_groups)
    if k % 2 == 0:
        y = y[:, :, :-1]
    return F.gelu(y)[0].t()


def encoder_layer(x, sd, p, H):
    """One post-norm TransformerSentenceEncoderLayer on x [T, D], no mask."""
    T, D = x.shape
    g = lambda k: sd[p + k].to(x.dtype)
    lin = lambda t, name: F.linear(t, g(name + ".weight"), g(name + ".bias"))
    ln = lambda t, name: F.layer_norm(t, (D,), g(name + ".weight"), g(name + ".bias"), 1e-5)
    heads = lambda t: t.view(T, H, D // H).transpose(0, 1)
    q, k, v = heads(lin(x, "self_attn.q_proj") * (D // H) ** -0.5), heads(lin(x, "self_attn.k_proj")), heads(lin(x, "self_attn.v_proj"))
    a = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(1, 2)), -1), v).transpose(0, 1).reshape(T, D)
    x = ln(x + lin(a, "self_attn.out_proj"), "self_attn_layer_norm")
    return ln(x + lin(F.gelu(lin(x, "fc1")), "fc2"), "final_layer_norm")


def extract_features(sd, cfg, wave, layer, dtype=torch.float64):
    """HubertModel.extract_features(wave[None], padding_mask=None, mask=False, output_layer=layer)[0][0]: [T, D] in `dtype`."""
    g = lambda k: sd[k].to(dtype)
    x = conv_features(sd, cfg, wave, dtype)
    x = F.layer_norm(x, (x.shape[1],), g("layer_norm.weight"), g("layer_norm.bias"), 1e-5)
    if "post_extract_proj.weight" in sd:
        x = F.linear(x, g("post_extract_proj.weight"), g("post_extract_proj.bias"))
    x = x + pos_conv(sd, cfg, x)
    x = F.layer_norm(x, (x.shape[1],), g("encoder.layer_norm.weight"), g("encoder.layer_norm.bias"), 1e-5)
    for l in range(layer):
        x = encoder_layer(x, sd, f"encoder.layers.{l}.", cfg.encoder_attention_heads)
    return x


def read_feats(sd, cfg, wave, layer, max_chunk, dtype=torch.float64):
    """The reader's chunk loop (hubert_feature_reader.py:51-64)."""
    return torch.cat([extract_features(sd, cfg, wave[s: s + max_chunk], layer, dtype) for s in range(0, wave.numel(), max_chunk)], 0)


def kmeans_distances(x, centers):
    """|x|^2 - 2 x . c + |c|^2 in float64 (dump_km_label.py:38-53): [M, n]."""
    x, c = torch.as_tensor(x).double(), torch.as_tensor(centers).double()
    return x.pow(2).sum(1, keepdim=True) - 2 * x @ c.t() + c.pow(2).sum(1)[None]


def kmeans_units(x, centers):
    """-> (units int64 [M], the top-2 margin of the distances relative to their scale [M])."""
    d = kmeans_distances(x, centers)
    two = torch.topk(d, 2, dim=1, largest=False).values
    return d.argmin(1), (two[:, 1] - two[:, 0]) / d.abs().max(1).values


def make_centers(n, D, seed, scale=1.0):
    return _normal(seed, "centers", (n, D), scale)


def kmeans_near_tie_case(M, n=1000, D=768, seed=77):
    """Inputs on which the unit IS a close decision: centroids of clearly different norms (scales 0.5 .. 1.5) round a common mean of
    about 3 per dimension (as features have one: the products x . c are then far larger than the distances), and every row a point
    beside the bisector of two of them, x = (c_a + c_b) / 2 + t (c_a - c_b), |t| log-uniform in [2.5e-4, 5e-3] and of either sign, so
    that the float64 top-2 margins spread over about 1e-4 .. 1e-2 of the distance scale.  A score without the -|c|^2 / 2 term, or one
    from bf16-rounded operands, gets a visible share of these rows wrong (asserted in tests/test_hubert_host.py).
    -> (x fp32 [M, D], centers fp32 [n, D])."""
    rs = np.random.RandomState(seed * 1009 + M)
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, size=(n, 1)))
    c = (_normal(seed, "centers", (n, D), 1.0).double() * scale + 3.0 * _normal(seed, "mean", (1, D), 1.0).double()).float()
    a = torch.from_numpy(rs.randint(0, n, size=M))
    b = (a + 1 + torch.from_numpy(rs.randint(0, n - 1, size=M))) % n
    t = torch.from_numpy(np.exp(rs.uniform(np.log(2.5e-4), np.log(5e-3), size=(M, 1))) * rs.choice([-1.0, 1.0], size=(M, 1)))
    x = 0.5 * (c[a] + c[b]).double() + t * (c[a] - c[b]).double()
    return x.float(), c
