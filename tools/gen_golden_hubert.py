#!/usr/bin/env python3
"""tests/golden/hubert.npz: the REAL reference classes -- ConvFeatureExtractionModel, make_conv_pos, TransformerEncoder and
TransformerSentenceEncoderLayer compiled from their statements in fairseq/models/wav2vec/wav2vec2.py over the real Fp32GroupNorm,
SamePad, TransposeLast, LayerNorm, MultiheadAttention and init_bert_params, and HubertModel compiled from its class statement in
fairseq/models/hubert/hubert.py over a namespace config (the modules around both import the dataclass / registry machinery; when
the HubertModel statement does not compile here its forward(features_only=True) composition is run over the real parts instead, and
the file says which) -- on the tiny configuration and seeded weights of tests/hubert_ref.py, on the CPU.
load_state_dict(strict=True) pins the key names.  The float32 model is the classes as they lie.  The float64 model is the same
modules cast to float64 with TWO exchanges: Fp32GroupNorm and fairseq's gelu (the layers' activation_fn) compute in float32 whatever
their input is, so the float64 run uses nn.GroupNorm with the same parameters and F.gelu in their places -- the same equations, in
float64 throughout.
Stored (arrays only): per waveform (run ALONE, as the reader does) and output layer the features in float64 and float32, the
reference's own float32-vs-float64 max error, the frame counts, and the units of a seeded 50-centroid table on the last layer's
float64 features with their top-2 distance margins.  Run where the reference tree is present: python tools/gen_golden_hubert.py"""
import ast
import logging
import math
import os
import sys
import types
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import hubert_ref as R  # noqa: E402
import ref_loader  # noqa: E402


def _statements(rel, names):
    path = os.path.join(ref_loader.REF, rel)
    body = [n for n in ast.parse(open(path).read()).body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(body) == len(names), (rel, names)
    for n in body:  # the registry decorator of a model class is not on the path
        n.decorator_list = []
    return path, body


def load_classes():
    """-> (namespace of the wav2vec2.py classes, HubertModel or None)."""
    ref_loader.load_reference_nar()
    mods = sys.modules["fairseq.modules"]
    utils = sys.modules["fairseq.utils"]
    gn = ref_loader._load("fairseq.modules.fp32_group_norm", "fairseq/modules/fp32_group_norm.py")
    sp = ref_loader._load("fairseq.modules.same_pad", "fairseq/modules/same_pad.py")
    tl = ref_loader._load("fairseq.modules.transpose_last", "fairseq/modules/transpose_last.py")
    ln = sys.modules["fairseq.modules.layer_norm"]
    path, body = _statements("fairseq/modules/transformer_sentence_encoder.py", ["init_bert_params"])
    ns_init = {"nn": nn, "torch": torch, "MultiheadAttention": mods.MultiheadAttention}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns_init)
    path, body = _statements("fairseq/models/wav2vec/utils.py", ["pad_to_multiple"])
    ns_pad = {"math": math, "F": F, "torch": torch}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns_pad)
    ns = {"nn": nn, "torch": torch, "F": F, "np": np, "math": math, "List": List, "Tuple": Tuple, "utils": utils, "Wav2Vec2Config": object,
          "Fp32GroupNorm": gn.Fp32GroupNorm, "Fp32LayerNorm": ln.Fp32LayerNorm, "TransposeLast": tl.TransposeLast, "SamePad": sp.SamePad,
          "LayerNorm": ln.LayerNorm, "MultiheadAttention": mods.MultiheadAttention, "init_bert_params": ns_init["init_bert_params"],
          "index_put": utils.index_put, "pad_to_multiple": ns_pad["pad_to_multiple"], "fsdp_wrap": lambda m, **k: m,
          "checkpoint_wrapper": lambda m, **k: m, "ConformerWav2Vec2EncoderLayer": None, "__name__": "fairseq.models.wav2vec.wav2vec2"}
    path, body = _statements("fairseq/models/wav2vec/wav2vec2.py",
                             ["ConvFeatureExtractionModel", "make_conv_pos", "TransformerEncoder", "TransformerSentenceEncoderLayer"])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    hub = None
    try:
        class BaseFairseqModel(nn.Module):
            def upgrade_state_dict_named(self, state_dict, name):
                pass

        hns = {"nn": nn, "torch": torch, "np": np, "Dict": Dict, "List": List, "Optional": Optional, "Tuple": Tuple, "BaseFairseqModel": BaseFairseqModel,
               "HubertConfig": object, "HubertPretrainingConfig": object, "HubertPretrainingTask": object, "Dictionary": object,
               "ConvFeatureExtractionModel": ns["ConvFeatureExtractionModel"], "TransformerEncoder": ns["TransformerEncoder"],
               "LayerNorm": ln.LayerNorm, "GradMultiply": None, "compute_mask_indices": None, "logger": logging.getLogger("hubert"),
               "__name__": "fairseq.models.hubert.hubert"}
        path, body = _statements("fairseq/models/hubert/hubert.py", ["HubertModel"])
        exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), hns)
        hub = hns["HubertModel"]
    except Exception as e:  # noqa: BLE001
        print("HubertModel's class statement did not compile (%s: %s): using its forward(features_only=True) composition" % (type(e).__name__, e))
    return ns, hub


def namespace_cfg(c):
    return types.SimpleNamespace(
        conv_feature_layers=c.conv_feature_layers, extractor_mode=c.extractor_mode, conv_bias=c.conv_bias, label_rate=50,
        encoder_embed_dim=c.encoder_embed_dim, encoder_ffn_embed_dim=c.encoder_ffn_embed_dim, encoder_layers=c.encoder_layers,
        encoder_attention_heads=c.encoder_attention_heads, conv_pos=c.conv_pos, conv_pos_groups=c.conv_pos_groups, layer_norm_first=c.layer_norm_first,
        layer_type=c.layer_type, required_seq_len_multiple=c.required_seq_len_multiple, activation_fn=c.activation_fn, dropout=0.1,
        attention_dropout=0.1, activation_dropout=0.0, encoder_layerdrop=0.0, checkpoint_activations=False, dropout_input=0.1, dropout_features=0.1,
        mask_prob=0.8, mask_selection="static", mask_other=0, mask_length=10, no_mask_overlap=False, mask_min_space=1, mask_channel_prob=0.0,
        mask_channel_selection="static", mask_channel_other=0, mask_channel_length=10, no_mask_channel_overlap=False, mask_channel_min_space=1,
        feature_grad_mult=1.0, logit_temp=0.1, skip_masked=False, skip_nomask=False, final_dim=0, target_glu=False, untie_final_proj=False)


class Composition(nn.Module):
    """HubertModel's submodules under its attribute names and its forward(features_only=True, mask=False) (hubert.py:439-476)."""

    def __init__(self, ns, cfg):
        super().__init__()
        layers = eval(cfg.conv_feature_layers)
        self.feature_extractor = ns["ConvFeatureExtractionModel"](conv_layers=layers, dropout=0.0, mode=cfg.extractor_mode, conv_bias=cfg.conv_bias)
        self.post_extract_proj = nn.Linear(layers[-1][0], cfg.encoder_embed_dim) if layers[-1][0] != cfg.encoder_embed_dim else None
        self.mask_emb = nn.Parameter(torch.zeros(cfg.encoder_embed_dim))
        self.encoder = ns["TransformerEncoder"](cfg)
        self.layer_norm = ns["LayerNorm"](layers[-1][0])
        self.final_proj = nn.Linear(cfg.encoder_embed_dim, cfg.encoder_embed_dim)

    def extract_features(self, source, padding_mask=None, mask=False, output_layer=None):
        features = self.layer_norm(self.feature_extractor(source).transpose(1, 2))
        if self.post_extract_proj is not None:
            features = self.post_extract_proj(features)
        x, _ = self.encoder(features, padding_mask=padding_mask, layer=None if output_layer is None else output_layer - 1)
        return x, padding_mask


def build(ns, hub, sd, dtype):
    cfg = namespace_cfg(R.TINY)
    m = hub(cfg, types.SimpleNamespace(sample_rate=16000), [None]) if hub is not None else Composition(ns, cfg)
    m.load_state_dict(sd, strict=True)
    m = m.eval()
    if dtype == torch.float64:
        old = m.feature_extractor.conv_layers[0][2]
        new = nn.GroupNorm(old.num_groups, old.num_channels, eps=old.eps, affine=True)
        new.load_state_dict(old.state_dict())
        m.feature_extractor.conv_layers[0][2] = new
        for layer in m.encoder.layers:  # fairseq.modules.gelu.gelu is F.gelu(x.float()).type_as(x): the same exchange
            layer.activation_fn = F.gelu
    return m.to(dtype)


def main():
    ns, hub = load_classes()
    sd = R.make_state_dict(R.TINY, R.TINY_SEED)
    m64, m32 = build(ns, hub, sd, torch.float64), build(ns, hub, sd, torch.float32)
    out = {"lengths": np.array(R.GOLDEN_LENGTHS), "layers": np.array(R.GOLDEN_LAYERS), "model_class": np.array(type(m64).__name__)}
    frames, worst = [], 0.0
    with torch.no_grad():
        for i, n in enumerate(R.GOLDEN_LENGTHS):
            wave = R.make_wave(n, 100 + i)
            for layer in R.GOLDEN_LAYERS:
                f64 = m64.extract_features(source=wave.double()[None], padding_mask=None, mask=False, output_layer=layer)[0][0]
                f32 = m32.extract_features(source=wave[None], padding_mask=None, mask=False, output_layer=layer)[0][0]
                mine = R.extract_features(sd, R.TINY, wave, layer, torch.float64)
                d = (mine - f64).abs().max().item() / f64.abs().max().item()
                e32 = (f32.double() - f64).abs().max().item()
                print(f"wave {i} ({n} samples) layer {layer}: {tuple(f64.shape)}, scale {f64.abs().max().item():.3f}, e_ref32 {e32:.3e}, restatement {d:.3e}")
                assert d < 1e-9, "tests/hubert_ref.py disagrees with the reference"
                out[f"feat_w{i}_l{layer}"], out[f"feat32_w{i}_l{layer}"], out[f"e_ref32_w{i}_l{layer}"] = f64.numpy(), f32.numpy(), np.float64(e32)
                worst = max(worst, e32)
            frames.append(f64.shape[0])
            assert f64.shape[0] == R.out_frames(R.TINY, n)
        out["frames"], out["e_ref32"] = np.array(frames), np.float64(worst)
        centers = R.make_centers(R.KM_CENTROIDS, R.TINY.encoder_embed_dim, R.KM_SEED, 0.6)
        feats = torch.cat([torch.from_numpy(out[f"feat_w{i}_l{R.GOLDEN_LAYERS[-1]}"]) for i in range(len(R.GOLDEN_LENGTHS))])
        units, margin = R.kmeans_units(feats, centers)
        out["centers"], out["units"], out["margins"] = centers.numpy(), units.numpy(), margin.numpy()
        print(f"{units.numel()} units over {len(set(units.tolist()))} centroids, smallest margin {margin.min().item():.3e}")
    path = os.path.join(ROOT, "tests", "golden", "hubert.npz")
    with open(path, "wb") as fh:  # (np.savez through a file object: no timestamps, a re-run is byte-identical)
        np.savez_compressed(fh, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
