#!/usr/bin/env python3
"""tests/golden/wav2vec_ctc.npz: the REAL reference classes -- ConvFeatureExtractionModel (mode "layer_norm", conv_bias True),
TransformerEncoder and TransformerSentenceEncoderLayer (layer_norm_first True, required_seq_len_multiple 2) compiled from their class
statements in fairseq/models/wav2vec/wav2vec2.py over the real Fp32LayerNorm, SamePad, TransposeLast and MultiheadAttention, through
tools/gen_golden_hubert.py's loader -- on the tiny configuration and seeded weights of tests/wav2vec_ref.py, on the CPU.
Wav2Vec2Model and Wav2VecEncoder sit in modules that import the dataclass / registry / task machinery, so their forward is COMPOSED
here over the real parts, under their attribute names: Wav2Vec2Model.forward(features_only=True, mask=False) (wav2vec2.py: feature
extractor, layer_norm, post_extract_proj, encoder) and Wav2VecEncoder.forward (wav2vec2_asr.py:473-501: proj behind it); the file
records that ("model_class").  load_state_dict(strict=True) pins the key names.  The float64 twin is the same modules cast to float64
with two exchanges: Fp32LayerNorm and fairseq's gelu compute in float32 whatever their input is, so nn.LayerNorm with the same
parameters and F.gelu stand in their places -- the same equations, in float64 throughout.
Each waveform is normalised (F.layer_norm over its own samples, asr_bleu/utils.py:240-244) and run ALONE.  Stored (arrays only): the
emissions in float64 and float32, the reference's own float32-vs-float64 error, the layer-k features of the reader path, the float64
frame arg-max with its top-2 margin, the collapsed token ids; and for a tiny Hugging Face Wav2Vec2ForCTC built FROM A CONFIG OBJECT
with seeded weights its state-dict key list, shapes and float64 logits for one waveform, which pin hf_to_fairseq_state_dict.
Run where the reference tree is present: python tools/gen_golden_wav2vec_ctc.py"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import gen_golden_hubert as GH  # noqa: E402
import wav2vec_ref as W  # noqa: E402

BARS = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 6e-2}  # ENGINE_TOL of tests/test_hip_nar_widths.py: the cap on near-tie frames is asserted for each


class W2VModel(nn.Module):
    """Wav2Vec2Model's inference submodules under its attribute names; forward(features_only=True, mask=False, layer=...)."""

    def __init__(self, ns, cfg):
        super().__init__()
        layers = eval(cfg.conv_feature_layers)
        self.feature_extractor = ns["ConvFeatureExtractionModel"](conv_layers=layers, dropout=0.0, mode=cfg.extractor_mode, conv_bias=cfg.conv_bias)
        self.post_extract_proj = nn.Linear(layers[-1][0], cfg.encoder_embed_dim) if layers[-1][0] != cfg.encoder_embed_dim else None
        self.mask_emb = nn.Parameter(torch.zeros(cfg.encoder_embed_dim))
        self.encoder = ns["TransformerEncoder"](cfg)
        self.layer_norm = ns["LayerNorm"](layers[-1][0])

    def extract_features(self, source, layer=None):
        features = self.layer_norm(self.feature_extractor(source).transpose(1, 2))
        if self.post_extract_proj is not None:
            features = self.post_extract_proj(features)
        return self.encoder(features, padding_mask=None, layer=layer)[0]


class W2VEncoder(nn.Module):
    def __init__(self, ns, cfg, vocab):
        super().__init__()
        self.w2v_model = W2VModel(ns, cfg)
        self.proj = nn.Linear(cfg.encoder_embed_dim, vocab)

    def forward(self, source):
        return self.proj(self.w2v_model.extract_features(source))


class Ctc(nn.Module):
    def __init__(self, ns, cfg, vocab):
        super().__init__()
        self.w2v_encoder = W2VEncoder(ns, cfg, vocab)


def build(ns, sd, dtype):
    m = Ctc(ns, GH.namespace_cfg(W.TINY), W.VOCAB)
    m.load_state_dict(sd, strict=True)
    m = m.eval()
    w2v = m.w2v_encoder.w2v_model
    assert w2v.encoder.layer_norm_first and w2v.encoder.required_seq_len_multiple == 2
    if dtype == torch.float64:
        for block in w2v.feature_extractor.conv_layers:
            old = block[2][1]
            assert type(old).__name__ == "Fp32LayerNorm"
            new = nn.LayerNorm(old.normalized_shape, eps=old.eps)
            new.load_state_dict(old.state_dict())
            block[2][1] = new
        for layer in w2v.encoder.layers:
            layer.activation_fn = F.gelu
    return m.to(dtype)


def hf_pin(out):
    """A tiny Wav2Vec2ForCTC from a config object (nothing is fetched): key list, shapes, float64 logits of golden wave 1."""
    from diffnorm_amd import asr

    Wav2Vec2Config, Wav2Vec2ForCTC = HF

    conv = W.conv_layers(W.TINY)
    cfg = Wav2Vec2Config(vocab_size=W.VOCAB, hidden_size=64, num_hidden_layers=3, num_attention_heads=4, intermediate_size=128, hidden_act="gelu",
                         hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0,
                         feat_extract_norm="layer", feat_extract_activation="gelu", conv_dim=[c for c, _, _ in conv], conv_kernel=[k for _, k, _ in conv],
                         conv_stride=[s for _, _, s in conv], conv_bias=True, num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4,
                         do_stable_layer_norm=True, apply_spec_augment=False, layer_norm_eps=1e-5)
    model = Wav2Vec2ForCTC(cfg).eval()
    keys = list(model.state_dict().keys())
    shapes = [tuple(v.shape) for v in model.state_dict().values()]
    sd = W.hf_weights(keys, shapes)
    model.load_state_dict(sd, strict=True)
    wave = W.golden_wave(1)
    with torch.no_grad():
        logits = model.double()(W.wave_norm(wave)[None]).logits[0]
    fs = asr.hf_to_fairseq_state_dict(sd, cfg)
    ns = asr.hf_config_namespace(cfg)
    mine = W.emissions(fs, ns, wave)
    d = (mine - logits).abs().max().item() / logits.abs().max().item()
    print(f"HF Wav2Vec2ForCTC ({len(keys)} keys): logits {tuple(logits.shape)}, key map + restatement vs HF {d:.3e}")
    assert d < 1e-9, "hf_to_fairseq_state_dict / wav2vec_ref disagree with transformers' Wav2Vec2ForCTC"
    out["hf_keys"], out["hf_logits"] = np.array(keys), logits.numpy()
    out["hf_shapes"] = np.array([",".join(str(v) for v in s) for s in shapes])


def main():
    global HF
    try:  # (before the reference loader puts its stand-in modules on the path)
        from transformers import Wav2Vec2Config, Wav2Vec2ForCTC

        HF = (Wav2Vec2Config, Wav2Vec2ForCTC)
    except Exception as e:  # noqa: BLE001
        HF = None
        print(f"transformers' Wav2Vec2ForCTC does not build here ({type(e).__name__}: {e}): the key map is pinned by names alone")
    ns, _ = GH.load_classes()
    sd = W.make_state_dict()
    m64, m32 = build(ns, sd, torch.float64), build(ns, sd, torch.float32)
    out = {"model_class": np.array("composition over the real ConvFeatureExtractionModel / TransformerEncoder"), "layers": np.array(W.GOLDEN_LAYERS),
           "samples": np.array([n for n, _ in W.GOLDEN_WAVES])}
    frames, worst, risky, total = [], 0.0, {k: 0 for k in BARS}, 0
    with torch.no_grad():
        for i in range(len(W.GOLDEN_WAVES)):
            wave = W.golden_wave(i)
            e64 = m64.w2v_encoder(W.wave_norm(wave, torch.float64)[None])[0]
            e32 = m32.w2v_encoder(W.wave_norm(wave, torch.float32)[None])[0]
            mine = W.emissions(sd, W.TINY, wave)
            scale = e64.abs().max().item()
            d, err32 = (mine - e64).abs().max().item() / scale, (e32.double() - e64).abs().max().item()
            assert d < 1e-9, "tests/wav2vec_ref.py disagrees with the reference"
            margin, ids = W.top2_margin(e64), W.ctc_greedy(e64)
            total += margin.numel()
            for k, tol in BARS.items():
                risky[k] += int((margin < 2 * tol * max(1.0, scale / 4)).sum())
            print(f"wave {i} ({wave.numel()} samples, dc {W.GOLDEN_WAVES[i][1]}): {tuple(e64.shape)}, scale {scale:.2f}, e_ref32 {err32:.3e}, restatement {d:.3e}, "
                  f"text {W.text(ids)!r}")
            out[f"em_w{i}"], out[f"em32_w{i}"], out[f"e_ref32_w{i}"] = e64.numpy(), e32.numpy(), np.float64(err32)
            out[f"argmax_w{i}"], out[f"margin_w{i}"], out[f"ids_w{i}"] = e64.argmax(-1).numpy(), margin.numpy(), np.array(ids, dtype=np.int64)
            for layer in W.GOLDEN_LAYERS:
                f64 = m64.w2v_encoder.w2v_model.extract_features(W.wave_norm(wave, torch.float64)[None], layer=layer - 1)[0]
                f32 = m32.w2v_encoder.w2v_model.extract_features(W.wave_norm(wave, torch.float32)[None], layer=layer - 1)[0]
                d = ((W.features(sd, W.TINY, wave, layer) - f64).abs().max() / f64.abs().max()).item()
                assert d < 1e-9, "tests/wav2vec_ref.py (layer features) disagrees with the reference"
                out[f"feat_w{i}_l{layer}"], out[f"e_ref32_w{i}_l{layer}"] = f64.numpy(), np.float64((f32.double() - f64).abs().max().item())
            frames.append(e64.shape[0])
            assert e64.shape[0] == W.out_frames(W.TINY, wave.numel())
            worst = max(worst, err32)
    assert any(f % 2 == 1 for f in frames), "one golden waveform must give an odd frame count"
    seen = set(np.concatenate([out[f"argmax_w{i}"] for i in range(len(W.GOLDEN_WAVES))]).tolist())
    assert 0 in seen and len(seen) >= 4, f"the golden frames must decode to the blank and to several letters, got rows {sorted(seen)}"
    print(f"frames under 2 x bar of {total}: {risky}")
    assert max(risky.values()) <= 0.1 * total, f"{risky} of {total} frames are near-ties: scale the seeded proj weights (HEAD_GAIN, HEAD_LEAD)"
    out["frames"], out["e_ref32"] = np.array(frames), np.float64(worst)
    if HF is not None:
        hf_pin(out)
    path = os.path.join(ROOT, "tests", "golden", "wav2vec_ctc.npz")
    with open(path, "wb") as fh:  # (np.savez through a file object: no timestamps, a re-run is byte-identical)
        np.savez_compressed(fh, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
