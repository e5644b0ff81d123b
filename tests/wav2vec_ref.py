"""TEST INFRASTRUCTURE ONLY.  The recogniser of the recipe's ASR-BLEU restated in plain torch from its equations
(research/TranSpeech/asr_bleu/utils.py:221-308: per-utterance F.layer_norm of the waveform, Wav2VecEncoder.forward in eval mode
(fairseq/models/wav2vec/wav2vec2_asr.py:473-501) over Wav2Vec2Model.extract_features, the Linear to the letters, best-path CTC
decoding and the post-processing strings), for the LARGE form: ConvFeatureExtractionModel in mode "layer_norm" with conv biases
(fairseq/models/wav2vec/wav2vec2.py:849-859), TransformerEncoder with layer_norm_first True (:1001-1076) and pre-norm
TransformerSentenceEncoderLayers (:1235-1257); ONE utterance at a time, parametrised by dtype; a tiny configuration and seeded
formula weights under the fairseq Wav2VecCtc state-dict names.  tools/gen_golden_wav2vec_ctc.py checks this file against the real
classes and writes tests/golden/wav2vec_ctc.npz.  What it shares with the base form comes from tests/hubert_ref.py."""
import types

import torch
import torch.nn.functional as F

import hubert_ref as R

_COMMON = dict(extractor_mode="layer_norm", conv_bias=True, layer_norm_first=True, layer_type="transformer", required_seq_len_multiple=2,
               activation_fn="gelu", normalize=True)
TINY = types.SimpleNamespace(conv_feature_layers="[(64,10,5)] + [(64,3,2)] * 4 + [(64,2,2)] * 2", encoder_embed_dim=64, encoder_ffn_embed_dim=128,
                             encoder_layers=3, encoder_attention_heads=4, conv_pos=8, conv_pos_groups=4, **_COMMON)
RECIPE2 = types.SimpleNamespace(conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", encoder_embed_dim=1024,
                                encoder_ffn_embed_dim=4096, encoder_layers=2, encoder_attention_heads=16, conv_pos=128, conv_pos_groups=16,
                                **_COMMON)  # the large recognisers' widths, two layers
VOCAB = 32
LETTERS = list("|etaonihsrdlucmwfgypbvk'xjqz")  # dict.ltr.txt's order: 28 letters behind the four specials = 32 tokens
TOKENS = ["<s>", "<pad>", "</s>", "<unk>"] + LETTERS
SIL_TOKENS = list(TOKENS)  # a vocabulary in another order (the Hugging Face ones have their own): `|` on a row that wins golden frames
SIL_TOKENS[4], SIL_TOKENS[12] = SIL_TOKENS[12], SIL_TOKENS[4]
TINY_SEED = 40231
HEAD_GAIN, HEAD_LEAD, HEAD_LEAD_ROWS = 6.0, 3.0, (0, 4, 23)  # the seeded proj weights times 6; the rows of the blank, of `|` and of one letter
# times 3 more, so that the golden frames decode to blanks between and beside letters (a trained CTC head is mostly blank) and few frames
# are near-ties (the generator asserts the 10 % cap for every engine bar).  `|` itself wins no golden frame: SIL_TOKENS covers it
GOLDEN_WAVES = ((3000, 0.0), (1999, 0.0), (2650, 25.0))  # (samples, DC offset); 3000 samples give 9 frames: odd under the multiple of 2
GOLDEN_LAYERS = (2, 3)
W2V, PROJ = "w2v_encoder.w2v_model.", "w2v_encoder.proj."
conv_layers, out_frames, _normal = R.conv_layers, R.out_frames, R._normal


def golden_wave(i):
    n, dc = GOLDEN_WAVES[i]
    return R.make_wave(n, 500 + i, dc=dc)


def make_state_dict(cfg=TINY, seed=TINY_SEED, vocab=VOCAB, head_gain=HEAD_GAIN):
    """Wav2VecCtc.state_dict() names (w2v_encoder.w2v_model.* of a Wav2Vec2Model without its quantiser, w2v_encoder.proj.*), fp32."""
    layers = conv_layers(cfg)
    Cw, D = layers[0][0], cfg.encoder_embed_dim
    base = types.SimpleNamespace(**dict(vars(cfg), extractor_mode="default"))
    sd = {k: v for k, v in R.make_state_dict(base, seed).items() if not k.startswith(("final_proj", "feature_extractor.conv_layers.0.2."))}
    for i in range(len(layers)):
        p = f"feature_extractor.conv_layers.{i}."
        if cfg.conv_bias:
            sd[p + "0.bias"] = _normal(seed, f"conv{i}.b", (Cw,), 0.2)
        sd[p + "2.1.weight"] = 1.0 + _normal(seed, f"conv{i}.ln.w", (Cw,), 0.1)
        sd[p + "2.1.bias"] = _normal(seed, f"conv{i}.ln.b", (Cw,), 0.1)
    out = {W2V + k: v for k, v in sd.items()}
    out[PROJ + "weight"] = _normal(seed, "proj.w", (vocab, D), head_gain * D ** -0.5)
    out[PROJ + "weight"][list(HEAD_LEAD_ROWS)] *= HEAD_LEAD
    out[PROJ + "bias"] = _normal(seed, "proj.b", (vocab,), 0.1)
    return out


def wave_norm(wave, dtype=torch.float64):
    """F.layer_norm(wave, wave.shape) (utils.py:240-244): biased variance, eps 1e-5."""
    w = wave.to(dtype)
    return F.layer_norm(w, w.shape)


def conv_features(sd, cfg, wave, dtype=torch.float64):
    """ConvFeatureExtractionModel in mode "layer_norm" on one waveform [n] -> [T, C]: Conv1d (+ bias) -> LayerNorm over C -> GELU."""
    g = lambda k: sd[W2V + k].to(dtype)
    x = wave.to(dtype).view(1, 1, -1)
    for i, (Cw, k, s) in enumerate(conv_layers(cfg)):
        p = f"feature_extractor.conv_layers.{i}."
        x = F.conv1d(x, g(p + "0.weight"), g(p + "0.bias") if cfg.conv_bias else None, s)
        x = F.layer_norm(x.transpose(1, 2), (Cw,), g(p + "2.1.weight"), g(p + "2.1.bias"), 1e-5).transpose(1, 2)
        x = F.gelu(x)
    return x[0].t()


def encoder_layer(x, sd, p, H):
    """One pre-norm TransformerSentenceEncoderLayer on x [T, D], no mask."""
    T, D = x.shape
    g = lambda k: sd[p + k].to(x.dtype)
    lin = lambda t, name: F.linear(t, g(name + ".weight"), g(name + ".bias"))
    ln = lambda t, name: F.layer_norm(t, (D,), g(name + ".weight"), g(name + ".bias"), 1e-5)
    heads = lambda t: t.view(T, H, D // H).transpose(0, 1)
    y = ln(x, "self_attn_layer_norm")
    q, k, v = heads(lin(y, "self_attn.q_proj") * (D // H) ** -0.5), heads(lin(y, "self_attn.k_proj")), heads(lin(y, "self_attn.v_proj"))
    a = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(1, 2)), -1), v).transpose(0, 1).reshape(T, D)
    x = x + lin(a, "self_attn.out_proj")
    return x + lin(F.gelu(lin(ln(x, "final_layer_norm"), "fc1")), "fc2")


def features(sd, cfg, wave, layer=None, dtype=torch.float64):
    """layer k: HubertModel / Wav2Vec2Model.extract_features(..., output_layer / layer = k - 1): the stream behind layer k, WITHOUT
    encoder.layer_norm.  layer None: every layer, then encoder.layer_norm (TransformerEncoder.forward, layer None).  required_seq_len_multiple
    appends masked frames that are cut off again: nothing to restate."""
    g = lambda k: sd[W2V + k].to(dtype)
    x = conv_features(sd, cfg, wave_norm(wave, dtype) if cfg.normalize else wave, dtype)
    x = F.layer_norm(x, (x.shape[1],), g("layer_norm.weight"), g("layer_norm.bias"), 1e-5)
    if W2V + "post_extract_proj.weight" in sd:
        x = F.linear(x, g("post_extract_proj.weight"), g("post_extract_proj.bias"))
    p = W2V + "encoder.pos_conv.0."  # (either spelling of the weight-norm: weight_g / weight_v, or the parametrization's originals)
    gv = [sd[p + n] for n in ("weight_g", "weight_v")] if p + "weight_g" in sd else [sd[p + f"parametrizations.weight.original{j}"] for j in (0, 1)]
    x = x + R.pos_conv({"encoder.pos_conv.0.weight_g": gv[0], "encoder.pos_conv.0.weight_v": gv[1], "encoder.pos_conv.0.bias": sd[p + "bias"]}, cfg, x)
    for l in range(cfg.encoder_layers if layer is None else layer):
        x = encoder_layer(x, sd, f"{W2V}encoder.layers.{l}.", cfg.encoder_attention_heads)
    if layer is None:
        x = F.layer_norm(x, (x.shape[1],), g("encoder.layer_norm.weight"), g("encoder.layer_norm.bias"), 1e-5)
    return x


def emissions(sd, cfg, wave, dtype=torch.float64):
    """Wav2VecEncoder.forward(...)["encoder_out"] of one utterance: [T, V]."""
    return F.linear(features(sd, cfg, wave, None, dtype), sd[PROJ + "weight"].to(dtype), sd[PROJ + "bias"].to(dtype))


def ctc_greedy(em, blank=0):
    """Best path: the frame arg-max (the first maximum), repeats merged, blanks dropped -> a list of token ids."""
    out, prev = [], -1
    for row in torch.as_tensor(em).tolist():
        tok = max(range(len(row)), key=lambda v: (row[v], -v))
        if tok != blank and tok != prev:
            out.append(tok)
        prev = tok
    return out


def top2_margin(em):
    two = torch.topk(torch.as_tensor(em), 2, dim=-1).values
    return two[..., 0] - two[..., 1]


def text(ids, tokens=TOKENS, mode="collapse"):
    """post_process_fn + strip + lower (utils.py:79-88, 308)."""
    sil = "|" if "|" in tokens else tokens[2]
    hypo = [tokens[i] for i in ids]
    return ("".join(hypo) if mode == "collapse" else " ".join(hypo)).replace(sil, " ").strip().lower()


def hf_weights(keys, shapes, seed=TINY_SEED):
    """Seeded values for a Hugging Face Wav2Vec2ForCTC state dict by key name: norm weights round 1, weight_g positive, the rest
    N(0, fan_in^-1/2) (biases 0.1), lm_head with HEAD_GAIN."""
    sd = {}
    for k, shape in zip(keys, shapes):
        shape = tuple(int(v) for v in shape)
        fan = 1
        for v in shape[1:]:
            fan *= v
        if "layer_norm.weight" in k:
            sd[k] = 1.0 + _normal(seed, k, shape, 0.1)
        elif k.endswith(("weight_g", "original0")):
            sd[k] = 1.0 + _normal(seed, k, shape, 0.2).abs()
        elif k.endswith("bias") or len(shape) == 1:
            sd[k] = _normal(seed, k, shape, 0.1)
        else:
            sd[k] = _normal(seed, k, shape, (HEAD_GAIN if k.startswith("lm_head") else 1.3) * fan ** -0.5)
    return sd
