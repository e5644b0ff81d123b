"""Host-side checks of the wav2vec 2.0 CTC recogniser (no GPU): the plain-torch restatement against the golden of the real classes,
the configuration checks, the packed table's shapes, the Hugging Face key map and the post-processing strings."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wav2vec_ref as W  # noqa: E402

from diffnorm_amd import _lib, asr, hubert  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return W.make_state_dict()


def test_restatement_equals_the_golden_of_the_real_classes(golden, sd):
    G = golden("wav2vec_ctc")
    assert any(int(f) % 2 == 1 for f in G["frames"])  # an odd frame count under required_seq_len_multiple 2
    for i in range(len(W.GOLDEN_WAVES)):
        wave = W.golden_wave(i)
        em = W.emissions(sd, W.TINY, wave)
        want = torch.from_numpy(G[f"em_w{i}"])
        assert em.shape == want.shape and float((em - want).abs().max()) <= 1e-9 * float(want.abs().max())
        assert W.ctc_greedy(em) == G[f"ids_w{i}"].tolist() and em.argmax(-1).tolist() == G[f"argmax_w{i}"].tolist()
        for layer in W.GOLDEN_LAYERS:  # the reader path: no encoder.layer_norm, not even behind the last layer
            f = W.features(sd, W.TINY, wave, layer)
            assert float((f - torch.from_numpy(G[f"feat_w{i}_l{layer}"])).abs().max()) <= 1e-9 * float(f.abs().max())
        e32 = float((W.emissions(sd, W.TINY, wave, torch.float32).double() - want).abs().max())
        assert e32 <= 8 * float(G[f"e_ref32_w{i}"]) + 1e-5


def test_the_normaliser_matters_on_the_golden_wave_with_a_dc_offset(sd):
    raw = types.SimpleNamespace(**dict(vars(W.TINY), normalize=False))
    wave = W.golden_wave(2)
    assert float((W.emissions(sd, raw, wave) - W.emissions(sd, W.TINY, wave)).abs().max()) > 1.0


def test_the_large_form_is_accepted_as_a_whole():
    """extractor_mode 'layer_norm' with layer_norm_first; conv_bias, normalize and the sequence multiple are free inside it."""
    for cfg in (W.TINY, W.RECIPE2, hubert.WAV2VEC2_LARGE, hubert.HUBERT_LARGE):
        hubert.check_hubert_args(cfg)
        for field, value in (("conv_bias", not cfg.conv_bias), ("normalize", False), ("required_seq_len_multiple", 1), ("required_seq_len_multiple", 4)):
            hubert.check_hubert_args(types.SimpleNamespace(**dict(vars(cfg), **{field: value})))


@pytest.mark.parametrize("field,value", [("extractor_mode", "default"), ("layer_norm_first", False)])
def test_half_a_large_form_is_refused(field, value):
    with pytest.raises(ValueError, match="go together"):
        hubert.check_hubert_args(types.SimpleNamespace(**dict(vars(W.TINY), **{field: value})))


@pytest.mark.parametrize("field,value", [("layer_type", "conformer"), ("pos_conv_depth", 2), ("training", True), ("mask", True), ("activation_fn", "relu"),
                                         ("extractor_mode", "group"), ("required_seq_len_multiple", 0),
                                         ("conv_feature_layers", "[(1024,10,5)] + [(1024,3,2)] * 2")])
def test_the_other_refusals_stay(field, value):
    with pytest.raises(ValueError, match="hubert"):
        hubert.check_hubert_args(types.SimpleNamespace(**dict(vars(W.TINY), **{field: value})))


def test_conv_bias_needs_the_layer_norm_extractor_and_the_state_dict_must_agree(sd):
    import hubert_ref as R

    with pytest.raises(ValueError, match="conv_bias"):
        hubert.check_hubert_args(types.SimpleNamespace(**dict(vars(R.TINY), conv_bias=True)))
    inner = {k[len(W.W2V):]: v for k, v in sd.items() if k.startswith(W.W2V)}
    with pytest.raises(ValueError, match="conv biases"):
        hubert.pack_hubert(inner, types.SimpleNamespace(**dict(vars(W.TINY), conv_bias=False)), _lib.DN_F32)
    with pytest.raises(ValueError, match="layer_norm"):
        hubert.pack_hubert({k: v for k, v in inner.items() if not k.endswith(".0.bias") or "pos_conv" in k}, types.SimpleNamespace(**dict(vars(W.TINY), extractor_mode="default", layer_norm_first=False, normalize=False, required_seq_len_multiple=1, conv_bias=False)), _lib.DN_F32)


def test_packed_table_shapes_and_config(sd):
    inner = {k[len(W.W2V):]: v for k, v in sd.items() if k.startswith(W.W2V)}
    table = hubert.pack_hubert(inner, W.TINY, _lib.DN_F32)
    assert len(table) == 21 + 7 + 3
    bias, lng, lnb = table[-3:]
    assert bias.shape == lng.shape == lnb.shape == (7, 64)
    assert torch.equal(bias[3], inner["feature_extractor.conv_layers.3.0.bias"]) and torch.equal(lng[0], table[1]) and torch.equal(lnb[0], table[2])
    head = hubert.pack_ctc_head(torch.ones(45, 64), torch.ones(45))
    assert head[0].shape == (128, 64) and float(head[0][45:].abs().max()) == 0.0 and head[1].shape == (48,) and head[1][45:].tolist() == [0.0] * 3
    c = hubert.hubert_config(W.TINY, _lib.DN_F16, True, 32)
    assert (c.wave_norm, c.extractor_ln, c.conv_bias, c.pre_norm, c.vocab, c.has_proj, c.n_conv) == (1, 1, 1, 1, 32, 1, 7)
    import hubert_ref as R

    c = hubert.hubert_config(R.TINY, _lib.DN_F16, False)
    assert (c.wave_norm, c.extractor_ln, c.conv_bias, c.pre_norm, c.vocab) == (0, 0, 0, 0, 0)
    assert hubert.out_frames(W.TINY, 3000) == 9


def test_the_reader_refuses_more_than_one_chunk_of_a_normalised_model():
    """The reference normalises the whole waveform, then cuts it (hubert_feature_reader.py:47-53); per-chunk statistics would differ."""
    import hubert_ref as R

    class Engine:
        def forward(self, batch, lens, layer):
            return torch.zeros(batch.shape[0], hubert.out_frames(W.TINY, batch.shape[1]), 1), None

    wave = R.make_wave(2500, 7, dc=3.0)
    whole = W.features(W.make_state_dict(), W.TINY, wave, 2)
    chunked = torch.cat([W.features(W.make_state_dict(), W.TINY, wave[s:e], 2) for s, e in hubert.chunk_bounds(2500, 1000)])
    assert whole.shape[0] != chunked.shape[0] or float((whole - chunked).abs().max()) > 1e-3  # (why it matters)
    with pytest.raises(ValueError, match="whole waveform"):
        hubert.HubertFeatureReader(None, W.TINY, layer=2, max_chunk=1000, engine=Engine()).get_feats(wave)
    assert hubert.HubertFeatureReader(None, W.TINY, layer=2, max_chunk=2500, engine=Engine()).get_feats(wave).shape[0] == hubert.out_frames(W.TINY, 2500)
    raw = types.SimpleNamespace(**dict(vars(W.TINY), normalize=False))  # without the normaliser the chunk loop is the reference's
    assert hubert.HubertFeatureReader(None, raw, layer=2, max_chunk=1000, engine=Engine()).get_feats(wave).shape[0] == 2 * hubert.out_frames(raw, 1000) + hubert.out_frames(raw, 500)


def test_hf_config_checks(golden):
    _, _, cfg = _hf(golden)
    assert asr.hf_config_namespace(cfg).normalize is True and asr.hf_config_namespace(cfg, normalize=False).normalize is False
    with pytest.raises(ValueError, match="layer_norm_eps"):
        asr.hf_config_namespace(dict(cfg, layer_norm_eps=1e-12))
    with pytest.raises(ValueError, match="feat_extract_activation"):
        asr.hf_config_namespace(dict(cfg, feat_extract_activation="relu"))
    with pytest.raises(ValueError, match="hidden_act"):
        asr.hf_config_namespace(dict(cfg, hidden_act="gelu_new"))


def _hf(golden):
    G = golden("wav2vec_ctc")
    if "hf_keys" not in G:
        pytest.fail("the golden holds no Hugging Face pin")
    keys = [str(k) for k in G["hf_keys"]]
    shapes = [tuple(int(v) for v in str(s).split(",")) for s in G["hf_shapes"]]
    conv = W.conv_layers(W.TINY)
    cfg = dict(feat_extract_norm="layer", do_stable_layer_norm=True, conv_dim=[c for c, _, _ in conv], conv_kernel=[k for _, k, _ in conv],
               conv_stride=[s for _, _, s in conv], conv_bias=True, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4,
               num_conv_pos_embeddings=8, num_conv_pos_embedding_groups=4, hidden_act="gelu")
    return G, W.hf_weights(keys, shapes), cfg


def test_hf_key_map_is_pinned_by_the_logits_of_a_real_wav2vec2forctc(golden):
    G, hf_sd, cfg = _hf(golden)
    fs = asr.hf_to_fairseq_state_dict(hf_sd, cfg)
    ns = asr.hf_config_namespace(cfg)
    hubert.check_hubert_args(ns)
    assert len(fs) == len(hf_sd) and all(k.startswith(("w2v_encoder.w2v_model.", "w2v_encoder.proj.")) for k in fs)
    em = W.emissions(fs, ns, W.golden_wave(1))
    want = torch.from_numpy(G["hf_logits"])
    assert float((em - want).abs().max()) <= 1e-9 * float(want.abs().max())
    inner = {k[len(W.W2V):]: v for k, v in fs.items() if k.startswith(W.W2V)}
    assert len(hubert.pack_hubert(inner, ns, _lib.DN_F32)) == 31  # both weight-norm spellings reach the same packing
    g, v = (next(val for k, val in hf_sd.items() if k.endswith(n)) for n in ("original0", "original1"))
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): val for k, val in hf_sd.items()}
    fs_old = asr.hf_to_fairseq_state_dict(old, cfg)
    assert torch.equal(fs_old[W.W2V + "encoder.pos_conv.0.weight_g"], g) and torch.equal(fs_old[W.W2V + "encoder.pos_conv.0.weight_v"], v)


def test_hf_key_map_refusals(golden):
    _, hf_sd, cfg = _hf(golden)
    with pytest.raises(ValueError, match="feat_extract_norm"):
        asr.hf_to_fairseq_state_dict(hf_sd, dict(cfg, feat_extract_norm="group"))
    with pytest.raises(ValueError, match="do_stable_layer_norm"):
        asr.hf_to_fairseq_state_dict(hf_sd, dict(cfg, do_stable_layer_norm=False))
    with pytest.raises(ValueError, match="adapters"):
        asr.hf_to_fairseq_state_dict(hf_sd, dict(cfg, add_adapter=True))
    with pytest.raises(ValueError, match="no fairseq name"):
        asr.hf_to_fairseq_state_dict(dict(hf_sd, **{"wav2vec2.adapter.layers.0.conv.weight": torch.zeros(1)}), cfg)
    with pytest.raises(ValueError, match="lacks"):
        asr.hf_to_fairseq_state_dict({k: v for k, v in hf_sd.items() if not k.startswith("lm_head")}, cfg)


def test_post_processing_strings_and_token_roles():
    toks = asr.fairseq_tokens(["| 94802", "E 51860", "T 38431", "A 33152", ""])
    assert toks == ["<s>", "<pad>", "</s>", "<unk>", "|", "E", "T", "A"]
    t = asr.AsrTranscriber(None, toks)
    assert (t.blank_token, t.sil_token) == ("<s>", "|")
    ids = [4, 6, 5, 7, 4, 4, 7, 6, 4]  # | T E A | | A T |
    assert t.text(ids) == "tea  at"  # consecutive spaces are not squeezed
    assert asr.AsrTranscriber(None, toks, "none").text(ids) == "t e a     a t"
    hok = asr.AsrTranscriber(None, ["<s>", "<pad>", "</s>", "<unk>", "a", "b"])  # no '|': the silence token falls back to tokens[2]
    assert hok.sil_token == "</s>" and hok.text([4, 2, 5]) == "a b" and asr.AsrTranscriber(None, hok.tokens, "none").text([4, 2, 5]) == "a   b"
    assert t.text([]) == ""
    with pytest.raises(NotImplementedError):
        asr.AsrTranscriber(None, toks, "letter")
    assert W.text(ids, toks) == t.text(ids) and W.text(ids, toks, "none") == "t e a     a t"
    assert W.ctc_greedy(torch.tensor([[0., 1, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1.]])) == [1, 1, 2]  # a a _ a b b
    assert W.ctc_greedy(torch.tensor([[1., 1, 0], [0, 2, 2.]])) == [1]  # ties: the lowest index


def test_a_ctc_head_on_the_base_form_is_refused(sd):
    import hubert_ref as R

    base = {W.W2V + k: v for k, v in R.make_state_dict(R.TINY, R.TINY_SEED).items()}
    base.update({k: v for k, v in sd.items() if k.startswith(W.PROJ)})
    with pytest.raises(ValueError, match="large form"):
        asr.Wav2VecCtcEngine(base, R.TINY, W.TOKENS, device="cuda:0")


def test_engine_refuses_a_state_dict_in_another_layout(sd):
    with pytest.raises(ValueError, match="Wav2VecCtc layout"):
        asr.Wav2VecCtcEngine({k[len(W.W2V):]: v for k, v in sd.items() if k.startswith(W.W2V)}, W.TINY, W.TOKENS, device="cuda:0")
    with pytest.raises(ValueError, match="tokens"):
        asr.Wav2VecCtcEngine(sd, W.TINY, W.TOKENS[:-1], device="cuda:0")
