"""The recogniser behind the recipe's ASR-BLEU (scripts/s2ut/eval.sh -> research/TranSpeech/asr_bleu/utils.py:221-308) on the HIP
engine: waveform -> per-utterance layer_norm -> wav2vec 2.0 encoder -> Linear to the letter vocabulary -> best-path CTC decoding
(the reference's beam-1, lexicon-free, LM-free decoder) -> string.

`Wav2VecCtcEngine` is dn_hubert_ctc_forward + dn_ctc_greedy of libdiffnorm_hip.so (include/diffnorm_hip.h; csrc/hubert.hip): the
HuBERT / wav2vec 2.0 engine with a CTC head, one forward, one head contraction and one decode launch for a ragged batch, every
utterance computed as if alone (the reference transcribes one file at a time).  `AsrTranscriber` restates ASRGenerator's surface
without its downloads; `hf_to_fairseq_state_dict` maps a Hugging Face Wav2Vec2ForCTC state dict onto the fairseq names.  BLEU and
audio files other than 16-bit PCM WAV are not done here: waveforms arrive as tensors at the model's sample rate (the vocoder emits
16 kHz) or at any other integer rate named with `sample_rate`, converted on the device first as utils.py:231-237 does on the host.
"""
import re
from typing import Dict, List, Sequence

import torch

from . import _lib
from .hubert import (WAV2VEC2_LARGE, HubertEngine, _as_wave, _resampled, _resampler_of, check_hubert_args, hubert_config, out_frames, pack_ctc_head,
                     pack_hubert)

_W2V, _PROJ = "w2v_encoder.w2v_model.", "w2v_encoder.proj."
FAIRSEQ_SPECIALS = ["<s>", "<pad>", "</s>", "<unk>"]


def fairseq_tokens(dict_lines: Sequence[str]) -> List[str]:
    """The lines of a dict.ltr.txt (`<letter> <count>`) -> the token list of prepare_fairseq_model (utils.py:201-204)."""
    return FAIRSEQ_SPECIALS + [str(line).split()[0] for line in dict_lines if str(line).strip()]


class Wav2VecCtcEngine(HubertEngine):
    """state_dict in the fairseq Wav2VecCtc layout (w2v_encoder.w2v_model.*, w2v_encoder.proj.*); tokens: the vocabulary, one entry
    per row of proj; blank: its CTC blank (tokens[0] for the fairseq models)."""

    STAGES = HubertEngine.STAGES[:4] + ("final norm + CTC head",)

    def __init__(self, state_dict, cfg=WAV2VEC2_LARGE, tokens=None, dtype="f16", device="cuda:0", blank: int = 0):
        from .engine import _dtype_code

        check_hubert_args(cfg)
        if not getattr(cfg, "layer_norm_first", False):
            raise ValueError("Wav2VecCtcEngine: the CTC head is built for the large form (extractor_mode 'layer_norm', layer_norm_first), "
                             "which the recipe's recognisers have; a head on the base form is not supported")
        sd = {k[len(_W2V):]: v for k, v in state_dict.items() if k.startswith(_W2V)}
        if _PROJ + "weight" not in state_dict or not sd:
            raise ValueError(f"Wav2VecCtcEngine: the state dict has no {_W2V}* / {_PROJ}* entries (the fairseq Wav2VecCtc layout)")
        W, b = state_dict[_PROJ + "weight"], state_dict[_PROJ + "bias"]
        self.vocab = int(W.shape[0])
        if tokens is not None and len(tokens) != self.vocab:
            raise ValueError(f"Wav2VecCtcEngine: {len(tokens)} tokens for a head of {self.vocab} rows")
        if W.shape[1] != cfg.encoder_embed_dim or not 0 <= int(blank) < self.vocab:
            raise ValueError(f"Wav2VecCtcEngine: head {tuple(W.shape)} on embed width {cfg.encoder_embed_dim}, blank {blank}")
        self.cfg, self.dim, self.tokens, self.blank = cfg, cfg.encoder_embed_dim, None if tokens is None else list(tokens), int(blank)
        self.dtype = _dtype_code(dtype)
        table = pack_hubert(sd, cfg, self.dtype) + pack_ctc_head(W, b)
        self._create(device, table, hubert_config(cfg, self.dtype, "post_extract_proj.weight" in sd, self.vocab))

    def emissions(self, wave: torch.Tensor, lengths):
        """wave [B, L] (anything behind an utterance's samples), lengths [B] -> (emissions fp32 [B, S, V] with zero rows behind each
        utterance's frames, frame counts int32 [B])."""
        B, L = wave.shape
        wave, ln, S, (wp, wn) = self._inputs(wave, lengths)
        em = torch.empty(B, S, self.vocab, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_hubert_ctc_forward(self.handle, wave.data_ptr(), ln.data_ptr(), B, L, em.data_ptr(), lens.data_ptr(), wp, wn,
                                                      _lib.current_stream()), "dn_hubert_ctc_forward")
        return em, lens

    def decode(self, emissions: torch.Tensor, lens: torch.Tensor):
        """dn_ctc_greedy -> (token ids int32 [B, S], -1 behind counts[b]; counts int32 [B]), both on the device."""
        return ctc_greedy(emissions, lens, self.blank)

    def forward(self, wave: torch.Tensor, lengths, layer=None):
        """-> (emissions, frame counts, token ids, token counts); nothing is brought to the host."""
        if layer is not None:
            return HubertEngine.forward(self, wave, lengths, layer)
        em, lens = self.emissions(wave, lengths)
        return (em, lens) + self.decode(em, lens)


def ctc_greedy(emissions: torch.Tensor, lengths: torch.Tensor, blank: int):
    """dn_ctc_greedy on device tensors: emissions fp32 [B, S, V], lengths [B] -> (tokens int32 [B, S], -1 behind counts[b]; counts)."""
    assert emissions.is_cuda and emissions.dtype == torch.float32 and emissions.dim() == 3, "emissions: a CUDA fp32 [B, S, V] tensor"
    B, S, V = emissions.shape
    emissions = emissions.contiguous()
    ln = lengths.to(emissions.device, torch.int32).contiguous()
    tokens = torch.full((B, S), -1, dtype=torch.int32, device=emissions.device)
    counts = torch.empty(B, dtype=torch.int32, device=emissions.device)
    with torch.cuda.device(emissions.device):
        _lib.check(_lib.load().dn_ctc_greedy(emissions.data_ptr(), ln.data_ptr(), B, S, V, int(blank), tokens.data_ptr(), counts.data_ptr(),
                                             _lib.current_stream()), "dn_ctc_greedy")
    return tokens, counts


def post_process(hypo: Sequence[str], mode: str, sil_token: str) -> str:
    """ASRGenerator.post_process_fn (utils.py:79-88) and transcribe_audiofile's strip + lower (:308).  Consecutive spaces stay."""
    if mode == "collapse":
        text = "".join(hypo).replace(sil_token, " ")
    elif mode == "none":
        text = " ".join(hypo).replace(sil_token, " ")
    else:
        raise NotImplementedError(f"post_process {mode!r} (only 'collapse' and 'none')")
    return text.strip().lower()


class AsrTranscriber:
    """ASRGenerator of the reference (utils.py:40-308) over an engine: tokens is the full vocabulary (fairseq_tokens(...) for a
    dict.ltr.txt); the blank is tokens[0] and the silence token `|`, else tokens[2], as prepare_fairseq_model infers them."""

    def __init__(self, engine, tokens: Sequence[str], post_process: str = "collapse"):
        if post_process not in ("collapse", "none"):
            raise NotImplementedError(f"post_process {post_process!r} (only 'collapse' and 'none')")
        self.engine, self.tokens, self.post_process = engine, list(tokens), post_process
        self._resamplers = None
        self.blank_token = self.tokens[0]
        self.sil_token = "|" if "|" in self.tokens else self.tokens[2]
        if engine is not None and (engine.vocab != len(self.tokens) or engine.blank != 0):
            raise ValueError(f"AsrTranscriber: {len(self.tokens)} tokens (blank first) for an engine of {engine.vocab} rows, blank {engine.blank}")

    def text(self, ids: Sequence[int]) -> str:
        return post_process([self.tokens[int(i)] for i in ids], self.post_process, self.sil_token)

    def resampler(self, sample_rate):
        """The cached Resampler from `sample_rate` to the model's rate (cfg.sample_rate, 16 000 where the config carries none); None
        when there is nothing to convert."""
        return None if sample_rate is None else _resampler_of(self, self.engine.cfg, self.engine.device, sample_rate)

    def transcribe(self, waves: Sequence, sample_rate=None) -> List[str]:
        """A ragged batch of waveforms (1-D, at the model's sample rate) -> one string each: one forward, one head contraction, one
        decode launch, then one copy of the token ids to the host.  sample_rate: the waveforms' rate when it is not the model's
        (utils.py:231-237): they are resampled on the device first ([n] or [n, C], fp32 or int16, as Resampler.forward takes them)."""
        _, _, tokens, counts = self.forward(waves, sample_rate=sample_rate)
        tokens, counts = tokens.cpu(), counts.cpu()
        return [self.text(tokens[j, : int(counts[j])].tolist()) for j in range(len(waves))]

    def score(self, waves: Sequence, references: Sequence[str], sample_rate=None, unit: str = "word"):
        """transcribe() followed by the error rate against `references` -> (transcripts, metrics.ErrorRate): word error rate
        (unit "word": str.split() tokens) or character error rate (unit "char": code points), the distances on the device
        (metrics.wer / metrics.cer).  The transcripts are what transcribe() returns (stripped, lower case); the references are
        compared as they are given: case and punctuation are the caller's."""
        from . import metrics

        if unit not in ("word", "char"):
            raise ValueError(f"AsrTranscriber.score: unit {unit!r} ('word' or 'char')")
        if len(references) != len(waves):
            raise ValueError(f"AsrTranscriber.score: {len(references)} references for {len(waves)} waveforms")
        hyps = self.transcribe(waves, sample_rate=sample_rate)
        return hyps, (metrics.wer if unit == "word" else metrics.cer)(hyps, list(references), device=self.engine.device)

    def asr_bleu(self, waves: Sequence, references: Sequence[str], sample_rate=None, lowercase: bool = True, smooth: str = "exp"):
        """transcribe() followed by BLEU against `references` -> (transcripts, metrics.BleuScore): ASR-BLEU as
        compute_asr_bleu.py:138-153 forms it, the n-gram statistics on the device (metrics.bleu).  The transcripts are what
        transcribe() returns; lowercase lowers both sides before they are compared (the recipe lowers the transcripts).  Tokens are
        str.split(): punctuation in the references is the caller's to normalise."""
        from . import metrics

        metrics._check_smooth(smooth)
        if isinstance(references, str):
            raise ValueError("AsrTranscriber.asr_bleu: a list of reference strings is expected, not one string")
        if len(references) != len(waves):
            raise ValueError(f"AsrTranscriber.asr_bleu: {len(references)} references for {len(waves)} waveforms")
        hyps = self.transcribe(waves, sample_rate=sample_rate)
        return hyps, metrics.bleu(hyps, list(references), smooth=smooth, lowercase=lowercase, device=self.engine.device)

    def forward(self, waves: Sequence, sample_rate=None):
        """The engine's forward on the padded batch transcribe() builds -> (emissions, frame counts, token ids, token counts)."""
        waves = _resampled(self.resampler(sample_rate), waves)
        waves = [_as_wave(w) for w in waves]
        lens = torch.tensor([w.numel() for w in waves], dtype=torch.int32)
        for n in lens.tolist():
            if out_frames(self.engine.cfg, n) < 1:
                raise ValueError(f"a waveform of {n} samples is shorter than one frame of the conv stack")
        batch = torch.zeros(len(waves), int(lens.max()), device=waves[0].device if all(w.device == waves[0].device for w in waves) else "cpu")
        for j, w in enumerate(waves):
            batch[j, : w.numel()] = w
        return self.engine.forward(batch, lens)


_HF_LAYER = {"attention.q_proj": "self_attn.q_proj", "attention.k_proj": "self_attn.k_proj", "attention.v_proj": "self_attn.v_proj",
             "attention.out_proj": "self_attn.out_proj", "layer_norm": "self_attn_layer_norm", "feed_forward.intermediate_dense": "fc1",
             "feed_forward.output_dense": "fc2", "final_layer_norm": "final_layer_norm"}
_HF_RULES = [
    (r"wav2vec2\.feature_extractor\.conv_layers\.(\d+)\.conv\.(weight|bias)", lambda m: f"feature_extractor.conv_layers.{m[1]}.0.{m[2]}"),
    (r"wav2vec2\.feature_extractor\.conv_layers\.(\d+)\.layer_norm\.(weight|bias)", lambda m: f"feature_extractor.conv_layers.{m[1]}.2.1.{m[2]}"),
    (r"wav2vec2\.feature_projection\.layer_norm\.(weight|bias)", lambda m: f"layer_norm.{m[1]}"),
    (r"wav2vec2\.feature_projection\.projection\.(weight|bias)", lambda m: f"post_extract_proj.{m[1]}"),
    (r"wav2vec2\.encoder\.pos_conv_embed\.conv\.(bias|weight_g|weight_v|parametrizations\.weight\.original[01])", lambda m: f"encoder.pos_conv.0.{m[1]}"),
    (r"wav2vec2\.encoder\.layers\.(\d+)\.(" + "|".join(re.escape(k) for k in _HF_LAYER) + r")\.(weight|bias)",
     lambda m: f"encoder.layers.{m[1]}.{_HF_LAYER[m[2]]}.{m[3]}"),
    (r"wav2vec2\.encoder\.layer_norm\.(weight|bias)", lambda m: f"encoder.layer_norm.{m[1]}"),
    (r"wav2vec2\.masked_spec_embed", lambda m: "mask_emb"),
]


def hf_to_fairseq_state_dict(sd: Dict[str, torch.Tensor], config) -> Dict[str, torch.Tensor]:
    """A Hugging Face Wav2Vec2ForCTC state dict -> the fairseq Wav2VecCtc names Wav2VecCtcEngine takes.  The two encoder forms of
    that class share their key names, so the model's config says which one it is: only feat_extract_norm 'layer' with
    do_stable_layer_norm True (the large / XLSR recognisers: LayerNorm extractor, pre-norm layers) is mapped; adapters and any
    key outside the map are refused."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    if get("feat_extract_norm") != "layer" or not get("do_stable_layer_norm"):
        raise ValueError(f"hf_to_fairseq_state_dict: feat_extract_norm {get('feat_extract_norm')!r}, do_stable_layer_norm {get('do_stable_layer_norm')!r}: "
                         "only the 'layer' / True form is mapped")
    if get("add_adapter", False) or get("position_embeddings_type", None) not in (None, "absolute"):
        raise ValueError("hf_to_fairseq_state_dict: adapters and relative position embeddings are not mapped")
    out = {}
    for k, v in sd.items():
        if k.startswith("lm_head."):
            out[_PROJ + k[len("lm_head."):]] = v
            continue
        for pat, name in _HF_RULES:
            m = re.fullmatch(pat, k)
            if m:
                out[_W2V + name(m)] = v
                break
        else:
            raise ValueError(f"hf_to_fairseq_state_dict: no fairseq name for {k!r}")
    if _PROJ + "weight" not in out or _W2V + "feature_extractor.conv_layers.1.2.1.weight" not in out:
        raise ValueError("hf_to_fairseq_state_dict: the state dict lacks lm_head or the LayerNorm behind conv layer 1")
    return out


def hf_config_namespace(config, normalize: bool = True):
    """The fields of a Hugging Face Wav2Vec2Config the engine needs, as the fairseq-style namespace check_hubert_args reads.  HF's
    waveform normalisation belongs to its processor, not to the model config: the reference applies its own layer_norm when the
    preprocessor's do_normalize is set (utils.py:150, 240-244), so the caller passes that flag as `normalize`.  The engine's norms
    have eps 1e-5 and its activations are GELU: a config that says otherwise is refused."""
    from types import SimpleNamespace

    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    if abs(float(get("layer_norm_eps", 1e-5)) - 1e-5) > 1e-12:
        raise ValueError(f"hf_config_namespace: layer_norm_eps {get('layer_norm_eps')} (the engine's norms have 1e-5)")
    if get("feat_extract_activation", "gelu") != "gelu" or get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hf_config_namespace: feat_extract_activation {get('feat_extract_activation')!r} / hidden_act {get('hidden_act')!r}: only 'gelu'")
    return SimpleNamespace(conv_feature_layers=[(d, k, s) for d, k, s in zip(get("conv_dim"), get("conv_kernel"), get("conv_stride"))],
                           extractor_mode="layer_norm", conv_bias=bool(get("conv_bias")), encoder_embed_dim=get("hidden_size"),
                           encoder_ffn_embed_dim=get("intermediate_size"), encoder_layers=get("num_hidden_layers"),
                           encoder_attention_heads=get("num_attention_heads"), conv_pos=get("num_conv_pos_embeddings"),
                           conv_pos_groups=get("num_conv_pos_embedding_groups"), layer_norm_first=True, layer_type="transformer",
                           required_seq_len_multiple=1, activation_fn="gelu", normalize=bool(normalize))
