"""The model inside the mask-predict loop: the decoder side of the reference's NAR S2UT model
`NARS2UTTransformerModel` (research/TranSpeech/nar_transformer.py:569-976, task speech_to_speech_fasttranslate,
fairseq/tasks/nat_s2s_task.py:107-127) on the HIP engine, with the interface the research IterativeRefinementGenerator drives
(research/TranSpeech/iterative_refinement_generator.py:131-160; mirror: diffnorm_amd/iterative_refinement.py with
`speech_source=True`): forward_encoder / initialize_output_tokens / forward_decoder / regenerate_length_beam /
encoder.reorder_encoder_out.

Scope: `TransformerUnitDecoder.forward` (:321-420: token embedding + sinusoidal positions, pre-norm self-attention / encoder
attention / ReLU FFN layers, final LayerNorm, output projection), the length predictor (:436-480) and `forward_decoder`'s
mask-predict update (:791-842, one kernel: dn_cmlm_step).  The speech ENCODER (conv subsampler + transformer over fbank frames) is
out of scope: its output is a given tensor -- the `encoder` here only carries it and re-orders it.  Weights come from a state dict
under the reference decoder's parameter names (`decoder.*` of the model's checkpoint).

Classifier-free guidance (the reference's `nar_cg` evaluation: scripts/s2ut/eval_cg.sh -> research/TranSpeech/nat_gen.py --cg_scale):
`NarDecoderEngine.forward_guided` is the two decoder passes of an iteration (TransformerUnitDecoder.forward and .cg_forward,
nar_transformer.py:123-183) as one pass over 2 B rows, `NARS2UTDecoderModel.guided_mask_predict` the loop of nat_gen.py:192-236.
"""
import ctypes as C
import itertools
import math
from typing import Dict, List, Optional

import torch

from . import _lib, packing
from .engine import _Engine, _dtype_code, capture_graph
from .iterative_refinement import DecoderOut, cmlm_update


_src_ids = itertools.count(1)  # enc["_src_id"]: one per `_ckv` that comes into being; what a captured iteration's source copy is keyed by


def sinusoidal_table(num: int, dim: int, padding_idx: int) -> torch.Tensor:
    """SinusoidalPositionalEmbedding.get_embedding (fairseq/modules/sinusoidal_positional_embedding.py:36-58): [sin | cos], row
    padding_idx zeroed; built in fp32 like upstream."""
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    ang = torch.arange(num, dtype=torch.float).unsqueeze(1) * f.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).view(num, -1)
    tab[padding_idx, :] = 0
    return tab.contiguous()


def _cat_proj(sd, prefix, names):
    """(weight, bias) of the projections `names` under `prefix` as one: q ; k ; v or k ; v along the output rows."""
    return tuple(torch.cat([sd[prefix + n + "." + part].float() for n in names]) for part in ("weight", "bias"))


def _conv_mat(w, dtype, cols=None):
    """Conv1d weight [out, in, k] -> [out, k * in], column j * in + c (the gathered rows' order)."""
    w2 = w.permute(0, 2, 1).reshape(w.shape[0], -1)
    return packing._mat(w2, dtype, cols=cols or w2.shape[1])


def _subsampler_tensors(sd, input_dim, conv_channels, kernel, dim, dtype) -> List[torch.Tensor]:
    """The Conv1dSubsampler's two convs: the four tensors both speech encoders' tables open with."""
    g = lambda k: sd[k].float()
    c0, c1 = g("subsample.conv_layers.0.weight"), g("subsample.conv_layers.1.weight")
    assert c0.shape == (conv_channels, input_dim, kernel) and c1.shape == (2 * dim, conv_channels // 2, kernel), (c0.shape, c1.shape)
    return [_conv_mat(c0, dtype, cols=packing.padk(kernel * input_dim)), g("subsample.conv_layers.0.bias").contiguous(), _conv_mat(c1, dtype),
            g("subsample.conv_layers.1.bias").contiguous()]


def pack_nar(sd: Dict[str, torch.Tensor], dim: int, ffn: int, layers: int, vocab: int, max_pos: int, pad: int, dtype: int) -> List[torch.Tensor]:
    """Reference-named decoder state dict -> the tensor table of dn_nar_create (include/diffnorm_hip.h)."""
    g = lambda k: sd[k].float()
    mat = lambda w: packing._mat(w, dtype, cols=w.shape[1])  # rows -> multiple of 128, K = the (64-multiple) width itself
    stack = lambda items: torch.stack(items).contiguous()
    qkv_W, qkv_b, so_W, so_b, cq_W, cq_b, ckv_W, ckv_b, co_W, co_b, f1W, f1b, f2W, f2b, lng, lnb = ([] for _ in range(16))
    for l in range(layers):
        p = f"layers.{l}."
        sa, ea = p + "self_attn.", p + "encoder_attn."
        W, b = _cat_proj(sd, sa, ("q_proj", "k_proj", "v_proj"))
        qkv_W.append(mat(W)); qkv_b.append(b)
        so_W.append(mat(g(sa + "out_proj.weight"))); so_b.append(g(sa + "out_proj.bias"))
        cq_W.append(mat(g(ea + "q_proj.weight"))); cq_b.append(g(ea + "q_proj.bias"))
        W, b = _cat_proj(sd, ea, ("k_proj", "v_proj"))
        ckv_W.append(mat(W)); ckv_b.append(b)
        co_W.append(mat(g(ea + "out_proj.weight"))); co_b.append(g(ea + "out_proj.bias"))
        f1W.append(mat(g(p + "fc1.weight"))); f1b.append(g(p + "fc1.bias"))
        f2W.append(mat(g(p + "fc2.weight"))); f2b.append(g(p + "fc2.bias"))
        lng.append(torch.stack([g(p + "self_attn_layer_norm.weight"), g(p + "encoder_attn_layer_norm.weight"), g(p + "final_layer_norm.weight")]))
        lnb.append(torch.stack([g(p + "self_attn_layer_norm.bias"), g(p + "encoder_attn_layer_norm.bias"), g(p + "final_layer_norm.bias")]))
    len_W = torch.zeros(256, dim)
    len_W[:] = g("embed_length.weight")
    return [g("embed_tokens.weight").contiguous(), sinusoidal_table(max_pos, dim, pad), packing._mat(len_W, _lib.DN_F32, cols=dim),
            stack(qkv_W), stack(qkv_b), stack(so_W), stack(so_b), stack(cq_W), stack(cq_b), stack(ckv_W), stack(ckv_b), stack(co_W), stack(co_b),
            stack(f1W), stack(f1b), stack(f2W), stack(f2b), stack(lng), stack(lnb), g("layer_norm.weight").contiguous(),
            g("layer_norm.bias").contiguous(), mat(g("output_projection.weight"))]


def pack_nar_encoder(sd: Dict[str, torch.Tensor], input_dim: int, conv_channels: int, kernel: int, dim: int, ffn: int, layers: int, max_pos: int,
                     pad: int, dtype: int) -> List[torch.Tensor]:
    """Reference-named encoder state dict (S2TTransformerEncoder.state_dict()) -> the tensor table of dn_nar_encoder_create."""
    g = lambda k: sd[k].float()
    mat = lambda w: packing._mat(w, dtype, cols=w.shape[1])
    stack = lambda items: torch.stack(items).contiguous()
    sub = _subsampler_tensors(sd, input_dim, conv_channels, kernel, dim, dtype)
    qkv_W, qkv_b, so_W, so_b, f1W, f1b, f2W, f2b, lng, lnb = ([] for _ in range(10))
    for l in range(layers):
        p = f"transformer_layers.{l}."
        sa = p + "self_attn."
        W, b = _cat_proj(sd, sa, ("q_proj", "k_proj", "v_proj"))
        qkv_W.append(mat(W)); qkv_b.append(b)
        so_W.append(mat(g(sa + "out_proj.weight"))); so_b.append(g(sa + "out_proj.bias"))
        f1W.append(mat(g(p + "fc1.weight"))); f1b.append(g(p + "fc1.bias"))
        f2W.append(mat(g(p + "fc2.weight"))); f2b.append(g(p + "fc2.bias"))
        lng.append(torch.stack([g(p + "self_attn_layer_norm.weight"), g(p + "final_layer_norm.weight")]))
        lnb.append(torch.stack([g(p + "self_attn_layer_norm.bias"), g(p + "final_layer_norm.bias")]))
    return sub + [sinusoidal_table(max_pos, dim, pad), stack(qkv_W), stack(qkv_b), stack(so_W), stack(so_b),
                  stack(f1W), stack(f1b), stack(f2W), stack(f2b), stack(lng), stack(lnb), g("layer_norm.weight").contiguous(), g("layer_norm.bias").contiguous()]


class _NarEngine(_Engine):
    """An engine behind dn_<_sym>_create / dn_<_sym>_destroy: a subclass names `_sym` and hands `_create` its packed table and config."""
    _sym = None

    def _create(self, device, tensors, cfg):
        super().__init__(device, tensors)
        name = f"dn_{self._sym}_create"
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(C.byref(cfg), self._table, len(self.tensors), C.byref(self.handle)), name)

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            getattr(self.lib, f"dn_{self._sym}_destroy")(self.handle)
            self.handle = C.c_void_p()


class _SpeechEncoderEngine(_NarEngine):
    """The pass of a speech encoder, dn_<_sym>_workspace_bytes / dn_<_sym>_forward: once per utterance batch, in front of the refinement loop."""

    def workspace_bytes(self, B: int, L: int) -> int:
        return int(getattr(self.lib, f"dn_{self._sym}_workspace_bytes")(self.handle, B, L))

    def forward(self, feats: torch.Tensor, src_lengths: torch.Tensor):
        """feats [B, L, input_dim], src_lengths [B] -> (enc_out fp32 [B, S, dim] batch-major, lengths int32 [B])."""
        B, L, Fd = feats.shape
        assert Fd == self.input_dim
        feats = feats.to(self.device, torch.float32).contiguous()
        sl = src_lengths.to(self.device, torch.int32).contiguous()
        S = int(self.lib.dn_nar_encoder_out_frames(L))  # (the one Conv1dSubsampler in front of both encoders)
        out = torch.empty(B, S, self.dim, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        wp, wn = self._aligned(self._workspace(self.workspace_bytes(B, L)))
        name = f"dn_{self._sym}_forward"
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(self.handle, feats.data_ptr(), sl.data_ptr(), B, L, out.data_ptr(), lens.data_ptr(), wp, wn,
                                               _lib.current_stream()), name)
        return out, lens


class NarEncoderEngine(_SpeechEncoderEngine):
    """dn_nar_encoder_* of libdiffnorm_hip.so: the speech encoder of the NAR S2UT model (S2STransformerEncoder,
    research/TranSpeech/nar_transformer.py:40-76)."""
    _sym = "nar_encoder"

    def __init__(self, state_dict, input_dim=80, conv_channels=1024, kernel=5, dim=512, ffn=2048, layers=12, heads=8, max_pos=6002, pad=1,
                 dtype="bf16", device="cuda:0"):
        self.dim, self.input_dim = dim, input_dim
        self.dtype = _dtype_code(dtype)
        self._create(device, pack_nar_encoder(state_dict, input_dim, conv_channels, kernel, dim, ffn, layers, max_pos, pad, self.dtype),
                     _lib.NarEncConfig(input_dim, conv_channels, kernel, dim, ffn, layers, heads, max_pos, pad, self.dtype))


def rel_pos_table(max_frames: int, dim: int) -> torch.Tensor:
    """RelPositionalEncoding's table (fairseq/modules/positional_encoding.py:94-112) for the offsets d = -(max_frames - 1) ..
    max_frames - 1, offset d at row max_frames - 1 + d: pe(d)[2m] = sin(d w_m), pe(d)[2m+1] = cos(d w_m), w_m = exp(-2m ln(1e4) / dim),
    built in FLOAT32 like upstream (`position * div_term` in float32 included; -1 * position * div_term = (-position) * div_term exactly)."""
    d = torch.arange(-(max_frames - 1), max_frames, dtype=torch.float32).unsqueeze(1)
    div = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(2 * max_frames - 1, dim)
    pe[:, 0::2] = torch.sin(d * div)
    pe[:, 1::2] = torch.cos(d * div)
    return pe


def fold_batch_norm(w: torch.Tensor, gamma, beta, mean, var, eps: float = 1e-5):
    """Depthwise Conv1d weight [C, 1, k] (no bias) followed by BatchNorm1d in eval mode -> (w' [C, k], shift [C]) with
    BatchNorm(conv_w(x)) = conv_w'(x) + shift: w' = w gamma / sqrt(var + eps), shift = beta - mean gamma / sqrt(var + eps)."""
    s = gamma / torch.sqrt(var + eps)
    return (w[:, 0, :] * s[:, None]).contiguous(), (beta - mean * s).contiguous()


def check_conformer_args(attn_type="espnet", pos_enc_type="rel_pos", conv_version="s2t_transformer", depthwise_kernel=31):
    """What of S2TConformerEncoder's variants the engine runs; the rest is refused here, on the host."""
    if attn_type != "espnet":
        raise ValueError(f"conformer encoder: attn_type {attn_type!r} (the fairseq MultiheadAttention variant) is not supported, only 'espnet'")
    if pos_enc_type != "rel_pos":
        raise ValueError(f"conformer encoder: pos_enc_type {pos_enc_type!r} is not supported, only 'rel_pos'")
    if conv_version != "s2t_transformer":
        raise ValueError(f"conformer encoder: conv_version {conv_version!r} (Conv2dSubsampler) is not supported, only 's2t_transformer'")
    if depthwise_kernel % 2 != 1 or not 1 <= depthwise_kernel <= 63:
        raise ValueError(f"conformer encoder: depthwise kernel {depthwise_kernel} must be odd ('same' padding) and <= 63")


def pack_conformer_encoder(sd: Dict[str, torch.Tensor], input_dim: int, conv_channels: int, kernel: int, dim: int, ffn: int, layers: int, heads: int,
                           depthwise_kernel: int, max_frames: int, dtype: int, attn_type: str = "espnet", pos_enc_type: str = "rel_pos",
                           conv_version: str = "s2t_transformer") -> List[torch.Tensor]:
    """Reference-named encoder state dict (S2TConformerEncoder.state_dict(), attn_type espnet + pos_enc_type rel_pos) -> the tensor
    table of dn_conformer_encoder_create (include/diffnorm_hip.h).  The BatchNorm of the convolution module is folded into the
    depthwise weights, the half step of the two FFNs into w_2 (a factor 0.5: exact in every arithmetic)."""
    check_conformer_args(attn_type, pos_enc_type, conv_version, depthwise_kernel)
    if any("spk_emb_proj" in k for k in sd):
        raise ValueError("conformer encoder: the target-speaker projection (spk_emb_proj) is not supported")
    if any(".self_attn.q_proj." in k for k in sd):
        raise ValueError("conformer encoder: this state dict holds fairseq MultiheadAttention layers; only attn_type 'espnet' is supported")
    if "subsample.conv_layers.0.weight" not in sd:
        raise ValueError("conformer encoder: no Conv1dSubsampler in the state dict (conv_version 'convtransformer' is not supported)")
    if "conformer_layers.0.self_attn.linear_pos.weight" not in sd:
        raise ValueError("conformer encoder: no linear_pos in the state dict: only pos_enc_type 'rel_pos' is supported")
    g = lambda k: sd[k].float()
    mat = lambda w: packing._mat(w, dtype, cols=w.shape[1])
    stack = lambda items: torch.stack(items).contiguous()
    sub = _subsampler_tensors(sd, input_dim, conv_channels, kernel, dim, dtype)
    names = ("f1w1", "f1b1", "f1w2", "f1b2", "f2w1", "f2b1", "f2w2", "f2b2", "qkvW", "qkvb", "posW", "outW", "outb", "u", "v", "pw1", "dww", "dws",
             "pw2", "lng", "lnb")
    t = {n: [] for n in names}
    for l in range(layers):
        p = f"conformer_layers.{l}."
        for tag, ff in (("f1", "ffn1."), ("f2", "ffn2.")):
            t[tag + "w1"].append(mat(g(p + ff + "w_1.weight"))); t[tag + "b1"].append(g(p + ff + "w_1.bias"))
            t[tag + "w2"].append(mat(0.5 * g(p + ff + "w_2.weight"))); t[tag + "b2"].append(0.5 * g(p + ff + "w_2.bias"))
        sa, cm = p + "self_attn.", p + "conv_module."
        W, b = _cat_proj(sd, sa, ("linear_q", "linear_k", "linear_v"))
        t["qkvW"].append(mat(W)); t["qkvb"].append(b)
        t["posW"].append(mat(g(sa + "linear_pos.weight")))
        t["outW"].append(mat(g(sa + "linear_out.weight"))); t["outb"].append(g(sa + "linear_out.bias"))
        u, v = g(sa + "pos_bias_u"), g(sa + "pos_bias_v")
        assert u.shape == v.shape == (heads, dim // heads), u.shape
        t["u"].append(u.reshape(-1)); t["v"].append(v.reshape(-1))
        dw = g(cm + "depthwise_conv.weight")
        if dw.shape != (dim, 1, depthwise_kernel) or (cm + "depthwise_conv.bias") in sd or (cm + "pointwise_conv1.bias") in sd:
            raise ValueError(f"conformer encoder: depthwise conv {tuple(dw.shape)} (expected {(dim, 1, depthwise_kernel)}, no conv biases)")
        w, shift = fold_batch_norm(dw, g(cm + "batch_norm.weight"), g(cm + "batch_norm.bias"), g(cm + "batch_norm.running_mean"),
                                   g(cm + "batch_norm.running_var"))
        t["pw1"].append(mat(g(cm + "pointwise_conv1.weight")[:, :, 0])); t["dww"].append(w); t["dws"].append(shift)
        t["pw2"].append(mat(g(cm + "pointwise_conv2.weight")[:, :, 0]))
        order = ("ffn1.layer_norm", "self_attn_layer_norm", "conv_module.layer_norm", "ffn2.layer_norm", "final_layer_norm")
        t["lng"].append(torch.stack([g(p + n + ".weight") for n in order])); t["lnb"].append(torch.stack([g(p + n + ".bias") for n in order]))
    pe = packing._arith(rel_pos_table(max_frames, dim), dtype, weight=False)
    return sub + [mat(g("linear.weight")), g("linear.bias").contiguous(), pe] + [stack(t[n]) for n in names] + [torch.zeros(2 * dim)]


class ConformerEncoderEngine(_SpeechEncoderEngine):
    """dn_conformer_encoder_* of libdiffnorm_hip.so: the Conformer speech encoder of the recipe's NAR S2UT model (S2SConformerEncoder,
    research/TranSpeech/nar_conformer.py:42-74, attn_type espnet + pos_enc_type rel_pos, no speaker embedding), eval mode."""
    _sym = "conformer_encoder"

    def __init__(self, state_dict, input_dim=80, conv_channels=1024, kernel=5, dim=512, ffn=2048, layers=12, heads=8, depthwise_kernel=31,
                 max_source_positions=6000, dtype="bf16", device="cuda:0", attn_type="espnet", pos_enc_type="rel_pos",
                 conv_version="s2t_transformer"):
        self.dim, self.input_dim = dim, input_dim
        self.dtype = _dtype_code(dtype)
        max_frames = int(_lib.load().dn_nar_encoder_out_frames(max_source_positions))  # frames of the longest source behind the subsampler
        self._create(device, pack_conformer_encoder(state_dict, input_dim, conv_channels, kernel, dim, ffn, layers, heads, depthwise_kernel,
                                                    max_frames, self.dtype, attn_type, pos_enc_type, conv_version),
                     _lib.ConformerEncConfig(input_dim, conv_channels, kernel, dim, ffn, layers, heads, depthwise_kernel, max_frames, self.dtype))

    def forward(self, feats: torch.Tensor, src_lengths: torch.Tensor):
        """feats [B, L, input_dim], src_lengths [B] (each >= 1) -> (enc_out fp32 [B, S, dim] batch-major, lengths int32 [B]).
        Lengths on the host are checked here; lengths already on the device are not read back (no synchronisation, as
        NarEncoderEngine.forward): an empty utterance there is the caller's to exclude -- the kernels stay inside their tensors (the
        attention treats it as one key) but its rows mean nothing."""
        src_lengths = torch.as_tensor(src_lengths)
        if src_lengths.device.type == "cpu" and int(src_lengths.min()) < 1:
            raise ValueError("ConformerEncoderEngine.forward: an empty utterance has no attention softmax")
        return super().forward(feats, src_lengths)


class _HipEncoder:
    """`model.encoder` of the NAR S2UT model on the HIP engine: __call__(src_tokens [B, L, 80], src_lengths) -> the reference's encoder
    dict (encoder_out [S, B, D], encoder_padding_mask [B, S] -- an empty list when nothing is padded, s2t_transformer.py:364-373), with
    the batch-major copy and the subsampled lengths the decoder engine wants riding along; reorder_encoder_out as upstream (:387-420)."""

    def __init__(self, engine, fbank=None):  # a NarEncoderEngine or a ConformerEncoderEngine; fbank: a FbankEngine in front of it
        self.engine, self.fbank = engine, fbank

    def __call__(self, src_tokens, src_lengths=None, sample_rate=None):
        if sample_rate is not None and self.fbank is None:
            raise ValueError("sample_rate belongs to waveform input (waveform_input=...): features have no sample rate to convert")
        if self.fbank is not None:  # src_tokens [B, L] waveforms, src_lengths in samples -> features; their lengths stay on the device
            src_tokens, src_lengths = self.fbank.forward(src_tokens, src_lengths, sample_rate=sample_rate)
        x, lens = self.engine.forward(src_tokens, src_lengths)
        S = x.shape[1]
        pad = torch.arange(S, device=x.device)[None, :] >= lens[:, None]
        return {"encoder_out": [x.transpose(0, 1)], "encoder_padding_mask": [pad] if bool(pad.any()) else [], "encoder_embedding": [],
                "encoder_states": [], "src_tokens": [], "src_lengths": []}

    def reorder_encoder_out(self, enc, order):
        return _GivenEncoder.reorder_encoder_out(self, enc, order)


class NarDecoderEngine(_NarEngine):
    """dn_nar_* of libdiffnorm_hip.so: cross-attention keys / values once per batch, length prediction, one decoder pass."""
    _sym = "nar"

    def __init__(self, state_dict, dim=512, ffn=2048, layers=6, heads=8, vocab=1004, max_pos=1026, pad=1, dtype="bf16", device="cuda:0"):
        self.dim, self.ffn, self.layers, self.heads, self.vocab, self.pad = dim, ffn, layers, heads, vocab, pad
        self.dtype = _dtype_code(dtype)
        self._create(device, pack_nar(state_dict, dim, ffn, layers, vocab, max_pos, pad, self.dtype),
                     _lib.NarConfig(dim, ffn, layers, heads, vocab, max_pos, pad, self.dtype))

    def _pass_bytes(self, B, T, S, guided: bool = False) -> int:
        size = self.lib.dn_nar_guided_workspace_bytes if guided else self.lib.dn_nar_workspace_bytes
        return int(size(self.handle, B, T, S))

    def _ws_for(self, B, T, S, guided: bool = False):
        return self._aligned(self._workspace(self._pass_bytes(B, T, S, guided)))

    def cross_kv(self, enc_out: torch.Tensor) -> torch.Tensor:
        """enc_out fp32 [B, S, D] -> the layers' encoder-attention keys / values [layers, B, S, 2 D] (engine dtype; fp32 for bf16x3)."""
        B, S, D = enc_out.shape
        assert D == self.dim and enc_out.is_contiguous() and enc_out.dtype == torch.float32 and enc_out.device == self.device
        tdt = self._kv_dtype
        raw = _lib.alloc_workspace(self.lib.dn_nar_cross_kv_bytes(self.handle, B, S), self.device)
        off = (-raw.data_ptr()) % 256
        ckv = raw[off: off + self.layers * B * S * 2 * D * tdt.itemsize].view(tdt).view(self.layers, B, S, 2 * D)
        wp, wn = self._ws_for(B, 1, S)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_nar_cross_kv(self.handle, enc_out.data_ptr(), B, S, ckv.data_ptr(), wp, wn, _lib.current_stream()), "dn_nar_cross_kv")
        return ckv

    def predict_lengths(self, enc_out: torch.Tensor, src_lengths: torch.Tensor) -> torch.Tensor:
        B, S, _ = enc_out.shape
        out = torch.empty(B, dtype=torch.int32, device=self.device)
        sl = src_lengths.to(self.device, torch.int32).contiguous()
        wp, wn = self._ws_for(B, 1, S)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_nar_predict_lengths(self.handle, enc_out.data_ptr(), sl.data_ptr(), B, S, out.data_ptr(), wp, wn, _lib.current_stream()),
                       "dn_nar_predict_lengths")
        return out

    @property
    def _kv_dtype(self) -> torch.dtype:
        return torch.bfloat16 if self.dtype == _lib.DN_BF16 else torch.float16 if self.dtype == _lib.DN_F16 else torch.float32

    def _pass(self, guided: bool, tokens, ckv, src_lengths, out, workspace) -> torch.Tensor:
        """One decoder pass, plain ([B, T, vocab]) or guided ([2, B, T, vocab]).  workspace: (aligned address, bytes) of the caller's,
        else the engine's (which a larger later call re-allocates: a captured pass brings its own)."""
        B, T = tokens.shape
        S = ckv.shape[2]
        assert tokens.dtype == torch.int32 and tokens.is_contiguous() and ckv.is_contiguous() and ckv.shape[1] == B
        sl = src_lengths if (src_lengths.dtype == torch.int32 and src_lengths.device == self.device) else src_lengths.to(self.device, torch.int32)
        shape = ((2,) if guided else ()) + (B, T, self.vocab)
        logits = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else out
        assert logits.shape == shape and logits.dtype == torch.float32 and logits.is_contiguous()
        wp, wn = self._ws_for(B, T, S, guided) if workspace is None else workspace
        name = "dn_nar_decoder_forward_guided" if guided else "dn_nar_decoder_forward"
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(self.handle, tokens.data_ptr(), ckv.data_ptr(), sl.contiguous().data_ptr(), B, T, S, logits.data_ptr(),
                                               wp, wn, _lib.current_stream()), name)
        return logits

    def forward(self, tokens: torch.Tensor, ckv: torch.Tensor, src_lengths: torch.Tensor, out: Optional[torch.Tensor] = None,
                workspace=None) -> torch.Tensor:
        """tokens int32 [B, T] -> logits fp32 [B, T, vocab]."""
        return self._pass(False, tokens, ckv, src_lengths, out, workspace)


    # ---- classifier-free guidance (nat_gen.py:196-236; cg_forward, nar_transformer.py:123-183)
    null_generation = 0  # counts the tables formed: a captured pass holds the address of the one it was captured with
    null_token = None  # the token whose embedding row stands in for the dropped source (None: dn_nar_null_cross has not run)

    def null_cross(self, null_token: int = 0) -> torch.Tensor:
        """dn_nar_null_cross: the fp32 [layers, dim] table of c_l = W_o (W_v emb[null_token] + b_v) + b_o, formed on the device in the
        engine's arithmetic, once per engine and token.  -> a view of the table (it lives in a buffer this engine keeps)."""
        if self.null_token != int(null_token):
            buf = _lib.alloc_workspace(self.lib.dn_nar_null_cross_bytes(self.handle), self.device)
            wp, wn = self._aligned(buf)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.dn_nar_null_cross(self.handle, int(null_token), wp, wn, _lib.current_stream()), "dn_nar_null_cross")
                torch.cuda.current_stream().synchronize()  # the previous buffer (another token's table) may go only after this
            off = int(self.lib.dn_nar_null_table(self.handle)) - buf.data_ptr()
            self._null_buf, self.null_token, self.null_generation = buf, int(null_token), self.null_generation + 1
            self._null_tab = buf[off: off + self.layers * self.dim * 4].view(torch.float32).view(self.layers, self.dim)
        return self._null_tab

    def forward_guided(self, tokens: torch.Tensor, ckv: torch.Tensor, src_lengths: torch.Tensor, out: Optional[torch.Tensor] = None,
                       workspace=None) -> torch.Tensor:
        """tokens int32 [B, T] -> logits fp32 [2, B, T, vocab]: [0] attends to the encoder (`ckv`), [1] to the null source.
        `null_cross` must have run (the C entry refuses otherwise)."""
        return self._pass(True, tokens, ckv, src_lengths, out, workspace)

    def guided_logits(self, tokens: torch.Tensor, ckv: torch.Tensor, src_lengths: torch.Tensor, cg_scale: float) -> torch.Tensor:
        """scaled_logits = cond + cg_scale * (cond - null) (nat_gen.py:223), fp32 [B, T, vocab] -- for callers and tests: the loop's
        update kernel (dn_cmlm_guided_step) forms the same values in registers and never writes them."""
        both = self.forward_guided(tokens, ckv, src_lengths)
        return both[0] + float(cg_scale) * (both[0] - both[1])


class _GivenEncoder:
    """The speech encoder is out of this row's scope: `__call__` hands back the encoder output it is given (the reference's dict:
    encoder_out [S,B,D], encoder_padding_mask [B,S]); `reorder_encoder_out` follows S2TTransformerEncoder's
    (fairseq/models/speech_to_text/s2t_transformer.py:383-411) and also re-orders the cached encoder-attention keys / values."""

    def __call__(self, encoder_out, src_lengths=None):
        return encoder_out

    def reorder_encoder_out(self, enc, order):
        order = order.reshape(-1)
        out = {"encoder_out": [x.index_select(1, order) for x in enc["encoder_out"]],
               "encoder_padding_mask": [x.index_select(0, order) for x in enc["encoder_padding_mask"]],
               "encoder_embedding": [], "encoder_states": [], "src_tokens": [], "src_lengths": []}
        if "_ckv" in enc:  # engine-side caches travel with the rows, as a NEW source: the id is never inherited
            out["_ckv"], out["_src_len"] = enc["_ckv"].index_select(1, order).contiguous(), enc["_src_len"].index_select(0, order).contiguous()
            out["_src_id"] = next(_src_ids)
        return out


class _IterationGraph:
    """ONE iteration of a mask-predict loop -- the decoder pass (about 70 launches), the CMLM update with the iteration index read
    from a device counter, the counter's increment -- captured into a hipGraph over static buffers and replayed: an iteration is one
    graph launch.  Three forms:
      scale set             the guided loop (nat_gen.py:196-236): the pass over 2 B rows, dn_cmlm_guided_step_dev (which writes the
                            scores and never reads them: the reset of :197 is inside the kernel)
      scale None, reset     the same loop without the null half (:225): the scores zeroed, the plain pass, dn_cmlm_step_dev
      scale None, no reset  forward_decoder / refine: the plain pass, dn_cmlm_step_dev on the scores of the earlier iterations
    Everything a captured launch touches is held here -- tokens, scores, predicted, step, logits, a copy of the encoder-attention
    keys / values and source lengths, a workspace of its own (the engine's is re-allocated by a larger later call) -- except the
    engine's packed weights and null table.  The source is copied when its id (`_src_id`, stamped where a `_ckv` comes into being)
    differs from the one copied last: once per utterance batch or re-ordering, whatever addresses the allocator hands out."""

    def __init__(self, model, B, T, S, n_iters, scale, reset_scores):
        eng, dev = model.engine, model.device
        self.model, self.n_iters, self.scale, self.reset_scores, self.graph = model, int(n_iters), scale, reset_scores, None
        self.tokens = torch.empty(B, T, dtype=torch.int32, device=dev)
        self.scores = torch.zeros(B, T, dtype=torch.float32, device=dev)
        self.predicted = torch.empty(B, T, dtype=torch.int32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.logits = torch.empty(((2,) if scale is not None else ()) + (B, T, eng.vocab), dtype=torch.float32, device=dev)
        self.ckv = torch.empty(eng.layers, B, S, 2 * eng.dim, dtype=eng._kv_dtype, device=dev)
        self.slen = torch.empty(B, dtype=torch.int32, device=dev)
        self._src_id = None
        self._ws = _lib.alloc_workspace(eng._pass_bytes(B, T, S, scale is not None), dev)

    def load(self, enc, tokens, scores=None, step=None):
        """The state the next run() starts from; `enc` has been through the model's _prepared()."""
        if enc["_src_id"] != self._src_id:
            self.ckv.copy_(enc["_ckv"])
            self.slen.copy_(enc["_src_len"])
            self._src_id = enc["_src_id"]
        self.tokens.copy_(tokens)
        if scores is not None:
            self.scores.copy_(scores)
        if step is None:
            self.step.zero_()
        else:
            self.step.fill_(int(step))

    def _iteration(self):
        m, eng = self.model, self.model.engine
        B, T, V = self.logits.shape[-3:]
        ws = eng._aligned(self._ws)
        args = (self.tokens.data_ptr(), self.scores.data_ptr(), self.predicted.data_ptr(), B, T, V, self.step.data_ptr(), self.n_iters, int(m.unk),
                int(m.pad), _lib.current_stream())
        if self.scale is not None:
            eng.forward_guided(self.tokens, self.ckv, self.slen, out=self.logits, workspace=ws)
            _lib.check(eng.lib.dn_cmlm_guided_step_dev(self.logits.data_ptr(), float(self.scale), *args), "dn_cmlm_guided_step_dev")
        else:
            if self.reset_scores:
                self.scores.zero_()
            eng.forward(self.tokens, self.ckv, self.slen, out=self.logits, workspace=ws)
            _lib.check(eng.lib.dn_cmlm_step_dev(self.logits.data_ptr(), *args), "dn_cmlm_step_dev")
        self.step.add_(1)

    def run(self, n: int = 1):
        """n iterations from the state in the static buffers (tokens, scores, step)."""
        with torch.cuda.device(self.model.device):
            if self.graph is None:
                self._iteration()  # eager first: kernel attributes settle outside capture
                n -= 1
                self.graph = capture_graph(self.model.device, self._iteration)
            for _ in range(n):
                self.graph.replay()


class NARS2UTDecoderModel:
    """forward_decoder / initialize_output_tokens / regenerate_length_beam of NARS2UTTransformerModel (:791-912) over the HIP decoder.
    `use_graph` (default on): an iteration of `forward_decoder` and of `guided_mask_predict` runs as ONE captured hipGraph launch
    (_IterationGraph, one bounded cache for both loops) instead of ~70 host launches -- same kernels on the same inputs,
    bit-identical results; `refine(state, enc, n)` runs n iterations back to back with no host work in between (a generator without
    the adaptive early stop, and the benchmark).  The captured iteration decodes against its own copy of the encoder-attention keys /
    values, refreshed whenever the encoder dict it is handed carries another `_src_id`."""
    allow_length_beam = True

    def __init__(self, decoder_state_dict, dim=512, ffn=2048, layers=6, heads=8, vocab=1004, pad=1, unk=3, dtype="bf16", device="cuda:0",
                 use_graph: bool = True, encoder_state_dict=None, encoder_kw=None, eos: int = 2, encoder_arch: str = "transformer",
                 waveform_input=None):
        """encoder_state_dict (S2TTransformerEncoder.state_dict() names; encoder_kw = NarEncoderEngine's sizes): with it `forward_encoder`
        runs the speech encoder on the HIP engine from [B, L, 80] features, as NARS2UTTransformerModel.forward_encoder does (:566-567);
        without it the encoder output is a tensor the caller supplies.  encoder_arch "conformer": the state dict is
        S2TConformerEncoder.state_dict()'s and encoder_kw ConformerEncoderEngine's sizes (the recipe's --arch nar_s2ut_conformer).
        waveform_input (a diffnorm_amd.fbank.FbankConfig, or True for the recipe's: 16 kHz, 80 bins, utterance CMVN): the encoder takes
        src_tokens [B, L] waveforms with src_lengths in samples and runs the Kaldi fbank + CMVN front end (FbankEngine) in front of the
        speech encoder, so `generate()` works from waveforms; unset, it takes [B, L, 80] features as before."""
        if encoder_arch not in ("transformer", "conformer"):
            raise ValueError(f"encoder_arch {encoder_arch!r}: 'transformer' or 'conformer'")
        if waveform_input and encoder_state_dict is None:
            raise ValueError("waveform_input needs the speech encoder on the engine (encoder_state_dict)")
        self.engine = NarDecoderEngine(decoder_state_dict, dim, ffn, layers, heads, vocab, pad=pad, dtype=dtype, device=device)
        if encoder_state_dict is not None:
            kw = dict(dim=dim, heads=heads, dtype=dtype, device=device)
            kw.update(encoder_kw or {})
            fb = None
            if waveform_input:
                from .fbank import FbankConfig, FbankEngine

                fb = FbankEngine(FbankConfig() if waveform_input is True else waveform_input, device=device)
                if fb.n_mels != kw.get("input_dim", 80):
                    raise ValueError(f"waveform_input: {fb.n_mels} mel bins, but the speech encoder takes {kw.get('input_dim', 80)} features per frame")
            self.encoder = _HipEncoder((ConformerEncoderEngine if encoder_arch == "conformer" else NarEncoderEngine)(encoder_state_dict, **kw), fb)
        else:
            self.encoder = _GivenEncoder()
        self.pad, self.unk, self.eos, self.device = pad, unk, eos, self.engine.device
        self.use_graph, self._graphs = use_graph, {}

    def _graph_for(self, reset_scores: bool, B, T, S, n_iters, scale=None) -> "_IterationGraph":
        """The captured iteration for everything a capture bakes in: (reset_scores, B, T, S, n_iters, scale[, nar_cg_fold, null table])."""
        key = (bool(reset_scores), B, T, S, int(n_iters), scale)
        if scale is not None:
            key += (_lib.get_option("nar_cg_fold"), self.engine.null_generation)
        g = self._graphs.get(key)
        if g is None:
            if len(self._graphs) >= 16:  # a generator whose batch keeps shrinking: keep the cache bounded, oldest out
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[key] = _IterationGraph(self, B, T, S, n_iters, scale, reset_scores)
        return g

    def refine(self, decoder_out, encoder_out, n_iters: int):
        """n_iters mask-predict iterations from `decoder_out` (its `step` / `max_step` as the generator sets them) with no host work
        in between: the captured iteration replayed while the device step counter advances.  -> the DecoderOut after them."""
        ckv, slen = self._prepared(encoder_out)
        B, T = decoder_out.output_tokens.shape
        g = self._graph_for(False, B, T, ckv.shape[2], decoder_out.max_step)
        g.load(encoder_out, decoder_out.output_tokens, decoder_out.output_scores, decoder_out.step)
        g.run(n_iters)
        return decoder_out._replace(output_tokens=g.tokens.long(), output_scores=g.scores.clone(), attn=None, step=decoder_out.step + n_iters)

    def guided_mask_predict(self, encoder_out, lengths, n_iters: int, cg_scale, null_token: int = 0, history: Optional[list] = None):
        """The decoding loop of research/TranSpeech/nat_gen.py:192-236 (scripts/s2ut/eval_cg.sh: the `nar_cg` model with --cg_scale):
        rows of `unk` for lengths[b] positions, then `eos`, then `pad` (prepare_batch :109-113); n_iters iterations of decoder pass(es) +
        update, the scores starting from zero in every iteration (:197); with guidance every iteration decodes the tokens against the
        speech encoder's output and against the null source (cg_forward: embed_tokens.weight[null_token] at every source position, no
        padding mask) and takes the arg-max of log_softmax(cond + cg_scale * (cond - null)).  cg_scale None or <= 0: the same loop
        without the null half (use_cg = cg_scale > 0, :179-181, :225).  encoder_out: the reference's encoder dict (forward_encoder's).
        -> tokens int64 [B, T], T = max(lengths) + 1.  history (a list) receives (tokens, scores, predicted) after every iteration."""
        ckv, slen = self._prepared(encoder_out)
        scale = float(cg_scale) if (cg_scale is not None and float(cg_scale) > 0) else None
        lengths = torch.as_tensor(lengths).to(self.device).long()
        B, T = lengths.numel(), int(lengths.max()) + 1
        assert ckv.shape[1] == B and int(lengths.min()) >= 1 and int(n_iters) >= 1
        idx = torch.arange(T, device=self.device)[None, :]
        tok = torch.full((B, T), self.pad, dtype=torch.int32, device=self.device)
        tok = tok.masked_fill(idx < lengths[:, None], self.unk).masked_fill(idx == lengths[:, None], self.eos)
        eng = self.engine
        if scale is not None:
            eng.null_cross(null_token)
        keep = lambda t, sc, pr: history.append((t.long().clone(), sc.clone(), pr.long().clone())) if history is not None else None
        if self.use_graph:
            g = self._graph_for(True, B, T, ckv.shape[2], n_iters, scale)
            g.load(encoder_out, tok)
            if history is None:
                g.run(int(n_iters))
            else:
                for _ in range(int(n_iters)):
                    g.run(1)
                    keep(g.tokens, g.scores, g.predicted)
            return g.tokens.long()
        scores = torch.zeros(B, T, dtype=torch.float32, device=self.device)
        predicted = torch.empty(B, T, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for step in range(int(n_iters)):
                args = (tok.data_ptr(), scores.data_ptr(), predicted.data_ptr(), B, T, eng.vocab, step, int(n_iters), int(self.unk), int(self.pad),
                        _lib.current_stream())
                if scale is not None:
                    logits = eng.forward_guided(tok, ckv, slen)
                    _lib.check(eng.lib.dn_cmlm_guided_step(logits.data_ptr(), scale, *args), "dn_cmlm_guided_step")
                else:
                    scores.zero_()
                    logits = eng.forward(tok, ckv, slen)
                    _lib.check(eng.lib.dn_cmlm_step(logits.data_ptr(), *args), "dn_cmlm_step")
                keep(tok, scores, predicted)
        return tok.long()

    def eval(self):
        return self

    def forward_encoder(self, encoder_inputs, sample_rate=None):
        """sample_rate: the rate of waveform input when it is not the fbank front end's own (resampled on the device first)."""
        return self.encoder(*encoder_inputs) if sample_rate is None else self.encoder(*encoder_inputs, sample_rate=sample_rate)

    def _prepared(self, enc):
        """The engine's view of an encoder output, cached in the dict: batch-major fp32 copy -> cross keys / values; source lengths."""
        if "_ckv" not in enc:
            x = enc["encoder_out"][0].to(self.device, torch.float32).transpose(0, 1).contiguous()  # [S,B,D] -> [B,S,D]
            S, B = enc["encoder_out"][0].shape[:2]
            pad = enc["encoder_padding_mask"][0] if len(enc["encoder_padding_mask"]) > 0 else None
            enc["_src_len"] = ((~pad).sum(1) if pad is not None else torch.full((B,), S)).to(self.device, torch.int32)
            enc["_ckv"] = self.engine.cross_kv(x)
            enc["_bsd"] = x
            enc["_src_id"] = next(_src_ids)
        return enc["_ckv"], enc["_src_len"]

    def initialize_output_tokens(self, encoder_out, src_lengths, true_length=None):
        """(:844-885): lengths from the predictor (or given), rows of `unk` padded with `pad`, zero scores."""
        self._prepared(encoder_out)
        if true_length is not None:
            lengths = true_length.to(self.device).long()
        else:
            lengths = self.engine.predict_lengths(encoder_out["_bsd"], encoder_out["_src_len"]).long()
        return DecoderOut(*self._blank(lengths), None, 0, 0, None)

    def _blank(self, lengths):
        lengths = lengths.clamp(min=2)
        idx = torch.arange(int(lengths.max()), device=lengths.device)
        tok = torch.full((lengths.size(0), idx.numel()), self.pad, dtype=torch.long, device=lengths.device)
        tok = tok.masked_fill(idx[None, :] < lengths[:, None], self.unk)
        return tok, torch.zeros(tok.shape, dtype=torch.float32, device=lengths.device)

    def regenerate_length_beam(self, decoder_out, beam_size):
        """(:887-912)."""
        lengths = decoder_out.output_tokens.ne(self.pad).sum(1)
        lengths = (lengths[:, None] + torch.arange(beam_size, device=lengths.device)[None, :] - beam_size // 2).view(-1)
        tok, sc = self._blank(lengths)
        return decoder_out._replace(output_tokens=tok, output_scores=sc)

    def forward_decoder(self, decoder_out, encoder_out, decoding_format=None, **kwargs):
        """(:791-842): one decoder pass (HIP engine) + the mask-predict update (dn_cmlm_step: arg-max of the log-softmax into the masked
        positions, then re-masking of the lowest-scoring ones unless this is the last iteration)."""
        ckv, slen = self._prepared(encoder_out)
        step, max_step, history = decoder_out.step, decoder_out.max_step, decoder_out.history
        if self.use_graph:
            B, T = decoder_out.output_tokens.shape
            g = self._graph_for(False, B, T, ckv.shape[2], max_step)
            g.load(encoder_out, decoder_out.output_tokens, decoder_out.output_scores, step)
            g.run(1)
            if history is not None:
                history.append(g.predicted.long())
                if (step + 1) < max_step:
                    history.append(g.tokens.long())
            return decoder_out._replace(output_tokens=g.tokens.long(), output_scores=g.scores.clone(), attn=None, history=history)
        tokens = decoder_out.output_tokens.to(self.device, torch.int32).contiguous()
        scores = decoder_out.output_scores.to(self.device, torch.float32).contiguous().clone()
        logits = self.engine.forward(tokens, ckv, slen)
        predicted, tokens = cmlm_update(logits, tokens, scores, step, max_step, self.unk, self.pad)
        if history is not None:
            history.append(predicted.long())
            if (step + 1) < max_step:
                history.append(tokens.long().clone())
        return decoder_out._replace(output_tokens=tokens.long(), output_scores=scores, attn=None, history=history)
