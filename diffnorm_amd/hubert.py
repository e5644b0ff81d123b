"""The mHuBERT front end of the recipe on the HIP engine: waveform -> layer features -> k-means units, what the reference's
scripts/prepare/feature_dump.sh (examples/textless_nlp/gslm/speech2unit/clustering/dump_feats.py ->
pretrained/hubert_feature_reader.py) and scripts/prepare/quantize_unit.sh (quantize_with_kmeans.py) write on CUDA.

`HubertEngine` is dn_hubert_* of libdiffnorm_hip.so (include/diffnorm_hip.h; csrc/hubert.hip): HubertModel.extract_features(source,
padding_mask=None, mask=False, output_layer=k) (fairseq/models/hubert/hubert.py:429-476, 529-545) in eval mode, with the reader's
contract that an utterance is run ALONE -- a batch gives every utterance exactly that.  `HubertFeatureReader` is the reader's chunk
loop over it, `KMeansQuantizer` the unit assignment, `dump_features` the `{split}.manifest.tsv` + `.npy` layout diffnorm_amd/data.py
reads.  Waveforms arrive as tensors or arrays at the model's sample rate, or at any other integer rate named with `sample_rate`,
which is converted on the device first (diffnorm_amd/resample.py); decoding audio files other than 16-bit PCM WAV is not done here.
"""
from types import SimpleNamespace
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, data, packing
from .engine import _dtype_code
from .nar_decoder import _NarEngine, _cat_proj, _conv_mat

MHUBERT_BASE = SimpleNamespace(conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", extractor_mode="default", conv_bias=False,
                               encoder_embed_dim=768, encoder_ffn_embed_dim=3072, encoder_layers=12, encoder_attention_heads=12, conv_pos=128,
                               conv_pos_groups=16, layer_norm_first=False, layer_type="transformer", required_seq_len_multiple=1,
                               activation_fn="gelu", normalize=False)
# The large form: a LayerNorm behind every (biased) conv, pre-norm layers, waveform normalisation in the task (wav2vec 2.0 large /
# LV-60 / XLSR and HuBERT large / xlarge's recipe; the widths here are the large ones)
_LARGE = dict(conv_feature_layers="[(512,10,5)] + [(512,3,2)] * 4 + [(512,2,2)] * 2", extractor_mode="layer_norm", conv_bias=True, encoder_embed_dim=1024,
              encoder_ffn_embed_dim=4096, encoder_layers=24, encoder_attention_heads=16, conv_pos=128, conv_pos_groups=16, layer_norm_first=True,
              layer_type="transformer", activation_fn="gelu", normalize=True)
WAV2VEC2_LARGE = SimpleNamespace(required_seq_len_multiple=2, **_LARGE)
HUBERT_LARGE = SimpleNamespace(required_seq_len_multiple=2, **dict(_LARGE, conv_bias=False))
_FIRST_KMAX = 16  # taps of the first conv the kernel holds (C0_KMAX in csrc/hubert.hip)
_LN_CMAX = 512    # conv width of the LayerNorm extractor's first-layer kernel (C0_LN_CMAX)


def conv_layers(cfg) -> List[Tuple[int, int, int]]:
    """cfg.conv_feature_layers, the reference's python-expression string (HubertModel.__init__ evaluates it) or a list -> [(dim, k,
    stride)].  The string is evaluated (without builtins: `[..] + [..] * 4` is no literal), so a configuration is TRUSTED input, as it
    is upstream."""
    spec = cfg.conv_feature_layers
    if isinstance(spec, str):
        spec = eval(spec, {"__builtins__": {}})  # the reference's own format: a list expression of int tuples
    return [tuple(int(v) for v in cl) for cl in spec]


def check_hubert_args(cfg) -> None:
    """What of HubertModel's / Wav2Vec2Model's variants the engine runs, each as a whole: the base form (extractor_mode 'default',
    post-norm layers, nothing else) exactly as before, and the large form (extractor_mode 'layer_norm' WITH layer_norm_first; with
    them conv_bias, task normalize and any required_seq_len_multiple, whose appended frames are masked keys that are cut off again).
    These are the forms released checkpoints have and the goldens pin; a single large-form property on the base form is no model
    anyone has and stays refused here, on the host, as does everything else."""
    g = lambda k, d: getattr(cfg, k, d)
    if g("extractor_mode", "default") not in ("default", "layer_norm"):
        raise ValueError(f"hubert: extractor_mode {cfg.extractor_mode!r} is not supported, only 'default' and 'layer_norm'")
    large = g("extractor_mode", "default") == "layer_norm"
    if bool(g("layer_norm_first", False)) != large:
        raise ValueError(f"hubert: extractor_mode {g('extractor_mode', 'default')!r} with layer_norm_first={bool(g('layer_norm_first', False))} is not supported: "
                         "a LayerNorm behind every conv and pre-norm layers go together (the large form)")
    if g("conv_bias", False) and not large:
        raise ValueError("hubert: conv_bias=True is supported in the large form only (extractor_mode 'layer_norm' with layer_norm_first)")
    if g("layer_type", "transformer") != "transformer":
        raise ValueError(f"hubert: layer_type {cfg.layer_type!r} is not supported, only 'transformer'")
    if int(g("required_seq_len_multiple", 1)) < 1 or (int(g("required_seq_len_multiple", 1)) != 1 and not large):
        raise ValueError("hubert: required_seq_len_multiple must be 1 in the base form (at least 1 in the large form)")
    if g("normalize", False) and not large:
        raise ValueError("hubert: task normalize=True (waveform layer_norm in the reader) is supported in the large form only")
    if g("activation_fn", "gelu") != "gelu":
        raise ValueError(f"hubert: activation_fn {cfg.activation_fn!r} is not supported, only 'gelu'")
    if g("pos_conv_depth", 1) != 1:
        raise ValueError("hubert: pos_conv_depth > 1 is not supported")
    if g("training", False) or g("mask", False):
        raise ValueError("hubert: training and masking are not supported: this is the feature reader's eval pass")
    layers = conv_layers(cfg)
    if not 2 <= len(layers) <= 8 or len({d for d, _, _ in layers}) != 1:
        raise ValueError("hubert: 2 .. 8 conv layers of one width are supported")
    if layers[0][1] > _FIRST_KMAX or layers[0][2] > 8:
        raise ValueError(f"hubert: first conv kernel {layers[0][1]} (<= {_FIRST_KMAX}) / stride {layers[0][2]} (<= 8)")
    if g("extractor_mode", "default") == "layer_norm" and layers[0][0] > _LN_CMAX:
        raise ValueError(f"hubert: extractor_mode 'layer_norm' with conv width {layers[0][0]} (<= {_LN_CMAX})")


def out_frames(cfg, L: int) -> int:
    """Wav2Vec2Model._get_feat_extract_output_lengths (wav2vec2.py:564-579) for one length; 0 when L gives no frame."""
    for _, k, s in conv_layers(cfg):
        L = (L - k) // s + 1 if L >= k else 0
    return L


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """nn.utils.weight_norm(conv, name="weight", dim=2) (make_conv_pos, wav2vec2.py:912): w = g v / |v|, the norm over every
    dimension but 2, in float64."""
    v = v.double()
    return g.double() * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()


def pos_conv_weight(sd) -> torch.Tensor:
    """The positional conv's effective weight [dim, dim / groups, k] in float64 from either parametrisation of the weight-norm."""
    p = "encoder.pos_conv.0."
    if p + "weight_g" in sd:
        return fold_weight_norm(sd[p + "weight_g"], sd[p + "weight_v"])
    if p + "parametrizations.weight.original0" in sd:
        return fold_weight_norm(sd[p + "parametrizations.weight.original0"], sd[p + "parametrizations.weight.original1"])
    return sd[p + "weight"].double()


def pack_hubert(sd: Dict[str, torch.Tensor], cfg, dtype: int) -> List[torch.Tensor]:
    """HubertModel.state_dict() under the reference's key names -> the tensor table of dn_hubert_create (include/diffnorm_hip.h).
    Pre-training leftovers (mask_emb, final_proj, label_embs_concat) are ignored."""
    check_hubert_args(cfg)
    dtype = _dtype_code(dtype)
    layers = conv_layers(cfg)
    Cw, D, G, kp, nl = layers[0][0], cfg.encoder_embed_dim, cfg.conv_pos_groups, cfg.conv_pos, cfg.encoder_layers
    g = lambda k: sd[k].float()
    mat = lambda w: packing._mat(w, dtype, cols=w.shape[1])
    stack = lambda items: torch.stack(items).contiguous()
    has_proj = "post_extract_proj.weight" in sd  # (absent when the conv width is the embed width, hubert.py:264-268)
    if not has_proj and Cw != D:
        raise ValueError(f"hubert: no post_extract_proj in the state dict but conv width {Cw} != embed width {D}")
    ext_ln, conv_bias = getattr(cfg, "extractor_mode", "default") == "layer_norm", bool(getattr(cfg, "conv_bias", False))
    if any(k.startswith("feature_extractor.conv_layers.") and k.endswith(".0.bias") for k in sd) != conv_bias:
        raise ValueError(f"hubert: conv biases in the state dict do not agree with conv_bias={conv_bias}")
    if ("feature_extractor.conv_layers.1.2.1.weight" in sd) != ext_ln:
        raise ValueError(f"hubert: the state dict {'lacks' if ext_ln else 'has'} the LayerNorm behind conv layer 1 (extractor_mode 'layer_norm') but "
                         f"cfg.extractor_mode is {'layer_norm' if ext_ln else 'default'!r}")
    w0 = g("feature_extractor.conv_layers.0.0.weight")
    assert w0.shape == (Cw, 1, layers[0][1]), w0.shape
    conv0 = torch.zeros(_FIRST_KMAX, Cw)
    conv0[: layers[0][1]] = w0[:, 0, :].t()
    n0 = "feature_extractor.conv_layers.0.2.1." if ext_ln else "feature_extractor.conv_layers.0.2."
    out = [conv0, g(n0 + "weight").contiguous(), g(n0 + "bias").contiguous()]
    for i, (_, k, _) in enumerate(layers[1:], 1):
        w = g(f"feature_extractor.conv_layers.{i}.0.weight")
        assert w.shape == (Cw, Cw, k), w.shape
        out.append(_conv_mat(w, dtype))
    w = pos_conv_weight(sd)
    assert w.shape == (D, D // G, kp), w.shape
    pos_w = w.view(G, D // G, D // G, kp).permute(0, 3, 2, 1).contiguous().float()  # [g][co][ci][j] -> [g][j][ci][co]
    out += [g("layer_norm.weight").contiguous(), g("layer_norm.bias").contiguous(), mat(g("post_extract_proj.weight") if has_proj else torch.zeros(D, Cw)),
            g("post_extract_proj.bias").contiguous() if has_proj else torch.zeros(D), pos_w, g("encoder.pos_conv.0.bias").contiguous(), g("encoder.layer_norm.weight").contiguous(),
            g("encoder.layer_norm.bias").contiguous()]
    qkv_W, qkv_b, so_W, so_b, f1W, f1b, f2W, f2b, lng, lnb = ([] for _ in range(10))
    for l in range(nl):
        p = f"encoder.layers.{l}."
        W, b = _cat_proj(sd, p + "self_attn.", ("q_proj", "k_proj", "v_proj"))
        qkv_W.append(mat(W)); qkv_b.append(b)
        so_W.append(mat(g(p + "self_attn.out_proj.weight"))); so_b.append(g(p + "self_attn.out_proj.bias"))
        f1W.append(mat(g(p + "fc1.weight"))); f1b.append(g(p + "fc1.bias"))
        f2W.append(mat(g(p + "fc2.weight"))); f2b.append(g(p + "fc2.bias"))
        lng.append(torch.stack([g(p + "self_attn_layer_norm.weight"), g(p + "final_layer_norm.weight")]))
        lnb.append(torch.stack([g(p + "self_attn_layer_norm.bias"), g(p + "final_layer_norm.bias")]))
    out = out + [stack(t) for t in (qkv_W, qkv_b, so_W, so_b, f1W, f1b, f2W, f2b, lng, lnb)] + [torch.zeros(Cw)]
    if ext_ln:  # per conv layer: bias (zeros without conv_bias), LayerNorm weight and bias
        ce = "feature_extractor.conv_layers.{}.{}"
        out += [stack([g(ce.format(i, "0.bias")) if conv_bias else torch.zeros(Cw) for i in range(len(layers))]),
                stack([g(ce.format(i, "2.1.weight")) for i in range(len(layers))]), stack([g(ce.format(i, "2.1.bias")) for i in range(len(layers))])]
    return out


def pack_ctc_head(weight: torch.Tensor, bias: torch.Tensor) -> List[torch.Tensor]:
    """Wav2VecEncoder.proj (Linear(dim -> V)) -> the two entries behind pack_hubert's table: the fp32 weight (the head runs the
    DN_F32 contraction in every mode) with zero rows up to the contraction's packed height, the bias with zeros up to a multiple of 4
    (columns the engine never copies into the emissions)."""
    V = weight.shape[0]
    return [packing._mat(weight.float(), _lib.DN_F32, cols=weight.shape[1]), packing._vec(bias, (V + 3) // 4 * 4)]


def hubert_config(cfg, dtype: int, has_proj: bool, vocab: int = 0) -> "_lib.HubertConfig":
    """cfg -> DnHubertConfig (include/diffnorm_hip.h)."""
    layers = conv_layers(cfg)
    c = _lib.HubertConfig()
    c.n_conv, c.conv_dim = len(layers), layers[0][0]
    for i, (_, k, s) in enumerate(layers):
        c.conv_kernel[i], c.conv_stride[i] = k, s
    c.dim, c.ffn, c.layers, c.heads = cfg.encoder_embed_dim, cfg.encoder_ffn_embed_dim, cfg.encoder_layers, cfg.encoder_attention_heads
    c.conv_pos, c.conv_pos_groups, c.dtype, c.has_proj = cfg.conv_pos, cfg.conv_pos_groups, dtype, int(has_proj)
    c.wave_norm, c.extractor_ln = int(bool(getattr(cfg, "normalize", False))), int(getattr(cfg, "extractor_mode", "default") == "layer_norm")
    c.conv_bias, c.pre_norm, c.vocab = int(bool(getattr(cfg, "conv_bias", False))), int(bool(getattr(cfg, "layer_norm_first", False))), int(vocab)
    return c


def _as_wave(w) -> torch.Tensor:
    w = torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).float()
    if w.dim() != 1:
        raise ValueError(f"a waveform is one row of samples, got shape {tuple(w.shape)}")
    return w


class HubertEngine(_NarEngine):
    """dn_hubert_* of libdiffnorm_hip.so.  dtype 'f32', 'bf16x3', 'f16' or 'bf16': the arithmetic of the contractions and of the
    attention; the first conv's statistics, the positional conv and the norms are fp32 in every mode."""
    _sym = "hubert"

    def __init__(self, state_dict, cfg=MHUBERT_BASE, dtype="f16", device="cuda:0"):
        self.cfg, self.dim = cfg, cfg.encoder_embed_dim
        self.dtype = _dtype_code(dtype)
        self._create(device, pack_hubert(state_dict, cfg, self.dtype), hubert_config(cfg, self.dtype, "post_extract_proj.weight" in state_dict))

    def out_frames(self, L: int) -> int:
        return int(self.lib.dn_hubert_out_frames(self.handle, int(L)))

    STAGES = ("first conv + GroupNorm", "conv layers 1..", "layer_norm + proj + pos_conv", "transformer layers", "output copy")

    def set_profile(self, on: bool) -> None:
        """Stage timing of the following forwards (dn_hubert_set_profile); read with stage_times()."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_hubert_set_profile(self.handle, int(on)), "dn_hubert_set_profile")

    def stage_times(self) -> List[float]:
        """ms per stage (STAGES) of the last profiled forward; waits for it."""
        import ctypes as C

        ms = (C.c_float * len(self.STAGES))()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_hubert_stage_times(self.handle, ms, len(self.STAGES)), "dn_hubert_stage_times")
        return list(ms)

    def _inputs(self, wave: torch.Tensor, lengths):
        """The checks and device copies both passes share -> (wave, lengths int32, S, (workspace pointer, bytes))."""
        B, L = wave.shape
        lengths = torch.as_tensor(lengths)
        if lengths.device.type == "cpu" and (out_frames(self.cfg, int(lengths.min())) < 1 or int(lengths.max()) > L):
            raise ValueError(f"HubertEngine.forward: lengths {lengths.tolist()} (each must give at least one frame and fit the {L} samples)")
        S = self.out_frames(L)
        if S < 1:
            raise ValueError(f"HubertEngine.forward: {L} samples are shorter than one frame of the conv stack")
        wave = wave.to(self.device, torch.float32).contiguous()
        ln = lengths.to(self.device, torch.int32).contiguous()
        return wave, ln, S, self._aligned(self._workspace(int(self.lib.dn_hubert_workspace_bytes(self.handle, B, L))))

    def forward(self, wave: torch.Tensor, lengths, layer: int):
        """wave [B, L] (anything behind an utterance's samples), lengths [B], layer = output_layer (1-based) -> (features fp32
        [B, S, dim] with zero rows behind each utterance's frames, frame counts int32 [B]).  In the pre-norm form this is the
        un-normalised stream for every layer, as HubertModel.extract_features(output_layer=k) hands TransformerEncoder a layer."""
        B, L = wave.shape
        wave, ln, S, (wp, wn) = self._inputs(wave, lengths)
        out = torch.empty(B, S, self.dim, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_hubert_forward(self.handle, wave.data_ptr(), ln.data_ptr(), B, L, int(layer), out.data_ptr(), lens.data_ptr(), wp, wn,
                                                  _lib.current_stream()), "dn_hubert_forward")
        return out, lens


def _resampler_of(owner, cfg, device, sample_rate):
    """owner's cached Resampler from `sample_rate` to cfg's own rate (16 000 where cfg carries none); None: nothing to convert."""
    if sample_rate is None:
        return None
    if getattr(owner, "_resamplers", None) is None:
        from .resample import ResamplerCache

        owner._resamplers = ResamplerCache(getattr(cfg, "sample_rate", 16000), device)
    return owner._resamplers.get(sample_rate)


def _resampled(rs, waves: Sequence) -> Sequence:
    """The waveforms as they are (rs None), or each one's own samples of the resampled batch, on the device."""
    if rs is None:
        return waves
    out, lens = rs.forward(list(waves))
    return [out[i, :n] for i, n in enumerate(lens.tolist())]


def chunk_bounds(n: int, max_chunk: int) -> List[Tuple[int, int]]:
    """The reader's chunk loop (hubert_feature_reader.py:52-53): [start, start + max_chunk) over n samples."""
    return [(s, min(s + max_chunk, n)) for s in range(0, n, max_chunk)]


class HubertFeatureReader:
    """HubertFeatureReader of the reference (hubert_feature_reader.py:12-64) over HubertEngine: features of layer `layer`, the waveform
    cut into chunks of max_chunk samples that are run independently and concatenated."""

    def __init__(self, state_dict, cfg=MHUBERT_BASE, layer: int = 11, max_chunk: int = 1_600_000, dtype="f16", device="cuda:0", engine=None):
        check_hubert_args(cfg)
        if not 1 <= layer <= cfg.encoder_layers:
            raise ValueError(f"layer {layer} outside 1 .. {cfg.encoder_layers}")
        self.cfg, self.layer, self.max_chunk = cfg, layer, int(max_chunk)
        self.engine = engine if engine is not None else HubertEngine(state_dict, cfg, dtype=dtype, device=device)
        self._resamplers = None

    def resampler(self, sample_rate):
        """The cached Resampler from `sample_rate` to the model's rate (cfg.sample_rate, 16 000 where the config carries none); None
        when there is nothing to convert."""
        return None if sample_rate is None else _resampler_of(self, self.cfg, self.engine.device, sample_rate)

    def _check_chunks(self, n: int):
        bounds = chunk_bounds(n, self.max_chunk)
        if len(bounds) > 1 and getattr(self.cfg, "normalize", False):
            # the reference normalises the WHOLE waveform once and cuts it afterwards (hubert_feature_reader.py:47-53); the engine
            # takes its statistics per forward call, so a chunk would be normalised over its own samples
            raise ValueError(f"a waveform of {n} samples is more than one chunk of {self.max_chunk}: with task normalize=True the statistics "
                             "belong to the whole waveform, which the chunk loop does not carry; raise max_chunk")
        for s, e in bounds:
            if out_frames(self.cfg, e - s) < 1:
                raise ValueError(f"a chunk of {e - s} samples (at {s} of {n}) is shorter than one frame of the conv stack")
        return bounds

    def get_feats(self, wave, sample_rate=None) -> torch.Tensor:
        """One waveform [n] -> features [T, dim] on the engine's device."""
        return self.get_feats_batch([wave], sample_rate=sample_rate)[0]

    def get_feats_batch(self, waves: Sequence, sample_rate=None) -> List[torch.Tensor]:
        """A ragged batch of waveforms, one chunk round at a time: round r runs chunk r of every waveform that has one as one batch.
        sample_rate: the waveforms' rate when it is not the model's -- they are resampled on the device first ([n] or [n, C], fp32 or
        int16, as Resampler.forward takes them) and the chunk loop runs over the resampled waveforms, as the reference's reader
        sees audio its loader has already converted."""
        waves = _resampled(self.resampler(sample_rate), waves)
        waves = [_as_wave(w) for w in waves]
        bounds = [self._check_chunks(w.numel()) for w in waves]
        parts: List[List[torch.Tensor]] = [[] for _ in waves]
        for r in range(max(len(b) for b in bounds)):
            idx = [i for i, b in enumerate(bounds) if r < len(b)]
            chunks = [waves[i][bounds[i][r][0]: bounds[i][r][1]] for i in idx]
            lens = torch.tensor([c.numel() for c in chunks], dtype=torch.int32)
            batch = torch.zeros(len(chunks), int(lens.max()))
            for j, c in enumerate(chunks):
                batch[j, : c.numel()] = c
            out, _ = self.engine.forward(batch, lens, self.layer)
            for j, i in enumerate(idx):
                parts[i].append(out[j, : out_frames(self.cfg, int(lens[j]))])
        return [torch.cat(p, 0) for p in parts]


def kmeans_scores_tables(centers) -> Tuple[torch.Tensor, torch.Tensor]:
    """centers [n, D] -> (the packed fp32 centroid matrix [n -> multiple of 128, D], -|c|^2 / 2 as fp32 [n -> multiple of 4]), the
    norms in float64: argmax_j (x . c_j - |c_j|^2 / 2) = argmin_j |x - c_j|^2."""
    c = torch.as_tensor(np.asarray(centers) if not isinstance(centers, torch.Tensor) else centers).double()
    n = c.shape[0]
    half = torch.zeros((n + 3) // 4 * 4, dtype=torch.float64)
    half[:n] = -0.5 * c.pow(2).sum(1)
    return packing._mat(c.float(), _lib.DN_F32, cols=c.shape[1]), half.float()


class KMeansQuantizer:
    """ApplyKmeans (examples/hubert/simple_kmeans/dump_km_label.py:20-53) / sklearn's predict on the device: dn_kmeans_assign."""

    def __init__(self, centers, device="cuda:0"):
        from .engine import _require_cuda

        self.device = _require_cuda(device)
        self.lib = _lib.load()
        C_, h = kmeans_scores_tables(centers)
        self.n, self.D = len(centers), C_.shape[1]
        if self.D % 32:
            raise ValueError(f"KMeansQuantizer: feature width {self.D} must be a multiple of 32")
        self.centers, self.half = C_.to(self.device).contiguous(), h.to(self.device).contiguous()

    def predict(self, feats: torch.Tensor) -> torch.Tensor:
        """feats [M, D] -> units int32 [M] on the device."""
        feats = torch.as_tensor(feats).to(self.device, torch.float32).contiguous()
        M, D = feats.shape
        assert D == self.D, (D, self.D)
        units = torch.empty(M, dtype=torch.int32, device=self.device)
        if M == 0:
            return units
        ws = _lib.alloc_workspace(self.lib.dn_kmeans_workspace_bytes(M, self.n), self.device)
        wp, wn = _lib.aligned(ws)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_kmeans_assign(feats.data_ptr(), self.centers.data_ptr(), self.half.data_ptr(), M, D, self.n, units.data_ptr(), wp,
                                                 wn, _lib.current_stream()), "dn_kmeans_assign")
        return units


def dump_features(reader: HubertFeatureReader, items: Iterable[Tuple[str, object]], out_features_path: str, batch: int = 8, sample_rate=None) -> str:
    """(file id, waveform) pairs -> `{out_features_path}/{id}.feat.npy` and the `{split}.manifest.tsv` beside it, through
    data.write_feature_manifest: the layout load_samples / load_normalization_inputs read.  Returns the manifest path.
    sample_rate: the waveforms' rate when it is not the model's (get_feats_batch resamples each group on the device)."""
    items = list(items)
    rate = {} if sample_rate is None else {"sample_rate": sample_rate}  # (a reader without the keyword keeps working at its own rate)

    def feats():
        for s in range(0, len(items), batch):
            group = items[s: s + batch]
            for (fid, _), f in zip(group, reader.get_feats_batch([w for _, w in group], **rate)):
                yield fid, f.cpu().numpy()

    return data.write_feature_manifest(out_features_path, feats())
