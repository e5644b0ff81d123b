"""CodeHiFiGAN unit vocoder on the HIP library: discrete units -> 16 kHz waveform, batched.

The last stage of the reference's unit pipelines (research/TranSpeech/nat_gen.py:58-66 `vocoder_inference`, scripts/s2ut/eval.sh,
eval_cg.sh): `CodeHiFiGANVocoder` (fairseq/models/text_to_speech/vocoder.py:214-235) = `CodeGenerator` (codehifigan.py) over the
HiFiGAN `Generator` (hifigan.py) with the FastSpeech 2 `VariancePredictor` as duration predictor (fastspeech2.py:117-151).
Single-speaker, no f0: the configuration the public mHuBERT unit vocoders ship with.  Kernels: csrc/vocoder.hip (dn_voc_*).

    voc = CodeHiFiGANVocoder("g_00500000", json.load(open("config.json")), dtype="f16")
    wav = voc({"code": units[None]}, dur_prediction=True)              # the reference's contract: one utterance, 1-D waveform
    wavs = voc.generate([u0, u1, u2], dur_prediction=True)             # ragged batch; each equals forward() on it alone
"""
import ctypes as C
from typing import Dict, List, Optional, Sequence, Union

import torch

from . import _lib
from .engine import _Engine, _dtype_code

_KNOWN_KEYS = {"code", "dur_prediction"}


# ------------------------------------------------------------------------------------------------ host-side checks
def check_config(cfg: dict) -> None:
    """Refuses what the engine does not compute (ValueError), before any device work."""
    if cfg.get("multispkr"):
        raise ValueError("CodeHiFiGAN: multispkr (speaker-conditioned) vocoders are not supported")
    if cfg.get("embedder_params"):
        raise ValueError("CodeHiFiGAN: embedder_params (speaker embedder) is not supported")
    if cfg.get("f0") or cfg.get("f0_quant_num_bin"):
        raise ValueError("CodeHiFiGAN: f0-conditioned vocoders are not supported")
    if cfg.get("model_in_dim", cfg["embedding_dim"]) != cfg["embedding_dim"]:
        raise ValueError(f"CodeHiFiGAN: model_in_dim {cfg.get('model_in_dim')} != embedding_dim {cfg['embedding_dim']}: extra conditioning channels are not supported")
    dp = cfg.get("dur_predictor_params")
    if dp:
        if dp.get("var_pred_kernel_size", 3) != 3:
            raise ValueError(f"CodeHiFiGAN: var_pred_kernel_size {dp['var_pred_kernel_size']} != 3 (the reference's second conv pads by 1 whatever the size)")
        if dp.get("encoder_embed_dim", cfg["embedding_dim"]) != cfg["embedding_dim"]:
            raise ValueError("CodeHiFiGAN: dur_predictor_params.encoder_embed_dim != embedding_dim")
    if len(cfg["upsample_rates"]) != len(cfg["upsample_kernel_sizes"]):
        raise ValueError("CodeHiFiGAN: upsample_rates and upsample_kernel_sizes differ in length")
    for k, u in zip(cfg["upsample_kernel_sizes"], cfg["upsample_rates"]):
        if k < u or (k - u) % 2:
            raise ValueError(f"CodeHiFiGAN: transposed conv k = {k}, u = {u}: k - u must be even and >= 0 (its output is then exactly L * u frames)")
        if k > 3 * u:
            raise ValueError(f"CodeHiFiGAN: transposed conv k = {k}, u = {u}: k > 3 u reaches beyond the neighbouring input frames")
    for d in cfg["resblock_dilation_sizes"]:
        if len(d) != 3:
            raise ValueError("CodeHiFiGAN: a ResBlock has three dilations")


def check_inputs(x: dict) -> None:
    if "code" not in x:
        raise ValueError('CodeHiFiGAN: x needs "code"')
    extra = sorted(set(x) - _KNOWN_KEYS)
    if extra:
        raise ValueError(f"CodeHiFiGAN: conditioning inputs {extra} are not supported (single-speaker, no f0)")


def check_dur_prediction(cfg: dict, dur_prediction: bool) -> None:
    if dur_prediction and not cfg.get("dur_predictor_params"):
        raise ValueError("CodeHiFiGAN: dur_prediction needs a model with dur_predictor_params")


def check_frames(frames: torch.Tensor, upsample: int) -> None:
    """The per-utterance frame counts read back from the device (a sum that would overflow comes back saturated at 2^31 - 1)."""
    lo, hi = int(frames.min()), int(frames.max())
    if lo < 1 or hi * upsample >= 2 ** 31:
        raise ValueError(f"CodeHiFiGAN: an utterance of {lo if lo < 1 else hi} frames (x {upsample} samples) is empty or overflows int32: the "
                         "duration predictor's output is not usable")


def clean_units(code: torch.Tensor, num_embeddings: int) -> torch.Tensor:
    """One utterance's units: negative codes dropped (vocoder.py:232-233), the rest checked against the dictionary."""
    code = torch.as_tensor(code).reshape(-1).cpu().long()
    code = code[code >= 0]
    if code.numel() == 0:
        raise ValueError("CodeHiFiGAN: empty utterance (no code >= 0)")
    if int(code.max()) >= num_embeddings:
        raise ValueError(f"CodeHiFiGAN: code {int(code.max())} >= num_embeddings {num_embeddings}")
    return code.int()


# ------------------------------------------------------------------------------------------------ packing
def fold_weight_norm(sd: Dict[str, torch.Tensor], name: str) -> torch.Tensor:
    """`name`.weight from either form, in fp32.  weight_norm's default dim = 0 keeps one gain per slice of the FIRST axis: the
    out-channel of a Conv1d [out, in, k] and the in-channel of a ConvTranspose1d [in, out, k]; both fold as v * (g / ||v||_(1,2)),
    by the function remove_weight_norm itself applies."""
    if name + ".weight" in sd:
        return sd[name + ".weight"].float()
    g, v = sd[name + ".weight_g"].float(), sd[name + ".weight_v"].float()
    return torch._weight_norm(v, g, 0)


def polyphase(w: torch.Tensor, bias: Optional[torch.Tensor], u: int):
    """ConvTranspose1d(C_in, C_out, k, stride u, padding (k - u) / 2) weight [C_in, C_out, k] -> the 3-tap Conv1d weight
    [u * C_out, C_in, 3] whose [L, u * C_out] output is the [L * u, C_out] result: output frame s u + r reads input frame s + delta
    through tap j = r + p - delta u, delta = -1, 0, 1; phases without such a tap keep zeros.  The bias repeats per phase."""
    C_in, C_out, k = w.shape
    if k < u or (k - u) % 2:
        raise ValueError(f"polyphase: k = {k}, u = {u}: k - u must be even and >= 0")
    if k > 3 * u:
        raise ValueError(f"polyphase: k = {k} > 3 u = {3 * u}")
    p = (k - u) // 2
    out = w.new_zeros(u * C_out, C_in, 3)
    for r in range(u):
        for delta in (-1, 0, 1):
            j = r + p - delta * u
            if 0 <= j < k:
                out[r * C_out:(r + 1) * C_out, :, delta + 1] = w[:, :, j].t()
    return out, (None if bias is None else bias.repeat(u))


def pack_conv_weight(w: torch.Tensor, dtype: int) -> torch.Tensor:
    """Conv1d weight [C_out, C_in, k] -> the operand of dn_voc_conv (include/diffnorm_hip.h): [ceil16(C_out)][passes][(tap, channel)
    of the pass, zero-padded to the MFMA k-step] in half (DN_F16) or fp32."""
    C_out, C_in, k = w.shape
    if dtype not in (_lib.DN_F32, _lib.DN_F16):
        raise ValueError("the vocoder runs in f32 or f16 (bf16 / bf16x3 are refused: eight significand bits are no audio arithmetic)")
    if C_in % 16 or (C_in > 128 and C_in % 128):
        raise ValueError(f"pack_conv_weight: C_in = {C_in} must be a multiple of 16 (of 128 beyond 128)")
    ck = min(C_in, 128)
    ks = 32 if dtype == _lib.DN_F16 else 16
    per = -(-k * ck // ks) * ks
    out = torch.zeros(-(-C_out // 16) * 16, C_in // ck, per, dtype=torch.float32)
    for c in range(C_in // ck):
        out[:C_out, c, :k * ck] = w[:, c * ck:(c + 1) * ck, :].float().permute(0, 2, 1).reshape(C_out, k * ck)
    out = out.reshape(out.shape[0], -1)
    return (out.half() if dtype == _lib.DN_F16 else out).contiguous()


def _dtype(dtype) -> int:
    code = dtype if isinstance(dtype, int) else _dtype_code(dtype)
    if code not in (_lib.DN_F32, _lib.DN_F16):
        raise ValueError("the vocoder runs in f32 or f16 (bf16 / bf16x3 are refused: eight significand bits are no audio arithmetic)")
    return code


def pack_vocoder(sd: Dict[str, torch.Tensor], cfg: dict, dtype) -> List[torch.Tensor]:
    """Generator state dict (weight-norm pairs or folded weights) -> the tensor table of dn_voc_create."""
    check_config(cfg)
    dt = _dtype(dtype)
    f = lambda k: sd[k].float().contiguous()
    conv = lambda name, d=dt: [pack_conv_weight(fold_weight_norm(sd, name), d), f(name + ".bias")]
    out = [f("dict.weight")] + conv("conv_pre")
    nk = len(cfg["resblock_kernel_sizes"])
    for i, u in enumerate(cfg["upsample_rates"]):
        w3, b3 = polyphase(fold_weight_norm(sd, f"ups.{i}"), f(f"ups.{i}.bias"), u)
        out += [pack_conv_weight(w3, dt), b3.contiguous()]
        for j in range(nk):
            for m in range(3):
                out += conv(f"resblocks.{i * nk + j}.convs1.{m}") + conv(f"resblocks.{i * nk + j}.convs2.{m}")
    out += conv("conv_post")
    if cfg.get("dur_predictor_params"):
        p = "dur_predictor."
        out += conv(p + "conv1.0", _lib.DN_F32) + [f(p + "ln1.weight"), f(p + "ln1.bias")]
        out += conv(p + "conv2.0", _lib.DN_F32) + [f(p + "ln2.weight"), f(p + "ln2.bias")]
        out += [f(p + "proj.weight").reshape(-1).contiguous(), f(p + "proj.bias").reshape(-1).contiguous()]
    return out


def voc_config(cfg: dict, dtype: int) -> "_lib.VocConfig":
    c = _lib.VocConfig()
    c.embedding_dim, c.num_embeddings, c.initial_channel = cfg["embedding_dim"], cfg["num_embeddings"], cfg["upsample_initial_channel"]
    ups, ks, rk, rd = cfg["upsample_rates"], cfg["upsample_kernel_sizes"], cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    if len(ups) > 8 or len(rk) > 4 or len(rd) != len(rk):
        raise ValueError("CodeHiFiGAN: at most 8 upsampling stages and 4 ResBlock kernels, one dilation triple per kernel")
    c.n_ups, c.n_kernels = len(ups), len(rk)
    for i, (u, k) in enumerate(zip(ups, ks)):
        c.up_rates[i], c.up_kernels[i] = u, k
    for j, (k, d) in enumerate(zip(rk, rd)):
        c.res_kernels[j] = k
        for m in range(3):
            c.res_dilations[j][m] = d[m]
    dp = cfg.get("dur_predictor_params")
    c.dur_hidden = dp["var_pred_hidden_dim"] if dp else 0
    c.dtype = dtype
    return c


# ------------------------------------------------------------------------------------------------ operator-level entry
def voc_conv(x, w, bias, lengths, k, d=1, dtype="f32", slope=1.0, post=_lib.VOC_POST_NONE, res=None, out=None, div=1.0):
    """dn_voc_conv on caller tensors: x fp32 [B, Lmax, C_in] (cuda), w the Conv1d weight [C_out, C_in, k] (packed here), lengths [B]."""
    lib = _lib.load()
    dt = _dtype(dtype)
    B, Lmax, C_in = x.shape
    C_out = w.shape[0]
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and w.shape[1] == C_in and w.shape[2] == k
    wp = pack_conv_weight(w.cpu(), dt).to(x.device)
    assert wp.numel() == lib.dn_voc_conv_weight_elems(dt, C_in, C_out, k), "packed weight does not match the library's layout"
    ln = lengths.to(x.device, torch.int32).contiguous()
    b = None if bias is None else bias.to(x.device, torch.float32).contiguous()
    if out is None:
        out = torch.zeros(B, Lmax, C_out, dtype=torch.float32, device=x.device)
    p = _lib.VocConvParams(_lib.ptr(x), _lib.ptr(wp), _lib.ptr(b), _lib.ptr(res), _lib.ptr(out), _lib.ptr(ln), B, Lmax, C_in, C_out, k, d, C_in,
                           out.shape[2], 0 if res is None else res.shape[2], dt, post, slope, div)
    with torch.cuda.device(x.device):
        _lib.check(lib.dn_voc_conv(C.byref(p), _lib.current_stream()), "dn_voc_conv")
    return out


# ------------------------------------------------------------------------------------------------ engine
class CodeHiFiGANEngine(_Engine):
    """dn_voc_* of libdiffnorm_hip.so over padded unit batches: codes int32 [B, Tmax] + lengths."""

    def __init__(self, state_dict, cfg: dict, dtype="f16", device="cuda:0"):
        check_config(cfg)
        self.cfg, self.dtype = cfg, _dtype(dtype)
        super().__init__(device, pack_vocoder(state_dict, cfg, self.dtype))
        c = voc_config(cfg, self.dtype)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_voc_create(C.byref(c), self._table, len(self.tensors), C.byref(self.handle)), "dn_voc_create")
        self.upsample = int(self.lib.dn_voc_upsample(self.handle))

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.dn_voc_destroy(self.handle)
            self.handle.value = None  # in place: whoever holds the handle sees it cleared

    def _ws_for(self, B, L):
        return self._aligned(self._workspace(int(self.lib.dn_voc_workspace_bytes(self.handle, B, L))))

    def durations(self, codes: torch.Tensor, lengths: torch.Tensor):
        """-> (durations int32 [B, Tmax], their per-row sums int32 [B]), both on the device."""
        B, T = codes.shape
        assert codes.dtype == torch.int32 and codes.is_contiguous() and codes.device == self.device
        dur = torch.empty(B, T, dtype=torch.int32, device=self.device)
        sums = torch.empty(B, dtype=torch.int32, device=self.device)
        wp, wn = self._ws_for(B, T)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_voc_durations(self.handle, codes.data_ptr(), lengths.data_ptr(), B, T, dur.data_ptr(), sums.data_ptr(), wp, wn,
                                                 _lib.current_stream()), "dn_voc_durations")
        return dur, sums

    def forward(self, codes: torch.Tensor, lengths: torch.Tensor, durations: Optional[torch.Tensor], Lmax0: int):
        """-> (wav fp32 [B, Lmax0 * upsample], wav_lengths int32 [B]); samples behind a row's length are zero."""
        B, T = codes.shape
        assert codes.dtype == torch.int32 and codes.is_contiguous() and codes.device == self.device and lengths.dtype == torch.int32
        wav = torch.zeros(B, Lmax0 * self.upsample, dtype=torch.float32, device=self.device)
        wl = torch.empty(B, dtype=torch.int32, device=self.device)
        wp, wn = self._ws_for(B, max(Lmax0, T))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_voc_forward(self.handle, codes.data_ptr(), lengths.data_ptr(), _lib.ptr(durations), B, T, Lmax0, wav.data_ptr(),
                                               wl.data_ptr(), wp, wn, _lib.current_stream()), "dn_voc_forward")
        return wav, wl

    def set_profile(self, on: bool):
        _lib.check(self.lib.dn_voc_set_profile(self.handle, int(on)), "dn_voc_set_profile")

    def stage_times(self) -> List[float]:
        """ms of the last profiled forward: embedding + conv_pre, each upsampling stage, conv_post."""
        buf = (C.c_float * 16)()
        n = _lib.check(self.lib.dn_voc_stage_times(self.handle, buf, 16), "dn_voc_stage_times")
        return [float(buf[i]) for i in range(n)]


class CodeHiFiGANVocoder:
    """The reference's CodeHiFiGANVocoder on the HIP engine.  `model` is the generator's state dict (weight-norm pairs or folded
    weights) or the path of a checkpoint holding it under "generator"; `cfg` the vocoder's config dict."""

    def __init__(self, model: Union[str, Dict[str, torch.Tensor]], cfg: dict, dtype="f16", device="cuda:0"):
        check_config(cfg)
        _dtype(dtype)
        if isinstance(model, str):
            model = torch.load(model, map_location="cpu")["generator"]
        self.cfg = cfg
        self.engine = CodeHiFiGANEngine(model, cfg, dtype=dtype, device=device)
        self.last_durations: List[torch.Tensor] = []

    def generate(self, units: Sequence[torch.Tensor], dur_prediction: bool = True) -> List[torch.Tensor]:
        """Ragged utterances -> 1-D fp32 waveforms (valid samples only) in the caller's order.  Longest first internally; an
        utterance's waveform is bit for bit what forward() gives on it alone."""
        check_dur_prediction(self.cfg, dur_prediction)
        if len(units) == 0:
            return []
        eng = self.engine
        clean = [clean_units(u, self.cfg["num_embeddings"]) for u in units]
        order = sorted(range(len(clean)), key=lambda i: -clean[i].numel())
        B, T = len(clean), clean[order[0]].numel()
        codes = torch.zeros(B, T, dtype=torch.int32)
        for row, i in enumerate(order):
            codes[row, :clean[i].numel()] = clean[i]
        lengths = torch.tensor([clean[i].numel() for i in order], dtype=torch.int32)
        codes, lengths = codes.to(eng.device), lengths.to(eng.device)
        if dur_prediction:
            dur, sums = eng.durations(codes, lengths)
            frames = sums.cpu()  # the one synchronisation of a batch: the frame counts size the buffers
        else:
            dur, frames = None, lengths.cpu()
        check_frames(frames, eng.upsample)
        wav, _ = eng.forward(codes, lengths, dur, int(frames.max()))
        out: List[Optional[torch.Tensor]] = [None] * B
        self.last_durations = [None] * B
        for row, i in enumerate(order):
            out[i] = wav[row, :int(frames[row]) * eng.upsample].clone()
            self.last_durations[i] = None if dur is None else dur[row, :clean[i].numel()]
        return out

    def forward(self, x: Dict[str, torch.Tensor], dur_prediction: bool = False) -> torch.Tensor:
        """The reference's contract (vocoder.py:229-235): one utterance, codes < 0 dropped, 1-D waveform."""
        check_inputs(x)
        code = torch.as_tensor(x["code"])
        if code.dim() > 1 and code.shape[0] != 1:
            raise ValueError("CodeHiFiGAN.forward takes one utterance (B = 1); use generate() for a batch")
        return self.generate([code], dur_prediction=dur_prediction)[0]

    __call__ = forward
