"""Sample-rate conversion on the HIP engine, in front of the three waveform front ends: what the reference does inside its loaders
with torchaudio.functional.resample (examples/speech_to_speech/asr_bleu/utils.py:231-237; research/TranSpeech/asr_bleu/utils.py:237)
and with convert_waveform's to_mono (fairseq/data/audio/audio_utils.py:49-50).  sox's `rate` effect, which convert_waveform itself
calls, is another filter and is not restated.

`resample_tables` is the windowed-sinc polyphase bank of torchaudio.functional.resample, in float64, rounded once; `Resampler` is
dn_resample_* of libdiffnorm_hip.so (include/diffnorm_hip.h; csrc/resample.hip): one launch for a ragged batch, every utterance what
it gets alone, bit for bit, nothing at or behind its own samples read.  `read_wav` reads 16-bit PCM WAV files with the standard
library; every other container or sample format is out of scope.
"""
import ctypes as C
import math
import wave as _wave
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .nar_decoder import _NarEngine

KAISER_BETA = 14.769656459379492  # torchaudio's default for sinc_interp_kaiser
_METHODS = ("sinc_interp_hann", "sinc_interp_kaiser")


def _int_rate(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"resample: {name} {v!r} is not a number")
    if float(v) != int(v):
        raise ValueError(f"resample: {name} {v!r} is not an integer rate")
    if int(v) <= 0:
        raise ValueError(f"resample: {name} {v!r} must be positive")
    return int(v)


@dataclass
class ResampleConfig:
    """torchaudio.functional.resample's signature."""
    orig_freq: int
    new_freq: int
    lowpass_filter_width: int = 6
    rolloff: float = 0.99
    resampling_method: str = "sinc_interp_hann"
    beta: Optional[float] = None

    def __post_init__(self):
        self.orig_freq, self.new_freq = _int_rate(self.orig_freq, "orig_freq"), _int_rate(self.new_freq, "new_freq")
        if int(self.lowpass_filter_width) != self.lowpass_filter_width or self.lowpass_filter_width < 1:
            raise ValueError(f"resample: lowpass_filter_width {self.lowpass_filter_width!r} must be an integer of at least 1")
        if not 0.0 < float(self.rolloff) <= 1.0:
            raise ValueError(f"resample: rolloff {self.rolloff!r} outside (0, 1]")
        if self.resampling_method not in _METHODS:
            raise ValueError(f"resample: resampling_method {self.resampling_method!r} is not supported, only {' and '.join(_METHODS)}")

    @property
    def reduced(self) -> Tuple[int, int]:
        """(orig, new) divided by their gcd."""
        g = math.gcd(self.orig_freq, self.new_freq)
        return self.orig_freq // g, self.new_freq // g

    @property
    def passthrough(self) -> bool:
        return self.orig_freq == self.new_freq

    @property
    def width(self) -> int:
        orig, new = self.reduced
        return int(math.ceil(self.lowpass_filter_width * orig / (min(orig, new) * self.rolloff)))

    @property
    def taps(self) -> int:
        """K = 2 width + orig."""
        return 2 * self.width + self.reduced[0]

    def out_length(self, n: int) -> int:
        """ceil(new * n / orig), in exact integer arithmetic."""
        orig, new = self.reduced
        n = int(n)
        return -((-new * n) // orig) if n > 0 else 0


def resample_tables(cfg: ResampleConfig) -> np.ndarray:
    """The filter bank fp32 [new, K] of torchaudio.functional.resample (its _get_sinc_resample_kernel), in float64, rounded once:
    t = (-p / new + (k - width) / orig) * base clamped to +-lowpass_filter_width, base = min(orig, new) * rolloff;
    tap = sinc(pi t) * window(t) * base / orig."""
    orig, new = cfg.reduced
    lpw, width = int(cfg.lowpass_filter_width), cfg.width
    base = min(orig, new) * float(cfg.rolloff)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, :] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp_(-lpw, lpw)
    if cfg.resampling_method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lpw / 2) ** 2
    else:
        beta = torch.tensor(KAISER_BETA if cfg.beta is None else float(cfg.beta), dtype=torch.float64)
        window = torch.i0(beta * torch.sqrt(1 - (t / lpw) ** 2)) / torch.i0(beta)
    t = t * math.pi
    scale = base / orig
    taps = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * (window * scale)
    return taps.to(torch.float32).numpy()


def out_length(cfg: ResampleConfig, n: int) -> int:
    return cfg.out_length(n)


def read_wav(path) -> Tuple[torch.Tensor, int]:
    """A 16-bit PCM WAV file -> (int16 tensor [n, C], sample rate), with the standard library's `wave`; any other sample width is
    refused."""
    with _wave.open(str(path), "rb") as f:
        sw, ch, sr, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
        if sw != 2:
            raise ValueError(f"read_wav: {path}: a sample width of {sw} bytes ({8 * sw}-bit) is not supported, only 16-bit PCM")
        raw = f.readframes(n)
    a = np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, ch)
    return torch.from_numpy(a.copy()), int(sr)


def _as_samples(w) -> torch.Tensor:
    """One waveform [n] or [n, C] as it is when int16, else as fp32."""
    w = torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w)
    if w.dtype != torch.int16:
        w = w.float()
    if w.dim() not in (1, 2):
        raise ValueError(f"a waveform is [n] samples or [n, C] interleaved channels, got shape {tuple(w.shape)}")
    return w


class Resampler(_NarEngine):
    """dn_resample_* of libdiffnorm_hip.so.  Resampler(ResampleConfig(...)) or Resampler(orig_freq, new_freq, **ResampleConfig's
    keywords).  `tile` is the kernel's tile in output samples; `table_in_lds` tells which of the two bank paths the handle took
    (force_global=True: the global-memory one even where the bank fits LDS; the bits are the same)."""
    _sym = "resample"

    def __init__(self, cfg_or_orig, new_freq=None, device="cuda:0", force_global: bool = False, **kw):
        if isinstance(cfg_or_orig, ResampleConfig):
            if new_freq is not None or kw:
                raise ValueError("Resampler: a ResampleConfig carries the rates and the filter's parameters")
            self.cfg = cfg_or_orig
        elif isinstance(cfg_or_orig, (tuple, list)):
            self.cfg = ResampleConfig(*cfg_or_orig, **kw)
        else:
            self.cfg = ResampleConfig(cfg_or_orig, new_freq, **kw)
        self.handle = None
        self.tile = 0
        if self.cfg.passthrough:  # no handle, no launch
            self.device = torch.device(device)
            return
        orig, new = self.cfg.reduced
        bank = torch.from_numpy(resample_tables(self.cfg))
        self._create(device, [bank, bank.t().contiguous()], _lib.ResampleConfig(orig, new, self.cfg.width, self.cfg.taps, int(bool(force_global))))
        self.tile = int(self.lib.dn_resample_tile(self.handle))
        self.table_in_lds = (not force_global) and new * (self.cfg.taps | 1) <= 8192

    def out_length(self, n: int) -> int:
        return self.cfg.out_length(n)

    def forward(self, wave, lengths=None):
        """wave [B, L] or [B, L, C] (fp32 or int16; anything, NaN included, may lie behind an utterance's samples) with lengths [B] in
        samples, or a list of [n] / [n, C] waveforms of unequal length, padded here -> (out fp32 [B, Lo] mono with zeros behind each
        utterance's samples, sample counts int32 [B]), both on the device.  Equal rates: the input and its lengths, untouched."""
        if not isinstance(wave, torch.Tensor):
            waves = [_as_samples(w) for w in wave]
            if not waves:
                raise ValueError("Resampler.forward: an empty list of waveforms")
            if len({(w.dtype, w.shape[1:]) for w in waves}) != 1:
                raise ValueError("Resampler.forward: the waveforms of a list share one dtype and one channel count")
            lengths = torch.tensor([w.shape[0] for w in waves], dtype=torch.int32)
            wave = torch.zeros((len(waves), max(1, int(lengths.max()))) + tuple(waves[0].shape[1:]), dtype=waves[0].dtype)
            for i, w in enumerate(waves):
                wave[i, : w.shape[0]] = w
        elif lengths is None:
            raise ValueError("Resampler.forward: a [B, L] batch needs its lengths")
        if wave.dim() not in (2, 3):
            raise ValueError(f"Resampler.forward: waveforms are [B, L] or [B, L, C], got shape {tuple(wave.shape)}")
        B, L = wave.shape[:2]
        ch = wave.shape[2] if wave.dim() == 3 else 1
        lengths = torch.as_tensor(lengths)
        if lengths.numel() != B:
            raise ValueError(f"Resampler.forward: {lengths.numel()} lengths for {B} waveforms")
        if lengths.device.type == "cpu" and B and (int(lengths.min()) < 0 or int(lengths.max()) > L):
            raise ValueError(f"Resampler.forward: lengths {lengths.tolist()} do not fit the {L} samples")
        if self.cfg.passthrough:
            return wave, lengths
        if B < 1 or L < 1 or ch < 1:
            raise ValueError(f"Resampler.forward: an empty batch {tuple(wave.shape)}")
        code = _lib.DN_I16 if wave.dtype == torch.int16 else _lib.DN_F32
        wave = wave.to(self.device, torch.int16 if code == _lib.DN_I16 else torch.float32).contiguous()
        ln = lengths.to(self.device, torch.int32).contiguous()
        Lo = self.out_length(L)
        out = torch.empty(B, Lo, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        wp, wn = self._aligned(self._workspace(int(self.lib.dn_resample_workspace_bytes(self.handle, B, L))))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_resample_forward(self.handle, wave.data_ptr(), code, ch, ln.data_ptr(), B, L, out.data_ptr(), lens.data_ptr(), wp, wn,
                                                    _lib.current_stream()), "dn_resample_forward")
        return out, lens


class ResamplerCache:
    """What a consumer of waveforms keeps: one Resampler per (input rate, its own rate), built at first use."""

    def __init__(self, rate, device):
        self.rate, self.device, self._by_rate = _int_rate(rate, "the consumer's sample rate"), device, {}

    def get(self, sample_rate) -> Optional[Resampler]:
        """None when `sample_rate` is None or the consumer's own rate: the caller runs the code it ran before."""
        if sample_rate is None:
            return None
        sr = _int_rate(sample_rate, "sample_rate")
        if sr == self.rate:
            return None
        if sr not in self._by_rate:
            self._by_rate[sr] = Resampler(sr, self.rate, device=self.device)
        return self._by_rate[sr]
