"""The first box of the S2UT leg on the HIP engine: waveform -> Kaldi-compliant log-mel filterbank features -> utterance CMVN, what
the reference computes on the CPU one utterance at a time with get_fbank (fairseq/data/audio/audio_utils.py:242-277:
torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=sr) at its defaults) and UtteranceCMVN
(fairseq/data/audio/feature_transforms/utterance_cmvn.py:30-41), which prep_s2ut_data.py:73 puts in every S2UT config.

`FbankEngine` is dn_fbank_* of libdiffnorm_hip.so (include/diffnorm_hip.h; csrc/fbank.hip).  The device path is the deterministic
torchaudio form, dither 0 (pyKaldi's own default adds random dither 1.0).  A batch gives every utterance what it gets alone, bit for
bit, and nothing at or behind an utterance's own samples is read.  Waveforms arrive as tensors or arrays at the configured sample
rate, or at any other integer rate named with `sample_rate`, which is converted on the device first (diffnorm_amd/resample.py);
decoding audio files other than 16-bit PCM WAV is not done here.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .nar_decoder import _NarEngine

POINTS_PER_WORKGROUP = 4096  # FB_POINTS in csrc/fbank.hip: a workgroup of the frames kernel takes 4096 / n_fft consecutive frames
CMVN_CHUNK = 64              # FB_CHUNK: frames per chunk of the CMVN statistics
MAX_MELS = 128


@dataclass
class FbankConfig:
    """torchaudio.compliance.kaldi.fbank's signature as far as the device path goes, plus UtteranceCMVN's two switches.  The defaults
    are the recipe's: 16 kHz, 80 bins, CMVN on.  Everything the kernels do not compute is refused here, by name (check_fbank_args)."""
    sample_rate: float = 16000.0
    n_mels: int = 80
    frame_length_ms: float = 25.0
    frame_shift_ms: float = 10.0
    low_freq: float = 20.0
    high_freq: float = 0.0          # 0 = Nyquist
    preemphasis: float = 0.97
    remove_dc_offset: bool = True
    input_scale: float = 1.0        # 1.0: int16-scale samples, as the reference feeds; 32768.0: [-1, 1] waveforms (HubertFeatureReader's)
    cmvn: bool = True               # False: the raw log-mel energies
    norm_means: bool = True
    norm_vars: bool = True
    n_fft: Optional[int] = None     # None: the next power of two >= the window (round_to_power_of_two)
    # the rest of torchaudio's signature: only these values are supported
    dither: float = 0.0
    use_energy: bool = False
    htk_compat: bool = False
    vtln_warp: float = 1.0
    window_type: str = "povey"
    snip_edges: bool = True
    subtract_mean: bool = False
    round_to_power_of_two: bool = True
    channel: int = -1
    min_duration: float = 0.0

    def __post_init__(self):
        check_fbank_args(self)

    @property
    def frame_length(self) -> int:
        return int(self.sample_rate * self.frame_length_ms * 0.001)

    @property
    def frame_shift(self) -> int:
        return int(self.sample_rate * self.frame_shift_ms * 0.001)

    @property
    def fft_size(self) -> int:
        return int(self.n_fft) if self.n_fft is not None else 1 << max(self.frame_length - 1, 1).bit_length()

    def c_struct(self) -> "_lib.FbankConfig":
        return _lib.FbankConfig(float(self.sample_rate), int(self.n_mels), self.frame_length, self.frame_shift, self.fft_size, float(self.low_freq),
                                float(self.high_freq), float(self.preemphasis), int(bool(self.remove_dc_offset)), float(self.input_scale),
                                int(bool(self.norm_means)), int(bool(self.norm_vars)), int(bool(self.cmvn)))


def check_fbank_args(cfg) -> None:
    """What of torchaudio's kaldi.fbank the engine runs; the rest is refused here, on the host, not silently ignored."""
    g = lambda k, d: getattr(cfg, k, d)
    if g("dither", 0.0) != 0.0:
        raise ValueError(f"fbank: dither {cfg.dither} is not supported: the device path is the deterministic form (dither 0)")
    if g("use_energy", False):
        raise ValueError("fbank: use_energy=True (an energy column) is not supported")
    if g("htk_compat", False):
        raise ValueError("fbank: htk_compat=True is not supported")
    if g("vtln_warp", 1.0) != 1.0:
        raise ValueError("fbank: vtln warping is not supported (vtln_warp must be 1.0)")
    if g("window_type", "povey") != "povey":
        raise ValueError(f"fbank: window_type {cfg.window_type!r} is not supported, only 'povey'")
    if not g("snip_edges", True):
        raise ValueError("fbank: snip_edges=False is not supported")
    if g("subtract_mean", False):
        raise ValueError("fbank: subtract_mean=True is not supported (utterance CMVN is the `cmvn` switch)")
    if not g("round_to_power_of_two", True):
        raise ValueError("fbank: round_to_power_of_two=False is not supported")
    if g("channel", -1) not in (-1, 0) or g("min_duration", 0.0) != 0.0:
        raise ValueError("fbank: channel selection and min_duration are not supported: waveforms are mono rows")
    n_fft, W, S = cfg.fft_size, cfg.frame_length, cfg.frame_shift
    if n_fft not in (256, 512, 1024) or W > n_fft:
        raise ValueError(f"fbank: a window of {W} samples needs n_fft {n_fft}: 256, 512 and 1024 are supported")
    if not 2 <= W or not 1 <= S <= W:
        raise ValueError(f"fbank: frame length {W} / shift {S} samples (2 <= length, 1 <= shift <= length)")
    if not 1 <= cfg.n_mels <= MAX_MELS:
        raise ValueError(f"fbank: {cfg.n_mels} mel bins outside 1 .. {MAX_MELS}")
    nyq = 0.5 * cfg.sample_rate
    hi = nyq if cfg.high_freq == 0.0 else cfg.high_freq
    if not 0.0 <= cfg.low_freq < hi <= nyq:
        raise ValueError(f"fbank: mel band [{cfg.low_freq}, {cfg.high_freq}] Hz must satisfy 0 <= low < high <= Nyquist = {nyq} (high 0 = Nyquist)")


def host_tables(cfg: FbankConfig) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(window [W], mel [n_mels, n_fft / 2 + 1], twiddles [n_fft / 2, 2]) as fp32 arrays from dn_fbank_tables / dn_fbank_twiddles: host
    code of the library, no GPU involved."""
    lib, c = _lib.load(), cfg.c_struct()
    window = np.empty(c.frame_length, dtype=np.float32)
    mel = np.empty((c.n_mels, c.n_fft // 2 + 1), dtype=np.float32)
    tw = np.empty((c.n_fft // 2, 2), dtype=np.float32)
    _lib.check(lib.dn_fbank_tables(C.byref(c), window.ctypes.data, mel.ctypes.data), "dn_fbank_tables")
    _lib.check(lib.dn_fbank_twiddles(c.n_fft, tw.ctypes.data), "dn_fbank_twiddles")
    return window, mel, tw


def out_frames(cfg: FbankConfig, n: int) -> int:
    """snip_edges frame count of n samples."""
    return 1 + (n - cfg.frame_length) // cfg.frame_shift if n >= cfg.frame_length else 0


def _as_wave(w) -> torch.Tensor:
    w = torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).float()
    if w.dim() != 1:
        raise ValueError(f"a waveform is one row of samples, got shape {tuple(w.shape)}")
    return w


class FbankEngine(_NarEngine):
    """dn_fbank_* of libdiffnorm_hip.so: fp32 throughout, the CMVN sums in double."""
    _sym = "fbank"

    def __init__(self, cfg: Optional[FbankConfig] = None, device="cuda:0"):
        self.cfg = cfg if cfg is not None else FbankConfig()
        self.n_mels = int(self.cfg.n_mels)
        self.frames_per_workgroup = POINTS_PER_WORKGROUP // self.cfg.fft_size
        self._resamplers = None
        self._create(device, [torch.from_numpy(t) for t in host_tables(self.cfg)], self.cfg.c_struct())

    def out_frames(self, L: int) -> int:
        return int(self.lib.dn_fbank_out_frames(self.handle, int(L)))

    def resampler(self, sample_rate):
        """The cached Resampler from `sample_rate` to the configured rate; None when there is nothing to convert."""
        if self._resamplers is None:
            from .resample import ResamplerCache

            self._resamplers = ResamplerCache(self.cfg.sample_rate, self.device)
        return self._resamplers.get(sample_rate)

    def forward(self, wave, lengths=None, sample_rate=None):
        """wave [B, L] with lengths [B] in samples (host or device; anything, NaN included, may lie behind an utterance's samples), or
        a list of 1-D waveforms of unequal length, padded here -> (feats fp32 [B, Lf, n_mels] with zero rows behind each utterance's
        frames, frame counts int32 [B] on the device).  An utterance shorter than one frame gets zero frames, not an error.
        sample_rate: the rate of `wave` when it is not the configured one -- the batch goes through Resampler.forward first (which
        also takes int16 and [B, L, C] input and hands on [-1, 1]-scaled mono for int16) and the features are those of its output."""
        rs = self.resampler(sample_rate) if sample_rate is not None else None
        if rs is not None:
            wave, lengths = rs.forward(wave, lengths)
        if not isinstance(wave, torch.Tensor):
            waves = [_as_wave(w) for w in wave]
            if not waves:
                raise ValueError("FbankEngine.forward: an empty list of waveforms")
            lengths = torch.tensor([w.numel() for w in waves], dtype=torch.int32)
            wave = torch.zeros(len(waves), max(1, int(lengths.max())))
            for i, w in enumerate(waves):
                wave[i, : w.numel()] = w
        elif lengths is None:
            raise ValueError("FbankEngine.forward: a [B, L] batch needs its lengths")
        if wave.dim() != 2:
            raise ValueError(f"FbankEngine.forward: waveforms are [B, L] mono rows, got shape {tuple(wave.shape)}")
        B, L = wave.shape
        lengths = torch.as_tensor(lengths)
        if lengths.numel() != B:
            raise ValueError(f"FbankEngine.forward: {lengths.numel()} lengths for {B} waveforms")
        if lengths.device.type == "cpu" and B and (int(lengths.min()) < 0 or int(lengths.max()) > L):
            raise ValueError(f"FbankEngine.forward: lengths {lengths.tolist()} do not fit the {L} samples")
        wave = wave.to(self.device, torch.float32).contiguous()
        ln = lengths.to(self.device, torch.int32).contiguous()
        Lf = self.out_frames(L)
        out = torch.empty(B, Lf, self.n_mels, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        wp, wn = self._aligned(self._workspace(int(self.lib.dn_fbank_workspace_bytes(self.handle, B, L))))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.dn_fbank_forward(self.handle, wave.data_ptr(), ln.data_ptr(), B, L, out.data_ptr() if Lf else None, lens.data_ptr(), wp, wn,
                                                 _lib.current_stream()), "dn_fbank_forward")
        return out, lens
