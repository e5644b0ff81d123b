"""Restatements of the windowed-sinc polyphase resampler the device computes (include/diffnorm_hip.h, the resample section): what the
reference gets from torchaudio.functional.resample(waveform, orig, new) in its ASR loader (examples/speech_to_speech/asr_bleu/
utils.py:231-237).  A helper, not a test, written from the published formula: a float64 numpy form (the pin) and a plain float32
torch form of the same steps (what a straightforward float32 implementation loses against it: the yardstick of the device's error).

With orig and new divided by their gcd: base = min(orig, new) * rolloff, width = ceil(lpw * orig / base), K = 2 width + orig,
t[p, k] = (-p / new + (k - width) / orig) * base clamped to +-lpw, tap = sinc(pi t) * window(t) * base / orig; the waveform is padded
with (width, width + orig) zeros, correlated with the bank at stride orig, the phases interleaved, the result cut to
ceil(new * n / orig) samples."""
import math

import numpy as np
import torch

KAISER_BETA = 14.769656459379492


def reduce(orig, new):
    g = math.gcd(int(orig), int(new))
    return int(orig) // g, int(new) // g


def geometry(orig, new, lpw=6, rolloff=0.99):
    """(orig, new, base, width, K) of the reduced ratio."""
    orig, new = reduce(orig, new)
    base = min(orig, new) * rolloff
    width = int(math.ceil(lpw * orig / base))
    return orig, new, base, width, 2 * width + orig


def out_length(orig, new, n):
    orig, new = reduce(orig, new)
    return (new * int(n) + orig - 1) // orig


def table64(orig, new, lpw=6, rolloff=0.99, method="sinc_interp_hann", beta=None):
    """float64 [new, K]."""
    orig, new, base, width, K = geometry(orig, new, lpw, rolloff)
    k = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    p = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new
    t = np.clip((p + k) * base, -lpw, lpw)
    if method == "sinc_interp_hann":
        window = np.cos(t * math.pi / lpw / 2) ** 2
    elif method == "sinc_interp_kaiser":
        beta = KAISER_BETA if beta is None else float(beta)
        window = np.i0(beta * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(beta)
    else:
        raise ValueError(method)
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return sinc * (window * (base / orig))


def resample64(x, orig, new, table=None, **kw):
    """x: one waveform -> float64 [ceil(new n / orig)].  `table`: another bank [new, K] for the same ratio (the fp32 one, say)."""
    x = np.asarray(x, dtype=np.float64)
    orig, new, _, width, K = geometry(orig, new, kw.get("lpw", 6), kw.get("rolloff", 0.99))
    tab = table64(orig, new, **kw) if table is None else np.asarray(table, dtype=np.float64)
    n = x.size
    if n == 0:
        return np.zeros(0)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + orig)])
    frames = (xp.size - K) // orig + 1
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[::orig][:frames]  # [frames, K]
    out = win @ tab.T  # [frames, new]: frame-major, phase-minor = the interleave
    return out.reshape(-1)[: out_length(orig, new, n)]


def resample32(x, orig, new, table32):
    """The same steps in plain float32 torch: F.conv1d at stride orig over the padded waveform with the fp32 bank.  x: 1-D tensor."""
    orig, new, _, width, K = geometry(orig, new)
    x = torch.as_tensor(x, dtype=torch.float32)
    n = x.numel()
    if n == 0:
        return torch.zeros(0)
    w = torch.as_tensor(np.asarray(table32), dtype=torch.float32).view(new, 1, K)
    xp = torch.nn.functional.pad(x[None, None, :], (width, width + orig))
    y = torch.nn.functional.conv1d(xp, w, stride=orig)  # [1, new, frames]
    return y.transpose(1, 2).reshape(-1)[: out_length(orig, new, n)]


def noise_wave(n, seed):
    """Seeded noise in [-1, 1], fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) * 2 - 1


def two_tone(n, rate, f1=440.0, f2=3100.0):
    """0.6 sin(2 pi f1 t) + 0.3 sin(2 pi f2 t) at `rate`, fp32."""
    t = torch.arange(n, dtype=torch.float64) / rate
    return (0.6 * torch.sin(2 * math.pi * f1 * t) + 0.3 * torch.sin(2 * math.pi * f2 * t)).float()
