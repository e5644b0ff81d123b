"""Restatements of the Kaldi-compliant fbank + utterance CMVN the device front end computes (include/diffnorm_hip.h, the fbank
section): what the reference gets from torchaudio.compliance.kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=sr) at its
defaults with dither 0 (get_fbank, fairseq/data/audio/audio_utils.py:242-277) and from UtteranceCMVN.__call__
(fairseq/data/audio/feature_transforms/utterance_cmvn.py:30-41).  A helper, not a test: a float64 numpy form (the pin) and a plain
float32 torch form (what a straightforward float32 implementation loses against it: the yardstick of the device's own error)."""
import math

import numpy as np
import torch

FLOOR = 1.1920928955078125e-07  # torch.finfo(torch.float).eps: the log's floor in torchaudio's fbank


def sizes(sample_rate=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0):
    """(window W, shift S, transform N) in samples: N the next power of two >= W."""
    W, S = int(sample_rate * frame_length_ms * 0.001), int(sample_rate * frame_shift_ms * 0.001)
    return W, S, 1 << (W - 1).bit_length()


def n_frames(n, W, S):
    return 1 + (n - W) // S if n >= W else 0


def povey_window(W):
    j = np.arange(W, dtype=np.float64)
    return np.power(0.5 - 0.5 * np.cos(2.0 * np.pi * j / (W - 1)), 0.85)


def mel_of(hz):
    return 1127.0 * np.log(1.0 + np.asarray(hz, dtype=np.float64) / 700.0)


def mel_banks(n_mels, N, sample_rate, low_freq=20.0, high_freq=0.0):
    """float64 [n_mels, N / 2 + 1]: triangles in the mel domain over n_mels + 2 equally spaced mel points, Nyquist column zero."""
    hi = 0.5 * sample_rate if high_freq == 0.0 else high_freq
    mlo, mhi = float(mel_of(low_freq)), float(mel_of(hi))
    delta = (mhi - mlo) / (n_mels + 1)
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    left, centre, right = mlo + m * delta, mlo + (m + 1) * delta, mlo + (m + 2) * delta
    mel = mel_of(np.arange(N // 2, dtype=np.float64) * sample_rate / N)[None, :]
    w = np.maximum(0.0, np.minimum((mel - left) / (centre - left), (right - mel) / (right - centre)))
    return np.concatenate([w, np.zeros((n_mels, 1))], axis=1)


def fbank64(x, sample_rate=16000.0, n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc_offset=True, frame_length_ms=25.0,
            frame_shift_ms=10.0):
    """x: one waveform at int16 scale -> float64 [m, n_mels] log-mel energies."""
    x = np.asarray(x, dtype=np.float64)
    W, S, N = sizes(sample_rate, frame_length_ms, frame_shift_ms)
    m = n_frames(x.size, W, S)
    if m == 0:
        return np.zeros((0, n_mels))
    f = np.stack([x[i * S: i * S + W] for i in range(m)])
    if remove_dc_offset:
        f = f - f.mean(axis=1, keepdims=True)
    f = f - preemphasis * np.concatenate([f[:, :1], f[:, :-1]], axis=1)
    f = f * povey_window(W)[None, :]
    power = np.abs(np.fft.rfft(f, n=N, axis=1)) ** 2
    return np.log(np.maximum(power @ mel_banks(n_mels, N, sample_rate, low_freq, high_freq).T, FLOOR))


def cmvn_lines(x, norm_means=True, norm_vars=True):
    """UtteranceCMVN.__call__ verbatim in meaning, in x's own dtype (numpy)."""
    mean = x.mean(axis=0)
    square_sums = (x ** 2).sum(axis=0)
    if norm_means:
        x = np.subtract(x, mean)
    if norm_vars:
        var = square_sums / x.shape[0] - mean ** 2
        std = np.sqrt(np.maximum(var, 1e-10))
        x = np.divide(x, std)
    return x


def cmvn64(feats64, norm_means=True, norm_vars=True):
    return cmvn_lines(np.asarray(feats64, dtype=np.float64), norm_means, norm_vars) if len(feats64) else feats64


def cmvn32_of_64(feats64, norm_means=True, norm_vars=True):
    """The reference's float32 CMVN lines applied to the float64 features (rounded to float32 once, as its loader holds them)."""
    return cmvn_lines(np.asarray(feats64, dtype=np.float32), norm_means, norm_vars).astype(np.float64) if len(feats64) else feats64


def fbank32_torch(x, sample_rate=16000.0, n_mels=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97, remove_dc_offset=True, frame_length_ms=25.0,
                  frame_shift_ms=10.0, device="cpu"):
    """The plain float32 torch form: unfold, torch.fft.rfft, matmul with the mel matrix, clamp, log.  x [n] or [B, n] (every row of
    full length) -> float32 [m, n_mels] or [B, m, n_mels]."""
    x = torch.as_tensor(x, dtype=torch.float32, device=device)
    W, S, N = sizes(sample_rate, frame_length_ms, frame_shift_ms)
    if n_frames(x.shape[-1], W, S) == 0:
        return x.new_zeros(x.shape[:-1] + (0, n_mels))
    f = x.unfold(-1, W, S)
    if remove_dc_offset:
        f = f - f.mean(dim=-1, keepdim=True)
    f = f - preemphasis * torch.cat([f[..., :1], f[..., :-1]], dim=-1)
    f = f * torch.from_numpy(povey_window(W)).to(f)
    power = torch.fft.rfft(f, n=N, dim=-1).abs().pow(2.0)
    mel = torch.from_numpy(mel_banks(n_mels, N, sample_rate, low_freq, high_freq)).to(f)
    return torch.clamp(power @ mel.t(), min=FLOOR).log()


def cmvn32_torch(x, norm_means=True, norm_vars=True):
    """UtteranceCMVN's lines in float32 torch over dim -2 (frames)."""
    mean = x.mean(dim=-2, keepdim=True)
    square_sums = (x ** 2).sum(dim=-2, keepdim=True)
    if norm_means:
        x = x - mean
    if norm_vars:
        var = square_sums / x.shape[-2] - mean ** 2
        x = x / torch.sqrt(torch.clamp(var, min=1e-10))
    return x


def parity_wave(n, seed, sample_rate=16000.0):
    """The parity input: a signal on a noise floor -- seeded Gaussian noise of amplitude 300, tones at 440 Hz and 3 kHz of amplitude
    4000, a DC offset of 500, rounded to integers (bare tones would leave bins that hold only leakage, where float32 loses ten times
    more)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sample_rate
    x = 300.0 * rng.standard_normal(n) + 4000.0 * np.sin(2 * math.pi * 440.0 * t) + 4000.0 * np.sin(2 * math.pi * 3000.0 * t + 0.5) + 500.0
    return np.round(x)
