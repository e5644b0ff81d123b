"""CPU checks of the device resampler's host side (diffnorm_amd/resample.py): the filter bank against the float64 restatement of
tests/resample_ref.py bit for bit, the gcd reduction, output lengths in exact integers, the refusals, the pass-through, two sanity
checks of the restatement itself, and read_wav against files written with the standard library.  No GPU is needed."""
import math
import wave

import numpy as np
import pytest
import torch

import resample_ref as R

RATIOS = [(48000, 16000), (24000, 16000), (16000, 24000), (44100, 16000), (22050, 16000), (8000, 16000)]
METHODS = ["sinc_interp_hann", "sinc_interp_kaiser"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("orig,new", RATIOS)
def test_tables_are_the_float32_rounding_of_the_restatement(orig, new, method):
    from diffnorm_amd import resample

    cfg = resample.ResampleConfig(orig, new, resampling_method=method)
    got = resample.resample_tables(cfg)
    want = R.table64(orig, new, method=method).astype(np.float32)
    o, n, _, width, K = R.geometry(orig, new)
    assert got.dtype == np.float32 and got.shape == want.shape == (n, K) and (cfg.width, cfg.taps, cfg.reduced) == (width, K, (o, n))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{(got != want).sum()} of {got.size} taps differ"


def test_tap_counts_of_the_recipe_ratios():
    from diffnorm_amd import resample

    assert [resample.ResampleConfig(o, n).taps for o, n in RATIOS[:5]] == [R.geometry(o, n)[4] for o, n in RATIOS[:5]] == [41, 23, 16, 475, 459]
    assert resample.ResampleConfig(44100, 16000).reduced == (441, 160) and resample.ResampleConfig(22050, 16000).reduced == (441, 320)


@pytest.mark.parametrize("method", METHODS)
def test_gcd_reduction(method):
    from diffnorm_amd import resample

    a = resample.resample_tables(resample.ResampleConfig(48000, 16000, resampling_method=method))
    b = resample.resample_tables(resample.ResampleConfig(3, 1, resampling_method=method))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("orig,new", RATIOS + [(3, 1), (7, 5)])
def test_out_length_in_exact_integers(orig, new):
    from diffnorm_amd import resample

    cfg = resample.ResampleConfig(orig, new)
    o, n = cfg.reduced
    big = (1 << 31) // n
    for length in (0, 1, o - 1, o, o + 1, big - 1, big, big + 1, 3 * big + 7):
        want = 0 if length <= 0 else (n * length) // o + (1 if (n * length) % o else 0)
        assert cfg.out_length(length) == resample.out_length(cfg, length) == want == R.out_length(orig, new, max(length, 0)), (length, want)
        assert isinstance(cfg.out_length(length), int)


@pytest.mark.parametrize("kw", [dict(orig_freq=0), dict(new_freq=-16000), dict(orig_freq=44100.5), dict(new_freq=16000.25), dict(lowpass_filter_width=0),
                                dict(rolloff=0.0), dict(rolloff=1.01), dict(rolloff=-0.5), dict(resampling_method="linear"), dict(resampling_method="kaiser_best")])
def test_refusals(kw):
    from diffnorm_amd import resample

    args = dict(orig_freq=48000, new_freq=16000)
    args.update(kw)
    with pytest.raises(ValueError, match="resample"):
        resample.ResampleConfig(**args)


def test_accepted_edges_of_the_arguments():
    from diffnorm_amd import resample

    assert resample.ResampleConfig(48000.0, 16000.0).reduced == (3, 1)  # integer-valued floats are rates
    assert resample.ResampleConfig(3, 1, rolloff=1.0, lowpass_filter_width=1).taps == 2 * 3 + 3


def test_pass_through_for_equal_rates():
    """Equal rates: no handle (so no GPU and no launch) and the very input back."""
    from diffnorm_amd import Resampler, resample

    assert Resampler is resample.Resampler
    r = Resampler(16000, 16000, device="cpu")
    assert r.cfg.passthrough and r.handle is None
    w, ln = torch.randn(2, 50), torch.tensor([50, 20], dtype=torch.int32)
    out, ol = r.forward(w, ln)
    assert out is w and ol is ln
    assert resample.ResamplerCache(16000.0, "cpu").get(None) is None and resample.ResamplerCache(16000.0, "cpu").get(16000) is None


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("orig,new", [(48000, 16000), (24000, 16000), (44100, 16000), (22050, 16000)])
def test_downsampling_phases_sum_to_one(orig, new, method):
    """DC gain of every phase of a downsampling bank: 1 to within the window's DC error.  That error is the integral of the
    prototype sinc(pi t) window(t) over its support minus 1, taken here from the restatement itself as the bank of 64 : 1 (one
    phase, a Riemann sum 64 / min(orig, new) times denser than any phase below).  A phase is a Riemann sum of the same prototype
    at step base / orig: it differs from the integral by the prototype's spectrum at multiples of orig / base >= 2, deep in the
    stop band, where a windowed sinc's response is no larger than its error at DC.  So: |sum - 1| <= 2 x the DC error."""
    dc = abs(R.table64(64, 1, method=method).sum() - 1.0)
    sums = R.table64(orig, new, method=method).sum(axis=1)
    worst = np.abs(sums - 1.0).max()
    print(f"{orig} -> {new} {method}: phase sums in [{sums.min():.9f}, {sums.max():.9f}], window DC error {dc:.3e}")
    assert 0.0 < dc < 1e-3 and worst <= 2.0 * dc


def test_sine_through_the_restatement():
    """1 kHz at 48 kHz -> 16 kHz through the float64 restatement = the analytic 16 kHz sine away from the K edge samples (the edges
    see the zero padding).  The pass-band ripple of the 6-zero-crossing Hann-windowed sinc at 1 / 8 of the output Nyquist is what
    the bound allows: the bank's own gain at that frequency, computed from the bank, +- 1e-9."""
    n = 4800
    t = np.arange(n) / 48000.0
    y = R.resample64(np.sin(2 * math.pi * 1000.0 * t), 48000, 16000)
    assert y.size == 1600
    K = R.geometry(48000, 16000)[4]
    tab = R.table64(48000, 16000)[0]
    width = R.geometry(48000, 16000)[3]
    k = np.arange(K) - width
    gain = np.sum(tab * np.exp(2j * math.pi * 1000.0 * k / 48000.0))  # the filter's response at 1 kHz: its modulus and phase
    want = np.abs(gain) * np.sin(2 * math.pi * 1000.0 * np.arange(1600) / 16000.0 + np.angle(gain))
    err = np.abs(y - want)[K:-K].max()
    print(f"1 kHz sine 48 k -> 16 k: gain {abs(gain):.6f}, phase {np.angle(gain):.2e}, max error inside {err:.2e}")
    assert abs(abs(gain) - 1.0) < 1e-3 and abs(np.angle(gain)) < 1e-9 and err < 1e-9
    assert np.abs(y - np.sin(2 * math.pi * 1000.0 * np.arange(1600) / 16000.0))[K:-K].max() < 1e-3


def test_float32_restatement_follows_the_float64_one():
    """The two restatements are the same steps: they agree to float32 accuracy, and not exactly (the GPU tests' bar is not vacuous)."""
    from diffnorm_amd import resample

    for orig, new in ((3, 1), (3, 2), (2, 3), (441, 160)):
        x = R.noise_wave(5000, 1)
        tab = resample.resample_tables(resample.ResampleConfig(orig, new))
        a, b = R.resample64(x.numpy(), orig, new), R.resample32(x, orig, new, tab).double().numpy()
        assert a.shape == b.shape == (R.out_length(orig, new, 5000),)
        err = np.abs(a - b).max()
        assert 0.0 < err < 1e-5, (orig, new, err)


def _write_wav(path, data, rate, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(data.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data.tobytes())


def test_read_wav_round_trip(tmp_path):
    from diffnorm_amd import resample

    rng = np.random.default_rng(0)
    for ch, rate in ((1, 48000), (2, 22050)):
        data = rng.integers(-32768, 32768, size=(1234, ch)).astype("<i2")
        data[0, 0], data[1, 0] = -32768, 32767
        _write_wav(tmp_path / f"c{ch}.wav", data, rate)
        got, sr = resample.read_wav(tmp_path / f"c{ch}.wav")
        assert sr == rate and got.dtype == torch.int16 and tuple(got.shape) == (1234, ch)
        assert np.array_equal(got.numpy(), data.astype(np.int16))
    _write_wav(tmp_path / "u8.wav", rng.integers(0, 256, size=(100, 1)).astype(np.uint8), 16000, width=1)
    with pytest.raises(ValueError, match="8-bit"):
        resample.read_wav(tmp_path / "u8.wav")
