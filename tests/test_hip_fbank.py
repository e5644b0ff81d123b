"""The Kaldi fbank + utterance CMVN front end on the device (dn_fbank_*, csrc/fbank.hip; diffnorm_amd/fbank.py) against the float64
restatement of tests/fbank_ref.py.  No parity bar is a fixed number (check_parity): the raw log-mel error must be within 4 x the plain
float32 torch restatement's own error on the same input; the CMVN error within 4 x the error of the reference's float32 CMVN lines
applied to the float64 features, AND within 4 x the error of float64 CMVN applied to the float32 restatement's features (the first
CMVN yardstick collapses on inputs with tones; the second does not, and noise-only inputs keep the first one honest).  The 4 covers
another butterfly order and mel summation order than pocketfft's and torch's.  Then: geometry edges of the frames tile and the CMVN
chunk, the configuration switches, batch independence bit for bit, padding never read, short and empty utterances, silence and DC,
full scale, a second transform size, input_scale, lists and host lengths, refused calls, graph capture and the plumbing into the NAR
S2UT model."""
import numpy as np
import pytest
import torch

import fbank_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0
LOG_FLOOR = float(np.float32(np.log(np.float64(R.FLOOR))))
_engines = {}


def engine(cmvn, **kw):
    from diffnorm_amd import fbank

    key = (cmvn,) + tuple(sorted(kw.items()))
    if key not in _engines:
        _engines[key] = fbank.FbankEngine(fbank.FbankConfig(cmvn=cmvn, **kw), device=DEV)
    return _engines[key]


def pad_batch(waves, L=None, fill=0.0):
    lens = [len(w) for w in waves]
    batch = torch.full((len(waves), L or max(lens)), fill, dtype=torch.float32)
    for i, w in enumerate(waves):
        batch[i, : len(w)] = torch.as_tensor(np.asarray(w), dtype=torch.float32)
    return batch, torch.tensor(lens, dtype=torch.int32)


def run(eng, waves, L=None, fill=0.0):
    batch, lens = pad_batch(waves, L, fill)
    out, ol = eng.forward(batch.to(DEV), lens.to(DEV))
    torch.cuda.synchronize()
    return out.cpu(), ol.cpu()


def check_parity(waves, what, **kw):
    """The bars on a ragged batch.  kw: FbankConfig fields other than the defaults (tests/fbank_ref.py takes the same names).
    raw log-mel    device error <= 4 x the plain float32 torch restatement's own error (both against float64)
    CMVN, bar 1    device error <= 4 x the error of the reference's float32 CMVN lines applied to the float64 features.  On an input
                   with tones that yardstick collapses (E[x^2] - mean^2 cancels in the tone columns and the 1e-10 floor takes over:
                   errors of 0.3 .. 4.7e+3), so alone it would accept a wrong CMVN; test_cmvn_on_noise runs it where it holds.
                   It is the issue's bar for UtteranceCMVN as the recipe runs it, both halves on, and is asserted for that.  With
                   one half off it is no bar for a front end that computes its own features: mean-only normalisation in float32
                   loses 7e-6 on EXACT features, while the device's output carries its raw log-mel error (2.7e-4 measured, inside
                   the raw bar) one to one.  Those two cases are held to bar 2, which accounts for exactly that
    CMVN, bar 2    device error <= 4 x the error of FLOAT64 CMVN applied to the float32 restatement's features -- what the raw
                   error alone does to the output, the same margin as the raw bar -- plus the output format: the standard
                   deviation, the subtraction of the mean's low part and the division are three fp32 roundings of half an ulp
                   each, allowed as 2 ulp = 2 * 2^-23 of the largest |y|"""
    norm = {k: kw.pop(k) for k in ("norm_means", "norm_vars") if k in kw}
    sr = kw.get("sample_rate", 16000.0)
    raw, ol = run(engine(False, **kw), waves)
    nrm, ol2 = run(engine(True, **kw, **norm), waves)
    W, S, _ = R.sizes(sr)
    assert ol.tolist() == ol2.tolist() == [R.n_frames(len(w), W, S) for w in waves]
    e_raw = e_32 = e_cm = e_cm32 = e_y = y_max = 0.0
    for b, w in enumerate(waves):
        m = int(ol[b])
        ref = R.fbank64(w, **kw)
        assert torch.isfinite(raw[b]).all() and torch.isfinite(nrm[b]).all()
        assert not raw[b, m:].any() and not nrm[b, m:].any()
        if m == 0:
            continue
        t32 = R.fbank32_torch(w, **kw).double().numpy()
        want = R.cmvn64(ref, **norm)
        e_raw = max(e_raw, np.abs(raw[b, :m].double().numpy() - ref).max())
        e_32 = max(e_32, np.abs(t32 - ref).max())
        e_cm = max(e_cm, np.abs(nrm[b, :m].double().numpy() - want).max())
        e_cm32 = max(e_cm32, np.abs(R.cmvn32_of_64(ref, **norm) - want).max())
        e_y = max(e_y, np.abs(R.cmvn64(t32, **norm) - want).max())
        y_max = max(y_max, np.abs(want).max())
        if m == 1 and norm.get("norm_means", True):  # var 0, std floored at 1e-5, numerator 0
            assert not nrm[b, :1].any()
    bar2 = MARGIN * e_y + 2.0 * 2.0 ** -23 * y_max
    print(f"fbank {what}: raw {e_raw:.3e} vs float32 restatement {e_32:.3e} (ratio {e_raw / e_32:.2f}); CMVN {e_cm:.3e} vs float32 CMVN lines "
          f"{e_cm32:.3e} (ratio {e_cm / max(e_cm32, 1e-300):.2g}), vs float64 CMVN of the float32 features {e_y:.3e} (ratio {e_cm / max(e_y, 1e-300):.2f})")
    assert e_raw <= MARGIN * e_32, (what, e_raw, e_32)
    if not norm:
        assert e_cm <= MARGIN * e_cm32, (what, e_cm, e_cm32)
    assert e_cm <= bar2, (what, e_cm, e_y, bar2)


def ragged_waves(F, sr=16000.0):
    W, S, _ = R.sizes(sr)
    return [R.parity_wave(n, 20 + i, sr) for i, n in enumerate((W, W + 2 * S - 1, W + S * (F + 1)))]


def test_parity_against_float64_raw_and_cmvn():
    """1 frame, 2 frames, and one workgroup of frames plus a tail of two."""
    F = engine(False).frames_per_workgroup
    assert F == 8
    check_parity(ragged_waves(F), "ragged batch")


@pytest.mark.parametrize("unit,off", [("F", -1), ("F", 0), ("F", 1), ("C", -1), ("C", 0), ("C", 1)])
def test_geometry_edges(unit, off):
    """Frame counts round the frames tile (F) and the CMVN statistics chunk (C), one utterance each."""
    from diffnorm_amd import fbank

    frames = {"F": engine(False).frames_per_workgroup, "C": fbank.CMVN_CHUNK}[unit] + off
    check_parity([R.parity_wave(400 + 160 * (frames - 1), 30 + frames)], f"m = {unit}{off:+d} = {frames}")


@pytest.mark.parametrize("frames", [63, 64, 65, 129])
def test_cmvn_on_noise(frames):
    """Noise alone (amplitude 3000), where no column's variance is small against its squared mean, so the reference's float32 CMVN
    lines stay a real yardstick (their own error about 2e-3) and the issue's CMVN bar bites: one chunk less a frame, one chunk, one
    chunk plus a frame (the first cross-chunk merge), and two chunks plus a frame (a merge into an already merged pair)."""
    from diffnorm_amd import fbank

    assert fbank.CMVN_CHUNK == 64
    check_parity([np.round(3000.0 * np.random.default_rng(50 + frames).standard_normal(400 + 160 * (frames - 1)))], f"noise only, m = {frames}")


@pytest.mark.parametrize("kw", [dict(norm_means=False), dict(norm_vars=False), dict(remove_dc_offset=False), dict(preemphasis=0.0),
                                dict(low_freq=100.0, high_freq=7000.0, n_mels=64)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_switches(kw):
    """Each half of UtteranceCMVN alone, no DC removal, no pre-emphasis, another mel band and filter count: the same bars."""
    check_parity([R.parity_wave(400 + 160 * 9 + 77, 60), R.parity_wave(400 + 160 * 70, 61)], f"{kw}", **kw)


def test_lists_and_host_lengths():
    """forward() from a list of 1-D waveforms of unequal length (padded inside, lengths on the host) = the padded tensor with device
    lengths; host lengths that do not fit the samples are refused before anything runs."""
    eng = engine(True)
    waves = ragged_waves(eng.frames_per_workgroup)
    want, want_len = run(eng, waves)
    out, ol = eng.forward([torch.from_numpy(waves[0]), waves[1], list(waves[2])])
    assert ol.dtype == torch.int32 and torch.equal(ol.cpu(), want_len) and torch.equal(out.cpu(), want)
    batch, lens = pad_batch(waves)
    out, ol = eng.forward(batch, lens.tolist())  # host tensor, host lengths
    assert torch.equal(ol.cpu(), want_len) and torch.equal(out.cpu(), want)
    for bad in ([400, 719, batch.shape[1] + 1], [400, -1, 719], [400, 719]):
        with pytest.raises(ValueError):
            eng.forward(batch, bad)
    with pytest.raises(ValueError):
        eng.forward(batch)
    with pytest.raises(ValueError):
        eng.forward([np.zeros((2, 400))])


def test_a_refused_call_writes_nothing():
    """A workspace that is too small or misaligned is refused before the first launch: out and out_lengths keep their contents."""
    from diffnorm_amd import _lib

    eng = engine(True)
    batch, lens = pad_batch(ragged_waves(eng.frames_per_workgroup))
    batch, lens = batch.to(DEV), lens.to(DEV)
    B, L = batch.shape
    out = torch.full((B, eng.out_frames(L), 80), -7.0, device=DEV)
    ol = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    wp, wn = eng._aligned(eng._workspace(int(eng.lib.dn_fbank_workspace_bytes(eng.handle, B, L))))
    call = lambda p, n: eng.lib.dn_fbank_forward(eng.handle, batch.data_ptr(), lens.data_ptr(), B, L, out.data_ptr(), ol.data_ptr(), p, n, _lib.current_stream())
    assert call(wp, 256) == -3 and b"workspace" in eng.lib.dn_last_error()
    assert call(wp + 4, wn - 4) == -1 and b"aligned" in eng.lib.dn_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ol == -7).all())


def test_one_frame_cmvn_is_exactly_zero():
    nrm, ol = run(engine(True), [R.parity_wave(400, 5)])
    assert ol.tolist() == [1] and not nrm.any()


@pytest.mark.parametrize("cmvn", [False, True])
def test_batch_independence_bit_for_bit(cmvn):
    eng = engine(cmvn)
    waves = ragged_waves(eng.frames_per_workgroup)
    out, ol = run(eng, waves)
    rev, _ = run(eng, waves[::-1])
    longer, oll = run(eng, waves, L=len(waves[-1]) + 1777)
    assert oll.tolist() == ol.tolist() and not longer[:, out.shape[1]:].any()
    for b, w in enumerate(waves):
        m = int(ol[b])
        alone, _ = run(eng, [w])
        assert torch.equal(alone[0, :m], out[b, :m])
        assert torch.equal(rev[len(waves) - 1 - b, :m], out[b, :m])
        assert torch.equal(longer[b, :m], out[b, :m])


@pytest.mark.parametrize("cmvn", [False, True])
def test_padding_is_never_read(cmvn):
    eng = engine(cmvn)
    waves = ragged_waves(eng.frames_per_workgroup)
    clean, ol = run(eng, waves, L=len(waves[-1]) + 300)
    dirty, ol2 = run(eng, waves, L=len(waves[-1]) + 300, fill=float("nan"))
    assert ol.tolist() == ol2.tolist()
    assert torch.isfinite(dirty).all() and torch.equal(dirty, clean)
    for b in range(len(waves)):
        assert not dirty[b, int(ol[b]):].any()


@pytest.mark.parametrize("cmvn", [False, True])
def test_short_and_empty_utterances_are_handled(cmvn):
    w = R.parity_wave(400, 7)
    out, ol = run(engine(cmvn), [w[:399], w[:0], w], L=400)  # forward() checks the return code: 0
    assert ol.tolist() == [0, 0, 1] and out.shape == (3, 1, 80)
    assert not out[0].any() and not out[1].any()
    assert torch.isfinite(out[2]).all() and (cmvn or out[2].abs().min() > 0)


def test_silence_and_dc():
    n = 400 + 160 * 9
    waves = [np.zeros(n), np.full(n, 32767.0)]
    raw, ol = run(engine(False), waves)
    assert ol.tolist() == [10, 10]
    print(f"silence / DC: raw values {[v.item() for v in raw.unique()]}, floor {LOG_FLOOR!r}")
    assert torch.equal(raw, torch.full_like(raw, LOG_FLOOR))
    nrm, _ = run(engine(True), waves)
    assert not nrm.any()


def test_full_scale_square_wave():
    """+-32767 at 1 kHz, 3 frames: the power spectrum reaches ~1e14 and must neither overflow nor lose the floor."""
    t = np.arange(400 + 160 * 2)
    check_parity([np.where((t // 8) % 2 == 0, 32767.0, -32767.0)], "full-scale square wave")


def test_second_size_8khz_40_bins():
    eng = engine(False, sample_rate=8000.0, n_mels=40)
    assert eng.cfg.fft_size == 256 and eng.frames_per_workgroup == 16
    check_parity(ragged_waves(16, 8000.0), "8 kHz / 40 bins / N = 256", sample_rate=8000.0, n_mels=40)


@pytest.mark.parametrize("cmvn", [False, True])
def test_input_scale(cmvn):
    from diffnorm_amd import fbank

    waves = ragged_waves(8)
    out, ol = run(engine(cmvn), waves)
    unit = fbank.FbankEngine(fbank.FbankConfig(cmvn=cmvn, input_scale=32768.0), device=DEV)
    out1, ol1 = run(unit, [w / 32768.0 for w in waves])
    assert ol1.tolist() == ol.tolist() and torch.equal(out1, out)


def test_graph_capture_replays_the_eager_result():
    """dn_fbank_forward is stream-ordered and allocation-free: captured on a side stream (one branch) and replayed twice."""
    from diffnorm_amd import _lib
    from diffnorm_amd.engine import capture_graph

    eng = engine(True)
    batch, lens = pad_batch(ragged_waves(eng.frames_per_workgroup))
    batch, lens = batch.to(DEV), lens.to(DEV)
    B, L = batch.shape
    eager, eager_len = eng.forward(batch, lens)
    out, ol = torch.full_like(eager, -7.0), torch.full_like(eager_len, -7)
    wp, wn = eng._aligned(eng._workspace(int(eng.lib.dn_fbank_workspace_bytes(eng.handle, B, L))))

    def step():
        _lib.check(eng.lib.dn_fbank_forward(eng.handle, batch.data_ptr(), lens.data_ptr(), B, L, out.data_ptr(), ol.data_ptr(), wp, wn, _lib.current_stream()),
                   "dn_fbank_forward")

    graph = capture_graph(eng.device, step)
    for _ in range(2):
        out.fill_(-7.0)
        ol.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(ol, eager_len)


@pytest.mark.parametrize("arch", ["transformer", "conformer"])
def test_waveform_input_of_the_nar_model(arch):
    """model.encoder from waveforms = the encoder engine fed FbankEngine.forward's output, bit for bit; generate() from waveforms =
    generate() from those features; the same constructor call without waveform_input still takes [B, L, 80] features."""
    import conformer_ref
    import nar_oracle as N
    from diffnorm_amd import nar_decoder
    from diffnorm_amd.iterative_refinement import IterativeRefinementGenerator
    from gen_golden_nar_configs import CFG, ENC_CFG, Dict1004

    if arch == "conformer":
        c = conformer_ref.TINY
        enc_sd, extra = conformer_ref.make_state_dict(), dict(depthwise_kernel=c.depthwise_kernel)
    else:
        c = ENC_CFG
        enc_sd, extra = N.make_nar_encoder_state_dict(c, "narenc"), {}
    make = lambda **kw: nar_decoder.NARS2UTDecoderModel(
        N.make_nar_state_dict(CFG, "nar"), CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV, encoder_state_dict=enc_sd,
        encoder_arch=arch, encoder_kw=dict(input_dim=c.input_dim, conv_channels=c.conv_channels, kernel=c.kernel_sizes[0], ffn=c.ffn_dim, layers=c.layers, **extra),
        **kw)
    from_wave, from_feats = make(waveform_input=True), make()
    waves, lens = pad_batch([R.parity_wave(n, 40 + i) for i, n in enumerate((16000, 9000, 12345))])
    waves, lens = waves.to(DEV), lens.to(DEV)
    feats, flens = engine(True).forward(waves, lens)
    assert flens.tolist() == [98, 54, 75]
    a, b = from_wave.encoder(waves, lens), from_feats.encoder(feats, flens)
    assert torch.equal(a["encoder_out"][0], b["encoder_out"][0])
    assert torch.equal(a["encoder_padding_mask"][0], b["encoder_padding_mask"][0])
    gen = IterativeRefinementGenerator(Dict1004(), speech_source=True, max_iter=4, beam_size=1, adaptive=True)
    h_w = gen.generate([from_wave], {"net_input": {"src_tokens": waves, "src_lengths": lens}})
    h_f = gen.generate([from_feats], {"net_input": {"src_tokens": feats, "src_lengths": flens}})
    assert len(h_w) == len(h_f) == 3
    for x, y in zip(h_w, h_f):
        assert x[0]["tokens"].tolist() == y[0]["tokens"].tolist() and int(x[0]["steps"]) == int(y[0]["steps"])
        assert torch.equal(x[0]["positional_scores"], y[0]["positional_scores"])
