"""The device resampler (dn_resample_*, csrc/resample.hip; diffnorm_amd/resample.py) against the float64 restatement of
tests/resample_ref.py.  The parity bar is no fixed number: the device's max abs error over an utterance's own outputs must be within
4 x the plain float32 torch restatement's own error on the same input (both against float64) -- the factor of the fbank tests, for
the same reason: another fp32 summation order (here k ascending, one FMA chain, against conv1d's).  Then: the geometry edges of the
output tile, batch independence bit for bit, padding never read, the two bank paths, the input formats, and the `sample_rate`
keyword of the three front ends.  Measured ratios are printed and recorded in DESIGN 9g."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4.0
RATIOS = [(3, 1), (3, 2), (2, 3), (441, 160)]  # the last one: the bank is read from global memory
_RS, _REF = {}, {}


def resampler(orig, new, **kw):
    from diffnorm_amd import resample

    key = (orig, new) + tuple(sorted(kw.items()))
    if key not in _RS:
        _RS[key] = resample.Resampler(orig, new, device=DEV, **kw)
    return _RS[key]


def table32(orig, new):
    from diffnorm_amd import resample

    return resample.resample_tables(resample.ResampleConfig(orig, new))


def ref64(orig, new, wave, key):
    """The float64 restatement of a waveform, computed once per (ratio, key) and left unchanged."""
    k = (orig, new, key)
    if k not in _REF:
        _REF[k] = R.resample64(wave.double().numpy(), orig, new)
    return _REF[k]


def pad_batch(waves, L=None, fill=0.0):
    lens = [w.shape[0] for w in waves]
    batch = torch.full((len(waves), L or max(max(lens), 1)) + tuple(waves[0].shape[1:]), fill, dtype=waves[0].dtype)
    for i, w in enumerate(waves):
        batch[i, : w.shape[0]] = w
    return batch, torch.tensor(lens, dtype=torch.int32)


def run(rs, waves, L=None, fill=float("nan")):
    """A NaN-padded batch -> (out [B, Lo], out_lengths) on the CPU, after the checks every call must pass: the lengths, finite
    outputs, exact zeros behind each utterance's own."""
    fill = fill if waves[0].dtype != torch.int16 else 12345
    batch, lens = pad_batch(waves, L, fill)
    out, ol = rs.forward(batch.to(DEV), lens.to(DEV))
    torch.cuda.synchronize()
    out, ol = out.cpu(), ol.cpu()
    assert out.dtype == torch.float32 and ol.dtype == torch.int32 and out.shape == (len(waves), rs.out_length(batch.shape[1]))
    assert ol.tolist() == [rs.out_length(w.shape[0]) for w in waves] == [R.out_length(*rs.cfg.reduced, w.shape[0]) for w in waves]
    assert torch.isfinite(out).all()
    for b in range(len(waves)):
        assert not out[b, int(ol[b]):].any()
    return out, ol


def length_for(orig, new, m):
    """The shortest input with at least m output samples (exactly m when downsampling: every count is reached there)."""
    n = (m * orig) // new
    while R.out_length(orig, new, n) < m:
        n += 1
    return n


def signals(orig, n, seed):
    return [("noise", R.noise_wave(n, seed)), ("two-tone", R.two_tone(n, 16000.0 * orig))]


@pytest.mark.parametrize("orig,new", RATIOS)
def test_parity_against_float64(orig, new):
    rs = resampler(orig, new)
    assert rs.table_in_lds == ((orig, new) != (441, 160))
    tab = table32(orig, new)
    for n in (20000, 7001):
        for name, w in signals(orig, n, 11 + n):
            want = ref64(orig, new, w, (name, n))
            e32 = float(np.abs(R.resample32(w, orig, new, tab).double().numpy() - want).max())
            assert e32 > 0.0, "the float32 restatement is exact on this input: the bar would be vacuous"
            out, ol = run(rs, [w])
            err = float(np.abs(out[0, : int(ol[0])].double().numpy() - want).max())
            print(f"resample {orig}:{new} {name} n={n}: device {err:.3e}, float32 restatement {e32:.3e}, ratio {err / e32:.2f}")
            assert err <= MARGIN * e32


@pytest.mark.parametrize("orig,new", RATIOS)
def test_geometry_edges(orig, new):
    """Output lengths around the tile (1, Tt - 1, Tt, Tt + 1, 2 Tt + 1), input lengths around one frame (1, orig - 1, orig,
    orig + 1), an empty row inside the batch, the shortest row first and the longest last -- and each of them alone (B = 1)."""
    rs = resampler(orig, new)
    Tt = rs.tile
    assert Tt > 0 and Tt % new == 0
    ns = sorted({length_for(orig, new, m) for m in (1, Tt - 1, Tt, Tt + 1, 2 * Tt + 1)} | {n for n in (1, orig - 1, orig, orig + 1) if n > 0})
    if new <= orig:
        assert {rs.out_length(n) for n in ns} >= {1, Tt - 1, Tt, Tt + 1, 2 * Tt + 1}
    waves = [R.noise_wave(n, 100 + n) for n in ns]
    waves.insert(2, torch.zeros(0))
    assert len(waves[0]) == min(len(w) for w in waves if len(w)) and len(waves[-1]) == max(len(w) for w in waves)
    out, ol = run(rs, waves)
    tab = table32(orig, new)
    assert int(ol[2]) == 0
    for b, w in enumerate(waves):
        m = int(ol[b])
        if m == 0:
            continue
        want = R.resample64(w.double().numpy(), orig, new)
        e32 = float(np.abs(R.resample32(w, orig, new, tab).double().numpy() - want).max())
        err = float(np.abs(out[b, :m].double().numpy() - want).max())
        assert err <= MARGIN * e32 or err <= 2.0 ** -23 * float(np.abs(want).max()), (len(w), err, e32)  # (a sum of <= orig terms may round exactly in conv1d)
        alone, al = run(rs, [w])  # B = 1
        assert int(al[0]) == m and torch.equal(alone[0, :m], out[b, :m])


@pytest.mark.parametrize("orig,new", RATIOS)
def test_ragged_batch_is_each_utterance_alone(orig, new):
    rs = resampler(orig, new)
    Tt = rs.tile
    ns = [length_for(orig, new, m) for m in (Tt + 7, 3 * Tt - 1, 5, 2 * Tt)]
    waves = [R.noise_wave(n, 7 + i) for i, n in enumerate(ns)]
    out, ol = run(rs, waves)
    wide, wl = run(rs, waves, L=max(ns) + 3 * orig * Tt // new + 17)  # the same rows under a larger L
    assert wl.tolist() == ol.tolist() and wide.shape[1] > out.shape[1]
    for b, w in enumerate(waves):
        m = int(ol[b])
        alone, _ = run(rs, [w])
        assert torch.equal(alone[0, :m], out[b, :m]) and torch.equal(wide[b, :m], out[b, :m])
        assert not wide[b, m:].any()


def test_lds_bank_path_equals_global_bank_path():
    lds, glb = resampler(3, 2), resampler(3, 2, force_global=True)
    assert lds.table_in_lds and not glb.table_in_lds and lds.tile == glb.tile
    waves = [R.noise_wave(n, 40 + i) for i, n in enumerate((3001, 17, 7777))] + [R.two_tone(5000, 24000.0)]
    a, al = run(lds, waves)
    b, bl = run(glb, waves)
    assert al.tolist() == bl.tolist() and torch.equal(a, b)


@pytest.mark.parametrize("orig,new", [(3, 1), (441, 160)])
def test_input_formats(orig, new):
    """int16 = the same samples as fp32 x 2^-15; stereo / three channels = the fp32 mean in channel order fed as mono; all bit for bit."""
    rs = resampler(orig, new)
    g = torch.Generator().manual_seed(5)
    ns = (4000, 1501)
    pcm = [torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16) for n in ns]
    pcm[0][:2] = torch.tensor([-32768, 32767], dtype=torch.int16)
    a, al = run(rs, pcm)
    b, bl = run(rs, [p.float() * 2.0 ** -15 for p in pcm])
    assert al.tolist() == bl.tolist() and torch.equal(a, b)
    for ch in (2, 3):
        multi = [torch.rand(n, ch, generator=g) * 2 - 1 for n in ns]
        mono = []
        for w in multi:
            s = w[:, 0].clone()
            for c in range(1, ch):
                s = s + w[:, c]
            mono.append(s / float(ch))
        a, al = run(rs, multi)  # NaN behind every utterance's samples, in every channel
        b, bl = run(rs, mono)
        assert al.tolist() == bl.tolist() and torch.equal(a, b), ch
    stereo = [torch.stack([p, p.flip(0)], 1) for p in pcm]  # int16 stereo
    a, _ = run(rs, stereo)
    b, _ = run(rs, [(s[:, 0].float() * 2.0 ** -15 + s[:, 1].float() * 2.0 ** -15) / 2.0 for s in stereo])
    assert torch.equal(a, b)


def test_lists_host_lengths_and_refusals():
    rs = resampler(3, 2)
    waves = [R.noise_wave(n, i) for i, n in enumerate((900, 31, 2500))]
    out, ol = rs.forward(waves)
    batch, lens = pad_batch(waves)
    out2, ol2 = rs.forward(batch, lens)  # host tensors, host lengths
    assert out.is_cuda and ol.is_cuda and torch.equal(out, out2) and torch.equal(ol, ol2)
    with pytest.raises(ValueError):
        rs.forward(batch)
    with pytest.raises(ValueError):
        rs.forward(batch, torch.tensor([900, 31, 2501]))
    with pytest.raises(ValueError):
        rs.forward([])


def _waves48(ns=(9000, 4321, 7000), rate=48000.0):
    return [R.two_tone(n, rate) * 0.5 + 0.25 * R.noise_wave(n, 60 + i) for i, n in enumerate(ns)]


def test_fbank_takes_a_sample_rate():
    from diffnorm_amd import fbank

    eng = fbank.FbankEngine(fbank.FbankConfig(input_scale=32768.0), device=DEV)
    waves = _waves48()
    batch, lens = pad_batch(waves, fill=float("nan"))
    got, gl = eng.forward(batch, lens, sample_rate=48000)
    rs = resampler(48000, 16000)
    want, wl = eng.forward(*rs.forward(batch, lens))
    assert got.shape[1] > 10 and torch.equal(got, want) and torch.equal(gl, wl)
    lg, ll = eng.forward(waves, sample_rate=48000)  # a list
    assert torch.equal(ll, wl) and torch.equal(lg, want)
    first = eng.resampler(48000)
    assert first is not None and eng.resampler(48000) is first and eng.resampler(48000.0).handle.value == first.handle.value
    assert eng.resampler(None) is None and eng.resampler(16000) is None and eng.resampler(24000) is not first
    b16, l16 = pad_batch([R.noise_wave(n, 3) for n in (3000, 2000)])
    plain = eng.forward(b16, l16)
    for sr in (None, 16000, 16000.0):
        again = eng.forward(b16, l16, sample_rate=sr)
        assert torch.equal(plain[0], again[0]) and torch.equal(plain[1], again[1])


def test_hubert_reader_takes_a_sample_rate():
    import hubert_ref as H
    from diffnorm_amd import hubert

    eng = hubert.HubertEngine(H.make_state_dict(H.TINY, H.TINY_SEED), H.TINY, dtype="f32", device=DEV)
    rd = hubert.HubertFeatureReader(None, H.TINY, layer=2, max_chunk=4000, engine=eng)
    waves = _waves48((9000, 4500, 7000), 24000.0)  # 6000, 3000, 4667 samples at 16 kHz: the first and the last are two chunks
    got = rd.get_feats_batch(waves, sample_rate=24000)
    out, ol = resampler(24000, 16000).forward(waves)
    want = rd.get_feats_batch([out[i, :n] for i, n in enumerate(ol.tolist())])
    assert len(got) == len(want) == 3 and all(torch.equal(a, b) and a.shape[0] > 0 for a, b in zip(got, want))
    assert want[0].shape[0] == H.out_frames(H.TINY, 4000) + H.out_frames(H.TINY, 2000)  # chunked AFTER the conversion
    assert torch.equal(rd.get_feats(waves[1], sample_rate=24000), want[1])
    first = rd.resampler(24000)
    assert rd.resampler(24000) is first and first.handle.value
    w16 = [H.make_wave(3000, 1), H.make_wave(2100, 2)]
    plain = rd.get_feats_batch(w16)
    for sr in (None, 16000):
        assert all(torch.equal(a, b) for a, b in zip(plain, rd.get_feats_batch(w16, sample_rate=sr)))


def test_dump_features_takes_a_sample_rate(tmp_path):
    import hubert_ref as H
    from diffnorm_amd import hubert

    eng = hubert.HubertEngine(H.make_state_dict(H.TINY, H.TINY_SEED), H.TINY, dtype="f32", device=DEV)
    rd = hubert.HubertFeatureReader(None, H.TINY, layer=2, engine=eng)
    waves = _waves48((5000, 3100), 24000.0)
    hubert.dump_features(rd, [("a", waves[0]), ("b", waves[1])], str(tmp_path / "feats"), sample_rate=24000)
    want = rd.get_feats_batch(waves, sample_rate=24000)
    for fid, w in zip("ab", want):
        assert np.array_equal(np.load(tmp_path / "feats" / f"{fid}.feat.npy"), w.cpu().numpy())


def test_asr_transcriber_takes_a_sample_rate():
    import wav2vec_ref as W
    from diffnorm_amd import asr

    eng = asr.Wav2VecCtcEngine(W.make_state_dict(W.TINY), W.TINY, W.TOKENS, dtype="f32", device=DEV)
    tr = asr.AsrTranscriber(eng, W.TOKENS)
    waves = _waves48()
    out, ol = resampler(48000, 16000).forward(waves)
    at16 = [out[i, :n] for i, n in enumerate(ol.tolist())]
    assert tr.transcribe(waves, sample_rate=48000) == tr.transcribe(at16)
    a, b = tr.forward(waves, sample_rate=48000), tr.forward(at16)
    assert a[0].shape[1] > 1 and all(torch.equal(x, y) for x, y in zip(a, b))  # emissions, frame counts, tokens, counts
    first = tr.resampler(48000)
    assert tr.resampler(48000) is first and first.handle.value
    for sr in (None, 16000):
        c = tr.forward(at16, sample_rate=sr)
        assert all(torch.equal(x, y) for x, y in zip(b, c)) and tr.transcribe(at16, sample_rate=sr) == tr.transcribe(at16)


def test_nar_model_takes_a_sample_rate():
    """forward_encoder / generate() of the waveform-input NAR model at 48 kHz = the same calls on the resampled batch."""
    import nar_oracle as N
    from diffnorm_amd import nar_decoder
    from diffnorm_amd.iterative_refinement import IterativeRefinementGenerator
    from gen_golden_nar_configs import CFG, ENC_CFG, Dict1004

    c = ENC_CFG
    model = nar_decoder.NARS2UTDecoderModel(
        N.make_nar_state_dict(CFG, "nar"), CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV,
        encoder_state_dict=N.make_nar_encoder_state_dict(c, "narenc"), waveform_input=True,
        encoder_kw=dict(input_dim=c.input_dim, conv_channels=c.conv_channels, kernel=c.kernel_sizes[0], ffn=c.ffn_dim, layers=c.layers))
    waves = [w * 3000.0 for w in _waves48((48000, 30000))]  # int16 scale, as the recipe's fbank takes it
    batch, lens = pad_batch(waves)
    batch, lens = batch.to(DEV), lens.to(DEV)
    b16, l16 = resampler(48000, 16000).forward(batch, lens)
    a, b = model.forward_encoder([batch, lens], sample_rate=48000), model.forward_encoder([b16, l16])
    assert torch.equal(a["encoder_out"][0], b["encoder_out"][0])
    gen = IterativeRefinementGenerator(Dict1004(), speech_source=True, max_iter=3, beam_size=1, adaptive=True)
    h48 = gen.generate([model], {"net_input": {"src_tokens": batch, "src_lengths": lens, "sample_rate": 48000}})
    h16 = gen.generate([model], {"net_input": {"src_tokens": b16, "src_lengths": l16}})
    assert len(h48) == len(h16) == 2
    for x, y in zip(h48, h16):
        assert x[0]["tokens"].tolist() == y[0]["tokens"].tolist()
