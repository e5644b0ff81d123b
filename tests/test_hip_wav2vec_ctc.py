"""The wav2vec 2.0 CTC recogniser on the device (csrc/hubert.hip; diffnorm_amd/asr.py, diffnorm_amd/hubert.py) against the golden of
the real classes (tests/golden/wav2vec_ctc.npz) and the float64 restatement tests/wav2vec_ref.py.

Bars: the rule of tests/test_hip_nar_widths.py, ENGINE_TOL x max(1, scale / 4) on the max abs error against float64.  A frame whose
float64 top-2 margin is at least 2 x that bar cannot change its arg-max under an error within the bar; the frames below it are left
out of the arg-max comparison (at most 10 % of them).  Measured errors are printed and recorded in DESIGN 9f."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wav2vec_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

ENGINE_TOL = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 6e-2}  # tests/test_hip_nar_widths.py's
DEV = "cuda:0"
_ENGINES, _SD, _REF = {}, {}, {}


def _bar(dtype, ref):
    return ENGINE_TOL[dtype] * max(1.0, float(ref.abs().max()) / 4)


def state_dict(cfg):
    if id(cfg) not in _SD:
        _SD[id(cfg)] = W.make_state_dict(cfg)
    return _SD[id(cfg)]


def engine(dtype, cfg=W.TINY):
    from diffnorm_amd import asr

    key = (dtype, id(cfg))
    if key not in _ENGINES:
        _ENGINES[key] = asr.Wav2VecCtcEngine(state_dict(cfg), cfg, W.TOKENS, dtype=dtype, device=DEV)
    return _ENGINES[key]


def ref(cfg, wave, key):
    """The float64 emissions of a waveform, computed once."""
    if key not in _REF:
        _REF[key] = W.emissions(state_dict(cfg), cfg, wave)
    return _REF[key]


def run(eng, waves, pad=0.0):
    """A padded batch -> per utterance (emissions [T_i, V], token ids list) on the CPU, after checking frame counts and zero rows."""
    lens = torch.tensor([w.numel() for w in waves], dtype=torch.int32)
    batch = torch.full((len(waves), int(lens.max())), pad)
    for j, w in enumerate(waves):
        batch[j, : w.numel()] = w
    em, olens, toks, counts = eng.forward(batch, lens)
    em, olens, toks, counts = em.cpu(), olens.cpu(), toks.cpu(), counts.cpu()
    res = []
    for j, w in enumerate(waves):
        n = W.out_frames(eng.cfg, w.numel())
        assert int(olens[j]) == n and em.shape[2] == eng.vocab
        assert n == em.shape[1] or float(em[j, n:].abs().max()) == 0.0
        res.append((em[j, :n].clone(), toks[j, : int(counts[j])].tolist()))
    return res


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16", "bf16"])
def test_golden_parity_argmax_tokens_and_strings(golden, dtype):
    from diffnorm_amd import asr

    G = golden("wav2vec_ctc")
    waves = [W.golden_wave(i) for i in range(len(W.GOLDEN_WAVES))]
    got = run(engine(dtype), waves)
    texts = asr.AsrTranscriber(engine(dtype), W.TOKENS).transcribe(waves)
    sil_texts = asr.AsrTranscriber(engine(dtype), W.SIL_TOKENS, "none").transcribe(waves)  # `|` on a row that wins golden frames
    assert 0 in G["argmax_w0"] and any(" " in W.text(G[f"ids_w{i}"].tolist(), W.SIL_TOKENS) for i in range(len(waves)))
    left_out = total = 0
    for i, (em, ids) in enumerate(got):
        want = torch.from_numpy(G[f"em_w{i}"])
        err, bar, e32 = float((em.double() - want).abs().max()), _bar(dtype, want), float(G[f"e_ref32_w{i}"])
        print(f"wav2vec ctc golden {dtype} wave {i}: max abs err {err:.3e} (bar {bar:.1e}, scale {float(want.abs().max()):.2f}; reference's own float32 "
              f"{e32:.3e}, ratio {err / e32:.2f})")
        assert err <= bar
        safe = torch.from_numpy(G[f"margin_w{i}"]) >= 2 * bar
        left_out, total = left_out + int((~safe).sum()), total + safe.numel()
        assert torch.equal(em.argmax(-1)[safe], torch.from_numpy(G[f"argmax_w{i}"])[safe])
        assert ids == W.ctc_greedy(em)  # the device decode of the device emissions
        if dtype in ("f32", "bf16x3"):
            assert ids == G[f"ids_w{i}"].tolist() and texts[i] == W.text(G[f"ids_w{i}"].tolist())
            assert sil_texts[i] == W.text(G[f"ids_w{i}"].tolist(), W.SIL_TOKENS, "none")
    print(f"wav2vec ctc golden {dtype}: {left_out} of {total} frames under the margin")
    assert left_out <= 0.1 * total


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("layer", W.GOLDEN_LAYERS)
def test_layer_features_of_the_pre_norm_form_through_the_reader(golden, dtype, layer):
    """k < n and k = n: the un-normalised stream (HubertModel.extract_features(output_layer=k) hands the encoder a layer)."""
    from diffnorm_amd import hubert

    G = golden("wav2vec_ctc")
    rd = hubert.HubertFeatureReader(None, W.TINY, layer=layer, engine=engine(dtype))
    waves = [W.golden_wave(i) for i in range(len(W.GOLDEN_WAVES))]
    for i, f in enumerate(rd.get_feats_batch(waves)):
        want = torch.from_numpy(G[f"feat_w{i}_l{layer}"])
        err = float((f.cpu().double() - want).abs().max())
        print(f"wav2vec layer-{layer} features {dtype} wave {i}: max abs err {err:.3e} (bar {_bar(dtype, want):.1e})")
        assert f.shape == want.shape and err <= _bar(dtype, want)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ragged_batch_equals_each_alone_bit_for_bit_with_nan_padding(dtype):
    waves = [W.R.make_wave(n, 600 + i, dc=dc) for i, (n, dc) in enumerate(((3000, 0.0), (1999, 2.0), (731, 0.0)))]
    eng = engine(dtype)
    together = run(eng, waves, pad=float("nan"))
    for w, (em, ids) in zip(waves, together):
        alone_em, alone_ids = run(eng, [w])[0]
        assert torch.equal(alone_em, em) and alone_ids == ids and not torch.isnan(em).any()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_recipe_widths(dtype):
    wave = W.R.make_wave(16000, 700)
    want = ref(W.RECIPE2, wave, "recipe")
    em, ids = run(engine(dtype, W.RECIPE2), [wave])[0]
    err, bar = float((em.double() - want).abs().max()), _bar(dtype, want)
    print(f"wav2vec ctc recipe widths {dtype} ({want.shape[0]} frames, scale {float(want.abs().max()):.2f}): max abs err {err:.3e} (bar {bar:.1e})")
    assert em.shape == want.shape and err <= bar
    safe = W.top2_margin(want) >= 2 * bar
    assert torch.equal(em.argmax(-1)[safe], want.argmax(-1)[safe]) and int((~safe).sum()) <= 0.1 * safe.numel()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_vocabulary_that_is_no_multiple_of_four(dtype):
    """V = 45 (the Hugging Face letter models): the head's three pad columns stay out of the emissions."""
    from diffnorm_amd import asr

    sd = W.make_state_dict(W.TINY, W.TINY_SEED + 1, vocab=45)
    eng = asr.Wav2VecCtcEngine(sd, W.TINY, None, dtype=dtype, device=DEV)
    waves = [W.R.make_wave(n, 900 + i) for i, n in enumerate((2300, 1500))]
    for w, (em, ids) in zip(waves, run(eng, waves, pad=float("nan"))):
        want = W.emissions(sd, W.TINY, w)
        err = float((em.double() - want).abs().max())
        print(f"wav2vec ctc V=45 {dtype} ({want.shape[0]} frames): max abs err {err:.3e} (bar {_bar(dtype, want):.1e})")
        assert em.shape == want.shape == (W.out_frames(W.TINY, w.numel()), 45) and err <= _bar(dtype, want)
        assert ids == W.ctc_greedy(em)


def _odd_every_layer():
    for L in range(400, 20000):
        n, odd = L, True
        for i, (_, k, s) in enumerate(W.conv_layers(W.TINY)):
            n = (n - k) // s + 1
            odd = odd and (i == 0 or n % 2 == 1)
        if odd and n >= 3:
            return L
    raise AssertionError


@pytest.mark.parametrize("L", [400, 719, 720, 721, _odd_every_layer()])
def test_geometry_edges(L):
    w = W.R.make_wave(L, 800 + L)
    want = W.emissions(state_dict(W.TINY), W.TINY, w)
    em, ids = run(engine("f32"), [w])[0]
    err = float((em.double() - want).abs().max())
    print(f"wav2vec ctc f32 L={L} ({want.shape[0]} frames): max abs err {err:.3e} (bar {_bar('f32', want):.1e})")
    assert em.shape == want.shape and err <= _bar("f32", want)


def test_too_short_a_waveform_is_refused_with_nothing_launched():
    eng = engine("f32")
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(1, 399), torch.tensor([399]))
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(2, 800), torch.tensor([800, 399]))
    out = torch.zeros(4, device=DEV)
    rc = eng.lib.dn_hubert_ctc_forward(eng.handle, out.data_ptr(), out.data_ptr(), 1, 399, out.data_ptr(), out.data_ptr(), out.data_ptr(), 16, None)
    assert rc == -1 and b"dn_hubert_ctc_forward" in eng.lib.dn_last_error() and b"shorter than one frame" in eng.lib.dn_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def test_workspace_regrowth_large_small_large():
    from diffnorm_amd import asr

    eng = asr.Wav2VecCtcEngine(state_dict(W.TINY), W.TINY, W.TOKENS, dtype="f32", device=DEV)
    big, small = [W.R.make_wave(6000, 1), W.R.make_wave(4500, 2)], [W.R.make_wave(800, 3)]
    first = run(eng, big)
    run(eng, small)
    third = run(eng, big)
    assert all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(first, third))


@pytest.mark.parametrize("case", ["dc_offset", "constant", "long"])
def test_waveform_normaliser(case):
    """A DC offset of 1e3 on unit noise, a constant waveform (variance 0: the eps path), a length spanning many tiles."""
    if case == "dc_offset":
        w = (1e3 + W._normal(5, "wn", (5000,), 1.0).double()).float()
    elif case == "constant":
        w = torch.full((3000,), 0.75)
    else:
        w = W.R.make_wave(100_000, 8, dc=0.3)
    want = W.emissions(state_dict(W.TINY), W.TINY, w)
    em, _ = run(engine("f32"), [w])[0]
    err = float((em.double() - want).abs().max())
    print(f"wav2vec ctc f32 normaliser, {case} ({w.numel()} samples): max abs err {err:.3e} (bar {_bar('f32', want):.1e})")
    assert err <= _bar("f32", want)


def _host_greedy(em, lens, blank):
    out = []
    for e, n in zip(em, lens):
        tok = e[:n].argmax(-1).tolist() if n else []  # (torch.argmax: the first maximum; checked against the rows in the ties case below)
        out.append([t for i, t in enumerate(tok) if t != blank and (i == 0 or t != tok[i - 1])])
    return out


def _greedy(em, lens, blank):
    from diffnorm_amd import asr

    toks, counts = asr.ctc_greedy(em.to(DEV), torch.tensor(lens), blank)
    toks, counts = toks.cpu(), counts.cpu()
    return [toks[b, : int(counts[b])].tolist() for b in range(em.shape[0])]


def _one_hot(path, V):
    em = torch.full((1, len(path), V), -1.0)
    for t, v in enumerate(path):
        em[0, t, v] = 1.0
    return em


@pytest.mark.parametrize("path,blank,want", [([0, 0, 0, 0], 0, []), ([2, 2, 2], 0, [2]), ([1, 0, 1], 0, [1, 1]), ([1, 1], 0, [1]),
                                             ([0, 3, 3, 0, 2, 0], 0, [3, 2]), ([1, 4, 4, 1, 0, 0, 1], 1, [4, 0])])
def test_ctc_greedy_constructed_paths(path, blank, want):
    assert _greedy(_one_hot(path, 5), [len(path)], blank) == [want]


def test_ctc_greedy_exact_ties_take_the_lowest_index():
    em = torch.zeros(1, 6, 7)
    em[0, 1, 3] = em[0, 1, 5] = 2.0       # 3 and 5 tie
    em[0, 2, 6] = em[0, 2, 4] = 1.0       # 4 and 6 tie
    em[0, 3, :] = -1.0                    # all equal: index 0 (the blank)
    em[0, 4, 1:] = 0.5                    # 1 .. 6 tie
    assert _greedy(em, [6], 0) == [[3, 4, 1]]  # frames 0, 3, 5 are all-equal rows: blank


@pytest.mark.parametrize("S", [1, 255, 256, 257, 1025, 3000])
@pytest.mark.parametrize("V,blank", [(2, 0), (5, 4), (32, 0), (45, 44), (300, 7)])
def test_ctc_greedy_sizes_against_the_host_restatement(S, V, blank):
    """Runs of equal tokens and blanks across the 256-frame rounds; a ragged batch whose padding frames hold NaN and +inf."""
    g = torch.Generator().manual_seed(S * 1000 + V)
    lens = [S, max(1, S // 2), max(1, S - 1)]
    path = torch.randint(0, V, (3, S), generator=g)
    hold = torch.rand(3, S, generator=g) < 0.6  # repeat the previous frame's token
    for t in range(1, S):
        path[:, t] = torch.where(hold[:, t], path[:, t - 1], path[:, t])
    path[torch.rand(3, S, generator=g) < 0.2] = blank
    em = torch.randn(3, S, V, generator=g)
    em.scatter_(2, path[..., None], 6.0)
    want = _host_greedy(em, lens, blank)
    for b, n in enumerate(lens):
        em[b, n:, 0::2] = float("nan")
        em[b, n:, 1::2] = float("inf")
    assert _greedy(em, lens, blank) == want
