"""The HuBERT front end on the device (csrc/hubert.hip; diffnorm_amd/hubert.py) against the golden of the real classes
(tests/golden/hubert.npz) and the float64 restatement tests/hubert_ref.py.

Bars: the rule of tests/test_hip_nar_widths.py, ENGINE_TOL x max(1, scale / 4) on the max abs error; in f32 the error must also stay
within 8 x the float32 CPU restatement's own error against float64.  Measured errors are printed and recorded in DESIGN 9d."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubert_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ENGINE_TOL = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 6e-2}  # tests/test_hip_nar_widths.py's
DEV = "cuda:0"
_ENGINES, _SD = {}, {}


def _bar(dtype, ref):
    return ENGINE_TOL[dtype] * max(1.0, float(ref.abs().max()) / 4)


def state_dict(cfg):
    key = id(cfg)
    if key not in _SD:
        _SD[key] = R.make_state_dict(cfg, R.TINY_SEED)
    return _SD[key]


def engine(dtype, cfg=R.TINY):
    from diffnorm_amd import hubert

    key = (dtype, id(cfg))
    if key not in _ENGINES:
        _ENGINES[key] = hubert.HubertEngine(state_dict(cfg), cfg, dtype=dtype, device=DEV)
    return _ENGINES[key]


def run(eng, waves, layer):
    """A zero-padded batch of waveforms -> the list of [T_i, D] features (CPU), after checking the frame counts and the zero rows."""
    lens = torch.tensor([w.numel() for w in waves], dtype=torch.int32)
    batch = torch.zeros(len(waves), int(lens.max()))
    for j, w in enumerate(waves):
        batch[j, : w.numel()] = w
    out, olens = eng.forward(batch, lens, layer)
    out, olens = out.cpu(), olens.cpu()
    res = []
    for j, w in enumerate(waves):
        n = R.out_frames(eng.cfg, w.numel())
        assert int(olens[j]) == n
        assert float(out[j, n:].abs().max()) == 0.0 if n < out.shape[1] else True
        res.append(out[j, :n].clone())
    return res


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16", "bf16"])
def test_golden_parity(golden, dtype):
    G = golden("hubert")
    waves = [R.make_wave(n, 100 + i) for i, n in enumerate(R.GOLDEN_LENGTHS)]
    for layer in R.GOLDEN_LAYERS:
        got = run(engine(dtype), waves, layer)
        for i, g in enumerate(got):
            want = torch.from_numpy(G[f"feat_w{i}_l{layer}"])
            err, bar = float((g.double() - want).abs().max()), _bar(dtype, want)
            e32 = float((R.extract_features(state_dict(R.TINY), R.TINY, waves[i], layer, torch.float32).double() - want).abs().max())
            print(f"hubert golden {dtype} wave {i} layer {layer}: max abs err {err:.3e} (bar {bar:.1e}; float32 restatement {e32:.3e}, reference's own {float(G[f'e_ref32_w{i}_l{layer}']):.3e})")
            assert err <= bar
            if dtype == "f32":
                assert err <= 8 * e32


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ragged_batch_equals_each_alone_bit_for_bit(dtype):
    waves = [R.make_wave(n, 200 + i) for i, n in enumerate((3000, 1999, 731))]
    eng = engine(dtype)
    together = run(eng, waves, 3)
    for w, t in zip(waves, together):
        assert torch.equal(run(eng, [w], 3)[0], t)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_recipe_widths(dtype):
    sd = state_dict(R.RECIPE2)
    waves = [R.make_wave(n, 300 + i) for i, n in enumerate((8000, 5000, 400))]
    got = run(engine(dtype, R.RECIPE2), waves, 2)
    for w, g in zip(waves, got):  # the batch and each utterance alone land on different row tiles of the contractions: still the same bits
        assert torch.equal(run(engine(dtype, R.RECIPE2), [w], 2)[0], g)
    for i, (w, g) in enumerate(zip(waves, got)):
        want = R.extract_features(sd, R.RECIPE2, w, 2, torch.float64)
        err, bar = float((g.double() - want).abs().max()), _bar(dtype, want)
        msg = f"hubert recipe widths {dtype} wave {i} ({w.numel()} samples, {want.shape[0]} frames, scale {float(want.abs().max()):.2f}): max abs err {err:.3e} (bar {bar:.1e}"
        if dtype == "f32":
            e32 = float((R.extract_features(sd, R.RECIPE2, w, 2, torch.float32).double() - want).abs().max())
            print(msg + f"; float32 restatement {e32:.3e})")
            assert err <= 8 * e32
        else:
            print(msg + ")")
        assert err <= bar


def test_out_frames_entry_is_the_reference_formula():
    """dn_hubert_out_frames against _get_feat_extract_output_lengths (wav2vec2.py:564-579) over L = 400 .. 2000, both configurations."""
    import numpy as np

    for cfg in (R.TINY, R.RECIPE2):
        eng = engine("f32" if cfg is R.TINY else "f16", cfg)
        for L in range(380, 2001):
            n = L
            for _, k, s in R.conv_layers(cfg):
                n = int(np.floor((n - k) / s + 1)) if n >= k else 0
            assert eng.out_frames(L) == max(n, 0), L


def _odd_every_layer():
    """A length whose frame count is odd behind every stride-2 layer (and at least 3 frames at the end)."""
    for L in range(400, 20000):
        n, odd = L, True
        for i, (_, k, s) in enumerate(R.conv_layers(R.TINY)):
            n = (n - k) // s + 1
            odd = odd and (i == 0 or n % 2 == 1)
        if odd and n >= 3:
            return L
    raise AssertionError


@pytest.mark.parametrize("L", [400, 719, 720, 721, _odd_every_layer()])
def test_geometry_edges(L):
    w = R.make_wave(L, 400 + L)
    want = R.extract_features(state_dict(R.TINY), R.TINY, w, 3, torch.float64)
    got = run(engine("f32"), [w], 3)[0]
    e32 = float((R.extract_features(state_dict(R.TINY), R.TINY, w, 3, torch.float32).double() - want).abs().max())
    err = float((got.double() - want).abs().max())
    print(f"hubert f32 L={L} ({want.shape[0]} frames): max abs err {err:.3e} (float32 restatement {e32:.3e})")
    assert got.shape == want.shape and err <= _bar("f32", want)


def test_too_short_a_waveform_is_refused_with_nothing_launched():
    from diffnorm_amd import _lib

    eng = engine("f32")
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(1, 399), torch.tensor([399]), 3)
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(2, 800), torch.tensor([800, 399]), 3)
    out = torch.zeros(4, device=DEV)
    rc = eng.lib.dn_hubert_forward(eng.handle, out.data_ptr(), out.data_ptr(), 1, 399, 3, out.data_ptr(), out.data_ptr(), out.data_ptr(), 16, None)
    assert rc == -1 and b"shorter than one frame" in eng.lib.dn_last_error()
    rc = eng.lib.dn_hubert_forward(eng.handle, out.data_ptr(), out.data_ptr(), 1, 800, 4, out.data_ptr(), out.data_ptr(), out.data_ptr(), 16, None)
    assert rc == -1 and b"output layer" in eng.lib.dn_last_error()
    assert eng.lib.dn_hubert_workspace_bytes(eng.handle, 1, 399) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    # 2^31 elements: the first conv layer of a long batch at the recipe's width is refused, not launched
    big = engine("f16", R.RECIPE2)
    rc = big.lib.dn_hubert_forward(big.handle, out.data_ptr(), out.data_ptr(), 16, 1_600_000, 2, out.data_ptr(), out.data_ptr(), out.data_ptr(), 16, None)
    assert rc == -1 and b"2^31" in big.lib.dn_last_error()
    assert isinstance(_lib.DiffNormHipError("x"), RuntimeError)


@pytest.mark.parametrize("case", ["dc_offset", "long"])
def test_first_conv_statistics(case):
    """Per-utterance GroupNorm statistics over many tiles and on a mean far above the deviation: the same bar as everywhere."""
    w = R.make_wave(20_000, 7, dc=0.5, amp=1e-3) if case == "dc_offset" else R.make_wave(200_000, 8)
    want = R.extract_features(state_dict(R.TINY), R.TINY, w, 2, torch.float64)
    e32 = float((R.extract_features(state_dict(R.TINY), R.TINY, w, 2, torch.float32).double() - want).abs().max())
    got = run(engine("f32"), [w], 2)[0]
    err = float((got.double() - want).abs().max())
    print(f"hubert f32 statistics, {case} ({w.numel()} samples): max abs err {err:.3e} (bar {_bar('f32', want):.1e}; float32 restatement {e32:.3e})")
    assert err <= _bar("f32", want)


def test_workspace_regrowth_large_small_large():
    from diffnorm_amd import hubert

    eng = hubert.HubertEngine(state_dict(R.TINY), R.TINY, dtype="f32", device=DEV)
    big, small = [R.make_wave(6000, 1), R.make_wave(4500, 2)], [R.make_wave(800, 3)]
    first = run(eng, big, 3)
    run(eng, small, 3)
    third = run(eng, big, 3)
    assert all(torch.equal(a, b) for a, b in zip(first, third))


def test_stage_times_of_a_profiled_forward():
    """set_profile(True), one forward: stage_times() gives one finite, non-negative ms per stage of HubertEngine.STAGES; switched off
    again, the next forward returns the same bits."""
    import math

    eng = engine("f32")
    waves = [R.make_wave(3000, 300), R.make_wave(1999, 301)]
    base = run(eng, waves, 3)
    eng.set_profile(True)
    profiled = run(eng, waves, 3)
    times = eng.stage_times()
    eng.set_profile(False)
    assert len(times) == len(eng.STAGES) == 5 and all(math.isfinite(t) and t >= 0.0 for t in times), times
    after = run(eng, waves, 3)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(base, profiled, after))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_chunked_reader_equals_the_chunks_alone(dtype):
    from diffnorm_amd import hubert

    eng = engine(dtype)
    w = R.make_wave(10_000, 9)
    rd = hubert.HubertFeatureReader(None, R.TINY, layer=3, max_chunk=4000, engine=eng)
    got = rd.get_feats(w).cpu()
    alone = torch.cat([run(eng, [w[s:e]], 3)[0] for s, e in hubert.chunk_bounds(10_000, 4000)])
    assert torch.equal(got, alone)
    want = R.read_feats(state_dict(R.TINY), R.TINY, w, 3, 4000)
    assert got.shape == want.shape and float((got.double() - want).abs().max()) <= _bar(dtype, want)


def _kmeans_case(M):
    x, c = R.kmeans_near_tie_case(M)  # rows beside the bisector of two centroids of different norms: margins of 1e-4 .. 1e-2
    units, margin = R.kmeans_units(x, c)
    return x, c, units, margin


@pytest.mark.parametrize("M", [1, 63, 257])
def test_kmeans_assign(M):
    from diffnorm_amd import hubert

    x, c, units, margin = _kmeans_case(M)
    safe = margin >= 1e-4
    assert int((~safe).sum()) <= 0.01 * M  # (seeded inputs: checked on the CPU when they were chosen)
    assert int((margin[safe] <= 1e-2).sum()) >= 0.9 * M  # close decisions, not far ones (tests/test_hubert_host.py: bf16 operands or a missing bias fail them)
    got = hubert.KMeansQuantizer(c, device=DEV).predict(x).cpu().long()
    assert got.dtype == torch.int64 and torch.equal(got[safe], units[safe])


def test_kmeans_duplicated_centroid_yields_the_lower_index_and_golden_units(golden):
    from diffnorm_amd import hubert

    x, c, _, _ = _kmeans_case(63)
    c, x = c.clone(), x.clone()
    c[877] = c[123]  # identical rows give identical scores: an exact tie
    x[0] = c[123]
    got = hubert.KMeansQuantizer(c, device=DEV).predict(x).cpu()
    assert int(got[0]) == 123
    G = golden("hubert")
    feats = torch.cat([torch.from_numpy(G[f"feat_w{i}_l3"]) for i in range(3)]).float()
    assert float(G["margins"].min()) >= 1e-4
    assert hubert.KMeansQuantizer(torch.from_numpy(G["centers"]), device=DEV).predict(feats).cpu().tolist() == G["units"].tolist()


@pytest.mark.parametrize("k,groups,C,T", [(8, 4, 64, 37), (128, 16, 768, 61), (3, 1, 64, 200)])
def test_grouped_conv1d_operator(k, groups, C, T):
    """dn_grouped_conv1d alone against F.conv1d in float64: even and odd kernels, more than one tile, ragged lengths."""
    import torch.nn.functional as F

    from diffnorm_amd import _lib

    lib = _lib.load()
    B, Cg = 3, C // groups
    lens = torch.tensor([T, T // 2 + 1, 1], dtype=torch.int32)
    x = R._normal(k, "gc.x", (B, T, C), 1.0)
    w = R._normal(k, "gc.w", (C, Cg, k), (Cg * k) ** -0.5)
    bias = R._normal(k, "gc.b", (C,), 0.2)
    xd, out, bd, ld = x.to(DEV), torch.full((B, T, C), 7.0, device=DEV), bias.to(DEV), lens.to(DEV)
    wp = w.view(groups, Cg, Cg, k).permute(0, 3, 2, 1).contiguous().to(DEV)
    _lib.check(lib.dn_grouped_conv1d(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), ld.data_ptr(), B, T, C, groups, k,
                                     _lib.current_stream()), "dn_grouped_conv1d")
    out = out.cpu()
    for b in range(B):
        n = int(lens[b])
        xb = x[b, :n].double()
        y = F.conv1d(xb.t()[None], w.double(), bias.double(), 1, k // 2, 1, groups)[0, :, :n].t()
        want = xb + F.gelu(y)
        assert float((out[b, :n].double() - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))  # fp32 accumulation over k Cg <= 6144 terms
        assert float(out[b, n:].abs().max()) == 0.0 if n < T else True
