"""CPU checks of the HuBERT front end's host side: the plain-torch restatement against the golden of the real classes
(tools/gen_golden_hubert.py), the frame-count formula, the weight-norm fold and the packed table, the reader's chunk loop, the refusals
of the unsupported variants, the manifest round trip through diffnorm_amd/data.py and the k-means score formula."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hubert_ref as R  # noqa: E402

from diffnorm_amd import _lib, data, hubert, packing  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return R.make_state_dict(R.TINY, R.TINY_SEED)


def test_restatement_matches_the_golden_of_the_real_classes(golden, sd):
    G = golden("hubert")
    assert tuple(G["lengths"]) == R.GOLDEN_LENGTHS and tuple(G["layers"]) == R.GOLDEN_LAYERS
    for i, n in enumerate(R.GOLDEN_LENGTHS):
        wave = R.make_wave(n, 100 + i)
        for layer in R.GOLDEN_LAYERS:
            want = torch.from_numpy(G[f"feat_w{i}_l{layer}"])
            got = R.extract_features(sd, R.TINY, wave, layer, torch.float64)
            assert got.shape == want.shape == (int(G["frames"][i]), R.TINY.encoder_embed_dim)
            assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
            e32 = float((R.extract_features(sd, R.TINY, wave, layer, torch.float32).double() - want).abs().max())
            assert e32 < 50 * max(float(G[f"e_ref32_w{i}_l{layer}"]), 1e-7)  # float32 noise, like the reference's own
    units, margins = R.kmeans_units(torch.cat([torch.from_numpy(G[f"feat_w{i}_l3"]) for i in range(3)]), G["centers"])
    assert units.tolist() == G["units"].tolist() and np.allclose(margins.numpy(), G["margins"], rtol=1e-9, atol=1e-12)


def test_out_frames_is_the_reference_formula():
    """_get_feat_extract_output_lengths (wav2vec2.py:564-579): floor((len - k) / stride + 1) per layer, here against a conv stack run."""
    layers = hubert.conv_layers(hubert.MHUBERT_BASE)
    assert layers == [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2
    for L in range(400, 2001):
        n = L
        for _, k, s in layers:
            n = int(np.floor((n - k) / s + 1))
        assert hubert.out_frames(hubert.MHUBERT_BASE, L) == n == R.out_frames(R.RECIPE2, L)
    assert hubert.out_frames(hubert.MHUBERT_BASE, 399) == 0 and hubert.out_frames(hubert.MHUBERT_BASE, 400) == 1
    assert [hubert.out_frames(hubert.MHUBERT_BASE, L) for L in (719, 720, 721)] == [1, 2, 2]
    x = torch.zeros(1, 1, 1234)
    for _, k, s in layers:
        x = torch.nn.functional.conv1d(x, torch.zeros(1, 1, k), None, s)
    assert x.shape[-1] == hubert.out_frames(hubert.MHUBERT_BASE, 1234)


def test_weight_norm_fold_and_packed_shapes(sd):
    conv = torch.nn.Conv1d(64, 64, 8, padding=4, groups=4)
    with torch.no_grad():
        wn = torch.nn.utils.weight_norm(conv, name="weight", dim=2)
        wn.weight_g.copy_(sd["encoder.pos_conv.0.weight_g"])
        wn.weight_v.copy_(sd["encoder.pos_conv.0.weight_v"])
        wn(torch.zeros(1, 64, 9))  # (the hook recomputes .weight)
    w = hubert.pos_conv_weight(sd)
    assert w.dtype == torch.float64 and float((w.float() - wn.weight).abs().max()) < 1e-6
    assert float((w - R.pos_conv_weight(sd)).abs().max()) == 0.0
    for dtype in (_lib.DN_F32, _lib.DN_F16, _lib.DN_BF16X3):
        t = hubert.pack_hubert(sd, R.TINY, dtype)
        assert len(t) == 21 + 7
        assert t[0].shape == (16, 64) and float(t[0][10:].abs().max()) == 0 and torch.equal(t[0][:10].t(), sd["feature_extractor.conv_layers.0.0.weight"][:, 0])
        es = 2 if dtype == _lib.DN_BF16X3 else 1  # split rows: a bf16 tensor twice as wide
        assert t[3].shape == (128, 3 * 64 * es) and t[8].shape == (128, 2 * 64 * es)
        pos = t[13]
        assert pos.shape == (4, 8, 16, 16) and pos.dtype == torch.float32  # [g][tap][ci][co]
        assert float((pos[1, 3, 5, 7].double() - w[16 + 7, 5, 3]).abs()) < 1e-7
        assert t[17].shape[0] == 3 and t[25].shape == (3, 2, 64) and t[27].shape == (64,)
    big = hubert.pack_hubert(R.make_state_dict(R.RECIPE2, 5), R.RECIPE2, _lib.DN_F16)
    assert big[11].shape == (768, 512) and big[13].shape == (16, 128, 48, 48)


def test_chunk_loop_is_the_readers():
    assert hubert.chunk_bounds(10_000, 4000) == [(0, 4000), (4000, 8000), (8000, 10_000)]
    assert hubert.chunk_bounds(4000, 4000) == [(0, 4000)] and hubert.chunk_bounds(4001, 4000) == [(0, 4000), (4000, 4001)]
    sd = R.make_state_dict(R.TINY, R.TINY_SEED)
    wave = R.make_wave(2500, 7)
    whole = R.read_feats(sd, R.TINY, wave, 2, 1000)
    parts = [R.extract_features(sd, R.TINY, wave[s:e], 2) for s, e in hubert.chunk_bounds(2500, 1000)]
    assert torch.equal(whole, torch.cat(parts))

    class Engine:  # the loop itself, without a device: chunk r of every waveform that has one, as one zero-padded batch
        calls = []

        def forward(self, batch, lens, layer):
            Engine.calls.append((tuple(batch.shape), lens.tolist()))
            S = hubert.out_frames(R.TINY, batch.shape[1])
            out = torch.zeros(batch.shape[0], S, 1)
            for j, n in enumerate(lens.tolist()):
                out[j, : hubert.out_frames(R.TINY, n), 0] = batch[j, :n].sum()
            return out, None

    rd = hubert.HubertFeatureReader(None, R.TINY, layer=2, max_chunk=1000, engine=Engine())
    a, b = torch.arange(2500.0), torch.ones(900)
    fa, fb = rd.get_feats_batch([a, b])
    assert Engine.calls == [((2, 1000), [1000, 900]), ((1, 1000), [1000]), ((1, 500), [500])]
    assert fa.shape[0] == 2 * hubert.out_frames(R.TINY, 1000) + hubert.out_frames(R.TINY, 500) and fb.shape[0] == hubert.out_frames(R.TINY, 900)
    assert float(fa[0, 0]) == float(a[:1000].sum()) and float(fa[-1, 0]) == float(a[2000:].sum()) and float(fb[0, 0]) == 900.0
    with pytest.raises(ValueError, match="shorter than one frame"):
        rd.get_feats(torch.zeros(1100))  # the last chunk has 100 samples


@pytest.mark.parametrize("field,value", [("extractor_mode", "layer_norm"), ("layer_type", "conformer"), ("normalize", True), ("layer_norm_first", True),
                                         ("conv_bias", True), ("required_seq_len_multiple", 2), ("training", True), ("mask", True)])
def test_unsupported_variants_are_refused_on_the_host(sd, field, value):
    cfg = types.SimpleNamespace(**dict(vars(R.TINY), **{field: value}))
    with pytest.raises(ValueError, match="hubert"):
        hubert.pack_hubert(sd, cfg, _lib.DN_F32)
    with pytest.raises(ValueError, match="hubert"):
        hubert.HubertFeatureReader(sd, cfg, layer=2, engine=object())


def test_layer_norm_mode_state_dict_and_layer_range_are_refused(sd):
    bad = dict(sd)
    bad["feature_extractor.conv_layers.1.2.1.weight"] = torch.ones(64)
    with pytest.raises(ValueError, match="layer_norm"):
        hubert.pack_hubert(bad, R.TINY, _lib.DN_F32)
    with pytest.raises(ValueError, match="layer 4"):
        hubert.HubertFeatureReader(sd, R.TINY, layer=4, engine=object())


def test_dump_features_round_trips_through_the_data_reader(tmp_path):
    class Reader:
        def get_feats_batch(self, waves):
            return [torch.full((len(w) // 320, 4), float(len(w))) for w in waves]

    items = [(f"utt{i}.wav", np.zeros(640 * (i + 1), dtype=np.float32)) for i in range(3)]
    manifest = hubert.dump_features(Reader(), items, str(tmp_path / "train"), batch=2)
    assert manifest == str(tmp_path / "train.manifest.tsv")
    got = data.read_feature_manifest(manifest)
    assert sorted(got) == ["utt0", "utt1", "utt2"]
    for i in range(3):
        path, n = got[f"utt{i}"]
        f = np.load(path)
        assert int(n) == f.shape[0] == 2 * (i + 1) and f.shape[1] == 4 and float(f[0, 0]) == 640.0 * (i + 1)


def test_kmeans_score_is_the_arg_min_of_the_distances():
    """argmax_j (x . c_j - |c_j|^2 / 2) over the packed tables == argmin_j |x - c_j|^2 in float64, ties to the lowest index."""
    rs = np.random.RandomState(3)
    x, c = torch.from_numpy(rs.standard_normal((200, 64))), torch.from_numpy(rs.standard_normal((50, 64)))
    c[31] = c[12]  # a duplicated centroid
    x[5] = c[12]
    W, half = hubert.kmeans_scores_tables(c)
    assert W.shape == (128, 64) and half.shape == (52,) and W.dtype == torch.float32 and float(W[50:].abs().max()) == 0
    score = x @ W[:50].double().t() + half[:50].double()
    d = R.kmeans_distances(x, c)
    units, margin = R.kmeans_units(x, c)
    safe = margin >= 1e-6
    assert int(safe.sum()) >= 180  # (the rows nearest the duplicated centroid tie exactly)
    assert torch.equal(score.argmax(1)[safe], d.argmin(1)[safe]) and torch.equal(units, d.argmin(1))
    assert int(d.argmin(1)[5]) == 12 and int(score.argmax(1)[5]) == 12
    assert packing.padn(50) == 128


@pytest.mark.parametrize("M", [63, 257])
def test_near_tie_inputs_tell_fp32_class_scores_from_lesser_ones(M):
    """The seeded inputs of the device test (tests/test_hip_hubert.py::test_kmeans_assign): at most 1 % of the rows under the 1e-4
    margin, the rest close decisions that an fp32 score gets right and that bf16-rounded operands or a score without -|c|^2 / 2 do not."""
    x, c = R.kmeans_near_tie_case(M)
    units, margin = R.kmeans_units(x, c)
    safe = margin >= 1e-4
    assert int((~safe).sum()) <= 0.01 * M and int((margin[safe] <= 1e-2).sum()) >= 0.9 * M
    W, half = hubert.kmeans_scores_tables(c)
    f32 = (x @ W[:1000].t() + half[:1000]).argmax(1)
    assert torch.equal(f32[safe], units[safe])
    bf16 = (x.bfloat16().double() @ c.bfloat16().double().t() + half[:1000].double()).argmax(1)
    no_bias = (x.double() @ c.double().t()).argmax(1)
    assert int((bf16 != units)[safe].sum()) >= 0.05 * M and int((no_bias != units)[safe].sum()) >= 0.3 * M
