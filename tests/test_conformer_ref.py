"""The Conformer speech encoder off the device: the plain-torch restatement of tests/conformer_ref.py against the REAL reference's
float64 output (tests/golden/conformer_encoder.npz, tools/gen_golden_conformer.py), the packing of the engine's tensor table (BatchNorm
fold, half-step fold, the float32 position table, the refusals) and the resource check of the new attention unit."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import conformer_ref as R

T_ = torch.from_numpy


def _inputs(g):
    lens = T_(g["lens"])
    return R.make_features(lens.numel(), int(lens.max()), lens, R.TINY.input_dim, int(g["seed_feats"]))


def test_restatement_matches_the_real_reference_in_float64(golden):
    """float64 against float64: rounding is orders below 1e-9 x scale; the bar only separates a right restatement from a wrong one.
    Both the ragged batch and the shortest utterance alone (whose output differs from its rows in the batch: the convolution module
    is not masked)."""
    g = golden("conformer_encoder")
    feats, lens = _inputs(g)
    sd = R.make_state_dict()
    want = T_(g["encoder_out"]).transpose(0, 1)
    scale = want.abs().max().item()
    with torch.no_grad():
        got, ol = R.encode(sd, R.TINY, feats, lens, torch.float64)
        i = int(g["alone_index"])
        n = int(lens[i])
        alone, _ = R.encode(sd, R.TINY, feats[i:i + 1, :n], lens[i:i + 1], torch.float64)
    assert ol.tolist() == g["out_lens"].tolist()
    assert torch.equal(torch.arange(want.shape[1])[None, :] >= ol[:, None], T_(g["padding_mask"]))
    assert (got - want).abs().max().item() < 1e-9 * scale
    assert (alone[0] - T_(g["alone_out"])).abs().max().item() < 1e-9 * scale
    Si = alone.shape[1]
    assert abs((alone[0] - got[i, :Si]).abs().max().item() - float(g["alone_vs_batch"])) < 1e-9 * scale
    assert float(g["alone_vs_batch"]) > 1e3 * float(g["e_ref32"])


def test_packing_folds_reproduce_the_unfolded_form_in_float64():
    """BatchNorm folded into the depthwise weights and the half step folded into w_2, as pack_conformer_encoder does, against the
    unfolded restatement, both in float64."""
    from diffnorm_amd import nar_decoder

    sd = {k: v.double() for k, v in R.make_state_dict().items()}
    D, K = R.TINY.embed_dim, R.TINY.depthwise_kernel
    p = "conformer_layers.1.conv_module."
    x = torch.from_numpy(__import__("numpy").random.RandomState(5).standard_normal((3, 40, 2 * D)))
    want = R.glu_dwconv(x, sd[p + "depthwise_conv.weight"], sd[p + "batch_norm.weight"], sd[p + "batch_norm.bias"], sd[p + "batch_norm.running_mean"],
                        sd[p + "batch_norm.running_var"])
    w, shift = nar_decoder.fold_batch_norm(sd[p + "depthwise_conv.weight"], sd[p + "batch_norm.weight"], sd[p + "batch_norm.bias"],
                                           sd[p + "batch_norm.running_mean"], sd[p + "batch_norm.running_var"])
    assert w.shape == (D, K) and shift.shape == (D,)
    y = F.conv1d(F.glu(x, dim=-1).transpose(1, 2), w[:, None, :], None, 1, K // 2, 1, D) + shift[None, :, None]
    assert (F.silu(y).transpose(1, 2) - want).abs().max().item() < 1e-12 * want.abs().max().item()
    f = "conformer_layers.0.ffn2."
    h = x[..., :R.TINY.ffn_dim]
    want = 0.5 * F.linear(h, sd[f + "w_2.weight"], sd[f + "w_2.bias"])
    assert torch.equal(F.linear(h, 0.5 * sd[f + "w_2.weight"], 0.5 * sd[f + "w_2.bias"]), want)  # a power of two: exact


def test_packed_table_and_position_rows():
    """The packed table has the layout dn_conformer_encoder_create documents; the position table's d = 0 row is [0, 1, 0, 1, ...] and
    rows +-d are the float32 formula of RelPositionalEncoding bit for bit."""
    from diffnorm_amd import _lib, nar_decoder

    c = R.TINY
    M = 7
    t = nar_decoder.pack_conformer_encoder(R.make_state_dict(), c.input_dim, c.conv_channels, c.kernel_sizes[0], c.embed_dim, c.ffn_dim, c.layers, c.heads,
                                           c.depthwise_kernel, M, _lib.DN_F32)
    assert len(t) == 29
    pe = t[6]
    assert pe.shape == (2 * M - 1, c.embed_dim) and pe.dtype == torch.float32
    assert torch.equal(pe[M - 1], torch.tensor([0.0, 1.0] * (c.embed_dim // 2)))
    div = torch.exp(torch.arange(0, c.embed_dim, 2, dtype=torch.float32) * -(math.log(10000.0) / c.embed_dim))
    for d in (1, 3, M - 1):
        pos = torch.tensor(float(d), dtype=torch.float32)
        assert torch.equal(pe[M - 1 + d, 0::2], torch.sin(pos * div)) and torch.equal(pe[M - 1 + d, 1::2], torch.cos(pos * div))
        assert torch.equal(pe[M - 1 - d, 0::2], torch.sin(-1 * pos * div)) and torch.equal(pe[M - 1 - d, 1::2], torch.cos(-1 * pos * div))
    assert torch.equal(pe, R.rel_pe(M, c.embed_dim))
    assert t[23].shape == (c.layers, c.embed_dim, c.depthwise_kernel) and t[26].shape == (c.layers, 5, c.embed_dim)
    sd = R.make_state_dict()
    assert torch.equal(t[10][1], 0.5 * sd["conformer_layers.1.ffn1.w_2.bias"])
    assert torch.equal(t[20][0], sd["conformer_layers.0.self_attn.pos_bias_u"].reshape(-1))
    assert not any("num_batches_tracked" in k for k in sd)


@pytest.mark.parametrize("kw", [dict(pos_enc_type="abs"), dict(pos_enc_type="rope"), dict(attn_type=None), dict(conv_version="convtransformer"),
                                dict(depthwise_kernel=30)])
def test_unsupported_variants_are_refused_on_the_host(kw):
    from diffnorm_amd import _lib, nar_decoder

    c = R.TINY
    args = dict(depthwise_kernel=c.depthwise_kernel)
    args.update(kw)
    dk = args.pop("depthwise_kernel")
    with pytest.raises(ValueError):
        nar_decoder.pack_conformer_encoder(R.make_state_dict(), c.input_dim, c.conv_channels, c.kernel_sizes[0], c.embed_dim, c.ffn_dim, c.layers, c.heads,
                                           dk, 7, _lib.DN_F32, **args)


def test_speaker_projection_is_refused():
    from diffnorm_amd import _lib, nar_decoder

    c = R.TINY
    sd = R.make_state_dict()
    sd["spk_emb_proj.weight"] = torch.zeros(c.embed_dim, c.embed_dim + 8)
    with pytest.raises(ValueError):
        nar_decoder.pack_conformer_encoder(sd, c.input_dim, c.conv_channels, c.kernel_sizes[0], c.embed_dim, c.ffn_dim, c.layers, c.heads, c.depthwise_kernel,
                                           7, _lib.DN_F32)


def test_rel_attention_unit_has_no_scratch_in_its_loops():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import check_resources

    assert check_resources.check(["rel_attention.hip"]) == []
