"""The fold of the feed-forward block's CausalConv1d(inner, inner, 3) into the Linear(inner, dim) after it, restated in float64 on
the host: W'_j = W_out . W_conv_j, b' = W_out . b_conv + b_out applied as ONE causal conv of three taps equals the oracle's
Linear(CausalConv1d(g)) -- on whole sequences (the first two frames carry the causal zero padding) and on the flattened [B T, inner]
rows the kernels see, where a sequence starts in the middle of a 128- or 256-row tile."""
import pytest
import torch

import diffnorm_oracle as O
from diffnorm_amd import _lib, packing

SHAPES = [(64, 85), (128, 170), (512, 1365)]  # (dim, inner): two free pairs and the flagship model's
BATCHES = [(3, 100), (2, 515)]                # [B, T]: rows 100, 200 / 515 are sequence starts inside a row tile


def _weights(dim, inner, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(inner, inner, 3) / (3 * inner) ** 0.5, r(inner), r(dim, inner) / inner ** 0.5, r(dim)


def _folded_rows(g_rows, T, Wf, bf):
    """The contraction as the engine issues it on flattened rows: x[m] = sum_j W'_j g[m - (2 - j)] + b', a term dropped where the
    shifted row would lie before its sequence's start."""
    M = g_rows.shape[0]
    t = torch.arange(M) % T
    out = bf.expand(M, -1).clone()
    for j in range(3):
        sh = 2 - j
        src = torch.roll(g_rows, sh, 0)
        src[t < sh] = 0
        out += src @ Wf[j].T
    return out


@pytest.mark.parametrize("dim,inner", SHAPES)
@pytest.mark.parametrize("B,T", BATCHES)
def test_fold_equals_linear_of_causal_conv(dim, inner, B, T):
    cw, cb, ow, ob = _weights(dim, inner, dim + T)
    g = torch.randn(B, T, inner, generator=torch.Generator().manual_seed(T), dtype=torch.float64)
    want = torch.nn.functional.linear(O.causal_conv1d(g, cw, cb), ow, ob)
    Wf, bf = packing.ffn_fold_ref(cw, cb, ow, ob)
    assert Wf.shape == (3, dim, inner) and bf.shape == (dim,)
    got = _folded_rows(g.reshape(B * T, inner), T, Wf, bf).reshape(B, T, dim)
    scale = want.abs().max().item()
    assert (got - want).abs().max().item() < 1e-12 * scale
    assert (got[:, :2] - want[:, :2]).abs().max().item() < 1e-12 * scale  # the frames whose taps reach into the padding
    # the folded conv IS a causal conv: the oracle's own CausalConv1d on the folded weights gives the same
    conv = O.causal_conv1d(g, Wf.permute(1, 2, 0).contiguous(), bf)
    assert (conv - want).abs().max().item() < 1e-12 * scale


def test_fold_sources_and_offsets_follow_the_tables():
    """The packed fp32 sources dn_ffn_fold reads (a state dict's, a flat training buffer's) are the tables' ffconv / ffout entries,
    a constant distance apart from layer to layer; their padding is zero and the float64 fold of the packed tensors is the fold of
    the reference's tensors."""
    cfg = O.EpsConfig(dim=64, latent_dim=16, depth=3, heads=4, dim_head=16, wavenet_layers=2, wavenet_stacks=1)
    sd = O.make_eps_state_dict(cfg, "fold")
    inner = int(64 * 4 * 2 / 3)  # 170
    ip, Dn = packing.padk(inner), packing.padn(64)
    layers = packing._eps_entries(cfg)[2]
    entries = packing.eps_train_entries(cfg)
    offsets, total = [], 0
    for e in entries:
        offsets.append(total)
        n = 1
        for d in e.shape:
            n *= d
        total += (n + 63) // 64 * 64
    flat = packing.pack_flat(sd, entries, offsets, total)
    offs, strides = packing.ffn_fold_offsets(entries, offsets)
    for l, layer in enumerate(layers):
        cw, cb, ow, ob = packing.ffn_fold_sources(layer, sd)
        assert cw.shape == (3, packing.padn(inner), ip) and ow.shape == (Dn, ip) and cb.shape == (ip,) and ob.shape == (64,)
        for t, o, st in zip((cw, cb, ow, ob), offs, strides):
            assert torch.equal(flat[o + l * st: o + l * st + t.numel()], t.reshape(-1))
        assert cw[:, inner:].abs().max() == 0 and cw[:, :, inner:].abs().max() == 0 and ow[64:].abs().max() == 0 and ow[:, inner:].abs().max() == 0
        p = f"transformer.layers.{l}.5."
        Wf, bf = packing.ffn_fold_ref(sd[p + "2.1.weight"], sd[p + "2.1.bias"], sd[p + "3.weight"], sd[p + "3.bias"])
        Wp = torch.stack([ow.double() @ cw[j, :ip].double() for j in range(3)])
        assert (Wp[:, :64, :inner] - Wf).abs().max() < 1e-13 and Wp[:, 64:].abs().max() == 0 and Wp[:, :, inner:].abs().max() == 0
        assert (ow.double()[:64] @ cb.double() + ob.double() - bf).abs().max() < 1e-13
    (w_shape, w_dtype), b_shape = packing.ffn_fold_storage(64, 3, _lib.DN_F32)
    assert b_shape == (3, 64) and w_shape == (3, 3, Dn, ip) and w_dtype == torch.float32
    assert packing.ffn_fold_storage(64, 3, _lib.DN_BF16X3)[0] == ((3, 3, Dn, 2 * ip), torch.bfloat16)
