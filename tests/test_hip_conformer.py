"""The Conformer speech encoder on the device: dn_rel_attention and dn_glu_dwconv against float64 restatements of their formulas, the
engine against the REAL reference's float64 output (tests/golden/conformer_encoder.npz) and, at the recipe's widths, against the
float64 restatement of tests/conformer_ref.py evaluated here; generate() from features through a conformer encoder; the workspace's
growth and the longest source."""
import functools

import numpy as np
import pytest
import torch

import conformer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STORE = {"f32": torch.float32, "x3": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FWD_TOL = {"f32": 2e-5, "x3": 2e-5, "f16": 3e-3, "bf16": 2e-2}  # tests/test_hip_attention_grid.py's, relative to the output's max
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}  # unit roundoff of the 2-byte formats
ENGINE_TOL = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 6e-2}  # test_nar_speech_encoder_matches_the_real_reference's


def _randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).float()


def _rt(t, mode):
    """fp32 -> what the device holds in `mode`, as float64."""
    return t.to(STORE[mode]).double()


@functools.lru_cache(maxsize=None)
def _attn_case(dk, T):
    """Inputs (fp32) of one attention case: 2 heads, B = 3, ragged lengths with 1 and T among them, a table built for T + 37 frames."""
    H, B, Tmax = 2, 3, T + 37
    s = 1000 * dk + T
    q, k, v = (_randn(s + i, B, T, H * dk) for i in range(3))
    pos = _randn(s + 3, 2 * Tmax - 1, H * dk)
    u, vb = 0.5 * _randn(s + 4, H, dk), 0.5 * _randn(s + 5, H, dk)
    lens = torch.tensor([T, 1, max(1, (2 * T) // 3)])
    return q, k, v, pos, u, vb, lens, H, Tmax


def _attn_ref(q, k, v, pos, u, vb, lens, H, Tmax, rnd=None):
    """float64 restatement on [B, T, H dk] tensors; rnd: the roundings the 2-byte kernels apply inside (q + u, q + v, P)."""
    B, T, hd = q.shape
    dk = hd // H
    heads = lambda t: t.view(B, T, H, dk).transpose(1, 2)
    p = pos[Tmax - 1 - (T - 1): Tmax - 1 + T].view(2 * T - 1, H, dk).transpose(0, 1)
    qh, kh, vh = heads(q), heads(k), heads(v)
    if rnd is None:
        o = R.rel_attention(qh, kh, vh, p, u, vb, lens)
    else:
        qu, qv = rnd(qh + u[None, :, None, :]), rnd(qh + vb[None, :, None, :])
        ac = qu @ kh.transpose(-1, -2)
        bd_all = qv @ p.transpose(-1, -2)[None]
        idx = (T - 1) + torch.arange(T)[:, None] - torch.arange(T)[None, :]
        sc = (ac + torch.gather(bd_all, 3, idx[None, None].expand(B, H, T, T))) * dk ** -0.5
        sc = sc.masked_fill((torch.arange(T)[None, :] >= lens[:, None])[:, None, None, :], float("-inf"))
        e = torch.exp(sc - sc.max(-1, keepdim=True).values)
        o = rnd(rnd(e) @ vh / e.sum(-1, keepdim=True))  # P rounded once, the row sum of the unrounded P, the output stored in the format
    return o.transpose(1, 2).reshape(B, T, hd)


@pytest.mark.parametrize("mode", ["f32", "x3", "f16", "bf16"])
@pytest.mark.parametrize("T", [1, 17, 64, 65, 130, 300])
@pytest.mark.parametrize("dk", [16, 32, 64])
def test_rel_attention_matches_float64(mode, T, dk):
    """dn_rel_attention against the float64 restatement of score = ((q + u) k + (q + v) P(i - j)) / sqrt(dk) on the operands the device
    holds.  Bar: FWD_TOL of the attention grid for the mode, relative to the output's max; in the 2-byte modes the maximum of that and
    4 x the error the format alone costs (the same restatement with q + u, q + v, P and the output rounded to the format)."""
    from diffnorm_amd import ops

    q, k, v, pos, u, vb, lens, H, Tmax = _attn_case(dk, T)
    ins = [_rt(t, mode) for t in (q, k, v, pos)]
    want = _attn_ref(*ins, u.double(), vb.double(), lens, H, Tmax)
    scale = want.abs().max().item()
    bound, emu = FWD_TOL[mode], None
    if mode in UNIT:
        emu = (_attn_ref(*ins, u.double(), vb.double(), lens, H, Tmax, rnd=lambda t: _rt(t.float(), mode)) - want).abs().max().item() / scale
        bound = max(bound, 4 * emu)
    dev = [t.to(STORE[mode]).to(DEV) for t in (q, k, v, pos)]
    got = ops.rel_attention(*dev, u.to(DEV), vb.to(DEV), lens.to(DEV), H, Tmax - 1, x3=mode == "x3")
    err = (got.double().cpu() - want).abs().max().item() / scale
    print(f"rel_attention {mode} dk={dk} T={T}: emulated {emu if emu is None else f'{emu:.3e}'} bound {bound:.3e} measured {err:.3e}")
    assert torch.isfinite(got).all() and err < bound


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_rel_attention_does_not_depend_on_neighbours_or_table_size(mode):
    """A sequence's output is the same bits alone, beside other sequences, and with a position table built for a longer T_max."""
    from diffnorm_amd import ops

    q, k, v, pos, u, vb, lens, H, Tmax = _attn_case(64, 130)
    T = q.shape[1]
    dev = lambda t: t.to(STORE[mode]).to(DEV)
    run = lambda sl, table, zero: ops.rel_attention(dev(q[sl]), dev(k[sl]), dev(v[sl]), dev(table), u.to(DEV), vb.to(DEV), lens[sl].to(DEV), H, zero)
    batch = run(slice(0, 3), pos, Tmax - 1)
    for b in range(3):
        assert torch.equal(run(slice(b, b + 1), pos, Tmax - 1)[0], batch[b])
    tight = pos[Tmax - T: Tmax - 1 + T]  # the same offsets in a table built for exactly T frames
    assert torch.equal(run(slice(0, 3), tight, T - 1), batch)


def test_rel_attention_refuses_empty_sequences():
    from diffnorm_amd import ops

    q, k, v, pos, u, vb, lens, H, Tmax = _attn_case(16, 17)
    with pytest.raises(ValueError):
        ops.rel_attention(q.to(DEV), k.to(DEV), v.to(DEV), pos.to(DEV), u, vb, torch.tensor([17, 0, 3]), H, Tmax - 1)


def test_rel_attention_c_abi_refuses_a_table_that_is_too_short():
    """The C entry itself checks both ends of the position table (pos_rows): DN_EINVAL, no launch."""
    import ctypes as C

    from diffnorm_amd import _lib

    T, H, dk = 17, 2, 16
    q = torch.zeros(1, T, H * dk, device=DEV)
    pos = torch.zeros(2 * T - 1, H * dk, device=DEV)
    u = torch.zeros(H, dk, device=DEV)
    a = _lib.RelAttnParams()
    a.q = a.k = a.v = q.data_ptr()
    a.out, a.pos, a.bias_u, a.bias_v = torch.empty_like(q).data_ptr(), pos.data_ptr(), u.data_ptr(), u.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = a.ldp = H * dk
    a.B, a.T, a.heads, a.dim_head, a.dtype, a.scale = 1, T, H, dk, _lib.DN_F32, dk ** -0.5
    for zero, rows in ((T - 1, 2 * T - 2), (T - 2, 2 * T - 1)):
        a.pos_zero_row, a.pos_rows = zero, rows
        with pytest.raises(_lib.DiffNormHipError):
            _lib.check(_lib.load().dn_rel_attention(C.byref(a), _lib.current_stream()), "dn_rel_attention")


def _glu_dwconv_ref(xs, w, shift):
    """float64 swish(depthwise_conv(glu(xs)) + shift) on xs [B, S, 2 C] (float64, what the device holds), w [C, k], shift [C]."""
    C, k = w.shape
    y = torch.nn.functional.glu(xs, dim=-1).transpose(1, 2)
    y = torch.nn.functional.conv1d(y, w.double()[:, None, :], None, 1, k // 2, 1, C) + shift.double()[None, :, None]
    return torch.nn.functional.silu(y).transpose(1, 2)


def _glu_dwconv_bound(mode, scale):
    """1e-5 x scale in fp32 arithmetic; the 2-byte modes add one unit roundoff of the format, the split-row store of x3 2^-16."""
    return (1e-5 + UNIT.get(mode, 2.0 ** -16 if mode == "x3" else 0.0)) * scale


@pytest.mark.parametrize("mode", ["f32", "x3", "f16", "bf16"])
@pytest.mark.parametrize("S", [1, 14, 15, 16, 100])
@pytest.mark.parametrize("k,C", [(3, 64), (31, 64), (31, 512), (3, 512)])
def test_glu_dwconv_matches_float64(mode, S, k, C):
    """swish(sum_j w[c][j] glu(x)[t + j - k/2] + shift[c]) against float64 on the stored input.  Bar: 1e-5 x scale in fp32 arithmetic
    (fp32 accumulation of k <= 31 products and two exponentials); the 2-byte modes add the output's rounding, one unit roundoff of
    the format x scale; the split-row store of x3 adds 2^-16."""
    from diffnorm_amd import _lib, ops

    B = 3
    x = _randn(7 * S + k + C, B, S, 2 * C)
    w, shift = _randn(11 + k + C, C, k) * k ** -0.5, 0.3 * _randn(13 + k + C, C)
    want = _glu_dwconv_ref(_rt(x, mode), w, shift)
    scale = want.abs().max().item()
    got = ops.glu_dwconv(x.to(STORE[mode]).to(DEV), w.to(DEV), shift.to(DEV), dtype=_lib.DN_BF16X3 if mode == "x3" else None)
    err = (got.double().cpu() - want).abs().max().item()
    bound = _glu_dwconv_bound(mode, scale)
    print(f"glu_dwconv {mode} k={k} C={C} S={S}: bound {bound:.3e} measured {err:.3e}")
    assert got.shape == (B, S, C) and err < bound


def _tiny_engine(dtype, **kw):
    from diffnorm_amd import nar_decoder

    c = R.TINY
    return nar_decoder.ConformerEncoderEngine(R.make_state_dict(), c.input_dim, c.conv_channels, c.kernel_sizes[0], c.embed_dim, c.ffn_dim, c.layers, c.heads,
                                              c.depthwise_kernel, dtype=dtype, device=DEV, **kw)


def _golden_inputs(g):
    lens = torch.from_numpy(g["lens"])
    return R.make_features(lens.numel(), int(lens.max()), lens, R.TINY.input_dim, int(g["seed_feats"]))


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16", "bf16"])
def test_conformer_encoder_matches_the_real_reference(golden, dtype):
    """dn_conformer_encoder_forward against the REAL S2SConformerEncoder's float64 output on the ragged golden batch, valid frames;
    lengths exact.  f32 additionally: the shortest utterance alone against its own golden, and the device's batch-vs-alone difference
    for it within 2 x the bar of the reference's -- the unmasked convolution module is reproduced, not repaired."""
    g = golden("conformer_encoder")
    feats, lens = _golden_inputs(g)
    eng = _tiny_engine(dtype)
    out, ol = eng.forward(feats.to(DEV), lens.to(DEV))
    assert ol.cpu().tolist() == g["out_lens"].tolist()
    ref = torch.from_numpy(g["encoder_out"]).transpose(0, 1)
    valid = ~torch.from_numpy(g["padding_mask"])
    bar = ENGINE_TOL[dtype] * max(1.0, ref.abs().max().item() / 4)
    err = (out.double().cpu() - ref)[valid].abs().max().item()
    print(f"conformer encoder {dtype}: max abs err {err:.3e} bar {bar:.3e} (output scale {ref.abs().max().item():.2f}, reference fp32 {float(g['e_ref32']):.2e})")
    assert err < bar
    if dtype == "f32":
        i = int(g["alone_index"])
        n = int(lens[i])
        alone, al = eng.forward(feats[i:i + 1, :n].to(DEV), lens[i:i + 1].to(DEV))
        want = torch.from_numpy(g["alone_out"])
        Si = want.shape[0]
        assert int(al[0]) == Si and alone.shape[1] == Si
        e1 = (alone[0].double().cpu() - want).abs().max().item()
        diff = (alone[0] - out[i, :Si]).abs().max().item()
        print(f"  alone: err {e1:.3e}; batch-vs-alone {diff:.6f} (reference {float(g['alone_vs_batch']):.6f})")
        assert e1 < bar and abs(diff - float(g["alone_vs_batch"])) < 2 * bar


@functools.lru_cache(maxsize=None)
def _recipe():
    """Recipe widths, 2 layers: seeded weights, B = 2, L = 301 (lengths 301 / 170), the float64 restatement on the CPU -- once."""
    sd = R.make_state_dict(R.RECIPE2, 77)
    feats, lens = R.make_features(2, 301, (301, 170), 80, 78)
    with torch.no_grad():
        want, ol = R.encode(sd, R.RECIPE2, feats, lens, torch.float64)
    return sd, feats, lens, want, ol


@functools.lru_cache(maxsize=None)
def _recipe_engine(dtype):
    from diffnorm_amd import nar_decoder

    return nar_decoder.ConformerEncoderEngine(_recipe()[0], layers=R.RECIPE2.layers, dtype=dtype, device=DEV)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_conformer_encoder_at_the_recipe_widths(dtype):
    """D = 512, H = 8 (d_k = 64), FFN 2048, conv_channels 1024, depthwise 31, 2 layers, S = 76: more than one query and key tile."""
    sd, feats, lens, want, wl = _recipe()
    out, ol = _recipe_engine(dtype).forward(feats.to(DEV), lens.to(DEV))
    assert ol.cpu().tolist() == wl.tolist()
    valid = torch.arange(want.shape[1])[None, :] < wl[:, None]
    bar = ENGINE_TOL[dtype] * max(1.0, want.abs().max().item() / 4)
    err = (out.double().cpu() - want)[valid].abs().max().item()
    print(f"conformer encoder, recipe widths, {dtype}: max abs err {err:.3e} bar {bar:.3e} (output scale {want.abs().max().item():.2f})")
    assert err < bar


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_generate_from_features_through_the_conformer_encoder(golden, dtype):
    """generate() of the research generator from [B, L, 80] features with encoder_arch="conformer" reproduces the hypotheses the REAL
    generator produced with the REAL conformer encoder in front of the fixture decoder: tokens and steps exact, scores within 2e-4."""
    import nar_oracle as N
    from diffnorm_amd import nar_decoder
    from diffnorm_amd.iterative_refinement import IterativeRefinementGenerator
    from gen_golden_nar_configs import CFG, Dict1004

    g = golden("conformer_encoder")
    feats, lens = _golden_inputs(g)
    c = R.TINY
    model = nar_decoder.NARS2UTDecoderModel(
        N.make_nar_state_dict(CFG, "nar"), CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype=dtype, device=DEV,
        encoder_state_dict=R.make_state_dict(), encoder_arch="conformer",
        encoder_kw=dict(input_dim=c.input_dim, conv_channels=c.conv_channels, kernel=c.kernel_sizes[0], ffn=c.ffn_dim, layers=c.layers,
                        depthwise_kernel=c.depthwise_kernel))
    gen = IterativeRefinementGenerator(Dict1004(), speech_source=True, max_iter=4, beam_size=1, adaptive=True)
    hyps = gen.generate([model], {"net_input": {"src_tokens": feats.to(DEV), "src_lengths": lens.to(DEV)}})
    assert len(hyps) == int(g["gen_n"])
    for i, h in enumerate(hyps):
        assert h[0]["tokens"].cpu().tolist() == g[f"gen_h{i}_tokens"].tolist(), i
        assert int(h[0]["steps"]) == int(g[f"gen_h{i}_steps"])
        assert np.abs(h[0]["positional_scores"].cpu().numpy() - g[f"gen_h{i}_scores"]).max() < 2e-4


def test_workspace_is_linear_and_the_longest_source_runs():
    """Nothing quadratic: four times the frames cost at most 4.5 x the workspace at B = 8; and B = 1, L = 6000 (the reference's
    max_source_positions) runs in f16, S = 1500, finite."""
    eng = _recipe_engine("f16")
    assert eng.workspace_bytes(8, 6000) <= 4.5 * eng.workspace_bytes(8, 1500)
    feats, lens = R.make_features(1, 6000, (6000,), 80, 79)
    out, ol = eng.forward(feats.to(DEV), lens.to(DEV))
    assert out.shape == (1, 1500, 512) and int(ol[0]) == 1500 and bool(torch.isfinite(out).all())
