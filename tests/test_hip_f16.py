"""GPU parity of the DN_F16 arithmetic mode (round 4): IEEE-half contraction operands through v_mfma_f32_16x16x32_f16 -- the bf16
MFMA rate with 11 significand bits instead of 8 -- fp32 accumulation, and everything DN_BF16 keeps in fp32 kept in fp32.  The mode
exists to put the 2-byte headline inside north_star's 1e-2 max-abs budget (plain bf16 misses it by 1.4x on BASELINE config 2), so
the engine-level golden tests (tests/test_hip_engine.py, test_hip_fullsize.py, test_hip_refine.py) assert it at 1e-2 flat; here
the operators are held (a) TIGHT to the oracle fed the same half-rounded operands (only fp32 summation order differs) and (b) to
the fp32 oracle at the half rounding level, on every tile variant that takes 2-byte operands.
"""
import ctypes as C

import pytest
import torch

import diffnorm_oracle as O
from attention_ref import attention_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def seeded(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def f16r(t):
    return t.to(torch.float16).float()


def padk(c):
    return (c + 63) // 64 * 64


def pad_cols(t, n):
    out = torch.zeros(*t.shape[:-1], n, dtype=t.dtype)
    out[..., : t.shape[-1]] = t
    return out


def maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


def act(t):
    return t.to(DEV, torch.float16).contiguous()


@pytest.fixture(scope="module")
def ops():
    from diffnorm_amd import _lib, ops, packing

    _lib.load()
    return ops, packing, _lib


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("cin,cout,k,dil,B,T", [(192, 704, 3, 1, 3, 100), (64, 352, 3, 2, 2, 300), (128, 1056, 1, 1, 1, 515),
                                                (1408, 1408, 3, 1, 4, 512)])
def test_causal_conv_gemm_f16_every_tile(ops, tile, cin, cout, k, dil, B, T):
    """CausalConv1d on half operands through 128x128, 256x128, 256x256, the hand-scheduled 256x352 tile (its inline-asm MFMAs
    are the _f16 opcode in this mode) and 256x352 with the taps innermost (tile 5): ragged M, sequence starts inside tiles, fp32
    and half outputs; term-outer variants bit-identical to each other."""
    ops_, packing, _lib = ops
    x = seeded((B, T, cin), 11)
    w = seeded((cout, cin, k), 12, (1.0 / (cin * k)) ** 0.5)
    b = seeded((cout,), 13, 0.1)
    N = (cout + 31) // 32 * 32
    xa = act(pad_cols(x, padk(cin)).view(B * T, -1))
    W = packing._conv(w, _lib.DN_F16).to(DEV)
    assert W.dtype == torch.float16 and W.shape[1] >= N
    bias = packing._vec(b, W.shape[1]).to(DEV)
    terms = [(xa, W[j], (k - 1 - j) * dil) for j in range(k)]
    out = torch.full((B * T, N), float("nan"), device=DEV)
    ops_.conv_gemm(terms, out, T, N, bias=bias, tile=4 if tile == 5 else tile, taps_inner=(tile == 5) if tile else None)
    got = out.cpu().view(B, T, -1)
    tight = O.causal_conv1d(f16r(x), f16r(w), b, dil)
    assert maxerr(got[..., :cout], tight) < 2e-4          # same operands, fp32 accumulation: summation order only
    assert maxerr(got[..., :cout], O.causal_conv1d(x, w, b, dil)) < 4e-3  # 2^-11 operands on O(1) sums (bf16: 3e-2)
    if tile in (2, 3, 4, 8, 9):  # (8: the 256 x 192 form of the 256 x 256 tile; 9: 256 x 128, two workgroups per CU)
        ref_out = torch.empty_like(out)
        ops_.conv_gemm(terms, ref_out, T, N, bias=bias, tile=1, taps_inner=False)
        assert torch.equal(out, ref_out)
    outh = torch.full((B * T, N), float("nan"), device=DEV, dtype=torch.float16)
    ops_.conv_gemm(terms, outh, T, N, bias=bias, tile=4 if tile == 5 else tile, taps_inner=(tile == 5) if tile else None)
    assert torch.equal(outh.cpu(), out.cpu().to(torch.float16))  # the half store is the RNE rounding of the fp32 result


@pytest.mark.parametrize("half", ["f16", "bf16"])
@pytest.mark.parametrize("B,T,K,N", [(3, 200, 256, 384), (2, 515, 128, 768)])
def test_residual_epilogue_on_the_256x192_tile(ops, half, B, T, K, N):
    """RESADD (fp32 residual stream, in place) on the 256 x 192 form of the 256 x 256 kernel -- the tile a lone launch of an N = 768
    contraction is scored onto (training: 144 -> 192 workgroups): bit-identical to the 128 x 128 tile, ragged M."""
    ops_, packing, _lib = ops
    code, tdt = (_lib.DN_F16, torch.float16) if half == "f16" else (_lib.DN_BF16, torch.bfloat16)
    M = B * T
    x, w, b = seeded((M, K), 21), seeded((N, K), 22, K ** -0.5), seeded((N,), 23, 0.1)
    res = seeded((M, N), 24)
    xa, W = x.to(DEV, tdt).contiguous(), packing._mat(w, code).to(DEV)
    outs = []
    for tile in (_lib.TILE_256X192, _lib.TILE_128X128):
        stream = res.to(DEV).clone()
        ops_.conv_gemm([(xa, W, 0)], stream, T, N, bias=packing._vec(b, W.shape[0]).to(DEV), epilogue=_lib.EPI_RESADD, res=stream, tile=tile)
        outs.append(stream.cpu())
        p = _lib.GemmParams()
        p.M, p.N, p.K, p.T, p.groups, p.n_terms, p.epilogue, p.dtype, p.flags = M, N, K, T, 1, 1, _lib.EPI_RESADD, code, tile << _lib.GEMM_TILE_SHIFT
        assert _lib.load().dn_conv_gemm_tile(C.byref(p)) == tile
    assert torch.equal(outs[0], outs[1])
    want = res + x.to(tdt).float() @ w.to(tdt).float().t() + b
    assert maxerr(outs[0], want) < 2e-4


@pytest.mark.parametrize("half", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("tile", [0, 1, 3])
def test_geglu_epilogue_keeps_the_pre_activation(ops, half, tile):
    """Training forward: the GEGLU epilogue with pre_out also stores the projection it gates (packed [8 value ; 8 gate] columns, what
    the BIAS epilogue writes) -- bit-identical to the two-pass form's pre-activation, and the gated output unchanged by the extra store."""
    ops_, packing, _lib = ops
    code, tdt = {"f16": (_lib.DN_F16, torch.float16), "bf16": (_lib.DN_BF16, torch.bfloat16), "f32": (_lib.DN_F32, torch.float32)}[half]
    B, T, D, inner = 3, 171, 128, 85
    M, ip = B * T, padk(inner)
    x = seeded((M, D), 31).to(DEV, tdt).contiguous()
    w_in, b_in = seeded((2 * inner, D), 32, D ** -0.5), seeded((2 * inner,), 33, 0.1)
    rows = packing._geglu_rows(inner)
    keep = rows >= 0
    wp, bp = torch.zeros(2 * ip, D), torch.zeros(2 * ip)
    wp[keep] = w_in[rows[keep]]
    bp[keep] = b_in[rows[keep]]
    W, bias = wp.to(DEV, tdt).contiguous(), bp.to(DEV)
    pre_two = torch.empty(M, 2 * ip, device=DEV, dtype=tdt)
    ops_.conv_gemm([(x, W, 0)], pre_two, T, 2 * ip, bias=bias, tile=tile)
    gg_plain = torch.empty(M, ip, device=DEV, dtype=tdt)
    ops_.conv_gemm([(x, W, 0)], gg_plain, T, ip, bias=bias, epilogue=_lib.EPI_GEGLU, tile=tile)
    gg, pre = torch.empty_like(gg_plain), torch.full_like(pre_two, float("nan"))
    ops_.conv_gemm([(x, W, 0)], gg, T, ip, bias=bias, epilogue=_lib.EPI_GEGLU, tile=tile, pre_out=pre)
    assert torch.equal(gg, gg_plain)
    if tile:  # (chosen by shape, the two-pass projection may land on another tile: another summation order)
        assert torch.equal(pre, pre_two)
    assert maxerr(pre.float().cpu(), pre_two.float().cpu()) < (1e-5 if half == "f32" else 3e-2 if half == "bf16" else 4e-3)
    h = x.float().cpu() @ w_in.to(tdt).float().t() + b_in
    want = torch.nn.functional.gelu(h[:, inner:]) * h[:, :inner]
    assert maxerr(gg.float().cpu()[:, :inner], want) < (1e-4 if half == "f32" else 4e-2 if half == "bf16" else 6e-3)


def test_f16_wavenet_block_geglu_and_split_norm_chain(ops):
    """The epilogues that read or write half tensors: FiLM . tanh . sigmoid + half residual, GEGLU (8-column wide stores), the
    split RMSNorm's producer (row * gamma as half + sums of squares) and consumer (row factor + beta . W^T)."""
    ops_, packing, _lib = ops
    B, T, C, dil = 3, 90, 128, 4
    M = B * T
    x = seeded((B, T, C), 1)
    w, b = seeded((C, C, 3), 2, (3 * C) ** -0.5), seeded((C,), 3, 0.1)
    wr, br = seeded((C, C, 1), 4, C ** -0.5), seeded((C,), 5, 0.1)
    gb = torch.cat([seeded((B, C), 6, 0.3) + 1.0, seeded((B, C), 7, 0.3)], dim=-1).contiguous()
    xa = act(x.view(M, C))
    res = torch.empty(M, C, device=DEV, dtype=torch.float16)
    ops_.conv_gemm([(xa, packing._conv(wr, _lib.DN_F16).to(DEV)[0], 0)], res, T, C, bias=br.to(DEV))
    out = torch.empty(M, C, device=DEV, dtype=torch.float16)
    Wc = packing._conv(w, _lib.DN_F16).to(DEV)
    ops_.conv_gemm([(xa, Wc[j], (2 - j) * dil) for j in range(3)], out, T, C, bias=b.to(DEV), epilogue=_lib.EPI_FILM_GATE, res=res,
                   gamma_beta=gb.to(DEV), gb_half=C)
    xr = f16r(x)
    r_want = f16r(O.causal_conv1d(xr, f16r(wr), br, 1))
    h = O.causal_conv1d(xr, f16r(w), b, dil) * gb[:, None, :C] + gb[:, None, C:]
    want = h.tanh() * h.sigmoid() + r_want
    assert maxerr(out.float().cpu().view(B, T, C), want) < 2e-3  # one half rounding of an O(1) output: 2^-11 x 2..4

    D, inner = 64, 85
    ip = padk(inner)
    xs = seeded((B, T, D), 8)
    gamma = seeded((D,), 9, 0.3) + 1.0
    w_in, b_in = seeded((2 * inner, D), 10, D ** -0.5), seeded((2 * inner,), 11, 0.1)
    w_o = seeded((D, D), 12, D ** -0.5)
    stream = seeded((M, D), 13).to(DEV)
    res0 = stream.clone()
    xn = torch.zeros(M, D, device=DEV, dtype=torch.float16)
    ssq = torch.zeros(M, 8, device=DEV)
    ops_.conv_gemm([(act(xs.view(M, D)), packing._mat(w_o, _lib.DN_F16).to(DEV), 0)], stream, T, D, epilogue=_lib.EPI_RESADD, res=stream,
                   norm_out=xn, norm_D=D, norm_gamma=gamma.to(DEV), norm_ssq=ssq)
    want_s = res0.cpu() + f16r(xs.view(M, D)) @ f16r(w_o).t()
    assert maxerr(stream.cpu(), want_s) < 2e-4
    assert maxerr(xn.float().cpu(), want_s * gamma) < 4e-3
    rows = packing._geglu_rows(inner)
    keep = rows >= 0
    wp, bp = torch.zeros(2 * ip, D), torch.zeros(2 * ip)
    wp[keep] = w_in[rows[keep]]
    bp[keep] = b_in[rows[keep]]
    beta = seeded((D,), 14, 0.2)
    row_bias = (f16r(beta) @ f16r(wp).t()).contiguous()
    gg = torch.zeros(M, ip, device=DEV, dtype=torch.float16)
    ops_.conv_gemm([(xn, wp.to(DEV, torch.float16), 0)], gg, T, ip, bias=bp.to(DEV), epilogue=_lib.EPI_GEGLU, row_ssq=ssq,
                   row_D=D, row_bias=row_bias.to(DEV), row_bias_shared=True)
    normed = torch.nn.functional.normalize(want_s, dim=-1) * D ** 0.5 * gamma + beta
    hh = torch.nn.functional.linear(normed, w_in, b_in)
    want_g = torch.nn.functional.gelu(hh[..., inner:]) * hh[..., :inner]
    assert maxerr(gg.float().cpu()[:, :inner], want_g) < 1.5e-2  # two half roundings (row * gamma, weights) through a norm of gain ~1


@pytest.mark.parametrize("dh,heads,B,T", [(16, 4, 2, 70), (64, 8, 3, 200), (96, 8, 2, 130), (128, 2, 1, 257)])
def test_attention_f16(ops, dh, heads, B, T):
    """Attend.forward (latent_module.py:299-343) on half q / k / v: key mask, ragged lengths, a fully masked sequence."""
    ops_, _, _ = ops
    hd = heads * dh
    q, k, v = seeded((B, T, hd), 1), seeded((B, T, hd), 2), seeded((B, T, hd), 3)
    lens = torch.tensor(([T, T // 3, 0] * 2)[:B], dtype=torch.int32)
    out = torch.empty(B * T, hd, device=DEV, dtype=torch.float16)
    ops_.attention(act(q.view(-1, hd)), act(k.view(-1, hd)), act(v.view(-1, hd)), out, B, T, heads, dh, lens.to(DEV))
    want, _ = attention_ref(f16r(q), f16r(k), f16r(v), heads, lens.long())
    assert maxerr(out.float().cpu().view(B, T, hd), want) < 3e-3  # P and the output rounded to half (bf16 kernel: 2e-2)


@pytest.mark.parametrize("half", ["f16", "bf16", "x3"])
@pytest.mark.parametrize("dh,heads,B,T,Tk", [(64, 8, 3, 200, 0), (48, 4, 2, 515, 0), (64, 8, 2, 130, 64), (64, 2, 4, 64, 0), (16, 4, 2, 70, 0), (96, 8, 2, 300, 0),
                                             (128, 2, 1, 257, 0)])
def test_attention_on_eight_waves_is_bit_identical(ops, hip_option, half, dh, heads, B, T, Tk):
    """Option attn_waves8 (default on): eight waves of 16 queries per workgroup instead of four of 32 (four waves per SIMD instead of
    two up to 64-dim heads, two instead of one above).  Every query sees the same key tiles in the same order through the same MFMA shapes: bit-identical outputs, with
    key masks, ragged and fully masked sequences, and cross-attention (Tk != T, no mask)."""
    ops_, _, _lib = ops
    if half == "x3" and dh > 64:
        pytest.skip("split operands: heads over 64 dims run the exact-fp32 kernel")
    tdt = torch.float16 if half == "f16" else torch.bfloat16 if half == "bf16" else torch.float32  # (x3: q / k / v stay plain fp32)
    hd = heads * dh
    Tkv = Tk or T
    q, k, v = seeded((B, T, hd), 1), seeded((B, Tkv, hd), 2), seeded((B, Tkv, hd), 3)
    lens = None if Tk else torch.tensor(([T, T // 3, 0, T - 1] * 2)[:B], dtype=torch.int32).to(DEV)
    outs = []
    for on in (0, 1):
        hip_option("attn_waves8", on)
        out = torch.full((B * T, 2 * hd if half == "x3" else hd), float("nan"), device=DEV, dtype=torch.bfloat16 if half == "x3" else tdt)  # (x3: split rows)
        qa, ka, va = (z.view(-1, hd).to(DEV, tdt).contiguous() for z in (q, k, v))
        ops_.attention(qa, ka, va, out, B, T, heads, dh, lens, Tk=Tk, ldo=hd,
                       dtype={"f16": _lib.DN_F16, "bf16": _lib.DN_BF16, "x3": _lib.DN_BF16X3}[half])
        torch.cuda.synchronize()
        outs.append(out.cpu())
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1])


def test_f16_saturates_instead_of_overflowing(ops):
    """The format ends at 65504.  The DN_F16 kernels run with the MODE register's FP16_OVFL bit set, so a result beyond it is
    stored as +-65504, not inf (one inf operand turns a whole contraction row into NaN through inf - inf)."""
    ops_, packing, _lib = ops
    M, C = 128, 64
    x = torch.full((M, C), 300.0)
    w = torch.zeros(C, C)
    w[0, :] = 300.0   # column 0: 64 x 300 x 300 = 5.76e6
    w[1, :] = -300.0
    w[2, 0] = 1.0     # column 2: 300
    out = torch.empty(M, C, device=DEV, dtype=torch.float16)
    ops_.conv_gemm([(act(x), packing._mat(w, _lib.DN_F16).to(DEV), 0)], out, M, C, bias=torch.zeros(C, device=DEV))
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    assert (got[:, 0] == 65504.0).all() and (got[:, 1] == -65504.0).all() and (got[:, 2] == 300.0).all()
    big = torch.tensor([[1e6, -1e6, 70000.0, 65504.0, 1.0, 0.0, -0.0, 3e-8]]).repeat(4, 8).contiguous()
    dst = torch.empty(4, 64, device=DEV, dtype=torch.float16)
    ops_.convert_rows(big.to(DEV), dst, 64)
    d = dst.float().cpu()[0, :8]
    assert d.tolist()[:6] == [65504.0, -65504.0, 65504.0, 65504.0, 1.0, 0.0]
    assert packing._arith(torch.tensor([[1e9] * 32]), _lib.DN_F16).float().max().item() == 65504.0  # host-side packing saturates too
