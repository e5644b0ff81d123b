"""dn_voc_conv, the vocoder's one conv operator, in both arithmetic modes against a float64 conv of the operands AS THE MODE ROUNDS
THEM (pre-activation in fp32, then half in f16), so that only fp32 accumulation remains.

Bound per output element, derived, not measured: the MFMA chain is a k-ordered fp32 fma chain of n = k C_in terms, whose error is at
most n u S with u = 2^-24 and S = sum |x||w| over the taps and channels alone; the "+ 4" stands for the single roundings of the bias,
the residual, the previous value and the division / store, and the factor 2 allows for the order of the chain.
bound = 2 (k C_in + 4) 2^-24 S, divided by `div` where the accumulate form divides its result.  Neither |bias|, |res| nor |previous|
joins S, and tanh gets no slack of its own (its slope is <= 1, so it does not enlarge the error of its argument).
Measured on an MI355X: worst error / bound per shape and mode in DESIGN 9b."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from diffnorm_amd import _lib
from diffnorm_amd import vocoder as V

pytestmark = pytest.mark.gpu
SHAPES = [(16, 16), (32, 32), (64, 64), (256, 256), (16, 1), (32, 2 * 16), (32, 128),
          (16, 48), (32, 40),  # three channel fragments per wave, full and with a ragged last one
          (16, 80),            # the second block of 64 channels has one active wave
          (128, 100),          # co >= C_out inside an active fragment of the split-N arrangement
          (384, 32)]           # three passes of 128 input channels
STRIDED = [(16, 16), (32, 48), (64, 80)]
SLOPES = [0.1, 0.01, 1.0, 0.0]
POSTS = [_lib.VOC_POST_NONE, _lib.VOC_POST_RES, _lib.VOC_POST_RES_ACC, _lib.VOC_POST_RELU, _lib.VOC_POST_TANH]
WORST = {}


def reference(x, w, bias, lengths, k, d, mode, slope, post, res, prev, div):
    """float64 result and bound on the valid frames of each sequence: lists of [len, C_out]."""
    outs, bounds = [], []
    wr = (w.half() if mode == "f16" else w).double()
    for b, n in enumerate(lengths):
        xa = x[b, :n].float()
        xa = torch.where(xa > 0, xa, xa * torch.tensor(slope, dtype=torch.float32))
        xa = (xa.half() if mode == "f16" else xa).double().t()[None]
        pad = (k - 1) // 2 * d
        y = F.conv1d(xa, wr, None, padding=pad, dilation=d)[0].t() + bias.double()
        S = F.conv1d(xa.abs(), wr.abs(), None, padding=pad, dilation=d)[0].t()
        if post in (_lib.VOC_POST_RES, _lib.VOC_POST_RES_ACC):
            y = y + res[b, :n].double()
            if post == _lib.VOC_POST_RES_ACC:
                y = y + prev[b, :n].double()
            y = y / div
        elif post == _lib.VOC_POST_RELU:
            y = y.clamp(min=0)
        elif post == _lib.VOC_POST_TANH:
            y = torch.tanh(y)
        outs.append(y)
        bounds.append(2 * (k * x.shape[2] + 4) * 2.0 ** -24 * S / div)
    return outs, bounds


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("C_in,C_out", SHAPES)
def test_conv_grid(C_in, C_out, mode):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator().manual_seed(C_in * 1000 + C_out)
    worst, case = 0.0, 0
    for k, d in itertools.product((3, 7, 11), (1, 3, 5)):
        TILE = lib.dn_voc_conv_tile(_lib.DN_F16 if mode == "f16" else _lib.DN_F32, C_in, C_out, k)
        assert TILE > 0
        pool = [1, 2, d * (k - 1) // 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]
        w = torch.randn(C_out, C_in, k, generator=g) / (k * C_in) ** 0.5
        bias = torch.randn(C_out, generator=g) * 0.1
        for post in POSTS:
            lengths = [pool[(case + 3 * i) % 7] for i in range(3)]
            slope = SLOPES[case % 4]
            case += 1
            Lmax = max(lengths) + 3
            x = torch.randn(3, Lmax, C_in, generator=g)
            res = torch.randn(3, Lmax, C_out, generator=g)
            prev = torch.randn(3, Lmax, C_out, generator=g)
            div = 3.0 if post == _lib.VOC_POST_RES_ACC else 1.0
            want, bound = reference(x, w, bias, lengths, k, d, mode, slope, post, res, prev, div)
            xp, rp = x.clone(), res.clone()
            for b, n in enumerate(lengths):  # poison the padding: it must reach no valid frame
                xp[b, n:] = float("nan")
                rp[b, n:] = float("nan")
            out = prev.clone().to(dev)
            needs_res = post in (_lib.VOC_POST_RES, _lib.VOC_POST_RES_ACC)
            V.voc_conv(xp.to(dev), w, bias, torch.tensor(lengths), k, d, mode, slope, post, rp.to(dev) if needs_res else None, out, div)
            got = out.cpu()
            for b, n in enumerate(lengths):
                assert torch.isfinite(got[b, :n]).all(), (k, d, post, lengths)
                assert torch.equal(got[b, n:], prev[b, n:]), "frames behind a sequence's length were written"
                ratio = ((got[b, :n].double() - want[b]).abs() / bound[b]).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, d, post, slope, lengths, b, ratio)
                # the sequence alone: same bits
                o1 = prev[b:b + 1, :n].clone().to(dev)
                V.voc_conv(x[b:b + 1, :n].contiguous().to(dev), w, bias, torch.tensor([n]), k, d, mode, slope, post,
                           res[b:b + 1, :n].contiguous().to(dev) if needs_res else None, o1, div)
                assert torch.equal(o1.cpu()[0], got[b, :n]), (k, d, post, lengths, b)
    WORST[(C_in, C_out, mode)] = worst
    print(f"dn_voc_conv {mode} C_in {C_in} C_out {C_out}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("C_in,C_out", STRIDED)
def test_conv_strides(C_in, C_out, mode):
    """ldx > C_in, ldo > C_out, ldr > C_out through the C entry: the columns between the rows are NaN in x and res and keep their
    bits in out.  Same reference, same bound."""
    dev = torch.device("cuda:0")
    lib = _lib.load()
    dt = _lib.DN_F16 if mode == "f16" else _lib.DN_F32
    k, d, post, div, slope = 7, 3, _lib.VOC_POST_RES_ACC, 3.0, 0.1
    ldx, ldo, ldr = C_in + 4, C_out + 3, C_out + 5
    TILE = lib.dn_voc_conv_tile(dt, C_in, C_out, k)
    lengths = [TILE + 1, 2, 2 * TILE + 3]
    B, Lmax = 3, max(lengths) + 3
    g = torch.Generator().manual_seed(7 * C_in + C_out)
    w = torch.randn(C_out, C_in, k, generator=g) / (k * C_in) ** 0.5
    bias = torch.randn(C_out, generator=g) * 0.1
    x = torch.randn(B, Lmax, C_in, generator=g)
    res = torch.randn(B, Lmax, C_out, generator=g)
    prev = torch.randn(B, Lmax, C_out, generator=g)
    want, bound = reference(x, w, bias, lengths, k, d, mode, slope, post, res, prev, div)
    xs = torch.full((B, Lmax, ldx), float("nan"))
    rs = torch.full((B, Lmax, ldr), float("nan"))
    os_ = torch.full((B, Lmax, ldo), -3.5)
    os_[:, :, :C_out] = prev
    for b, n in enumerate(lengths):  # the frames behind a length stay NaN
        xs[b, :n, :C_in] = x[b, :n]
        rs[b, :n, :C_out] = res[b, :n]
    xd, rd, od = xs.to(dev), rs.to(dev), os_.to(dev)
    wp = V.pack_conv_weight(w, dt).to(dev)
    ln, bd = torch.tensor(lengths, dtype=torch.int32, device=dev), bias.to(dev)
    p = _lib.VocConvParams(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), rd.data_ptr(), od.data_ptr(), ln.data_ptr(), B, Lmax, C_in, C_out, k, d,
                           ldx, ldo, ldr, dt, post, slope, div)
    _lib.check(lib.dn_voc_conv(C.byref(p), _lib.current_stream()), "dn_voc_conv")
    got = od.cpu()
    assert torch.equal(got[:, :, C_out:], os_[:, :, C_out:]), "columns between the rows of out were written"
    worst = 0.0
    for b, n in enumerate(lengths):
        assert torch.isfinite(got[b, :n, :C_out]).all()
        assert torch.equal(got[b, n:, :C_out], prev[b, n:]), "frames behind a sequence's length were written"
        ratio = ((got[b, :n, :C_out].double() - want[b]).abs() / bound[b]).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (lengths, b, ratio)
    # dense rows: same bits
    dense = prev.clone().to(dev)
    xp, rp = x.clone(), res.clone()
    for b, n in enumerate(lengths):
        xp[b, n:] = float("nan")
        rp[b, n:] = float("nan")
    V.voc_conv(xp.to(dev), w, bias, torch.tensor(lengths), k, d, mode, slope, post, rp.to(dev), dense, div)
    assert torch.equal(dense.cpu(), got[:, :, :C_out])
    print(f"dn_voc_conv strided {mode} C_in {C_in} C_out {C_out}: worst error / bound = {worst:.3f}")


def test_bad_arguments_are_refused():
    dev = torch.device("cuda:0")
    x = torch.zeros(1, 8, 16, device=dev)
    w = torch.zeros(16, 16, 3)
    with pytest.raises(ValueError, match="significand"):
        V.voc_conv(x, w, None, torch.tensor([8]), 3, dtype="bf16")
    with pytest.raises(_lib.DiffNormHipError, match="needs res"):
        V.voc_conv(x, w, None, torch.tensor([8]), 3, post=_lib.VOC_POST_RES)
    with pytest.raises(_lib.DiffNormHipError, match="LDS"):
        V.voc_conv(torch.zeros(1, 8, 128, device=dev), torch.zeros(16, 128, 11), None, torch.tensor([8]), 11, d=7)
