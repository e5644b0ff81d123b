"""Helpers shared by the operator grids of dn_conv_gemm (tests/test_hip_x3_gemm_grid.py: split operands; tests/test_hip_gemm_grid.py:
f16, bf16, f32): nothing here depends on the arithmetic of a mode.  A plain module, not a test file."""
import ctypes as C

import torch

NAN = float("nan")
BIAS, SILU, GEGLU, FILM, RESADD, POSEMB, RELU = range(7)  # _lib.EPI_* (asserted by each grid's env fixture)
NAMES = ["bias", "silu", "geglu", "film", "resadd", "posemb", "relu"]
BAR = {BIAS: 1e-4, RELU: 1e-4, RESADD: 1e-4, POSEMB: 1e-4, SILU: 2e-4, GEGLU: 2e-4, FILM: 2e-4}  # tests/test_hip_bf16x3.py


def seeded(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def padn(c):
    return (c + 127) // 128 * 128


class Spy:
    """Stands between ops.conv_gemm and the library: edits the params (fields ops.conv_gemm has no argument for), asks
    dn_conv_gemm_route about them and hands the call on -- or not (launch=False: the route is all that is wanted)."""

    def __init__(self, lib, launch, edit):
        self._lib, self._launch, self._edit, self.tile, self.route = lib, launch, edit, None, None

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def dn_conv_gemm(self, ref, stream):
        from diffnorm_amd import _lib

        p = ref._obj
        if self._edit:
            self._edit(p)
        r = _lib.GemmRoute()
        assert self._lib.dn_conv_gemm_route(C.byref(p), C.byref(r)) == 0
        self.tile, self.route = r.tile, r
        return self._lib.dn_conv_gemm(ref, stream) if self._launch else 0


def call(*args, host=False, launch=True, edit=None, whole_route=False, **kw):
    """ops.conv_gemm(*args, **kw) through a Spy; returns the tile dn_conv_gemm_route names (whole_route: the DnGemmRoute).  host: no
    device is touched (stream 0; the tensors may live on the CPU as long as nothing is launched)."""
    from diffnorm_amd import _lib, ops

    spy = Spy(_lib.load(), launch, edit)
    saved = _lib.load, _lib.current_stream
    _lib.load = lambda: spy
    if host:
        _lib.current_stream = lambda: None
    try:
        ops.conv_gemm(*args, **kw)
    finally:
        _lib.load, _lib.current_stream = saved
    return spy.route if whole_route else spy.tile


def shift_rows(a, shift, T):
    """row m = row m - shift of the same sequence, zero outside it (gemm_kernels.h shift_valid)"""
    m = torch.arange(a.shape[0])
    t = m % T
    valid = (t >= shift) if shift >= 0 else (t - shift < T)
    return a[(m - shift).clamp(0, a.shape[0] - 1)] * valid.unsqueeze(1).to(a.dtype)


def gelu(x):
    return 0.5 * x * (1 + torch.special.erf(x * 0.7071067811865476))


def epilogue(acc, epi, bias=None, res=None, ga=None, be=None, pos=None, scale=None, rbias=None):
    """The epilogue of wave_epilogue_impl in acc's dtype (float64 or float32); side inputs are per row ([M, n]) or per column ([n])."""
    c = lambda t: t.to(acc.dtype)
    v = acc
    if scale is not None:  # split norm, consumer side
        v = v * c(scale).unsqueeze(1)
        if rbias is not None:
            v = v + c(rbias)
    if bias is not None:
        v = v + c(bias)
    if epi == GEGLU:  # packed columns: tiles of [8 value | 8 gate]
        v = v.view(v.shape[0], -1, 2, 8)
        return (gelu(v[:, :, 1]) * v[:, :, 0]).reshape(v.shape[0], -1)
    if epi == SILU:
        return v * torch.sigmoid(v)
    if epi == RELU:
        return v.clamp_min(0)
    if epi == FILM:
        if ga is not None:
            v = v * c(ga) + c(be)
        return torch.tanh(v) * torch.sigmoid(v) + c(res)
    if epi == RESADD:
        return v + c(res)
    if epi == POSEMB:
        return v + c(pos)
    return v


def all_nan(t):
    return bool(torch.isnan(t.float()).all().item())
