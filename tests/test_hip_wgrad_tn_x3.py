"""The split-operand (bf16x3) weight gradient straight from the row-major split rows (dn_conv_weight_grad_tn_x3, csrc/wgrad_tn.hip:
wgrad_tn_x3_kernel) and its route in the VAE training engine (option wgrad_tn_x3).

Operator level: fp32 operands with full mantissas, the reference is torch autograd of the oracle's causal conv in float64 on those
values, the bound is the project's split-operand contraction bound 1e-4 * max(1, max |want|) (test_hip_bf16x3.py::
test_causal_conv_gemm_x3, test_hip_ops.py::test_weight_gradient_from_row_major_operands).  The CPU test below evaluates the
kernel's arithmetic (packing.split_rows, then x_lo dy_hi + x_hi dy_lo + x_hi dy_hi) in float64 for every case and finds it well
inside that bound, so what the GPU adds is the order of its fp32 accumulation only.

The C entry has the bf16 entry's argument list (no groups), so the grouped launch is checked where it is used: through the engine,
with the WaveNet stacks' weight gradients grouped (option wgrad_groups = 1) against one launch per block (0).

Engine level: the fixtures and the 1e-3 per-tensor bar of test_hip_train_x3.py with the option on; staged == whole and side stream
on == off bit for bit; option 0 against 1: vectors (bias / norm gradients) identical in bits, matrices within the bar in both, and
at least one matrix different in bits (the new route ran)."""
import ctypes as C
import os
import re

import pytest
import torch

import diffnorm_oracle as O
import train_oracle as TO
from gen_golden_configs import CHAIN_VAE, FULL_VAE, seeded as gseeded

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# cin, cout, k, dil, B, T, slices: the cases of test_hip_ops.py::test_weight_gradient_from_row_major_operands
CASES = [(192, 96, 3, 1, 3, 100, 1), (64, 352, 3, 2, 2, 300, 4), (1408, 1408, 3, 1, 4, 512, 1), (128, 1000, 1, 1, 1, 515, 2),
         (1365, 1365, 3, 1, 2, 263, 3), (512, 1536, 1, 1, 5, 77, 1), (200, 72, 3, 16, 3, 130, 1)]


def seeded(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def padk(c):
    return (c + 63) // 64 * 64


def pad_cols(t, n, fill=0.0):
    out = torch.full((*t.shape[:-1], n), fill, dtype=t.dtype)
    out[..., : t.shape[-1]] = t
    return out


def operands(cin, cout, B, T):
    return seeded((B, T, cin), 41), seeded((B, T, cout), 43)


def wgrad64(x, dy, cout, cin, k, dil):
    """[k, cout, cin] float64: autograd of the oracle's causal conv on the given values"""
    w = torch.zeros(cout, cin, k, dtype=torch.float64, requires_grad=True)
    O.causal_conv1d(x.double(), w, None, dil).backward(dy.double())
    return w.grad.permute(2, 0, 1)


def bound(want):
    return 1e-4 * max(1.0, want.abs().max().item())


def split_hi_lo(t):
    """the two halves packing.split_rows stores, as float64 values"""
    from diffnorm_amd import packing

    n = t.shape[-1]
    s = packing.split_rows(pad_cols(t, (n + 31) // 32 * 32)).reshape(*t.shape[:-1], -1, 2, 32).double()
    hi, lo = s[..., 0, :].reshape(*t.shape[:-1], -1)[..., :n], s[..., 1, :].reshape(*t.shape[:-1], -1)[..., :n]
    assert (hi + lo - t.double()).abs().max() <= 2.0 ** -16 * t.abs().max()  # x = hi + lo to 16 mantissa bits
    return hi, lo


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("cin,cout,k,dil,B,T,slices", CASES)
def test_split_product_in_float64_is_inside_the_bound(cin, cout, k, dil, B, T, slices):
    """The kernel's arithmetic without its fp32 accumulation: the gradient is bilinear in (x, dy), so the three kept terms are the
    gradient of the split values minus the dropped lo lo term."""
    x, dy = operands(cin, cout, B, T)
    want = wgrad64(x, dy, cout, cin, k, dil)
    (xh, xl), (dh, dl) = split_hi_lo(x), split_hi_lo(dy)
    emu = wgrad64(xh + xl, dh + dl, cout, cin, k, dil) - wgrad64(xl, dl, cout, cin, k, dil)
    err = (emu - want).abs().max().item()
    print(f"x3 emulation cin {cin} cout {cout} k {k} dil {dil} frames {B * T}: err {err:.3e} bound {bound(want):.3e} max|want| {want.abs().max().item():.1f}")
    assert err < 0.1 * bound(want)  # a factor of 10 left for the order of the fp32 accumulation


@pytest.fixture(scope="module")
def lib():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def test_symbol_is_declared_and_bound(lib):
    from diffnorm_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffnorm_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dn_conv_weight_grad_tn_x3\s*\(", src)
    assert "dn_conv_weight_grad_tn_x3" in _lib.SYMBOLS and hasattr(lib, "dn_conv_weight_grad_tn_x3")
    assert _lib.SYMBOLS["dn_conv_weight_grad_tn_x3"] == _lib.SYMBOLS["dn_conv_weight_grad_tn"]  # the sibling's argument list


def test_option_is_known(lib):
    from diffnorm_amd import _lib

    before = _lib.get_option("wgrad_tn_x3")
    try:
        for v in (1, 0):
            assert lib.dn_set_option(b"wgrad_tn_x3", v) == 0
            assert _lib.get_option("wgrad_tn_x3") == v
    finally:
        _lib.set_option("wgrad_tn_x3", before)
    assert _lib.get_option("wgrad_tn") in (None, 0, 1)  # the 2-byte modes' option is still there


def test_bad_arguments_are_refused_on_the_host(lib):
    """ld % 32 != 0 and null operands: -1 before anything touches a device"""
    fn = lib.dn_conv_weight_grad_tn_x3
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    xs, sh = (C.c_void_p * 1)(p), (C.c_int32 * 1)(0)
    ld = lambda v: (C.c_int32 * 1)(v)
    ok = dict(dy=p, lddy=64, cout=40, x=xs, ldx=ld(64), shift=sh, n_taps=1, cin=40, B=1, T=32, slices=1, part=None, grad=p, stream=None)
    call = lambda **kw: fn(*{**ok, **kw}.values())
    assert call(lddy=72) == -1 and b"dn_conv_weight_grad_tn_x3" in lib.dn_last_error()  # a multiple of 8 (the bf16 entry's rule), not of 32
    assert call(ldx=ld(48)) == -1
    assert call(dy=None) == -1
    assert call(x=None) == -1
    assert call(x=(C.c_void_p * 1)(None)) == -1
    assert call(grad=None) == -1
    assert call(lddy=32) == -1  # does not cover cout


# ------------------------------------------------------------------------------------------------------------ operator
def _run(cin, cout, k, dil, B, T, slices, pad=0.0, grad0=None):
    from diffnorm_amd import ops, packing

    x, dy = operands(cin, cout, B, T)
    xs = packing.split_rows(pad_cols(x, padk(cin), pad).view(B * T, -1)).to(DEV)
    dys = packing.split_rows(pad_cols(dy, padk(cout), pad).view(B * T, -1)).to(DEV)
    shifts = [(k - 1 - j) * dil for j in range(k)]
    call = lambda: ops.conv_weight_grad_tn(xs, dys, T, cin, cout, shifts, slices=slices, dtype="bf16x3",
                                           grad=None if grad0 is None else grad0.clone().to(DEV)).cpu()
    return x, dy, call


@gpu
@pytest.mark.parametrize("cin,cout,k,dil,B,T,slices", CASES)
def test_weight_gradient_from_split_rows(cin, cout, k, dil, B, T, slices):
    x, dy, call = _run(cin, cout, k, dil, B, T, slices)
    want = wgrad64(x, dy, cout, cin, k, dil)
    got = call()
    assert got.shape == want.shape
    err = (got.double() - want).abs().max().item()
    print(f"x3 wgrad cin {cin} cout {cout} k {k} dil {dil} frames {B * T} slices {slices}: err {err:.3e} bound {bound(want):.3e}")
    assert err < bound(want)
    assert torch.equal(call().view(torch.int32), got.view(torch.int32))  # two runs, the same bits


@gpu
@pytest.mark.parametrize("slices", [1, 2])
def test_pad_columns_may_hold_nan(slices):
    cin, cout, k, dil, B, T = 200, 72, 3, 16, 3, 130  # 56 pad columns in both operands
    x, dy, call = _run(cin, cout, k, dil, B, T, slices, pad=float("nan"))
    want = wgrad64(x, dy, cout, cin, k, dil)
    got = call()
    assert torch.isfinite(got).all()
    err = (got.double() - want).abs().max().item()
    print(f"x3 wgrad, NaN pad columns, slices {slices}: err {err:.3e} bound {bound(want):.3e}")
    assert err < bound(want)


@gpu
@pytest.mark.parametrize("cin,cout,k,dil,B,T", [(192, 96, 3, 1, 3, 100), (200, 72, 3, 16, 3, 130), (512, 1536, 1, 1, 5, 77)])
def test_accumulates_into_a_gradient_that_is_not_zero(cin, cout, k, dil, B, T):
    Np, Kp = (cout + 127) // 128 * 128, padk(cin)
    grad0 = seeded((k, Np, Kp), 44, 3.0)
    x, dy, call = _run(cin, cout, k, dil, B, T, 1, grad0=grad0)
    want = wgrad64(x, dy, cout, cin, k, dil)
    got = call()
    assert got.shape == grad0.shape
    delta = got[:, :cout, :cin].double() - grad0[:, :cout, :cin].double()
    err = (delta - want).abs().max().item()
    print(f"x3 wgrad accumulated cin {cin} cout {cout}: err {err:.3e} bound {bound(want):.3e}")
    assert err < bound(want)
    untouched = torch.ones(k, Np, Kp, dtype=torch.bool)
    untouched[:, :cout, :] = False
    assert torch.equal(got[untouched], grad0[untouched])  # rows beyond cout
    assert torch.equal(got[:, :cout, cin:], grad0[:, :cout, cin:])  # pad columns: + 0


# ------------------------------------------------------------------------------------------------------------ engine
def _engine(cfg=CHAIN_VAE, tag="train"):
    from diffnorm_amd import training

    sd = O.make_vae_state_dict(cfg, tag)
    if cfg is FULL_VAE:
        return training.VaeTrainEngine(sd, dtype="bf16x3", device=DEV)
    return training.VaeTrainEngine(sd, dim=cfg.dim, latent_dim=cfg.latent_dim, dtype="bf16x3", device=DEV, depth=cfg.depth, heads=cfg.heads,
                                   dim_head=cfg.dim_head, stacks=cfg.stacks, layers=cfg.layers)


def _chain_batch(g):
    return gseeded((3, 48, CHAIN_VAE.dim), 31), torch.from_numpy(g["units"]), torch.from_numpy(g["lens"]), torch.from_numpy(g["post_noise"])


def _step(eng, feat, units, lens, noise):
    eng.forward(feat, units, lens, noise=noise, ntokens=int(lens.sum()))
    eng.zero_grad()
    eng.backward()
    torch.cuda.synchronize()


@gpu
def test_vae_gradients_match_reference_on_the_new_route(golden, hip_option):
    hip_option("wgrad_tn_x3", 1)
    g = golden("vae_train")
    eng = _engine()
    _step(eng, *_chain_batch(g))
    print("wgrad_tn_x3 vae_train: worst relative gradient error vs the reference:", TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3))


@gpu
def test_fullsize_vae_gradients_match_reference_on_the_new_route(golden, hip_option):
    hip_option("wgrad_tn_x3", 1)
    g = golden("vae_train_full")
    eng = _engine(FULL_VAE, "full")
    _step(eng, gseeded((2, 64, FULL_VAE.dim), 41), torch.from_numpy(g["units"]), torch.from_numpy(g["lens"]), torch.from_numpy(g["post_noise"]))
    print("wgrad_tn_x3 vae_train_full: worst relative gradient error vs the reference:", TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3))


@gpu
def test_bench_shape_vae_gradients_match_reference_on_the_new_route(golden, hip_option):
    from test_hip_train import _bench_batch

    hip_option("wgrad_tn_x3", 1)
    g = golden("vae_train_batch")
    eng = _engine(FULL_VAE, "full")
    feat, lens = _bench_batch(24, 512, FULL_VAE.dim, int(g["batch_seed"]))
    noise = gseeded(tuple(int(v) for v in g["post_noise_shape"]), int(g["post_noise_seed"])).transpose(1, 2).contiguous()
    _step(eng, feat, torch.from_numpy(g["units"]), lens, noise)
    print("wgrad_tn_x3 vae_train_batch: worst relative gradient error vs the reference:", TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3))


@gpu
def test_staged_backward_is_the_whole_backward_on_the_new_route(golden, hip_option):
    hip_option("wgrad_tn_x3", 1)
    feat, units, lens, noise = _chain_batch(golden("vae_train"))
    eng = _engine()
    _step(eng, feat, units, lens, noise)
    whole = eng.grads.clone()
    eng.forward(feat, units, lens, noise=noise, ntokens=int(lens.sum()))
    eng.zero_grad()
    for st in range(eng.n_stages):
        eng.backward(st, st)
    torch.cuda.synchronize()
    assert torch.equal(eng.grads, whole)


@gpu
def test_side_stream_changes_nothing_on_the_new_route(golden, hip_option):
    hip_option("wgrad_tn_x3", 1)
    batch = _chain_batch(golden("vae_train"))
    eng = _engine()
    first = None
    for mode in (0, 1, 1, 0):
        hip_option("wgrad_stream", mode)
        _step(eng, *batch)
        first = eng.grads.clone() if first is None else first
        assert torch.equal(eng.grads, first), mode


@gpu
def test_grouped_launch_against_one_launch_per_block(golden, hip_option):
    """The WaveNet stacks' weight gradients in one grouped launch (blockIdx.z, shifts scaled by 2^group) against one launch per
    block: both inside the reference's bar, and each tensor within the split-operand contraction bound of the other (the two
    may slice the frames differently: tile-slices count the groups)."""
    hip_option("wgrad_tn_x3", 1)
    g = golden("vae_train")
    batch = _chain_batch(g)
    eng = _engine()
    grads = {}
    for mode in (1, 0):
        hip_option("wgrad_groups", mode)
        _step(eng, *batch)
        TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3)
        grads[mode] = {k: v.clone().cpu() for k, v in eng.grad_dict().items()}
    worst = 0.0
    for k, a in grads[1].items():
        d = (a.double() - grads[0][k].double()).abs().max().item()
        worst = max(worst, d / max(1.0, a.abs().max().item()))
        assert d < 1e-4 * max(1.0, a.abs().max().item()), (k, d)
    print("wgrad_tn_x3 grouped vs per block: worst difference relative to max(1, max |g|):", worst)


@gpu
def test_option_off_against_on(golden, hip_option):
    g = golden("vae_train")
    batch = _chain_batch(g)
    eng = _engine()
    grads = {}
    for mode in (0, 1):
        hip_option("wgrad_tn_x3", mode)
        _step(eng, *batch)
        print(f"wgrad_tn_x3 = {mode}: worst relative gradient error vs the reference:", TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3))
        grads[mode] = {k: v.clone().cpu() for k, v in eng.grad_dict().items()}
    differ = []
    for k, a in grads[0].items():
        if a.dim() < 2:  # bias and norm gradients: those kernels are untouched
            assert torch.equal(a.view(torch.int32), grads[1][k].view(torch.int32)), k
        elif not torch.equal(a, grads[1][k]):
            differ.append(k)
    print(f"{len(differ)} weight-gradient tensors differ in bits between the two routes")
    assert differ
