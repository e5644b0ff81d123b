"""Operator grid of the inference pointwise and selection kernels of csrc/pointwise.hip against float64, at the edges of their
launch geometry: dn_rmsnorm, dn_time_cond, dn_ddim_step, dn_q_sample, dn_posterior_sample, dn_argmax_units, dn_convert_rows,
dn_cmlm_step / dn_cmlm_step_dev.  Every case below is there for a branch or a bound of a kernel or of its launcher (the comment at
each parametrisation says which).  Conventions of test_hip_train_ops_grid.py: seeded CPU inputs, the float64 restatement computed
in the test on the values the device holds, calls through diffnorm_amd.ops where a wrapper takes the arguments and through the C
ABI where it does not (a DN_BF16X3 store, out_act / ld_act, ldz, the ld of the arg-max, dn_cmlm_step_dev).  Every output is
pre-filled with NaN (integers: a sentinel), every input column or row the kernel must not read holds NaN (the arg-max: +inf).

Bounds (error over the largest reference magnitude unless it says per element).
  * Where test_hip_ops.py has a bound for the kernel it is used unchanged: rmsnorm 2e-6 (none / gamma) and 5e-6 (gamma_beta),
    time_cond 5e-5, posterior 1e-5 (z) and 1e-5 relative (KL row).
  * Those were set at D = 192 and 65 features.  rmsnorm at D > 1024 (the re-read loop) and time_cond at 401 features have no project
    figure: each such case measures a plain fp32 CPU restatement of the kernel's formulas (torch fp32, torch's summation order)
    against the float64 one, reference against reference, and the kernel gets 4 times that error (as dn_time_cond_backward in the
    training grid: the summation order differs, the device's sqrtf / sinf / expf are accurate to a few ulp), never less than one ulp
    of fp32 at the output's maximum.  The test prints restatement error, bound and kernel error.
  * A 2-byte store adds the format's unit roundoff (bf16 2^-8, f16 2^-11, test_hip_conformer.py's figures) times the element's
    reference magnitude, per element; a split store adds 2^-16 (X3_STORE).
  * Where a stricter statement can be derived it is asserted instead: an activation copy written beside an fp32 output equals that
    output rounded to the type, bit for bit (f16 saturates at 65504, as to_h16 does); pad columns are exactly 0 or untouched.
  * dn_ddim_step / dn_q_sample in fp32 are bit-equal to a CPU restatement that performs the kernel's operations in the kernel's
    order: every operation is a correctly rounded IEEE operation on both sides, so equality is derived, not measured.  The
    operations are the ones the kernels are built from, which csrc/pointwise.hip writes down at sched_update and
    chain_start_kernel (the device loops are tested bit-equal to them): hipcc's __fmul_rn / __fadd_rn / __fsub_rn are the plain
    operators, and a product is contracted into the sum that takes it -- x - s1 eps, x - sa x1, x1 c2 onto the rounded c3 pn, a x
    onto the rounded b noise are one fused multiply-add each, the divisions and the remaining products round on their own.
    `fma32` is that operation on the host, with one rounding.  The unfused chain (torch's own fp32 statements, what the reference
    runs) differs from it in the last bit of some elements; the test prints how many.  The 2e-6 / 1e-6 comparison of
    test_hip_ops.py against the oracle stays as a second assertion.
  * dn_convert_rows, dn_argmax_units and the tokens of dn_cmlm_step are exact; the cmlm scores take test_hip_nar_cg.py's
    rtol 1e-5 + atol 2e-6.
NaN logits are out of scope (dn_argmax_units, dn_cmlm_step): torch.argmax returns a NaN's index, the kernels skip it.
"""
import math

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
import nar_cg_ref as G
from test_hip_nar_cg import kernel_inputs
from test_hip_train_ops import DEV, ops, relerr, seeded  # noqa: F401  (ops: the module fixture)
from test_hip_train_ops_grid import TC_CASES, U, X3_STORE, _lib, _stream, pad32, tc_angle32, tc_inputs, x3_buf, x3_read, x3_src  # noqa: F401

pytestmark = pytest.mark.gpu

NAN = float("nan")
KINDS = ("f32", "bf16", "f16", "x3")
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
UNIT = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11, "x3": 0.0}  # per element; x3 adds X3_STORE over the maximum


def code(kind):
    L, _ = _lib()
    return {"f32": L.DN_F32, "bf16": L.DN_BF16, "f16": L.DN_F16, "x3": L.DN_BF16X3}[kind]


def act_buf(kind, rows, ld):
    """A [rows, ld] output of `kind` on the device, NaN everywhere."""
    return x3_buf(rows, ld) if kind == "x3" else torch.full((rows, ld), NAN, dtype=TD[kind], device=DEV)


def act_read(kind, buf, rows, ld):
    return x3_read(buf, rows, ld) if kind == "x3" else buf.double().cpu()


def rounded(kind, t):
    """fp32 -> float64 of what a store of `kind` keeps of it (to_h16 / store1_split restated; f16 saturates)."""
    t = t.float()
    if kind == "f32":
        return t.double()
    if kind == "bf16":
        return t.to(torch.bfloat16).double()
    if kind == "f16":
        return t.clamp(-65504.0, 65504.0).to(torch.float16).double()
    hi = t.to(torch.bfloat16).float()
    return (hi + (t - hi).to(torch.bfloat16).float()).double()


def stored_ratio(kind, got, want, tol):
    """-> worst |got - want| / bound, bound = (tol [+ 2^-16 for a split store]) max |want| + unit roundoff |want| per element."""
    want = want.double()
    bound = (tol + (X3_STORE if kind == "x3" else 0.0)) * want.abs().max() + UNIT[kind] * want.abs()
    return ((got.double() - want).abs() / bound.clamp_min(1e-300)).max().item()


def ulp_rel(m):
    """One ulp of fp32 at m, over m."""
    return 2 * U * 2.0 ** math.floor(math.log2(m)) / m


def untouched(t):
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------------------------ RMSNorm
# One wave per row, four rows per workgroup; lane l holds columns 4 (64 i + l) .. + 3 in register slot i = 0..3, columns from 1024
# on are re-read in passes of 256; the pad columns [D, ldy) are zeroed in passes of 256.
#   D = 4           one lane of slot 0
#   252, 256, 260   slot 0 short of one lane / full / slot 1 with one lane
#   1020, 1024      slot 3 short of one lane / every slot full, the re-read loop not entered
#   1028            the re-read loop's first pass with one lane
#   1280, 1284      its first pass full / the second pass with one lane
#   2052            four full passes and a fifth with one lane
# (i, D) -> ldy - D = (0, 4, 256, 260)[i % 4]: the zeroing loop runs zero, one (4: one lane; 256: every lane) and two passes;
# (B, T) = ((1, 1), (1, 5), (3, 5))[i % 3]: M = 1 (three waves leave), 5 (a short last workgroup of one row), 15 (the last
# workgroup has three rows; T = 5: the sample changes inside workgroups 1 and 2).
RMS_D = [4, 252, 256, 260, 1020, 1024, 1028, 1280, 1284, 2052]
RMS_PADS = (0, 4, 256, 260)
RMS_BT = ((1, 1), (1, 5), (3, 5))
RMS_MODES = ("none", "gamma", "gb", "gb_shared")


def rms_inputs(B, T, D, mode):
    """x [M, D + 4] with NaN behind D and (M > 1) one all-zero row; gamma [D]; gamma_beta with gb_half = D + 8 > D and NaN in every
    column that is neither a gamma nor a beta (per sample: rows of 2 gb_half + 4, the stride; shared: one row)."""
    M = B * T
    x = torch.full((M, D + 4), NAN)
    x[:, :D] = seeded((M, D), 1, 3.0)
    zero_row = M // 2 if M > 1 else None
    if zero_row is not None:
        x[zero_row, :D] = 0
    gamma = 1 + 0.1 * seeded((D,), 2) if mode == "gamma" else None
    gb, gb_half = None, 0
    if mode in ("gb", "gb_shared"):
        gb_half = D + 8
        rows = 1 if mode == "gb_shared" else B
        gb = torch.full((rows, 2 * gb_half + (0 if mode == "gb_shared" else 4)), NAN)
        gb[:, :D] = 1 + 0.3 * seeded((rows, D), 3)
        gb[:, gb_half:gb_half + D] = seeded((rows, D), 4)
    return x, zero_row, gamma, gb, gb_half


def rms_restate(x, D, T, gamma, gb, gb_half, dtype):
    """y = x / max(|x|, 1e-12) sqrt(D) [gamma] [g_c[row / T] + b_c[row / T]] in `dtype`, the kernel's order of operations."""
    v = x[:, :D].to(dtype)
    denom = (v * v).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    y = v / denom * torch.tensor(float(D), dtype=dtype).sqrt()
    if gamma is not None:
        y = y * gamma.to(dtype)
    if gb is not None:
        sample = torch.arange(x.shape[0]) // T if gb.shape[0] > 1 else torch.zeros(x.shape[0], dtype=torch.long)
        y = y * gb[sample, :D].to(dtype) + gb[sample, gb_half:gb_half + D].to(dtype)
    return y


def rms_bound(x, D, T, gamma, gb, gb_half, want):
    """-> (fp32 bound, the fp32 restatement's error or None where the project bound applies)"""
    if D <= 1024:
        return (2e-6 if gb is None else 5e-6), None
    e32 = relerr(rms_restate(x, D, T, gamma, gb, gb_half, torch.float32), want)
    return max(4 * e32, ulp_rel(want.abs().max().item())), e32


def rms_call(ops_, kind, x_d, M, D, T, ldy, gamma_d, gb_d, shared, gb_half):
    """-> float64 [M, ldy] on the host"""
    if kind != "x3":
        out = torch.full((M, ldy), NAN, dtype=TD[kind], device=DEV)
        ops_.rmsnorm(x_d, out, T, D=D, gamma=gamma_d, gamma_beta=gb_d, gb_shared=shared, gb_half=gb_half)
        return out.double().cpu()
    L, lib = _lib()
    out = x3_buf(M, ldy)
    gb_ld = 0 if (gb_d is None or shared) else gb_d.stride(0)
    L.check(lib.dn_rmsnorm(x_d.data_ptr(), x_d.shape[1], out.data_ptr(), ldy, L.DN_BF16X3, M, D, T, L.ptr(gamma_d), L.ptr(gb_d), gb_ld, gb_half,
                           _stream()), "dn_rmsnorm x3")
    return x3_read(out, M, ldy)


def rms_check(ops_, tag, kind, B, T, D, pad, mode, inputs, want, tol):
    x, zero_row, gamma, gb, gb_half = inputs
    dev = lambda t: t.to(DEV) if t is not None else None
    got = rms_call(ops_, kind, dev(x), B * T, D, T, D + pad, dev(gamma), dev(gb), mode == "gb_shared", gb_half)
    r = stored_ratio(kind, got[:, :D], want, tol)
    assert r <= 1.0, (tag, kind, mode, D, pad, r)
    assert (got[:, D:] == 0).all(), (tag, kind, mode, D, pad)  # exactly zero (and written: the buffer held NaN)
    if zero_row is not None:  # |x| = 0: 0 / 1e-12 = 0 -> beta, or 0; finite
        beta = gb[zero_row // T if gb.shape[0] > 1 else 0, gb_half:gb_half + D] if gb is not None else torch.zeros(D)
        assert torch.equal(got[zero_row, :D], rounded(kind, beta)), (tag, kind, mode, D)
    return r


@pytest.mark.parametrize("i,D", list(enumerate(RMS_D)))
def test_rmsnorm_every_width(ops, i, D):
    ops_, _, _ = ops
    (B, T), pad = RMS_BT[i % 3], RMS_PADS[i % 4]
    inputs = rms_inputs(B, T, D, "gamma")
    x, _, gamma, gb, gb_half = inputs
    want = rms_restate(x, D, T, gamma, gb, gb_half, torch.float64)
    tol, e32 = rms_bound(x, D, T, gamma, gb, gb_half, want)
    r = rms_check(ops_, "width", "f32", B, T, D, pad, "gamma", inputs, want, tol)
    print(f"GRID rmsnorm f32 gamma D={D} M={B * T} pad={pad}: fp32 restatement {e32 if e32 is None else format(e32, '.3e')} bound {tol:.3e} "
          f"measured {r * tol:.3e}")


# D = 260 (registers only, slot 1 with one lane) and 1028 (the re-read loop): every mode x every store x every pad width, at
# (B, T) = (3, 5) -- the per-sample gamma_beta row changes inside a workgroup, the last workgroup is short, row 7 is all zero.
@pytest.mark.parametrize("D", [260, 1028])
def test_rmsnorm_every_mode_and_store(ops, D):
    ops_, _, _ = ops
    B, T = 3, 5
    for mode in RMS_MODES:
        inputs = rms_inputs(B, T, D, mode)
        x, _, gamma, gb, gb_half = inputs
        want = rms_restate(x, D, T, gamma, gb, gb_half, torch.float64)
        tol, e32 = rms_bound(x, D, T, gamma, gb, gb_half, want)
        for kind in KINDS:
            worst = max(rms_check(ops_, "mode", kind, B, T, D, pad, mode, inputs, want, tol) for pad in RMS_PADS)
            print(f"GRID rmsnorm {kind} {mode} D={D}: fp32 restatement {e32 if e32 is None else format(e32, '.3e')} fp32 bound {tol:.3e} "
                  f"worst error / bound {worst:.3e}")


# ------------------------------------------------------------------------------------------------------------ time conditioning
def tc_forward(times, wf, W, bias, dtype):
    """silu(W [t, sin, cos] + bias) in `dtype` on the fp32 angle (test_hip_train_ops_grid.py: tc_f64 / tc_f32's convention)."""
    ang = tc_angle32(times, wf).to(dtype)
    feat = torch.cat((times.to(dtype)[:, None], ang.sin(), ang.cos()), dim=-1)
    z = (feat[:, None, :] * W.to(dtype)[None, :, :]).sum(-1) + bias.to(dtype)
    return z / (1.0 + torch.exp(-z))


# TC_CASES of the backward grid, for the forward kernel: grid (ceil(C / 16), B), wave w of a workgroup owns outputs 16 x + 4 w + i,
# 256 threads fill 2 half + 1 features in LDS.
#   (1, 1, 1)      C = 1: wave 0 breaks at i = 1, waves 1-3 own nothing; 3 features: 61 lanes of the dot product idle
#   (3, 8, 16)     one full workgroup; times 999, 0, 1
#   (5, 16, 250)   the last workgroup breaks at c = 250 in wave 2
#   (40, 64, 256)  129 features: the dot product strides three times; sixteen workgroups per sample
#   (2, 200, 20)   401 features: the LDS fill strides (256 threads), the dot product seven times -- no project bound here
# ldo = C + 3 at every case (the launcher asks no multiple of 4 of C or ldo): the three pad columns of `out` and of the copy stay
# as they were.  times come from tc_inputs: 999, 0, 1 first (B = 1 has 999 alone, B = 2 has 999 and 0).
@pytest.mark.parametrize("B,half,Cn", TC_CASES)
def test_time_cond_forward(ops, B, half, Cn):
    ops_, _, _ = ops
    L, lib = _lib()
    times, wf, W, bias, _, _ = tc_inputs(B, half, Cn)
    want = tc_forward(times, wf, W, bias, torch.float64)
    e32 = relerr(tc_forward(times, wf, W, bias, torch.float32), want)
    tol = 5e-5 if 2 * half + 1 <= 256 else max(4 * e32, ulp_rel(want.abs().max().item()))
    ldo = Cn + 3
    dev = lambda t: t.to(DEV).contiguous()
    t_d, wf_d, W_d, b_d = dev(times.int()), dev(wf), dev(W), dev(bias)
    first = None
    for kind in (None,) + KINDS:
        out = torch.full((B, ldo), NAN, device=DEV)
        act = act_buf(kind, B, ldo) if kind else None
        if kind == "x3":
            L.check(lib.dn_time_cond(t_d.data_ptr(), B, wf_d.data_ptr(), half, W_d.data_ptr(), b_d.data_ptr(), Cn, out.data_ptr(), act.data_ptr(),
                                     L.DN_BF16X3, ldo, _stream()), "dn_time_cond x3")
        else:
            ops_.time_cond(t_d, wf_d, W_d, b_d, out, out_act=act)
        out = out.cpu()
        e = relerr(out[:, :Cn], want)
        assert e <= tol, (kind, e, tol)
        assert untouched(out[:, Cn:])
        first = out if first is None else first
        assert torch.equal(out[:, :Cn], first[:, :Cn])  # the copy does not change the fp32 result
        if kind:
            got = act_read(kind, act, B, ldo)
            assert torch.equal(got[:, :Cn], rounded(kind, out[:, :Cn])), kind  # the fp32 value, rounded once
            assert untouched(got[:, Cn:]), kind
    print(f"GRID time_cond B={B} half={half} C={Cn}: fp32 restatement {e32:.3e} bound {tol:.3e} measured {e:.3e}")


# ------------------------------------------------------------------------------------------------------------ DDIM step, q_sample
# One thread per element of [M, C], at most 2048 workgroups of 256 (ew_grid), the rest by a grid-stride loop.
#   (3, 21, 16)     test_hip_ops.py's shape: 1008 elements, four workgroups, the last short
#   (2, 1025, 260)  533,000 elements > 2048 x 256 = 524,288: the loop takes a second trip for 8,712 threads; C = 260 is no power
#                   of two (the i / C split); T = 1025: the sample changes at element 266,500, inside the first trip
# ld = C + 4, ld_act = C + 8 != ld: pads of x and eps NaN, pads of both outputs untouched.
EW_SHAPES = [(3, 21, 16), (2, 1025, 260)]


def ew_times(B, top):
    """top, middle, 1 and 0 over two calls"""
    return ([top, top // 2, 1], [0, 1, top]) if B == 3 else ([top, top // 2], [1, 0])


def padded(t, ld):
    M, Cn = t.shape
    p = torch.full((M, ld), NAN)
    p[:, :Cn] = t
    return p


def fma32(a, b, c):
    """fl32(a b + c), one rounding: the product of two fp32 values is exact in float64, the sum is rounded to odd there (TwoSum gives
    its error; an inexact sum takes the neighbour with the odd last bit), and 53 >= 2 * 24 + 2 bits make the final rounding exact."""
    a, b, c = torch.broadcast_tensors(a.double(), b.double(), c.double())
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.contiguous().view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.tensor(float("inf"), dtype=torch.float64), torch.tensor(-float("inf"), dtype=torch.float64))
    return torch.where((err != 0) & even, torch.nextafter(s, toward), s).float()


def ddim_f32(x, e, cf, fused=True):
    """The kernel's chain on the host, one rounding per operation: cf [M, 4] = the sample's coefficient row.  fused: the products
    contracted as the kernel is built (module docstring); else torch's fp32 statements."""
    sa, s1, c2, c3 = (cf[:, i:i + 1] for i in range(4))
    if not fused:
        x1 = (x - s1 * e) / sa.clamp(min=1e-10)
        pn = (x - sa * x1) / s1.clamp(min=1e-10)
        return x1 * c2 + c3 * pn
    x1 = fma32(-s1, e, x) / sa.clamp(min=1e-10)
    pn = fma32(-sa, x1, x) / s1.clamp(min=1e-10)
    return fma32(c2, x1, c3 * pn)


def ew_check_outputs(kind, out, act, M, Cn, ld, ld_act, want, tag):
    out = out.cpu()
    assert torch.equal(out[:, :Cn], want), tag  # bit for bit
    assert untouched(out[:, Cn:]), tag
    if kind:
        got = act_read(kind, act, M, ld_act)
        assert torch.equal(got[:, :Cn], rounded(kind, want)), (tag, kind)
        assert untouched(got[:, Cn:]), (tag, kind)


@pytest.mark.parametrize("B,T,Cn", EW_SHAPES)
def test_ddim_step_and_q_sample(ops, B, T, Cn):
    from diffnorm_amd import scheduler

    L, lib = _lib()
    M, ld, ld_act = B * T, Cn + 4, Cn + 8
    tab, sched = O.ddpm_tables(200), scheduler.DDPMScheduler(200)
    x, eps = seeded((M, Cn), 1), seeded((M, Cn), 2)
    x_d, eps_d = padded(x, ld).to(DEV), padded(eps, ld).to(DEV)
    sample = torch.arange(M) // T
    coef = sched.ddim_coef_table()
    ca, cb = sched.f32("sqrt_alphas_cumprod"), sched.f32("sqrt_one_minus_alphas_cumprod")
    # a table of the test's own: the cosine schedule's sqrt(1 - abar_0) is 6e-3, not 0, so the two 1e-10 clamps are reached with
    # abar = 1 (sa = 1, s1 = 0: pn = (x - x) / 1e-10 = 0) and abar = 0 (sa = 0: x1 = (x - eps) / 1e-10, multiplied by sqrt(abar_prev) = 0)
    edge = torch.tensor([[1.0, 0.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0], [0.6, 0.8, 0.8, 0.6]])
    runs = [(coef, tv, True) for tv in ew_times(B, 199)] + [(edge, [0, 1, 2][:B], False)]
    for table, tvals, vs_oracle in runs:
        t = torch.tensor(tvals)
        t_d, tab_d = t.to(DEV).int(), table.to(DEV).contiguous()
        want = ddim_f32(x, eps, table[t][sample])
        assert torch.isfinite(want).all()
        for kind in (None,) + KINDS:
            out = torch.full((M, ld), NAN, device=DEV)
            act = act_buf(kind, M, ld_act) if kind else None
            L.check(lib.dn_ddim_step(x_d.data_ptr(), eps_d.data_ptr(), out.data_ptr(), L.ptr(act), code(kind or "f32"), ld_act, M, Cn, ld, T,
                                     tab_d.data_ptr(), t_d.data_ptr(), _stream()), "dn_ddim_step")
            ew_check_outputs(kind, out, act, M, Cn, ld, ld_act, want, ("ddim", tvals))
        # in place: every element is read and written by one thread
        io = x_d.clone()
        L.check(lib.dn_ddim_step(io.data_ptr(), eps_d.data_ptr(), io.data_ptr(), None, L.DN_F32, ld_act, M, Cn, ld, T, tab_d.data_ptr(),
                                 t_d.data_ptr(), _stream()), "dn_ddim_step in place")
        ew_check_outputs(None, io, None, M, Cn, ld, ld_act, want, ("ddim in place", tvals))
        if not vs_oracle:
            continue
        ref = O.ddim_update(tab, x.view(B, T, Cn), eps.view(B, T, Cn), t).view(M, Cn)
        assert (want - ref).abs().max().item() < 2e-6 * max(1.0, want.abs().max().item())
        # q_sample on the same tensors (eps as the noise)
        want_q = fma32(ca[t][sample][:, None], x, cb[t][sample][:, None] * eps)
        plain, plain_q = ddim_f32(x, eps, table[t][sample], fused=False), ca[t][sample][:, None] * x + cb[t][sample][:, None] * eps
        print(f"GRID ddim / q_sample {(B, T, Cn)} t={tvals}: bit-equal to the fused chain; the unfused chain differs in "
              f"{int((plain != want).sum())} / {int((plain_q != want_q).sum())} of {M * Cn} elements")
        ca_d, cb_d = ca.to(DEV), cb.to(DEV)
        for kind in (None,) + KINDS:
            out = torch.full((M, ld), NAN, device=DEV)
            act = act_buf(kind, M, ld_act) if kind else None
            L.check(lib.dn_q_sample(x_d.data_ptr(), eps_d.data_ptr(), out.data_ptr(), L.ptr(act), code(kind or "f32"), ld_act, M, Cn, ld, T,
                                    ca_d.data_ptr(), cb_d.data_ptr(), t_d.data_ptr(), _stream()), "dn_q_sample")
            ew_check_outputs(kind, out, act, M, Cn, ld, ld_act, want_q, ("q_sample", tvals))
        ref_q = tab.at("sqrt_alphas_cumprod", t, 3) * x.view(B, T, Cn) + tab.at("sqrt_one_minus_alphas_cumprod", t, 3) * eps.view(B, T, Cn)
        assert (want_q - ref_q.view(M, Cn)).abs().max().item() < 1e-6


# ------------------------------------------------------------------------------------------------------------ posterior sample
# One wave per frame, lane l takes columns l, l + 64, ... below Z and then the pad columns Z + l, Z + l + 64, ... below ldz.
#   Z = 4, 64, 68       one partial lane pass / one full / two
#   ldz - Z = 0, 4, 68  no pad column / one partial pass of the zeroing loop / two
#   (B, T) = (1, 1), (1, 5), (3, 3)   M = 1, 5, 9: three waves leave / a short last workgroup / the frame -> (sample, t) split
#   lengths NULL or (3, 1, 2)[:B] (ragged, a 1 in it); kl_rows NULL or given
# ldp = 2 Z + 4, ldn = Z + 4 with NaN pads.  Frame 0 carries log-variances 20, -30 (the clamp's ends, closed) and 25, -40 (beyond).
POST_BT = ((1, 1), (1, 5), (3, 3))


@pytest.mark.parametrize("Z", [4, 64, 68])
def test_posterior_sample(ops, Z):
    L, lib = _lib()
    worst_z = worst_kl = 0.0
    for B, T in POST_BT:
        M = B * T
        params = padded(seeded((M, 2 * Z), 4, 2.0), 2 * Z + 4)
        noise = padded(seeded((M, Z), 5), Z + 4)
        params[0, Z:Z + 4] = torch.tensor([20.0, -30.0, 25.0, -40.0])
        p64, n64 = params[:, :2 * Z].double(), noise[:, :Z].double()
        want = O.posterior_sample(p64, n64)
        edge = torch.zeros(M, Z, dtype=torch.bool)
        edge[0, :4] = True  # exp(10) |noise| would hide every other element under a tensor-wide maximum: judged each by its own size
        assert torch.equal(want[0, 2:4], p64[0, 2:4] + torch.exp(0.5 * torch.tensor([20.0, -30.0], dtype=torch.float64)) * n64[0, 2:4])
        p_d, n_d = params.to(DEV), noise.to(DEV)
        for lens in (None, torch.tensor([3, 1, 2][:B]).clamp(max=T)):
            mask = O.lengths_to_mask(lens if lens is not None else torch.full((B,), T), T)
            want_kl = 0.5 * (p64[:, :Z] ** 2 + torch.exp(p64[:, Z:].clamp(-30, 20)) - 1.0 - p64[:, Z:].clamp(-30, 20)).sum(-1) * mask.view(M)
            lens_d = lens.to(DEV).int() if lens is not None else None
            for pad in (0, 4, 68):
                ldz = Z + pad
                for kind in (None,) + KINDS:
                    with_kl = not (kind == "f32" and pad == 4)  # kl_rows NULL: the wave sum and the lengths read are skipped
                    z = torch.full((M, ldz), NAN, device=DEV)
                    act = act_buf(kind, M, ldz) if kind else None
                    kl = torch.full((M,), NAN, device=DEV) if with_kl else None
                    L.check(lib.dn_posterior_sample(p_d.data_ptr(), 2 * Z + 4, n_d.data_ptr(), Z + 4, z.data_ptr(), L.ptr(act), code(kind or "f32"),
                                                    ldz, M, Z, T, L.ptr(lens_d), L.ptr(kl), _stream()), "dn_posterior_sample")
                    z = z.cpu()
                    tag = (Z, M, pad, kind, lens is not None)
                    e = relerr(z[:, :Z][~edge], want[~edge]) if bool((~edge).any()) else 0.0
                    ee = ((z[:, :Z][edge].double() - want[edge]).abs() / want[edge].abs()).max().item()
                    worst_z = max(worst_z, e, ee)
                    assert e < 1e-5 and ee < 1e-5, (tag, e, ee)
                    assert (z[:, Z:] == 0).all(), tag
                    if kind:
                        got = act_read(kind, act, M, ldz)
                        assert torch.equal(got[:, :Z], rounded(kind, z[:, :Z])), tag
                        assert (got[:, Z:] == 0).all(), tag
                    if with_kl:
                        kl = kl.double().cpu()
                        valid = mask.view(M)
                        assert (kl[~valid] == 0).all(), tag
                        ek = ((kl[valid] - want_kl[valid]).abs() / want_kl[valid]).max().item()
                        worst_kl = max(worst_kl, ek)
                        assert ek < 1e-5, (tag, ek)
    print(f"GRID posterior Z={Z}: z bound 1.0e-05 measured {worst_z:.3e} | KL row bound 1.0e-05 measured {worst_kl:.3e}")


# ------------------------------------------------------------------------------------------------------------ arg-max
# One wave per row: lane l scans columns l, l + 64, ... below V, then five shuffle steps (32, 16, 8, 4, 2, 1) merge the lanes.
#   V = 1              one lane with a column, 63 with none (best = -inf, index 0x7fffffff)
#   63, 64, 65         one lane short / every lane once / lane 0 twice
#   256                the NAR length predictor's (with offset 0)
#   1004               the unit vocabulary's (with offset 4): the last pass has 44 lanes
# ld = V + 8 with +inf in the eight pad columns: a scan bounded by ld, or a lane that ran on, would return a column >= V.
# The rows (as far as V has the columns): equal maxima at (c, c + 64) -- one lane, two passes; (5, 6) -- neighbouring lanes;
# (0, 32) and (31, 33) -- the two halves of the first shuffle step; an all-equal row; an all -inf row; seeded rows.
# M = 1, 4, 5: three waves leave / one full workgroup / a second workgroup of one row; every chunk of the rows is run at each M.
def argmax_rows(V):
    c = min(7, V - 65)  # V = 65: (0, 64)
    rows = []
    for a, b in ((c, c + 64), (5, 6), (0, 32), (31, 33)):
        if 0 <= a and b < V:
            r = seeded((V,), 80 + a)
            r[a] = r[b] = r.max() + 1.0
            rows.append(r)
    rows += [torch.full((V,), 0.25), torch.full((V,), -float("inf"))]
    return torch.stack(rows + [seeded((V,), 70 + i) for i in range(5)])


@pytest.mark.parametrize("V", [1, 63, 64, 65, 256, 1004])
def test_argmax_units(ops, V):
    L, lib = _lib()
    rows = argmax_rows(V)
    R, ld = rows.shape[0], V + 8
    full = torch.full((R, ld), float("inf"))
    full[:, :V] = rows
    full_d = full.to(DEV)
    first_max = rows.argmax(-1)
    assert first_max[R - 6] == 0 and first_max[R - 7] == 0  # the all -inf and the all-equal row: torch takes the first of equal maxima
    for offset in (0, 4):
        for M in (1, 4, 5):
            for r0 in range(0, R - M + 1, M):
                units = torch.full((M + 4,), -777, dtype=torch.int32, device=DEV)
                L.check(lib.dn_argmax_units(full_d[r0:].data_ptr(), ld, M, V, offset, units.data_ptr(), _stream()), "dn_argmax_units")
                units = units.cpu()
                assert units[:M].tolist() == (first_max[r0:r0 + M] - offset).tolist(), (V, offset, M, r0)
                assert (units[M:] == -777).all()


# ------------------------------------------------------------------------------------------------------------ row conversion
def convert_source(kind, vals):
    """fp32 [M, lds] (NaN pads) -> (the device tensor of `kind`, the float32 values it holds)"""
    if kind == "x3":
        return x3_src(vals)
    held = rounded(kind, vals).float()
    return held.to(DEV, TD[kind]), held


def convert_call(src_kind, src_d, lds, dst_kind, M, Cn, ldd):
    L, lib = _lib()
    dst = act_buf(dst_kind, M, ldd)
    L.check(lib.dn_convert_rows(src_d.data_ptr(), code(src_kind), lds, dst.data_ptr(), code(dst_kind), ldd, M, Cn, _stream()), "dn_convert_rows")
    return act_read(dst_kind, dst, M, ldd)


# One thread per DESTINATION element of [M, ldd] (ew_grid: at most 2048 workgroups, then a grid-stride loop); a pad column writes 0
# without reading.  C = 20, lds = 24, ldd = 28: source pads NaN (never read), destination pads exactly 0; every (source,
# destination) pair: the value the source holds, rounded once to the destination's type.
@pytest.mark.parametrize("src_kind", KINDS)
def test_convert_rows_every_pair(ops, src_kind):
    M, Cn, lds, ldd = 5, 20, 24, 28
    src_d, held = convert_source(src_kind, padded(seeded((M, Cn), 90, 3.0), lds))
    for dst_kind in KINDS:
        got = convert_call(src_kind, src_d, lds, dst_kind, M, Cn, ldd)
        assert torch.equal(got[:, :Cn], rounded(dst_kind, held[:, :Cn])), (src_kind, dst_kind)
        assert (got[:, Cn:] == 0).all(), (src_kind, dst_kind)


# M ldd = 18,725 x 28 = 524,300 > 2048 x 256 = 524,288: twelve threads take a second trip of the grid-stride loop (the last
# twelve destination elements: row 18,724, columns 16..27 -- four values and the eight pads).
@pytest.mark.parametrize("dst_kind", ["bf16", "x3"])
def test_convert_rows_past_the_grid_cap(ops, dst_kind):
    M, Cn, lds, ldd = 18725, 20, 24, 28
    assert M * ldd > 2048 * 256 >= (M - 1) * ldd
    src_d, held = convert_source("f32", padded(seeded((M, Cn), 91, 3.0), lds))
    got = convert_call("f32", src_d, lds, dst_kind, M, Cn, ldd)
    assert torch.equal(got[:, :Cn], rounded(dst_kind, held[:, :Cn]))
    assert (got[:, Cn:] == 0).all()


# ------------------------------------------------------------------------------------------------------------ mask-predict update
CM = dict(V=1004, B=3, unk=3, pad=1, eos=2)


def cmlm_inputs(T, step, max_step):
    """kernel_inputs' batch with scale 0 (the conditioned logits alone) and the scores of `earlier iterations` at the positions
    that are not masked (pad / eos: 0).  In a row that re-masks (boundary k > 0) some masked positions are turned into decisions of
    earlier iterations (token = the arg-max, so the non-pad count stays) and the old scores are laid into the 0.05 gap that
    kernel_inputs leaves between the new scores to re-mask and the new scores to keep:
        r old scores below every kept new one (old decisions that are re-masked),
        a group of t_in + t_out equal scores v1 ACROSS the boundary (the t_in lowest positions are re-masked: the case under test),
        a pair of equal scores v2 > v1 right above it on the kept side, and the rest among the kept new scores.
    -> (logits, tokens, scores, [(row, the v1 group's positions, t_in)])"""
    V, B, unk, pad = CM["V"], CM["B"], CM["unk"], CM["pad"]
    cond, _, tok = kernel_inputs(T, 0.0, step, max_step)
    g = torch.Generator().manual_seed(7000 + 10 * T + step)
    rand = lambda n: torch.rand(n, generator=g)
    new_sc, new_tk = torch.log_softmax(cond.double(), -1).max(-1)
    scores = torch.zeros(B, T)
    groups = []
    for b in range(B):
        masked = tok[b].eq(unk)
        olds = tok[b].ge(4).nonzero().flatten().tolist()
        k = G._boundary(int(torch.where(masked, new_tk[b], tok[b]).ne(pad).sum()), step, max_step) if step + 1 < max_step else 0
        mpos = masked.nonzero().flatten()
        order = mpos[new_sc[b][mpos].argsort()].tolist()  # masked positions by ascending new score
        lows, keeps = order[:k], order[k:]
        ok = lambda ps: [p for p in ps if int(new_tk[b, p]) >= 4]  # a decision that is a regular token
        conv = ok(lows)[-3:] + ok(keeps[1:])[-4:]
        u = len([p for p in conv if p in lows])
        if k == 0 or len(order) < k or u == 0 or len(olds) + len(conv) - u == 0:
            scores[b, olds] = -(0.05 + 3 * rand(len(olds)))
            continue
        tok[b, conv] = new_tk[b, conv]
        left = lambda ps: [p for p in ps if p not in conv]
        ghi = float(new_sc[b][left(keeps)].min()) if left(keeps) else -0.05
        glo = float(new_sc[b][left(lows)].max()) if left(lows) else ghi - 1.0
        assert ghi - glo >= 0.04, (T, step, b, glo, ghi)
        perm = sorted(olds + conv)
        perm = [perm[i] for i in torch.randperm(len(perm), generator=g).tolist()]
        t_in = min(2, u)
        r = u - t_in
        t_out = min(2, len(perm) - r - t_in)
        pair = 2 if len(perm) - r - t_in - t_out >= 2 else 0
        below, tie, twins, rest = (perm[a:z] for a, z in ((0, r), (r, r + t_in + t_out), (r + t_in + t_out, r + t_in + t_out + pair),
                                                          (r + t_in + t_out + pair, len(perm))))
        scores[b, below] = glo - 0.01 - 2 * rand(len(below))
        scores[b, tie] = glo + 0.4 * (ghi - glo)
        scores[b, twins] = glo + 0.7 * (ghi - glo)
        scores[b, rest] = ghi * (0.05 + 0.85 * rand(len(rest)))
        groups.append((b, sorted(tie), t_in))
    scores[tok.eq(unk)] = -7.0  # stale: a masked position's score is replaced
    return cond, tok, scores, groups


def cmlm_run(entry, logits_d, tok, scores, step, max_step, V=None):
    """-> (tokens, scores, predicted) of dn_cmlm_step (`entry` "host") or dn_cmlm_step_dev ("dev") on copies of tok / scores"""
    L, lib = _lib()
    B, T = tok.shape
    t_d, s_d = tok.to(DEV).int().contiguous(), scores.to(DEV).contiguous()
    pred = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    args = (B, T, CM["V"] if V is None else V)
    if entry == "host":
        L.check(lib.dn_cmlm_step(logits_d, t_d.data_ptr(), s_d.data_ptr(), pred.data_ptr(), *args, step, max_step, CM["unk"], CM["pad"], _stream()),
                "dn_cmlm_step")
    else:
        step_d = torch.tensor([step], dtype=torch.int32, device=DEV)
        L.check(lib.dn_cmlm_step_dev(logits_d, t_d.data_ptr(), s_d.data_ptr(), pred.data_ptr(), *args, step_d.data_ptr(), max_step, CM["unk"],
                                     CM["pad"], _stream()), "dn_cmlm_step_dev")
    return t_d.cpu().long(), s_d.cpu(), pred.cpu().long()


def guarded(logits, guard=4096):
    """The logits between NaN guards on the device -> (the buffer, the address of the first logit)"""
    buf = torch.full((logits.numel() + 2 * guard,), NAN)
    buf[guard:guard + logits.numel()] = logits.reshape(-1)
    buf = buf.to(DEV)
    return buf, buf.data_ptr() + 4 * guard


# test_guided_update_kernel's grid for the kernel that KEEPS the scores (forward_decoder / refine, the captured iteration's).
# One workgroup per row, one wave per position (stride 4), the rank loop 256 threads stride T over s_sc[0..T).
#   T = 2       lengths (2, 2, 2): nothing to re-mask (boundary trunc(0 p) = 0)
#   T = 5       one turn of every loop, wave 0 takes two positions; rows of 5, 2, 2
#   T = 33      lengths 33, 16, 2: nine positions per wave and a tenth for wave 0
#   T = 257     the rank loop's second turn, for thread 0 alone
#   T = 2048    the whole of s_sc / s_tok (the refused size is 2049)
# steps 0, 4, 9 of 10: everything masked / a mix of old, new and zero scores / the last iteration, which re-masks nothing and
# passes every old score through.  V = 1004 is no multiple of 64: a lane that ran on would read the next row, or the guard.
@pytest.mark.parametrize("T", [2, 5, 33, 257, 2048])
def test_cmlm_step_keeps_earlier_scores(ops, T):
    max_step, unk, pad = 10, CM["unk"], CM["pad"]
    straddled_rows = 0
    for step in (0, 4, 9):
        logits, tok, scores, groups = cmlm_inputs(T, step, max_step)
        m_arg, gap, zeros, straddled = G.kept_margins(logits, tok, scores, step, max_step, unk, pad)
        assert m_arg >= G.MARGIN and gap >= G.MARGIN and zeros == 0, (T, step, m_arg, gap, zeros)
        assert straddled == len(groups), (T, step, straddled, groups)
        ref_tok, ref_sc, ref_pred = G.kept_update(logits, tok, scores, step, max_step, unk, pad)
        for b, tie, t_in in groups:  # the reference itself resolves the equal scores by position
            assert len(tie) > t_in >= 1 and len({float(scores[b, p]) for p in tie}) == 1
            assert [p for p in tie if ref_tok[b, p] == unk] == tie[:t_in], (T, step, b, tie)
            assert [float(ref_sc[b, p]) for p in tie[t_in:]] == [float(scores[b, p]) for p in tie[t_in:]]
        straddled_rows += len(groups)
        kept = tok.ge(4) & ref_tok.ne(unk)
        assert torch.equal(ref_sc[kept], scores[kept])  # an old score that survives is passed through, not recomputed
        buf, addr = guarded(logits)
        for entry in ("host", "dev"):
            got_tok, got_sc, got_pred = cmlm_run(entry, addr, tok, scores, step, max_step)
            assert got_tok.tolist() == ref_tok.tolist(), (T, step, entry)
            assert got_pred.tolist() == ref_pred.tolist(), (T, step, entry)
            np.testing.assert_allclose(got_sc.numpy(), ref_sc.numpy(), rtol=1e-5, atol=2e-6)
            assert torch.equal(got_sc[kept], scores[kept]), (T, step, entry)
    assert straddled_rows >= (0 if T == 2 else 2), straddled_rows  # steps 0 and 4 each lay a group across a boundary (T = 2: none to lay)


def test_cmlm_step_short_rows_and_both_entries_in_step(ops):
    """Rows with two, one and no non-pad token: the boundary trunc((n - 2) p) is 0, 0 (trunc(-0.9)) and -1 -- nothing is re-masked.
    And the two entries in step: max_step 1 (the first iteration is the last), 3 and 4 -- the device-stepped entry derives p and the
    last-iteration flag from its counter exactly as the host does, so tokens, scores and predicted agree bit for bit at every step."""
    V, unk, pad, eos = CM["V"], CM["unk"], CM["pad"], CM["eos"]
    T = 5
    logits = seeded((3, T, V), 95)
    logits[0, :, 17] += 6.0   # row 0: unk eos pad pad pad -> 17 eos: two non-pad tokens
    logits[1, :, 23] += 6.0   # row 1: unk pad pad pad pad -> 23: one
    logits[2, :, pad] += 6.0  # row 2: unk pad pad pad pad -> the arg-max IS pad: none
    tok = torch.full((3, T), pad)
    tok[:, 0] = unk
    tok[0, 1] = eos
    scores = torch.zeros(3, T)
    assert G.kept_margins(logits, tok, scores, 0, 10, unk, pad)[0] >= G.MARGIN
    ref_tok, ref_sc, ref_pred = G.kept_update(logits, tok, scores, 0, 10, unk, pad)
    assert ref_tok[:, 0].tolist() == [17, 23, pad] and not bool(ref_tok.eq(unk).any())
    buf, addr = guarded(logits)
    for entry in ("host", "dev"):
        got_tok, got_sc, got_pred = cmlm_run(entry, addr, tok, scores, 0, 10)
        assert got_tok.tolist() == ref_tok.tolist() and got_pred.tolist() == ref_pred.tolist(), entry
        np.testing.assert_allclose(got_sc.numpy(), ref_sc.numpy(), rtol=1e-5, atol=2e-6)
    T, B = 33, CM["B"]
    for max_step in (1, 3, 4):
        lens = [T, T // 2, 2]
        start = torch.full((B, T), pad)
        for b, n in enumerate(lens):
            start[b, :n - 1] = unk
            start[b, n - 1] = eos
        state = {e: (start, torch.zeros(B, T)) for e in ("host", "dev")}
        for step in range(max_step):
            buf, addr = guarded(seeded((B, T, V), 960 + 10 * max_step + step))
            out = {e: cmlm_run(e, addr, *state[e], step, max_step) for e in state}
            for a, d in zip(out["host"], out["dev"]):
                assert torch.equal(a, d), (max_step, step)
            n_masked = int(out["host"][0].eq(unk).sum())  # the boundaries of the rows, from the non-pad counts of `predicted`
            want_masked = sum(max(G._boundary(int(n), step, max_step), 0) for n in out["host"][2].ne(pad).sum(1)) if step + 1 < max_step else 0
            assert n_masked == want_masked, (max_step, step, n_masked)
            state = {e: out[e][:2] for e in out}


def narrow_inputs(T, V, step, max_step):
    """Every position of three ragged rows masked (rows of T, T // 2 and 2 tokens where T allows; T = 1: one masked, one eos, one
    pad), logits whose column 0 stands clear of the rest: by 1 .. 1.5 at the positions the iteration re-masks, by 3 .. 5 at those
    it keeps, so a gap stands at every re-mask boundary.  The margins are CHECKED by the caller, not assumed."""
    unk, pad, eos = CM["unk"], CM["pad"], CM["eos"]
    g = torch.Generator().manual_seed(7000 + 10 * T + V + step)
    logits = 0.1 * torch.randn(3, T, V, generator=g)
    tok = torch.full((3, T), pad)
    for b, n in enumerate([T, T // 2, 2] if T >= 4 else [1, 1, 0]):
        if n:
            tok[b, :n] = unk
            tok[b, n - 1] = eos if (T >= 4 or b == 1) else unk
        masked = int(tok[b].eq(unk).sum())
        k = max(G._boundary(n, step, max_step), 0) if step + 1 < max_step else 0
        low = torch.randperm(masked, generator=g)[:k]
        rise = 3.0 + 2.0 * torch.rand(T, generator=g)
        rise[low] = 1.0 + 0.5 * torch.rand(k, generator=g)
        logits[b, :, 0] += rise
    return logits, tok


# Both mask-predict kernels share one body: a single position (T = 1: nothing to rank), the rank loop's second turn (T = 257), and
# vocabularies narrower than a wave (V = 2: 62 idle lanes; V = 65: one lane takes a second column), against the host restatements.
@pytest.mark.parametrize("T,V", [(1, 2), (1, 65), (33, 65), (257, 2), (257, 65)])
def test_cmlm_steps_at_one_position_and_narrow_vocabularies(ops, T, V):
    L, lib = _lib()
    max_step, unk, pad, B = 10, CM["unk"], CM["pad"], 3
    for step in (0, 4, 9):
        logits, tok = narrow_inputs(T, V, step, max_step)
        zeros = torch.zeros(B, T)
        # ---- the kernel that keeps the scores
        m_arg, gap, nz, _ = G.kept_margins(logits, tok, zeros, step, max_step, unk, pad)
        assert m_arg >= G.MARGIN and gap >= G.MARGIN and nz == 0, (T, V, step, m_arg, gap, nz)
        ref_tok, ref_sc, ref_pred = G.kept_update(logits, tok, zeros, step, max_step, unk, pad)
        if T > 1 and step + 1 < max_step:
            assert bool(ref_tok.eq(unk).any())  # (something is re-masked)
        buf, addr = guarded(logits)
        for entry in ("host", "dev"):
            got_tok, got_sc, got_pred = cmlm_run(entry, addr, tok, zeros, step, max_step, V=V)
            assert got_tok.tolist() == ref_tok.tolist() and got_pred.tolist() == ref_pred.tolist(), (T, V, step, entry)
            np.testing.assert_allclose(got_sc.numpy(), ref_sc.numpy(), rtol=1e-5, atol=2e-6)
        # ---- the guided kernel: cond and null chosen so that cond + scale (cond - null) is `logits` up to rounding
        scale = 3.0
        null = 0.5 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(T + V))
        cond = (logits + scale * null) / (1 + scale)
        scaled = cond + scale * (cond - null)
        m_arg, gap, nz = G.margins(scaled, tok, step, max_step, unk, pad)
        assert m_arg >= G.MARGIN and gap >= G.MARGIN and nz == 0, (T, V, step, m_arg, gap, nz)
        ref_tok, ref_sc, ref_pred = G.guided_update(scaled, tok, step, max_step, unk, pad)
        buf2, addr2 = guarded(torch.cat([cond.reshape(-1), null.reshape(-1)]))
        step_d = torch.tensor([step], dtype=torch.int32, device=DEV)
        for entry in ("host", "dev"):
            t_d, s_d = tok.to(DEV).int().contiguous(), torch.full((B, T), 7.0, device=DEV)  # stale scores: the kernel starts from zero
            pred = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
            if entry == "host":
                L.check(lib.dn_cmlm_guided_step(addr2, scale, t_d.data_ptr(), s_d.data_ptr(), pred.data_ptr(), B, T, V, step, max_step, unk, pad,
                                                _stream()), "dn_cmlm_guided_step")
            else:
                L.check(lib.dn_cmlm_guided_step_dev(addr2, scale, t_d.data_ptr(), s_d.data_ptr(), pred.data_ptr(), B, T, V, step_d.data_ptr(), max_step,
                                                    unk, pad, _stream()), "dn_cmlm_guided_step_dev")
            assert t_d.cpu().long().tolist() == ref_tok.tolist() and pred.cpu().long().tolist() == ref_pred.tolist(), (T, V, step, entry)
            np.testing.assert_allclose(s_d.cpu().numpy(), ref_sc.numpy(), rtol=1e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------ refused arguments
def test_refused_arguments_leave_the_outputs(ops):
    """Sizes the kernels cannot take are refused by the launcher's argument check on the host: DN_EINVAL, nothing launched, the
    outputs keep what they held.  (Not parity coverage.)"""
    L, lib = _lib()
    EINVAL = -1
    keep = lambda *shape, dtype=torch.float32: torch.full(shape, 5, dtype=dtype, device=DEV)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    same = lambda *ts: all(bool((t == 5).all()) for t in ts)
    s = _stream()
    x, y = z(4, 16), keep(4, 16)
    # dn_rmsnorm: D % 4 != 0 (the float4 accesses); ldy < D (the row would overrun)
    assert lib.dn_rmsnorm(x.data_ptr(), 16, y.data_ptr(), 16, L.DN_F32, 4, 6, 1, None, None, 0, 0, s) == EINVAL
    assert lib.dn_rmsnorm(x.data_ptr(), 16, y.data_ptr(), 12, L.DN_F32, 4, 16, 1, None, None, 0, 0, s) == EINVAL
    assert b"dn_rmsnorm" in lib.dn_last_error()
    # dn_argmax_units: ld < V
    units = keep(4, dtype=torch.int32)
    assert lib.dn_argmax_units(x.data_ptr(), 12, 4, 16, 0, units.data_ptr(), s) == EINVAL
    # dn_cmlm_step / dn_cmlm_step_dev: T = 2049 does not fit the 2048 scores and tokens a workgroup holds in LDS
    T, V = 2049, 8
    logits, tok, sc, pred = z(1, T, V), keep(1, T, dtype=torch.int32), keep(1, T), keep(1, T, dtype=torch.int32)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.dn_cmlm_step(logits.data_ptr(), tok.data_ptr(), sc.data_ptr(), pred.data_ptr(), 1, T, V, 0, 4, 5, 1, s) == EINVAL
    assert b"2048" in lib.dn_last_error()
    assert lib.dn_cmlm_step_dev(logits.data_ptr(), tok.data_ptr(), sc.data_ptr(), pred.data_ptr(), 1, T, V, step.data_ptr(), 4, 5, 1, s) == EINVAL
    # dn_ddim_step: ld < C
    coef, t = z(4, 4), torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.dn_ddim_step(x.data_ptr(), x.data_ptr(), y.data_ptr(), None, L.DN_F32, 16, 4, 16, 12, 1, coef.data_ptr(), t.data_ptr(), s) == EINVAL
    torch.cuda.synchronize()
    assert same(y, units, tok, sc, pred)
