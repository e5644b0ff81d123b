"""Operator grid of the training backward kernels of csrc/train_ops.hip against float64, at the edges of their launch geometry: every
case below is there for a branch or a bound of a kernel or of its launcher (the comment at each parametrisation says which, worked
out from the launcher's arithmetic).  Conventions of test_hip_train_ops.py: seeded CPU inputs, a float64 restatement with torch
autograd fed the same stored values (bf16: the bf16-rounded inputs; x3: the fp32 inputs, and a split output is read back as hi + lo),
calls through diffnorm_amd.ops -- and through the C ABI where ops has no wrapper (a DN_BF16X3 store, dn_vec_sum, dn_add_broadcast,
dn_split_rows).

Split tensors.  The kernels address a DN_BF16X3 tensor by its flat element offset (common.h split_byte: groups of 32 elements, hi
then lo), and every access here starts at a multiple of 4, inside one group -- so a split tensor is well defined for any row stride
that is a multiple of 4, the engines' multiples of 32 being the special case.  `x3_buf` / `x3_read` / `x3_src` allocate and read such
a tensor flat, rounded up to whole groups.

Bounds.
  * Where test_hip_train_ops.py has a bound for the kernel and mode it is used unchanged (max error over the tensor's largest
    reference magnitude): rmsnorm dx 2e-5, parameter gradients 1e-4, bf16 copies 1e-2; lsce 1e-5 / 1e-2, its loss sums 1e-4; mse 1e-5;
    posterior 1e-5; colsum 1e-5; sum_groups 1e-6.
  * A split (x3) store adds 2^-16 to the fp32 bound (test_hip_attention_grid.py's figure for a split store).
  * Reductions longer than test_hip_train_ops.py's (colsum at 1024 and more rows, the norm's parameter gradients over 1030 and more
    rows, dn_vec_sum) take the summation bound per output, |got - want| <= n 2^-24 sum |term_i| with the sum in float64 (what the
    output is accumulated onto is counted in the sum of magnitudes).  At n = 32776 that alone would not see one lost row, so the row at each
    launch-geometry edge (the last row of every sample: the short last block) carries 1024 times the gradient of the others: losing or
    doubling it is more than ten bounds.
  * dn_time_cond_backward has no project bound: each case measures a plain fp32 CPU restatement (`tc_f32`: the kernel's formulas in
    torch fp32, torch's fixed summation order) against the float64 one (reference against reference) and gives the kernel 4 times that
    error: the device sinf / cosf / expf are accurate to a few ulp, the summation order differs.  The angle is the fp32 product
    ((t w) 2) pi_f32 rounded at each step, as the kernels' __fmul_rn chain and as diffnorm_oracle.time_cond forms it on fp32 weights
    (tests/test_hip_ops.py test_rmsnorm_and_time_cond); in float64 the oracle would form it in float64, and the comparison would
    measure 6000 * 2^-24 of angle rounding instead of the kernel, so `tc_f64` restates the angle locally: the fp32 value, with the
    exact derivative 2 pi t attached.  Each gradient is compared as stored (prefill + increment) over the largest increment; dW is
    judged in two parts, the t column (terms 999 times larger) and the sin / cos columns.
    Measured fp32-restatement errors (dW[:, 0], dW[:, 1:], dbias, dw_freq), the bound being 4 times each:
      (B, half, C)    dW[:, 0]   dW[:, 1:]  dbias      dw_freq
      (1, 1, 1)       3.19e-08   1.77e-07   6.51e-08   4.86e-08
      (3, 8, 16)      6.18e-08   1.30e-07   1.21e-07   1.14e-07
      (5, 16, 250)    7.37e-08   1.35e-07   8.61e-08   1.03e-07
      (40, 64, 256)   1.47e-07   1.47e-07   1.56e-07   1.75e-07
      (2, 200, 20)    1.36e-07   1.37e-07   4.78e-08   1.74e-07
    The test measures them again at every run (they move in the last digit with the host's fp32 sin / cos / exp) and prints them
    beside the kernel's.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import diffnorm_oracle as O
from test_hip_train_ops import DEV, bf16r, ops, relerr, seeded  # noqa: F401  (ops: the module fixture)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24   # unit roundoff of fp32
X3_STORE = 2.0 ** -16
NAN = float("nan")


def _lib():
    from diffnorm_amd import _lib

    return _lib, _lib.load()


def _stream():
    from diffnorm_amd import _lib

    return _lib.current_stream()


def pad32(n):
    return (n + 31) // 32 * 32


def x3_buf(rows, ld, fill=NAN):
    """A split [rows, ld] output on the device (flat, whole groups), pre-filled so that an element never written shows."""
    return torch.full((2 * pad32(rows * ld),), fill, dtype=torch.bfloat16, device=DEV)


def x3_read(buf, rows, ld):
    """hi + lo of a split [rows, ld] tensor -> float64 on the host."""
    from diffnorm_amd import packing

    return packing.unsplit_rows(buf.cpu())[:rows * ld].view(rows, ld).double()


def x3_src(t):
    """fp32 [rows, ld] -> (its flat split image on the device, the float32 values that image holds)."""
    from diffnorm_amd import packing

    flat = torch.zeros(pad32(t.numel()))
    flat[:t.numel()] = t.reshape(-1)
    s = packing.split_rows(flat)
    return s.to(DEV), packing.unsplit_rows(s)[:t.numel()].view(t.shape)


def act_tol(kind, f32_tol, bf16_tol=1e-2):
    return {"f32": f32_tol, "bf16": bf16_tol, "x3": f32_tol + X3_STORE}[kind]


def within_sum_bound(got, want, n, abs_sum):
    """-> the worst |got - want| / bound, with bound = n 2^-24 sum |term| per output; an output whose terms are all zero must be exact."""
    err = (got.double().cpu() - want.double().cpu()).abs()
    bound = n * U * abs_sum.double().cpu()
    assert (err[bound == 0] == 0).all()
    return (err[bound > 0] / bound[bound > 0]).max().item() if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------ time conditioning
def tc_inputs(B, half, Cn):
    nfeat = 2 * half + 1
    g = torch.Generator().manual_seed(100 + B + half + Cn)
    times = torch.tensor(([999, 0, 1] + torch.randint(2, 999, (B,), generator=g).tolist())[:B])
    wf = seeded((half,), 11)
    W = seeded((Cn, nfeat), 12, 0.05)
    W[:, 0] *= 0.02  # the raw step index reaches 999: keep W f + bias of order 1, where silu' is not saturated
    bias = seeded((Cn,), 13, 0.1)
    ldd = Cn + 3
    dcond = torch.full((B, ldd), NAN)  # pad columns NaN: a read past C shows
    dcond[:, :Cn] = seeded((B, Cn), 14)
    pre = (seeded((half,), 15), seeded((Cn, nfeat), 16), seeded((Cn,), 17))  # dw_freq, dW, dbias before the call
    return times, wf, W, bias, dcond, pre


def tc_angle32(times, wf):
    return ((times.float()[:, None] * wf[None, :]) * 2.0) * torch.tensor(3.14159265358979323846, dtype=torch.float32)


def tc_f64(times, wf, W, bias, dcond):
    """float64 gradients (dw_freq, dW, dbias) by autograd, on the fp32 angle."""
    Cn = W.shape[0]
    wf64, W64, b64 = (t.double().requires_grad_(True) for t in (wf, W, bias))
    t64 = times.double()[:, None]
    lin = t64 * wf64[None, :] * (2 * torch.pi)
    ang = tc_angle32(times, wf).double() + (lin - lin.detach())  # the fp32 value; d ang / d w = 2 pi t
    feat = torch.cat((t64, ang.sin(), ang.cos()), dim=-1)
    (F.silu(F.linear(feat, W64, b64)) * dcond[:, :Cn].double()).sum().backward()
    return wf64.grad, W64.grad, b64.grad


def tc_f32(times, wf, W, bias, dcond, pre):
    """The kernels' three stages in torch fp32 -> the stored (dw_freq, dW, dbias) after one call onto `pre`."""
    Cn, half = W.shape[0], wf.numel()
    t32 = times.float()
    ang = tc_angle32(times, wf)
    sin, cos = ang.sin(), ang.cos()
    feat = torch.cat((t32[:, None], sin, cos), dim=-1)
    z = (feat[:, None, :] * W[None, :, :]).sum(-1) + bias
    sg = 1.0 / (1.0 + torch.exp(-z))
    ds = dcond[:, :Cn] * (sg * (1.0 + z * (1.0 - sg)))
    dW = pre[1] + (ds[:, :, None] * feat[:, None, :]).sum(0)
    dbias = pre[2] + ds.sum(0)
    df = (ds[:, :, None] * W[None, :, :]).sum(1)
    two_pi_t = torch.tensor(6.28318530717958647692, dtype=torch.float32) * t32
    dwf = pre[0] + ((df[:, 1:1 + half] * cos - df[:, 1 + half:] * sin) * two_pi_t[:, None]).sum(0)
    return dwf, dW, dbias


def tc_errors(stored, pre, want):
    """Error of the stored (dw_freq, dW, dbias) in the four parts the bound is set for, each over its largest increment."""
    parts = lambda t3: {"dW_t": t3[1][:, 0], "dW_sincos": t3[1][:, 1:], "dbias": t3[2], "dw_freq": t3[0]}
    s, p, w = parts(stored), parts(pre), parts(want)
    return {k: (s[k].double().cpu() - (p[k].double() + w[k])).abs().max().item() / max(w[k].abs().max().item(), 1e-30) for k in s}


# (B, half, C).  ds kernel: grid (ceil(C / 16), B), wave w of workgroup x owns outputs 16 x + 4 w + i; dw kernel: one thread per
# (c, k), ceil(C nfeat / 256) workgroups; freq kernel: one workgroup per frequency, 256 threads stride C.
TC_CASES = [
    (1, 1, 1),      # the smallest: C = 1 breaks at i = 1 of wave 0, waves 1-3 own nothing; nfeat = 3 < 64 lanes; 3 of 256 dw threads
    (3, 8, 16),     # one full ds workgroup; times 999, 0, 1 (t = 0: every sin 0, the t column 0)
    (5, 16, 250),   # C = 250: the last ds workgroup breaks at c = 250 in wave 2; the freq kernel's c stride ends ragged (250 < 256)
    (40, 64, 256),  # B = 40 in the dw / freq loops over samples; nfeat = 129: the ds dot product strides three times
    (2, 200, 20),   # nfeat = 401 > 256: the feature loop of the ds kernel strides; 200 freq workgroups
]


@pytest.mark.parametrize("B,half,Cn", TC_CASES)
def test_time_cond_backward(ops, B, half, Cn):
    ops_, _, _ = ops
    times, wf, W, bias, dcond, pre = tc_inputs(B, half, Cn)
    want = tc_f64(times, wf, W, bias, dcond)
    e32 = tc_errors(tc_f32(times, wf, W, bias, dcond, pre), pre, want)
    dev = lambda t: t.to(DEV).contiguous()
    t_d, wf_d, W_d, b_d, dc_d = dev(times.int()), dev(wf), dev(W), dev(bias), dev(dcond)
    run = lambda bufs: ops_.time_cond_backward(t_d, wf_d, W_d, b_d, dc_d, *bufs)
    inc = run([torch.zeros_like(p, device=DEV) for p in pre])  # onto zeros: the increment itself
    got = run([dev(p) for p in pre])
    first = [g.clone() for g in got]
    e = tc_errors(first, pre, want)
    for k in e:
        print(f"GRID time_cond B={B} half={half} C={Cn} {k}: fp32 restatement {e32[k]:.3e} bound {4 * e32[k]:.3e} measured {e[k]:.3e}")
    for k in e:
        assert e[k] <= 4 * e32[k], (k, e[k], 4 * e32[k])
    # accumulation: each output is one fp32 add of the increment onto what is there, and a second call adds the same increment again
    for f, p, i in zip(first, pre, inc):
        assert torch.equal(f, dev(p) + i)
    again = run(got)
    for a, f, i in zip(again, first, inc):
        assert torch.equal(a, f + i)


# ------------------------------------------------------------------------------------------------------------ column sums
# (groups, rows, C, ld).  chunks = ceil(rows / 64), halved while groups chunks C > 2^20; per = ceil(rows / chunks); a partial
# workgroup owns 256 columns (32 threads of 8: lo = first 4 in range, hi = second 4) x 8 row lanes; the final kernel's sixteen waves
# take the chunks j = w, w + 16, ... two at a time while j + 16 < chunks.
# (per = ceil(rows / chunks) with chunks <= ceil(rows / 64) gives (chunks - 1) per < rows for every shape the launcher can form: a
# chunk that starts at or past the group's end cannot be launched, the ragged last chunk is the edge that can.)
COLSUM_CASES = [
    (1, 1, 4, 4),           # rows < 8: seven row lanes without a row; C = 4: hi false with lo true; one chunk, one partial
    (3, 7, 12, 16),         # ld > C; thread 1 has lo without hi (c = 8, C = 12); row lane 7 empty
    (2, 65, 260, 264),      # chunks 2, per 33: the last chunk is ragged (rows 33..64); C > 256: blockIdx.x = 1 with four columns
    (6, 300, 200, 200),     # test_hip_train_ops.py's shape: chunks 5, per 60
    (1, 1025, 516, 516),    # chunks 17, per 61: last chunk 49 rows; final kernel: wave 0 takes two chunks (j = 0, 16), three blocks of columns
    (5, 129, 1028, 1032),   # chunks 3, per 43; five blocks of columns, the last with four; ld > C
]


def colsum_x3(lib_, src_dev, ld, groups, rows, Cn, out, scale, accumulate):
    L, lib = lib_
    scratch = torch.empty(max(int(lib.dn_colsum_scratch_bytes(groups, rows, Cn)) // 4, 1), device=DEV)
    L.check(lib.dn_colsum(src_dev.data_ptr(), ld, L.DN_BF16X3, groups, rows, Cn, out.data_ptr(), out.stride(0), C.c_float(scale),
                          int(accumulate), scratch.data_ptr(), _stream()), "dn_colsum x3")


@pytest.mark.parametrize("groups,rows,Cn,ld", COLSUM_CASES)
def test_colsum(ops, groups, rows, Cn, ld):
    ops_, _, _ = ops
    base = torch.full((groups * rows, ld), NAN)  # pad columns [C, ld) NaN: a column read past C shows
    base[:, :Cn] = seeded((groups * rows, Cn), 21)
    pre = seeded((groups, Cn), 22)
    for kind in ("f32", "bf16", "x3"):
        if kind == "x3":
            src_dev, vals = x3_src(base)
        else:
            vals = bf16r(base) if kind == "bf16" else base
            src_dev = vals.to(DEV, torch.bfloat16 if kind == "bf16" else torch.float32)
        v = vals[:, :Cn].double().view(groups, rows, Cn)
        want, abs_sum = v.sum(1), v.abs().sum(1)
        for scale, accumulate in ((1.0, False), (-0.5, True)):
            full = torch.full((groups, Cn + 4), 7.0, device=DEV)  # out_ld > C: the columns past C stay
            out = full[:, :Cn]
            if accumulate:
                out.copy_(pre)
            if kind == "x3":
                colsum_x3(_lib(), src_dev, ld, groups, rows, Cn, out, scale, accumulate)
            else:
                ops_.colsum(src_dev, groups, rows, Cn, out=out, scale=scale, accumulate=accumulate)
            w = scale * want + (pre.double() if accumulate else 0.0)
            if rows >= 1024:
                r = within_sum_bound(out, w, rows, abs(scale) * abs_sum + (pre.double().abs() if accumulate else 0.0))
                print(f"GRID colsum {kind} {(groups, rows, Cn, ld)} scale={scale}: summation bound, worst error / bound {r:.3e}")
                assert r <= 1.0
            else:
                e = relerr(out, w)
                print(f"GRID colsum {kind} {(groups, rows, Cn, ld)} scale={scale}: bound 1.0e-05 measured {e:.3e}")
                assert e < 1e-5
            assert (full[:, Cn:] == 7.0).all()


def test_colsum_capped_chunks(ops):
    """groups ceil(rows / 64) C = 64 * 16 * 1028 > 2^20: the launcher halves the chunks to 8 (64 * 8 * 1028 <= 2^20), 128 rows each,
    sixteen per row lane.  67 M bf16 values: made and summed (float64) on the device."""
    ops_, _, _ = ops
    L, lib = _lib()
    groups, rows, Cn = 64, 1024, 1028
    assert int(lib.dn_colsum_scratch_bytes(groups, rows, Cn)) == groups * 8 * Cn * 4
    g = torch.Generator(device=DEV).manual_seed(23)
    src = torch.randn(groups * rows, Cn, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)
    out = torch.full((groups, Cn), NAN, device=DEV)
    ops_.colsum(src, groups, rows, Cn, out=out)
    v = src.view(groups, rows, Cn)
    want = v.sum(1, dtype=torch.float64)
    abs_sum = v.abs().sum(1, dtype=torch.float64)
    r = within_sum_bound(out, want, rows, abs_sum)
    print(f"GRID colsum bf16 capped {(groups, rows, Cn)}: summation bound, worst error / bound {r:.3e}")
    assert r <= 1.0


# colsum_final_kernel with per_group = B bps partial rows, through the learned-gamma reduction of the norm backward (rpb = 8 here:
# B ceil(T / 8) < 512 at every larger rpb too).  Wave w takes partial rows j = w, w + 16, ...: two per turn while j + 16 < per_group,
# then one if j < per_group.
#   1: only wave 0, its tail.  16: every wave its tail, no pair.  17: wave 0 one pair (0, 16), no tail.
#   32: every wave one pair, no tail.  33: wave 0 a pair and the tail (j = 32).
@pytest.mark.parametrize("B,T,per_group", [(1, 8, 1), (1, 128, 16), (1, 130, 17), (2, 128, 32), (3, 88, 33)])
def test_colsum_final_through_learned_gamma(ops, B, T, per_group):
    ops_, packing, _ = ops
    assert B * ((T + 7) // 8) == per_group
    D = 64
    x = seeded((B, T, D), 31).double().requires_grad_(True)
    dy = seeded((B, T, D), 32)
    gamma = (1 + 0.3 * seeded((D,), 33)).double().requires_grad_(True)
    (F.normalize(x, dim=-1) * D ** 0.5 * gamma).backward(dy.double())
    dgamma = torch.full((D,), 0.5, device=DEV)
    ops_.rmsnorm_backward(x.detach().float().view(B * T, D).to(DEV), dy.view(B * T, D).to(DEV), B, T, D,
                          gamma=gamma.detach().float().to(DEV), dgamma=dgamma)
    e = relerr(dgamma - 0.5, gamma.grad)
    print(f"GRID colsum_final per_group={per_group}: bound 1.0e-04 measured {e:.3e}")
    assert e < 1e-4


# ------------------------------------------------------------------------------------------------------------ RMSNorm backward
# (B, T, D).  norm_rows_per_block: rpb = 64, halved while rpb > 8 and B ceil(T / rpb) < 512.  A workgroup's four waves take the rows
# t0 + w, t0 + w + 4, ... of its block; lane l holds columns 4 (64 i + l) .. + 3 in register slot i = 0..3.
#   (1, 1, 4)      1, 1, 1, 1 workgroups < 512 -> rpb 8.  One row: waves 1-3 have none and still store their (zero) partial sums;
#                  D = 4: one lane of slot 0.
#   (2, 9, 260)    -> rpb 8, two blocks per sample, the last one row.  D = 260: slot 1 holds one float4 (lane 0).
#   (3, 37, 1024)  -> rpb 8, last block 5 rows.  D = 1024: every slot full, red[wave][1024 + c] written to its end.
#   (8, 1030, 64)  64: 8 * 17 = 136, 32: 8 * 33 = 264, 16: 8 * 65 = 520 >= 512 -> rpb 16; last block 1030 - 64 * 16 = 6 rows.
#   (8, 2051, 64)  64: 8 * 33 = 264, 32: 8 * 65 = 520 -> rpb 32; last block 2051 - 64 * 32 = 3 rows: wave 3 has none.
#   (8, 4097, 64)  64: 8 * 65 = 520 -> rpb 64; last block one row: waves 1-3 have none.
NORM_CASES = [(1, 1, 4), (2, 9, 260), (3, 37, 1024), (8, 1030, 64), (8, 2051, 64), (8, 4097, 64)]


def rmsnorm_backward_x3(x, dy, B, T, D, gamma, gb, gb_half, dres, dgamma, dgb):
    """ops.rmsnorm_backward with a split dx_act (the wrapper takes the copy's dtype from a torch dtype)."""
    L, lib = _lib()
    M, ldx = x.shape
    dx = torch.full_like(x, NAN)
    dx_act = x3_buf(M, ldx)
    scratch = torch.empty(max(int(lib.dn_rmsnorm_backward_scratch_bytes(B, T, D)) // 4, 1), device=DEV)
    L.check(lib.dn_rmsnorm_backward(x.data_ptr(), ldx, dy.data_ptr(), dy.shape[1], L.DN_F32, B, T, D, L.ptr(gamma), L.ptr(gb),
                                    gb.stride(0) if gb is not None else 0, gb_half, L.ptr(dres), dx.data_ptr(), dx_act.data_ptr(),
                                    L.DN_BF16X3, ldx, L.ptr(dgamma), L.ptr(dgb), dgb.stride(0) if dgb is not None else 0,
                                    scratch.data_ptr(), _stream()), "dn_rmsnorm_backward x3")
    return dx, x3_read(dx_act, M, ldx)


@pytest.mark.parametrize("mode", ["learned", "adaptive", "plain"])
@pytest.mark.parametrize("B,T,D", NORM_CASES)
def test_rmsnorm_backward(ops, mode, B, T, D):
    ops_, packing, _ = ops
    Dp = packing.padk(D)
    ldx = Dp + 64  # ldx > Dp: dx and dx_act zero their pad columns up to ldx
    M = B * T
    long_sum = T >= 1030  # more rows than test_hip_train_ops.py reduces: the summation bound
    xf = seeded((B, T, D), 1)
    groups = {"rows": torch.ones(M, dtype=torch.bool)}
    if M > 1:  # |x| = 0: r = 1 / 1e-12 on both sides, dx = 1e12 sqrt(D) G dy there -- judged apart, it would hide every other row
        zero_row = (B - 1) * T + T // 2
        xf.view(M, D)[zero_row] = 0
        groups["zero row"] = torch.zeros(M, dtype=torch.bool)
        groups["zero row"][zero_row] = True
    if long_sum:  # the last row of every sample, with 1024 times the gradient (module docstring): judged apart for the same reason
        groups["edge rows"] = torch.zeros(B, T, dtype=torch.bool)
        groups["edge rows"][:, -1] = True
        groups["edge rows"] = groups["edge rows"].view(M)
    for k in list(groups)[1:]:
        groups["rows"] &= ~groups[k]
    dres = seeded((B, T, D), 3)
    pad = lambda t, ld: torch.cat([t.reshape(M, D), torch.zeros(M, ld - D)], dim=1)
    gamma = (1 + 0.3 * seeded((D,), 4)) if mode == "learned" else None
    gb = seeded((B, 2 * Dp), 5) if mode == "adaptive" else None
    xa, dra = pad(xf, ldx).to(DEV), pad(dres, ldx).to(DEV)
    gd = gamma.to(DEV) if gamma is not None else None
    gbd = gb.to(DEV) if gb is not None else None
    pre_g = seeded((D,), 6) if mode == "learned" else None  # parameter gradients accumulate onto what is there
    pre_gb = seeded((B, 2 * Dp), 7) if mode == "adaptive" else None
    for kind in ("f32", "bf16", "x3"):
        dy = seeded((B, T, D), 2)
        if long_sum:
            dy[:, -1] *= 1024.0
        dy = bf16r(dy) if kind == "bf16" else dy
        x = xf.double().requires_grad_(True)
        g64 = gamma.double().requires_grad_(True) if gamma is not None else None
        gb64 = gb.double().requires_grad_(True) if gb is not None else None
        xn = F.normalize(x, dim=-1) * D ** 0.5  # x / max(|x|, 1e-12) sqrt(D)
        y = xn
        if g64 is not None:
            y = y * g64
        if gb64 is not None:
            y = y * gb64[:, None, :D] + gb64[:, None, Dp:Dp + D]
        y.backward(dy.double())
        want_dx = x.grad.view(M, D) + dres.view(M, D).double()
        dgamma = pre_g.to(DEV) if pre_g is not None else None
        dgb = pre_gb.to(DEV) if pre_gb is not None else None
        dya = pad(dy, Dp).to(DEV, torch.bfloat16 if kind == "bf16" else torch.float32)
        if kind == "x3":
            dx, dx_act = rmsnorm_backward_x3(xa, dya, B, T, D, gd, gbd, Dp, dra, dgamma, dgb)
        else:
            dx, dx_act = ops_.rmsnorm_backward(xa, dya, B, T, D, gamma=gd, gamma_beta=gbd, gb_half=Dp, dres=dra,
                                               act_dtype=torch.bfloat16 if kind == "bf16" else torch.float32, dgamma=dgamma, dgamma_beta=dgb)
            dx_act = dx_act.double().cpu()
        dx = dx.cpu()
        tol = act_tol(kind, 2e-5)
        figures = []
        for name, rows in groups.items():
            if rows.any():
                e, ea = relerr(dx[rows][:, :D], want_dx[rows]), relerr(dx_act[rows][:, :D], want_dx[rows])
                figures.append(f"{name} dx {e:.3e} dx_act {ea:.3e}")
                assert e < 2e-5 and ea < tol, (name, e, ea)
        assert (dx[:, D:] == 0).all() and (dx_act[:, D:] == 0).all()
        # parameter gradients: one term per row, dy x r s (gamma, g_c) or dy (b_c), added onto what the buffer held
        t_g = (dy.double() * xn.detach()).abs()
        if mode == "learned":
            checks = [("dgamma", dgamma.cpu(), pre_g, g64.grad, M, t_g.sum((0, 1)))]
        elif mode == "adaptive":
            got = dgb.cpu()
            assert torch.equal(got[:, D:Dp], pre_gb[:, D:Dp]) and torch.equal(got[:, Dp + D:], pre_gb[:, Dp + D:])
            checks = [("dg_c", got[:, :D], pre_gb[:, :D], gb64.grad[:, :D], T, t_g.sum(1)),
                      ("db_c", got[:, Dp:Dp + D], pre_gb[:, Dp:Dp + D], gb64.grad[:, Dp:Dp + D], T, dy.double().abs().sum(1))]
        else:
            checks = []
        for name, got, pre, want, n, abs_sum in checks:
            if long_sum:
                r = within_sum_bound(got, pre.double() + want, n, abs_sum + pre.double().abs())
                figures.append(f"{name} summation bound, worst error / bound {r:.3e}")
                assert r <= 1.0, (name, r)
            else:
                e = relerr(got - pre, want)
                figures.append(f"{name} bound 1.0e-04 measured {e:.3e}")
                assert e < 1e-4, (name, e)
        print(f"GRID rmsnorm_bwd {mode} {kind} {(B, T, D)}: dx bound 2.0e-05 dx_act bound {tol:.3e} | " + " | ".join(figures))


# ------------------------------------------------------------------------------------------------------------ label-smoothed CE
# One wave per row, lane l holds columns 64 i + l (i < 16); a workgroup takes 4 rows.
#   V = 2: two lanes of register 0, eps_i = eps / 1.  64 / 65: register 0 full / one lane of register 1.  1004: the recipe's.
#   1024: every register full (the refused size is V > 1024).
#   M = 1, 5, 37: M % 4 = 1, the last workgroup has one row and three waves that leave; M = 4: M % 4 = 0, a full last workgroup.
#   ldd = V rounded up to 8 / 1024: the columns [V, ldd) of dlogits are written zero.
LSCE_V = [2, 64, 65, 1004, 1024]
LSCE_M = [1, 4, 5, 37]


def lsce_inputs(V):
    """37 rows; the first seven are the edges (so that M = 1, 4, 5 hold some too):
      0, 1  the maximum twice, at columns (c, c + 1) -- neighbouring lanes -- with the target at the second / the first of them
      2, 3  the maximum twice, at (c, c + 64) -- one lane, two registers -- target at the second / the first (V <= 64: (c, c + 1) again)
      4, 5  logits around +80 / -80: only the subtraction of the row maximum keeps the exponentials in range
      6     a pad (target 0), as are rows 11 and 20.
    argmax takes the lowest index of a tied maximum: `correct` is 1 only for a target at the first.  Target 0 is the pad, so where the
    first of the pair is column 0 (V = 2, 65) both rows take the second."""
    logits = seeded((37, V), 41, 2.0)
    tgt = torch.randint(min(4, V - 1), V, (37,), generator=torch.Generator().manual_seed(42))
    a = min(5, V - 2)
    b = min(5, V - 65) if V > 64 else a
    gap = 64 if V > 64 else 1
    for row, (c, d, second) in enumerate(((a, 1, True), (a, 1, False), (b, gap, True), (b, gap, False))):
        logits[row, c] = logits[row, c + d] = logits[row].max() + 1.0
        tgt[row] = c + d if (second or c == 0) else c
        assert int(logits[row].argmax()) == c and logits[row, c] == logits[row, c + d]
    logits[4] += 80.0
    logits[5] -= 80.0
    tgt[6] = tgt[11] = tgt[20] = 0
    return logits, tgt


def lsce_call(ops_, logits_d, tgt_d, eps, gscale, kind, ldd):
    """-> (rows, dlogits as float64 [M, ldd] or None)"""
    M, V = logits_d.shape
    if kind is None:
        rows, dl = ops_.lsce_loss_grad(logits_d, tgt_d, eps, gscale)
        assert dl is None
        return rows, None
    if kind == "x3":
        L, lib = _lib()
        rows = torch.full((M, 4), NAN, device=DEV)
        dl = x3_buf(M, ldd)
        L.check(lib.dn_lsce_loss_grad(logits_d.data_ptr(), logits_d.stride(0), tgt_d.data_ptr(), M, V, C.c_float(eps), C.c_float(gscale),
                                      rows.data_ptr(), dl.data_ptr(), L.DN_BF16X3, ldd, _stream()), "dn_lsce_loss_grad x3")
        return rows, x3_read(dl, M, ldd)
    rows, dl = ops_.lsce_loss_grad(logits_d, tgt_d, eps, gscale, act_dtype=torch.bfloat16 if kind == "bf16" else torch.float32, ldd=ldd)
    return rows, dl.double().cpu()


@pytest.mark.parametrize("V", LSCE_V)
def test_lsce(ops, V):
    ops_, _, _ = ops
    eps, gscale = 0.1, 0.1 / 30
    logits_all, tgt_all = lsce_inputs(V)
    for M in LSCE_M:
        logits, tgt = logits_all[:M], tgt_all[:M]
        lg = logits.double().requires_grad_(True)
        lprobs = F.log_softmax(lg, dim=-1)
        loss, nll = O.label_smoothed_nll_loss(lprobs, tgt, eps, 0)
        (loss * gscale).backward()
        keep = tgt.ne(0)
        want_correct = ((lg.detach().argmax(1) == tgt) & keep).float()
        eps_i = eps / (V - 1)
        logits_d, tgt_d = logits.to(DEV), tgt.to(DEV, torch.int32)
        for ldd in sorted({(V + 7) // 8 * 8, 1024}):
            for kind in ("f32", "bf16", "x3", None):
                rows, dl = lsce_call(ops_, logits_d, tgt_d, eps, gscale, kind, ldd)
                rows = rows.cpu()
                assert torch.equal(rows[:, 3], keep.float()) and torch.equal(rows[:, 2], want_correct), (M, ldd, kind)
                assert (rows[~keep] == 0).all()
                r = rows.double()
                if keep.any():
                    assert abs(r[:, 0].sum().item() - nll.item()) < 1e-4 * abs(nll.item())
                    assert abs(((1 - eps - eps_i) * r[:, 0].sum() + eps_i * r[:, 1].sum()).item() - loss.item()) < 1e-4 * abs(loss.item())
                if kind is None:
                    continue
                tol = act_tol(kind, 1e-5)
                e = relerr(dl[:, :V], lg.grad) if keep.any() else dl[:, :V].abs().max().item()
                print(f"GRID lsce {kind} V={V} M={M} ldd={ldd}: bound {tol:.3e} measured {e:.3e}")
                assert e < tol if keep.any() else e == 0
                assert (dl[:, V:] == 0).all() and (dl[~keep] == 0).all()
    # an all-pad batch: nothing to average, rows and gradient zero
    tgt0 = torch.zeros(5, dtype=torch.int32, device=DEV)
    for kind in ("f32", "bf16", "x3"):
        rows, dl = lsce_call(ops_, logits_all[:5].to(DEV), tgt0, eps, gscale, kind, (V + 7) // 8 * 8)
        assert (rows == 0).all() and (dl == 0).all()


# ------------------------------------------------------------------------------------------------------------ masked MSE
# One wave per frame, lane l takes columns 4 l, 4 l + 256, ... below max(C, ldd, ld_act).
#   (3, 11, 48, 64, 64)    test_hip_train_ops.py's: one turn of the column loop, 12 lanes with data, 4 more that write pads
#   (2, 5, 516, 520, 576)  C > 512: three turns, the third with one lane of data; ld_act > ldd: the copy's pads reach past dpred's row
#   (4, 7, 4, 4, 32)       C = 4: one lane; ldd = C: dpred has no pad; the copy has 28 pad columns
MSE_CASES = [(3, 11, 48, 64, 64, [11, 0, 4]), (2, 5, 516, 520, 576, [5, 0]), (4, 7, 4, 4, 32, [7, 0, 3, 7])]


def mse_call(ops_, pred_d, tgt_d, T, lens_d, gscale, Cn, dpred, accumulate, kind, ld_act):
    """-> (sq rows, the operand copy as float64 [M, ld_act] or None)"""
    if kind != "x3":
        sq, dact = ops_.masked_mse_grad(pred_d, tgt_d, T, lens_d, gscale, Cn, dpred=dpred, accumulate=accumulate,
                                        act_dtype={"f32": torch.float32, "bf16": torch.bfloat16, None: None}[kind], ld_act=ld_act)
        return sq, dact.double().cpu() if dact is not None else None
    L, lib = _lib()
    M = pred_d.shape[0]
    sq = torch.full((M,), NAN, device=DEV)
    dact = x3_buf(M, ld_act)
    L.check(lib.dn_masked_mse_grad(pred_d.data_ptr(), pred_d.stride(0), tgt_d.data_ptr(), tgt_d.stride(0), M, Cn, T, L.ptr(lens_d),
                                   C.c_float(gscale), sq.data_ptr(), L.ptr(dpred), dpred.stride(0) if dpred is not None else 0, int(accumulate),
                                   dact.data_ptr(), L.DN_BF16X3, ld_act, _stream()), "dn_masked_mse_grad x3")
    return sq, x3_read(dact, M, ld_act)


@pytest.mark.parametrize("with_lengths", [True, False])
@pytest.mark.parametrize("B,T,Cn,ldd,ld_act,lens", MSE_CASES)
def test_masked_mse(ops, B, T, Cn, ldd, ld_act, lens, with_lengths):
    ops_, _, _ = ops
    M = B * T
    pred = torch.full((M, ldd), NAN)  # pad columns NaN: they are never read
    pred[:, :Cn] = seeded((M, Cn), 51)
    tgt = seeded((M, Cn), 52)
    lens_t = torch.tensor(lens) if with_lengths else torch.full((B,), T)  # lengths 0 and T; None: every frame counts
    valid = O.lengths_to_mask(lens_t, T).view(-1)
    p = pred[:, :Cn].double().requires_grad_(True)
    sel = valid.unsqueeze(1).expand(-1, Cn)
    mse = F.mse_loss(p[sel], tgt.double()[sel])
    (10 * mse).backward()
    n_valid = int(lens_t.sum())
    gscale = 10 * 2.0 / (n_valid * Cn)
    base = seeded((M, ldd), 53)
    pred_d, tgt_d = pred.to(DEV), tgt.to(DEV)
    lens_d = lens_t.to(DEV, torch.int32) if with_lengths else None
    for kind in ("f32", "bf16", "x3", None):
        tol = act_tol(kind, 1e-5) if kind else None
        for accumulate in (False, True):
            # accumulate = False: onto NaN -- every element of [0, ldd) has to be written; True: onto `base`, whose pads are replaced by 0
            dpred = torch.full((M, ldd), NAN, device=DEV) if not accumulate else base.to(DEV)
            sq, dact = mse_call(ops_, pred_d, tgt_d, T, lens_d, gscale, Cn, dpred, accumulate, kind, ld_act)
            want = p.grad + (base[:, :Cn].double() if accumulate else 0.0)
            assert abs(sq.double().sum().item() / (n_valid * Cn) - mse.item()) < 1e-5 * mse.item()
            assert (sq.cpu()[~valid] == 0).all()
            e = relerr(dpred[:, :Cn], want)
            assert e < 1e-5, (kind, accumulate, e)
            assert (dpred[:, Cn:] == 0).all()
            if not accumulate:
                assert (dpred.cpu()[~valid] == 0).all()
            ea = None
            if dact is not None:
                ea = relerr(dact[:, :Cn], want)
                assert ea < tol, (kind, accumulate, ea)
                assert (dact[:, Cn:] == 0).all()
            print(f"GRID masked_mse {kind} {(B, T, Cn, ldd, ld_act)} lengths={with_lengths} accumulate={accumulate}: dpred bound 1.0e-05 "
                  f"measured {e:.3e} | copy bound {tol} measured {ea}")
        if kind:  # only the operand copy
            sq, dact = mse_call(ops_, pred_d, tgt_d, T, lens_d, gscale, Cn, None, False, kind, ld_act)
            ea = relerr(dact[:, :Cn], p.grad)
            assert ea < tol, (kind, ea)
            assert (dact[:, Cn:] == 0).all() and (dact[~valid] == 0).all()


# ------------------------------------------------------------------------------------------------------------ posterior backward
def posterior_call(ops_, params_d, noise_d, dz_d, Z, T, lens_d, klw, kind, ldo):
    if kind != "x3":
        return ops_.posterior_backward(params_d, noise_d, dz_d, Z, T, lens_d, klw, torch.bfloat16 if kind == "bf16" else torch.float32,
                                       ldo).double().cpu()
    L, lib = _lib()
    M = params_d.shape[0]
    out = x3_buf(M, ldo)
    L.check(lib.dn_posterior_backward(params_d.data_ptr(), params_d.shape[1], noise_d.data_ptr(), noise_d.shape[1], dz_d.data_ptr(),
                                      dz_d.shape[1], out.data_ptr(), L.DN_BF16X3, ldo, M, Z, T, L.ptr(lens_d), C.c_float(klw), _stream()),
            "dn_posterior_backward x3")
    return x3_read(out, M, ldo)


@pytest.mark.parametrize("with_lengths", [True, False])
def test_posterior_backward(ops, with_lengths):
    """The clamp is closed: logvar exactly -30 and 20 pass their gradient (torch.clamp's own rule), the next fp32 value outside each
    and the largest finite values do not.  The clamp's ends are judged element by element (exp(10) at 20 would hide every other
    element under a tensor-wide maximum), the rest as test_hip_train_ops.py does."""
    ops_, _, _ = ops
    B, T, Z, ldo = 3, 20, 8, 64  # ldo > 2 Z: 48 pad columns, written zero
    M = B * T
    params = seeded((B, T, 2 * Z), 1, 2.0)
    lo, hi = torch.tensor(-30.0), torch.tensor(20.0)
    edges = {(0, 0, Z): 20.0, (0, 1, Z + 1): -30.0, (0, 2, Z + 2): torch.nextafter(hi, torch.tensor(100.0)).item(),
             (0, 3, Z + 3): torch.nextafter(lo, torch.tensor(-100.0)).item(), (1, 0, Z + 4): 3.0e38, (1, 1, Z + 5): -3.0e38,
             (2, 19, 2 * Z - 1): 20.0, (2, 18, Z): -30.0}  # the last two on frames past lens[2] = 13: no KL part there
    for k, v in edges.items():
        params[k] = v
    noise, dz = seeded((B, T, Z), 2), seeded((B, T, Z), 3)
    lens = torch.tensor([20, 7, 13]) if with_lengths else torch.full((B,), T)
    p = params.double().requires_grad_(True)
    z = O.posterior_sample(p, noise.double())
    kl = O.posterior_kl(p, O.lengths_to_mask(lens, T)).mean()
    ((z * dz.double()).sum() + 1e-2 * kl).backward()
    want = p.grad.view(M, 2 * Z)
    edge = torch.zeros(B, T, 2 * Z, dtype=torch.bool)
    for k in edges:
        edge[k] = True
    edge = edge.view(M, 2 * Z)
    assert (want[edge] == 0).sum() == 4 and (want[edge] != 0).sum() == 4  # outside: no gradient; at the ends: one
    dev = lambda t, w: t.reshape(M, w).to(DEV)
    for kind in ("f32", "bf16", "x3"):
        got = posterior_call(ops_, dev(params, 2 * Z), dev(noise, Z), dev(dz, Z), Z, T, lens.to(DEV, torch.int32) if with_lengths else None,
                             1e-2 / (B * Z * T), kind, ldo)
        tol = act_tol(kind, 1e-5)
        e = relerr(got[:, :2 * Z][~edge], want[~edge])
        ee = ((got[:, :2 * Z][edge] - want[edge]).abs() / want[edge].abs().clamp_min(1e-30)).max().item()
        print(f"GRID posterior_bwd {kind} lengths={with_lengths}: bound {tol:.3e} measured {e:.3e}, clamp ends (each by its own size) {ee:.3e}")
        assert e < tol and ee < tol
        assert (got[:, :2 * Z][edge][want[edge] == 0] == 0).all()
        assert (got[:, 2 * Z:] == 0).all()


# ------------------------------------------------------------------------------------------------------------ small helpers
# dn_vec_sum: 256 workgroups of 256 threads stride the vector by 65536.  n = 1, 255: one element / one short workgroup, 255
# partial sums of nothing; 256 / 257: workgroup 0 full, workgroup 1 with one element; 65537: the stride loop takes a second turn for
# exactly one thread (element 65536 -- it carries 1e4 times the size of the others, so that losing it is more than the bound).
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_vec_sum(ops, n):
    L, lib = _lib()
    v = seeded((n,), 61)
    v[-1] *= 1e4 if n > 65536 else 1.0
    v_d = v.to(DEV)
    scratch = torch.full((256,), NAN, device=DEV)
    for accumulate, pre in ((0, NAN), (1, 3.25)):
        out = torch.full((1,), pre, device=DEV)
        L.check(lib.dn_vec_sum(v_d.data_ptr(), n, out.data_ptr(), accumulate, scratch.data_ptr(), _stream()), "dn_vec_sum")
        want = v.double().sum() + (pre if accumulate else 0.0)
        r = within_sum_bound(out[0], want, n, v.double().abs().sum() + (abs(pre) if accumulate else 0.0))
        print(f"GRID vec_sum n={n} accumulate={accumulate}: summation bound, error / bound {r:.3e}")
        assert r <= 1.0


@pytest.mark.parametrize("kind", ["f32", "bf16", "x3"])
@pytest.mark.parametrize("count", [1, 5])  # count = 1: the k loop does not run, dst = src
def test_sum_groups(ops, count, kind):
    ops_, _, _ = ops
    R, Cc = 9, 36  # n / 4 = 81 float4s: one short workgroup
    grp = seeded((count, R, Cc), 62)
    if kind == "x3":
        L, lib = _lib()
        src_d, vals = x3_src(grp.view(count * R, Cc))
        out = x3_buf(R, Cc)
        stride = R * Cc  # group k starts at flat element k * stride, a multiple of 4
        L.check(lib.dn_sum_groups(src_d.data_ptr(), stride, count, out.data_ptr(), L.DN_BF16X3, stride, _stream()), "dn_sum_groups x3")
        got, want = x3_read(out, R, Cc), vals.view(count, R, Cc).double().sum(0)
    else:
        vals = bf16r(grp) if kind == "bf16" else grp
        got = ops_.sum_groups(vals.to(DEV, torch.bfloat16 if kind == "bf16" else torch.float32)).double().cpu()
        want = vals.double().sum(0)
    tol = act_tol(kind, 1e-6)
    e = relerr(got, want)
    print(f"GRID sum_groups {kind} count={count}: bound {tol:.3e} measured {e:.3e}")
    assert e < tol


def test_add_broadcast(ops):
    """dst[j ld + c] += src[c] for j < count with ld > C, C = 300 (a second workgroup of 44 threads): one fp32 add per element, bit
    for bit; the columns [C, ld) are not touched."""
    L, lib = _lib()
    Cn, ld, count = 300, 304, 3
    src, dst = seeded((Cn,), 63), seeded((count + 1, ld), 64)
    dst_d = dst.to(DEV)
    L.check(lib.dn_add_broadcast(src.to(DEV).data_ptr(), dst_d.data_ptr(), Cn, ld, count, _stream()), "dn_add_broadcast")
    want = dst.clone()
    want[:count, :Cn] += src
    assert torch.equal(dst_d.cpu(), want)


def test_transpose_weights_x3_non_square(ops):
    """Split weights ([lo | hi]) at R = 96 of Rp = 128 rows and Cc = Cp = 64: the tile's rows 96..127 come from no source row, and the
    result is the split of the transposed fp32 matrix, zero in the pad."""
    from diffnorm_amd import packing

    L, lib = _lib()
    count, R, Cc, Rp, Cp = 2, 96, 64, 128, 64
    w = seeded((count, R, Cc), 65)
    ws = packing.split_rows(w, weight=True).to(DEV)
    dst = torch.full((count, Cp, 2 * Rp), NAN, dtype=torch.bfloat16, device=DEV)
    L.check(lib.dn_transpose_weights(ws.data_ptr(), L.DN_BF16X3, count, R * Cc, R, Cc, dst.data_ptr(), Rp * Cp, Rp, Cp, _stream()),
            "dn_transpose_weights x3")
    want = torch.zeros(count, Cp, Rp)
    want[:, :Cc, :R] = packing.unsplit_rows(ws.cpu()).transpose(1, 2)
    assert torch.equal(dst.cpu().view(torch.int16), packing.split_rows(want, weight=True).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------ refused arguments
def test_refused_arguments_raise_before_any_launch(ops):
    """Sizes the kernels cannot take are refused by the launcher's argument check on the host: DiffNormHipError, and the output
    buffers keep what they held.  (Not parity coverage.)"""
    from diffnorm_amd import packing
    from diffnorm_amd._lib import DiffNormHipError

    ops_, _, _ = ops
    L, lib = _lib()
    keep = lambda *shape, dtype=torch.float32: torch.full(shape, 5.0, dtype=dtype, device=DEV)
    z = lambda *shape: torch.zeros(*shape, device=DEV)
    # RMSNorm backward: D > 1024 (a row no longer fits the four register slots)
    dgamma = keep(1028)
    with pytest.raises(DiffNormHipError):
        ops_.rmsnorm_backward(z(4, 1088), z(4, 1088), 2, 2, 1028, gamma=z(1028), dgamma=dgamma)
    assert (dgamma == 5.0).all()
    # LS-CE: V > 1024
    with pytest.raises(DiffNormHipError):
        ops_.lsce_loss_grad(z(4, 1025), torch.ones(4, dtype=torch.int32, device=DEV), 0.1, 1.0)
    # column sums and masked MSE: C % 4 != 0
    out = keep(2, 6)
    with pytest.raises(DiffNormHipError):
        ops_.colsum(z(6, 8), 2, 3, 6, out=out)
    assert (out == 5.0).all()
    dpred = keep(4, 8)
    with pytest.raises(DiffNormHipError):
        ops_.masked_mse_grad(z(4, 8), z(4, 8), 2, None, 1.0, 6, dpred=dpred)
    assert (dpred == 5.0).all()
    # split weights: Cc and Rp in whole 32-element groups
    ws = packing.split_rows(torch.zeros(1, 32, 64), weight=True).to(DEV)
    for R, Cc, Rp, Cp in ((32, 48, 32, 48), (32, 64, 48, 64)):
        dst = keep(1, Cp, 2 * Rp, dtype=torch.bfloat16)
        with pytest.raises(DiffNormHipError):
            L.check(lib.dn_transpose_weights(ws.data_ptr(), L.DN_BF16X3, 1, R * Cc, R, Cc, dst.data_ptr(), Rp * Cp, Rp, Cp, _stream()), "x3 transpose")
        assert (dst == 5.0).all()
    # dn_split_rows: n in whole groups, a 16-byte aligned source, a 128-byte aligned destination
    src, dst = z(128), keep(256, dtype=torch.bfloat16)
    for s, n, d in ((src, 48, dst), (src[1:], 64, dst), (src, 64, dst[8:])):
        with pytest.raises(DiffNormHipError):
            L.check(lib.dn_split_rows(s.data_ptr(), n, d.data_ptr(), 1, _stream()), "dn_split_rows")
    assert (dst == 5.0).all()
