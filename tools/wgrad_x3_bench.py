#!/usr/bin/env python3
"""The split-operand (bf16x3) weight gradient alone at training sizes, HIP-event times: the transposed-copies form the engine runs
with option wgrad_tn_x3 = 0 (dn_transpose_slices over dY and once per tap over X, dn_conv_gemm on the copies, dn_wgrad_reduce; sliced
as train_engine.hip: plan_wgrad slices it) against the row-major kernel (ops.conv_weight_grad_tn(dtype="bf16x3"), sliced as
weight_grad() slices it), with option wgrad_stages = 3 (default) and 2."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffnorm_amd import _lib, ops, packing

dev = torch.device("cuda:0")
pk = lambda c: (c + 63) // 64 * 64
pn = lambda c: (c + 127) // 128 * 128


def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def copies_form(xs, dys, B, T, cin, cout, shifts):
    """-> (callable, k_slices): plan_wgrad's slicing (target 128 tile-slices, unsliced from 160 tiles, >= 256 columns a slice)"""
    lib = _lib.load()
    n_taps, rows_w = len(shifts), pn(cin)
    N = n_taps * rows_w
    Tp = (T + max(shifts) + 63) // 64 * 64
    tiles = ((cout + 255) // 256) * ((N + 255) // 256)
    ks = 1
    while ks < 64 and tiles * ks < (160 if ks == 1 else 128) and B * Tp // (ks * 2) >= 256:
        ks *= 2
    cols_total = (B * Tp + 64 * ks - 1) // (64 * ks) * (64 * ks)
    chunk = cols_total // ks
    dyT = torch.empty((ks, cout, 2 * chunk), device=dev, dtype=torch.bfloat16)
    xT = torch.empty((ks, N, 2 * chunk), device=dev, dtype=torch.bfloat16)
    Np, Kp = pn(cout), pk(cin)
    grad = torch.zeros((n_taps, Np, Kp), device=dev)
    part = torch.empty((ks, cout, N), device=dev)
    st = _lib.current_stream()

    def tr(src, C_, front, dst, rows, rows_total, row0, order):
        _lib.check(lib.dn_transpose_slices(src.data_ptr(), _lib.DN_BF16X3, src.shape[1] // 2, B, T, C_, front, Tp, cols_total, chunk, dst.data_ptr(), rows,
                                           rows_total, row0, order, st), "dn_transpose_slices")

    def run():
        tr(dys, cout, 0, dyT, cout, cout, 0, 0)
        for j, s in enumerate(shifts):
            tr(xs, cin, s, xT, rows_w, N, j * rows_w, 1)
        if ks == 1:  # one group per tap, accumulating into the packed gradient
            ops.conv_gemm([(dyT[0], xT[0].view(n_taps, rows_w, 2 * chunk), 0)], grad, cout, Kp, epilogue=_lib.EPI_RESADD, groups=n_taps, res=grad,
                          a_grouped=False, x3=True)
        else:
            ops.conv_gemm([(dyT, xT, 0)], part, cout, N, groups=ks, x3=True)
            _lib.check(lib.dn_wgrad_reduce(part.data_ptr(), ks, cout, N, rows_w, n_taps, grad.data_ptr(), Np, Kp, st), "dn_wgrad_reduce")
        return grad

    return run, ks


def tn_slices(B, T, cin, cout, n_taps):
    tiles = ((cout + 255) // 256) * ((n_taps * pn(cin) + 255) // 256)
    s = 1
    while s < 16 and tiles * s < 160 and B * T // (s * 2) >= 256:
        s *= 2
    return s


for name, cin, cout, shifts, B, T in (("vae ffn conv 2048 k3", 2048, 2048, [2, 1, 0], 24, 512), ("projection 768 -> 768", 768, 768, [0], 24, 512),
                                      ("ffn_out 2048 -> 768", 2048, 768, [0], 24, 512)):
    x, dy = torch.randn(B * T, pk(cin)) * 0.5, torch.randn(B * T, pk(cout)) * 0.5
    x[:, cin:] = 0
    dy[:, cout:] = 0
    xs, dys = packing.split_rows(x).to(dev), packing.split_rows(dy).to(dev)
    flops = 2.0 * B * T * cin * cout * len(shifts)
    run, ks = copies_form(xs, dys, B, T, cin, cout, shifts)
    t0 = timeit(run)
    line = f"{name:24s} copies + contraction (k_slices {ks}) {t0:8.1f} us ({flops / t0 / 1e6:6.1f} TF/s)"
    sl = tn_slices(B, T, cin, cout, len(shifts))
    acc = torch.zeros((len(shifts), pn(cout), pk(cin)), device=dev)  # accumulated into, as the engine's gradient is
    for stages in (3, 2):
        with _lib.option("wgrad_stages", stages):
            t = timeit(lambda: ops.conv_weight_grad_tn(xs, dys, T, cin, cout, shifts, slices=sl, dtype="bf16x3", grad=acc))
        line += f" | row-major, {stages} stages, slices {sl} {t:8.1f} us ({flops / t / 1e6:6.1f} TF/s)"
    a = ops.conv_weight_grad_tn(xs, dys, T, cin, cout, shifts, slices=sl, dtype="bf16x3")
    g = run()
    g.zero_()
    b = run()[:, :cout, :cin]
    line += f" | max diff {(a - b).abs().max().item():.2e} of {a.abs().max().item():.2e}"
    print(line, flush=True)
