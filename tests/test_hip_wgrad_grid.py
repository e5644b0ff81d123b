"""Operator grid of the weight-gradient kernels against float64, at the edges of their launch geometry: the row-major kernels of
csrc/wgrad_tn.hip (wgrad_tn_kernel<4>, <5> and <4, 192>, wgrad_tn_x3_kernel<3> and <2>; ops.conv_weight_grad_tn with dtype "bf16" and
"bf16x3") and the transposed route (ops.conv_weight_grad: dn_transpose_pad / dn_transpose_pad_f32, grouped dn_conv_gemm,
dn_wgrad_reduce; bf16 and f32).  Conventions of test_hip_wgrad_tn_x3.py, whose helpers are imported: seeded operands, the reference
is torch autograd of the oracle's causal conv in float64 (wgrad64) on the values a route is given -- the bf16-rounded operands on the
bf16 routes, the full fp32 values on the f32 and split-operand routes -- and the bound is the project's 1e-4 * max(1, max |want|)
(test_hip_ops.py::test_weight_gradient_from_row_major_operands).  Every test prints err / bound; DESIGN.md (section 3, "Weight-
gradient grid") holds the worst ratio per route and axis.

What each axis is there for (line numbers of csrc/wgrad_tn.hip):
  * K-tiles per slice 1 .. 6 with one slice: the prologue and drain branches for 1, 2, 3 (4) K-tiles of 32 frames, exactly TSTAGES,
    and one turn of the steady loop (:172-179, :201-207; :373-378, :400-404), on both ring depths of both kernels.
  * Sequences shorter than a K-tile: the per-lane frame counter x_t = m % T, x_t += 32 % T, wrapped by hand (:107-125, :301-321), with
    several sequence starts inside one K-tile, T = 32 (the counter never moves) and T = 33, and taps whose shift is below T - 1,
    T - 1, T and above T (a tap with shift >= T contributes nothing: exactly 0.0).  T = 32 cannot have a frame count that is not a
    multiple of 32; it runs with 96 frames.
  * Slices: frames_per_slice is rounded up to 32, so late slices are short (1 frame), empty (K-tile count 0) or begin past the last
    frame (K-tile count -1), and must still write zero partial sums; a slice boundary inside a sequence at T = 7.
  * Widths 1 and one below, on and above 64, 128, 192 and 256 in cin and cout, on the 256-column tile and (option wgrad_k192 = 1:
    with one slice every launch below 256 workgroups selects it, :491-496) on the 192-column tile, whose tiles cut the taps' 128-column
    groups so that the tap, the shift and the row stride are per-lane values; the dY half-tile test n + 128 < cout of the
    split-operand kernel (:306) at cout = 128 and 129.
  * Pad columns and row strides: NaN in every column the kernels must not use, at rows of padk() and of 256 elements.  The epilogue
    masks k + r < cin and skips rows n >= cout (:216-226), so no operand needs zero pad columns: this holds for the bf16 kernel as
    for the split-operand one (include/diffnorm_hip.h: "pad columns may hold anything").
  * Accumulation into a gradient that is not zero (bf16 on both tiles; the split-operand kernel again, for its NaN variant): rows
    beyond cout and pad columns bit-unchanged, also with NaN behind the width.
  * Refusals of both C entries, with a sentinel-filled output that must stay as it was.

Exact assertions beside the bound (1e-4 absolute is loose for a sum over one or two frames): a tap with shift >= T is 0.0 everywhere;
with T = 1 and three taps only the zero-shift tap is not zero; two runs give the same bits; with one slice wgrad_k192 = 1,
wgrad_stages = 5 (bf16) and wgrad_stages = 2 (split operands) give the bits of the default (every output sums its frames in the same
order on every tile and ring depth).  Sliced results also agree with the one-slice result within twice the bound.

The CPU part evaluates the split-operand kernel's arithmetic (hi hi + hi lo + lo hi, lo lo dropped) in float64 for every
split-operand shape of the grid and asserts it under 0.1 of the bound, so the GPU adds the order of its fp32 accumulation only.

Out of scope: the grouped launch (blockIdx.z, shift_by_group) has no operator entry and stays covered through the engine tests
(test_hip_wgrad_tn_x3.py::test_grouped_launch_against_one_launch_per_block); no test reads kernel assembly; no sanitizer runs."""
import ctypes as C
import functools

import pytest
import torch

from test_hip_wgrad_tn_x3 import DEV, bound, lib, operands, pad_cols, padk, seeded, split_hi_lo, wgrad64  # noqa: F401  (lib: the module fixture)

gpu = pytest.mark.gpu
NAN = float("nan")
BASE = (72, 40)  # cin, cout of the frame axes: 3 x 128 = 384 packed columns (two tiles of 256 or of 192, three of the split kernel), one n tile


def padn(c):
    return (c + 127) // 128 * 128


def bf16r(t):
    return t.bfloat16().float()


def shifts_of(k, dil):
    return [(k - 1 - j) * dil for j in range(k)]


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def want_of(cin, cout, k, dil, B, T, rounded):
    """float64 reference of a case, computed once and shared (never written to)"""
    x, dy = operands(cin, cout, B, T)
    if rounded:
        x, dy = bf16r(x), bf16r(dy)
    return wgrad64(x, dy, cout, cin, k, dil)


def run(route, cin, cout, k, dil, B, T, slices=1, fill=0.0, ld=None, grad0=None):
    """One launch of a route: "bf16" / "x3" = the row-major kernels, "tr_bf16" / "tr_f32" = the transposed route (slices = k_slices).
    fill: what the columns behind cin / cout hold; ld: row stride of both operands in elements (default padk)."""
    from diffnorm_amd import ops, packing

    x, dy = operands(cin, cout, B, T)
    xp = pad_cols(x, ld or padk(cin), fill).view(B * T, -1)
    dyp = pad_cols(dy, ld or padk(cout), fill).view(B * T, -1)
    sh = shifts_of(k, dil)
    if route in ("bf16", "x3"):
        if route == "x3":
            xa, dya = packing.split_rows(xp).to(DEV), packing.split_rows(dyp).to(DEV)
        else:
            xa, dya = xp.bfloat16().to(DEV), dyp.bfloat16().to(DEV)
        g = None if grad0 is None else grad0.clone().to(DEV)
        return ops.conv_weight_grad_tn(xa, dya, T, cin, cout, sh, slices=slices, dtype="bf16x3" if route == "x3" else "bf16", grad=g).cpu().contiguous()
    dt = torch.bfloat16 if route == "tr_bf16" else torch.float32
    return ops.conv_weight_grad(xp.to(dt).to(DEV), dyp.to(dt).to(DEV), T, cin, cout, sh, k_slices=slices).cpu()


def check(axis, route, case, got, slices=1, note=""):
    """the float64 bound, err / bound printed first; taps that start at or behind the end of every sequence are exactly zero"""
    cin, cout, k, dil, B, T = case
    want = want_of(*case, route in ("bf16", "tr_bf16"))
    assert got.shape == want.shape
    err, b = (got.double() - want).abs().max().item(), bound(want)
    print(f"wgrad grid | {axis} | {route} | cin {cin} cout {cout} k {k} dil {dil} B {B} T {T} slices {slices}{note} | err {err:.3e} bound {b:.3e} err/bound {err / b:.4f}")
    assert err < b
    for j, s in enumerate(shifts_of(k, dil)):
        if s >= T:
            assert torch.count_nonzero(got[j]).item() == 0, (j, s, T)
    if T == 1:
        assert torch.count_nonzero(got[k - 1]).item() > 0  # the zero-shift tap: one frame per sequence, B products per output
    return want


# ------------------------------------------------------------------------------------------------------------ the cases
# 1. (B, T): 1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161 frames = 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6 K-tiles in one slice
KT_FRAMES = [(1, 1), (1, 31), (1, 32), (1, 33), (2, 32), (1, 65), (3, 32), (1, 97), (1, 128), (1, 129), (1, 160), (1, 161)]
KT_CASES = [(*BASE, 3, 1, B, T) for B, T in KT_FRAMES]

# 2. T -> (B, dilations): 70 <= B T <= 140 and B T % 32 != 0 (but T = 32); k = 3, the largest shift 2 dil is below T - 1 (dil 1
# where T > 3), T - 1 (odd T), T (even T) and above T, and the middle tap's shift dil reaches T - 1 and T at the small T
SHORT = {1: (77, [1]), 2: (39, [1, 2]), 3: (25, [1, 2, 3]), 5: (15, [1, 2, 3, 5]), 7: (11, [1, 3, 4]), 16: (5, [1, 8, 9]), 31: (3, [1, 15, 16]),
         32: (3, [1, 16, 17]), 33: (3, [1, 16, 17])}
SHORT_CASES = [(*BASE, 3, dil, B, T) for T, (B, dils) in SHORT.items() for dil in dils]
assert all(70 <= c[4] * c[5] <= 140 and (c[5] == 32 or c[4] * c[5] % 32) for c in SHORT_CASES)

# 3. (B, T, slices) -> frames of each slice: (1, 33, 2): 32 + 1; (1, 33, 3): 32 + 1 + K-tile count 0; (1, 33, 8): 32 + 1, then
# counts 0, -1, -2 ..; (1, 77, 4): 32 + 32 + 13 + count 0; (19, 7, 2): 96 + 37, the boundary 5 frames into sequence 13;
# (19, 7, 3): 64 + 64 + 5, boundaries inside sequences 9 and 18; (1, 160, 5): five slices of exactly one K-tile
SLICED = [(1, 33, 2), (1, 33, 3), (1, 33, 8), (1, 77, 4), (19, 7, 2), (19, 7, 3), (1, 160, 5)]
SLICED_CASES = [(*BASE, 3, 1, B, T) for B, T, _ in SLICED]
TR_SLICED = [(1, 33), (19, 7)]

# 4. every cin of 1, 8, 63 .. 65, 127 .. 129, 191 .. 193, 255 .. 257 and every cout of 1, 15 .. 17, 127 .. 129, 255 .. 257 at least once
WIDTHS = [(1, 1), (8, 15), (63, 16), (64, 17), (65, 127), (127, 128), (128, 129), (129, 255), (191, 256), (192, 257), (193, 1), (255, 128),
          (256, 129), (257, 257), (1, 257), (257, 16), (64, 128), (129, 129), (192, 255), (256, 256)]
assert {c for c, _ in WIDTHS} == {1, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257}
assert {c for _, c in WIDTHS} == {1, 15, 16, 17, 127, 128, 129, 255, 256, 257}
WIDTH_CASES = [(cin, cout, k, 1, 2, 50) for cin, cout in WIDTHS for k in (1, 3)]

# 5. (65, 17): the 16-byte chunks that straddle cin and cout are fetched with their NaN
PAD_CASES = [(cin, cout, 3, 2, 3, 45) for cin, cout in ((72, 40), (200, 72), (65, 17))]

# 6. cin, cout, k
ACC_CASES = [(72, 40, 3, 1, 3, 45), (129, 129, 1, 1, 3, 45), (200, 72, 3, 1, 3, 45)]

X3_CASES = sorted(set(KT_CASES + SHORT_CASES + SLICED_CASES + WIDTH_CASES + PAD_CASES + ACC_CASES))
assert all(max(c[0], c[1]) <= 260 and c[4] * c[5] <= 200 for c in X3_CASES)


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("case", X3_CASES, ids=lambda c: "-".join(map(str, c)))
def test_split_product_in_float64_is_inside_the_bound(case):
    """test_hip_wgrad_tn_x3.py's check at every split-operand shape of this grid: the gradient is bilinear in (x, dy), so the three
    kept terms are the gradient of the split values minus the dropped lo lo term."""
    cin, cout, k, dil, B, T = case
    x, dy = operands(cin, cout, B, T)
    want = want_of(*case, False)
    (xh, xl), (dh, dl) = split_hi_lo(x), split_hi_lo(dy)
    emu = wgrad64(xh + xl, dh + dl, cout, cin, k, dil) - wgrad64(xl, dl, cout, cin, k, dil)
    err = (emu - want).abs().max().item()
    print(f"wgrad grid | x3 emulation | {case} | err {err:.3e} bound {bound(want):.3e} err/bound {err / bound(want):.4f}")
    assert err < 0.1 * bound(want)


# ------------------------------------------------------------------------------------------------------------ 1. K-tiles
@gpu
@pytest.mark.parametrize("route,stages", [("bf16", 5), ("x3", 2)])
@pytest.mark.parametrize("B,T", KT_FRAMES)
def test_one_to_six_k_tiles_on_both_ring_depths(hip_option, route, stages, B, T):
    case = (*BASE, 3, 1, B, T)
    got = run(route, *case)
    check("k-tiles", route, case, got)
    assert torch.equal(bits(run(route, *case)), bits(got))  # two runs, the same bits
    hip_option("wgrad_stages", stages)
    other = run(route, *case)
    check("k-tiles", route, case, other, note=f" stages {stages}")
    assert torch.equal(bits(other), bits(got))


# ------------------------------------------------------------------------------------------------------------ 2. short sequences
@gpu
@pytest.mark.parametrize("route", ["bf16", "x3", "tr_bf16", "tr_f32"])
@pytest.mark.parametrize("case", SHORT_CASES, ids=lambda c: f"T{c[5]}-B{c[4]}-dil{c[3]}")
def test_sequences_shorter_than_a_k_tile(route, case):
    got = run(route, *case)
    check("short T", route, case, got)
    assert torch.equal(bits(run(route, *case)), bits(got))


# ------------------------------------------------------------------------------------------------------------ 3. slices
@gpu
@pytest.mark.parametrize("route", ["bf16", "x3"])
@pytest.mark.parametrize("B,T,slices", SLICED)
def test_short_and_empty_slices(route, B, T, slices):
    case = (*BASE, 3, 1, B, T)
    got = run(route, *case, slices=slices)
    want = check("slices", route, case, got, slices)
    assert torch.equal(bits(run(route, *case, slices=slices)), bits(got))
    one = run(route, *case)
    check("slices", route, case, one)
    assert (got.double() - one.double()).abs().max().item() < 2 * bound(want)


@gpu
@pytest.mark.parametrize("route", ["tr_bf16", "tr_f32"])
@pytest.mark.parametrize("k_slices", [1, 2, 4, 0])
@pytest.mark.parametrize("B,T", TR_SLICED)
def test_transposed_route_k_slices(route, k_slices, B, T):
    """explicit slice counts pad every sequence to a multiple of 64 k_slices frames (ops.conv_weight_grad: the slice count divides
    the padded frame index), 0 = the automatic count"""
    case = (*BASE, 3, 1, B, T)
    got = run(route, *case, slices=k_slices)
    check("k_slices", route, case, got, k_slices)
    assert torch.equal(bits(run(route, *case, slices=k_slices)), bits(got))


# ------------------------------------------------------------------------------------------------------------ 4. widths
@gpu
@pytest.mark.parametrize("route", ["bf16", "x3"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("cin,cout", WIDTHS)
def test_width_edges_on_every_tile(hip_option, route, cin, cout, k):
    case = (cin, cout, k, 1, 2, 50)
    got = run(route, *case)
    check("widths", route, case, got)
    assert torch.equal(bits(run(route, *case)), bits(got))
    if route == "bf16":  # one slice and fewer than 256 workgroups: the option selects the 192-column tile
        hip_option("wgrad_k192", 1)
        other = run(route, *case)
        check("widths", route, case, other, note=" k192")
        assert torch.equal(bits(other), bits(got))


# ------------------------------------------------------------------------------------------------------------ 5. pads and strides
@gpu
@pytest.mark.parametrize("route", ["bf16", "x3"])
@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("ld", [None, 256])
@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_nan_behind_the_width(route, slices, ld, case):
    """Every column from cin / cout to the end of the row holds NaN, in rows of padk() elements and in rows of 256: no product with
    one of them reaches an output (pins the epilogue's claim for the bf16 kernel as well)."""
    got = run(route, *case, slices=slices, fill=NAN, ld=ld)
    assert torch.isfinite(got).all()
    check("NaN pads", route, case, got, slices, note=f" ld {ld or 'padk'}")
    assert torch.equal(bits(got), bits(run(route, *case, slices=slices, ld=ld)))  # and they change no bit of it


# ------------------------------------------------------------------------------------------------------------ 6. bf16 accumulation
@gpu
@pytest.mark.parametrize("fill", [0.0, NAN], ids=["zero-pads", "nan-pads"])
@pytest.mark.parametrize("route,k192", [("bf16", 0), ("bf16", 1), ("x3", 0)])
@pytest.mark.parametrize("case", ACC_CASES, ids=lambda c: f"{c[0]}-{c[1]}-k{c[2]}")
def test_accumulates_into_a_gradient_that_is_not_zero(hip_option, route, k192, fill, case):
    """mirrors test_hip_wgrad_tn_x3.py::test_accumulates_into_a_gradient_that_is_not_zero for the bf16 kernel on both tiles, and for
    both kernels with NaN behind the width: at cin = 129 the chunk of columns 128 .. 135 is fetched, and only the epilogue's mask
    k + r < cin keeps its NaN out of the gradient's pad columns (at a cin that is a multiple of 8 no pad column is fetched at all)"""
    cin, cout, k = case[:3]
    Np, Kp = padn(cout), padk(cin)
    grad0 = seeded((k, Np, Kp), 44, 3.0)
    hip_option("wgrad_k192", k192)
    got = run(route, *case, grad0=grad0, fill=fill)
    assert got.shape == grad0.shape
    # the sum is rounded to fp32 once more: 2^-24 (|grad0| + |want|), three orders below the bound
    check("accumulate", route, case, (got[:, :cout, :cin].double() - grad0[:, :cout, :cin].double()), note=f" k192 {k192} fill {fill}")
    untouched = torch.ones(k, Np, Kp, dtype=torch.bool)
    untouched[:, :cout, :] = False
    assert torch.equal(bits(got[untouched]), bits(grad0[untouched]))  # rows beyond cout
    assert torch.equal(bits(got[:, :cout, cin:]), bits(grad0[:, :cout, cin:]))  # pad columns: + 0


# ------------------------------------------------------------------------------------------------------------ 7. refusals
@gpu
@pytest.mark.parametrize("entry", ["dn_conv_weight_grad_tn", "dn_conv_weight_grad_tn_x3"])
def test_refusals_leave_the_output_untouched(lib, entry):
    """Every operand is a device buffer large enough for the call as it would run if it were not refused; part and grad hold a
    sentinel.  With several slices a grad beside part is allowed and unused (include/diffnorm_hip.h)."""
    from diffnorm_amd import _lib

    fn = getattr(lib, entry)
    per = 2 if entry.endswith("x3") else 1
    cin, cout, B, T, taps = 72, 40, 1, 33, 9
    x = torch.zeros(B * T, per * 128, dtype=torch.bfloat16, device=DEV)
    dy = torch.zeros(B * T, per * 64, dtype=torch.bfloat16, device=DEV)
    grad = torch.full((taps, 128, 128), 7.0, device=DEV)
    part = torch.full((2, cout, 3 * 128), 7.0, device=DEV)  # (the calls that name it have three taps)
    arr = lambda v: (C.c_int32 * taps)(*([v] * taps))
    ok = dict(dy=dy.data_ptr(), lddy=64, cout=cout, x=(C.c_void_p * taps)(*([x.data_ptr()] * taps)), ldx=arr(128), shift=arr(0), n_taps=3, cin=cin,
              B=B, T=T, slices=1, part=None, grad=grad.data_ptr(), stream=_lib.current_stream())
    call = lambda **kw: fn(*{**ok, **kw}.values())
    for bad in (dict(slices=0), dict(n_taps=0), dict(n_taps=9), dict(shift=arr(-1)), dict(lddy=32), dict(part=part.data_ptr())):
        assert call(**bad) == -1, bad
        assert entry.encode() in lib.dn_last_error()
        torch.cuda.synchronize()
        assert (grad == 7.0).all() and (part == 7.0).all(), bad
    assert call(slices=2, part=part.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (grad == 7.0).all() and (part == 0.0).all()  # zero operands: zero partial sums, grad unused
    assert call() == 0
    torch.cuda.synchronize()
    assert (grad == 7.0).all()  # + 0
