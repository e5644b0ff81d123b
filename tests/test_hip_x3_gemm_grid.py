"""Operator grid of dn_conv_gemm in the split-operand mode (DN_BF16X3) against float64: every tile that takes split rows, every
epilogue, the split-norm producer / consumer chain and the geometry edges of csrc/gemm_kernels.h, through ops.conv_gemm(x3=True).
Operands are built on the CPU with packing.split_rows (activations [hi | lo], weights [lo | hi]).

Two float64 references per case, both on the CPU:
  * value: the operation on the numbers the device holds (hi + lo, exact in fp32), zero rows for frames outside a sequence, the
    epilogue's formula in float64.  Bars of tests/test_hip_bf16x3.py, relative to max(1, max |want|): 1e-4 for the linear epilogues
    (BIAS, RELU, RESADD, POSEMB), 2e-4 where an activation follows (SILU, GEGLU, FILM_GATE); a split-row output reproduces the fp32
    output of the same call to 2^-15 max |out|.
  * three products: sum (a_hi w_hi + a_hi w_lo + a_lo w_hi) from the four bf16 halves in float64, then the epilogue -- the kernel's
    arithmetic, so the device differs by fp32 accumulation and fp32 epilogue arithmetic only.  The bound comes from the reference
    side: the same sum with one torch float32 matmul per product, summed and finished in fp32, is measured against the float64 value
    and the device is allowed 8 x that error, with a floor of 2^-22 max |want| sqrt(K n_terms / 64) (another summation order: MFMA
    tiles against a CPU dot product).  A missing or doubled product, or swapped halves, is 2^-9 relative per product and far outside.
Every case prints one line "X3GRID <test> <case>: value err / bar, emulated error, bound, measured error, ratio".

Routes: every launch first asks dn_conv_gemm_route about the very params ops.conv_gemm built (Spy).  A forced 128 x 128, 256 x 128 or
256 x 256 tile is the tile that runs, the 256 x 192 form runs for BIAS; forced with another epilogue it is not taken and the call is
routed by shape like an unforced one (choose_tile, gemm_kernels.h: `force == DN_TILE_256X192 && p.epilogue == DN_EPI_BIAS`), so there
and for tile 0 the assertion is "one of the three tiles that take split rows".

K order (read in gemm_kernels.h): conv_gemm_kernel's mma_all adds, per 32 elements of K, w_lo a_hi, w_hi a_lo, w_hi a_hi; the
256 x 256 kernel adds w_lo a_hi on the even K-tile and w_hi a_lo, w_hi a_hi on the odd one; both walk the terms outermost.  One
accumulator therefore sees the same MFMAs in the same order on all four tiles and the outputs must agree to the last bit, as must a
sequence alone and the same sequence inside a batch.

K = 32 (one split row group of 128 bytes) is a supported width -- gemm.hip checks K % 32 for this mode, both K loops handle a single
K-tile (pair) -- so it is in the K grid; the width that is refused is one that is no multiple of 32.

Out of scope: the f16 mode, the weight-gradient kernels, timing; no test reads kernel assembly; no sanitizer runs."""
import math

import pytest
import torch

import gemm_grid_common as common
from gemm_grid_common import BAR, BIAS, FILM, GEGLU, NAMES, NAN, POSEMB, RELU, RESADD, SILU, all_nan, epilogue, gelu, padn, seeded, shift_rows  # noqa: F401

gpu = pytest.mark.gpu
DEV = "cuda:0"
TILES = [0, 1, 2, 3, 8]


@pytest.fixture(scope="module")
def env():
    from diffnorm_amd import _lib, ops, packing

    _lib.load()
    assert [_lib.EPI_BIAS, _lib.EPI_SILU, _lib.EPI_GEGLU, _lib.EPI_FILM_GATE, _lib.EPI_RESADD, _lib.EPI_POSEMB, _lib.EPI_RELU] == list(range(7))
    return ops, packing, _lib


def call(*args, **kw):
    """ops.conv_gemm(*args, x3=True, **kw) through the Spy of gemm_grid_common; returns the tile dn_conv_gemm_route names"""
    return common.call(*args, x3=True, **kw)


def check_route(tile, epi, got):
    if tile in (1, 2, 3) or (tile == 8 and epi == BIAS):
        assert got == tile, (tile, got)
    else:  # routed by shape (tile 0, or the 192-column form forced for an epilogue it is not built for)
        assert got in (1, 2, 3), (tile, got)


# ------------------------------------------------------------------------------------------ float64 / fp32 references
def halves(s, weight):
    """split rows (bf16 [.., 2 K], CPU) -> (hi, lo) in float64 [.., K]"""
    g = s.reshape(*s.shape[:-1], -1, 2, 32).double()
    a, b = (g[..., i, :].reshape(*s.shape[:-1], -1) for i in (0, 1))
    return (b, a) if weight else (a, b)


def contract(terms, T, K, rows):
    """terms: (split activations [M, 2 lda], split weights [>= rows, 2 K], shift).  Returns the accumulator three ways: float64 of
    (hi + lo) (hi + lo); float64 of the three products; fp32 of the three products (one float32 matmul each, summed in fp32)."""
    val = p64 = p32 = 0
    for xs, ws, shift in terms:
        ah, al = (shift_rows(h[:, :K], shift, T) for h in halves(xs, False))
        wh, wl = (h[:rows] for h in halves(ws, True))
        val = val + (ah + al) @ (wh + wl).t()
        p64 = p64 + ah @ wl.t() + al @ wh.t() + ah @ wh.t()
        for a, w in ((ah, wl), (al, wh), (ah, wh)):
            p32 = p32 + a.float() @ w.float().t()
    return val, p64, p32


WORST = {}


def judge(test, case, got, val, p64, p32, bar, K, n_terms):
    """Both references on one output (got: the device's fp32 values, CPU)."""
    got = got.double()
    v_bar = bar * max(1.0, val.abs().max().item())
    e_val = (got - val).abs().max().item()
    emu = (p32.double() - p64).abs().max().item()
    bound = max(8 * emu, 2.0 ** -22 * p64.abs().max().item() * math.sqrt(K * n_terms / 64))
    e3 = (got - p64).abs().max().item()
    w = WORST.setdefault(test, [0.0, 0.0])
    w[0], w[1] = max(w[0], e_val / v_bar), max(w[1], e3 / bound)
    print(f"X3GRID {test} {case}: value err {e_val:.3e} / bar {v_bar:.3e} | three products: emulated {emu:.3e} bound {bound:.3e} "
          f"measured {e3:.3e} ratio {e3 / bound:.3f} | worst so far {w[0]:.3f} {w[1]:.3f}")
    assert e_val <= v_bar, (case, e_val, v_bar)
    assert e3 <= bound, (case, e3, bound, emu)


# ------------------------------------------------------------------------------------------ one contraction with an epilogue
def build(env, epi, B, T, K, N, shifts, seed=1, groups=1, a_grouped=True, shift_by_group=False, lda=None, film="rows", lengths=None,
          dead=0):
    """CPU side of a case.  dead: the last `dead` of the N columns have zero weight rows and zero bias (padded channels).  GEGLU: N
    packed output columns of which N - 11 are live (packing._geglu_rows)."""
    _, packing, _ = env
    M, G, nt, lda = B * T, groups, len(shifts), lda or K
    P = 2 * N if epi == GEGLU else N
    c = dict(epi=epi, B=B, T=T, K=K, N=N, M=M, G=G, P=P, shifts=list(shifts), a_grouped=a_grouped and G > 1, shift_by_group=shift_by_group, film=film)
    x = seeded((G if c["a_grouped"] else 1, M, lda), seed)  # junk (not zero) in the columns past K when lda > K
    w = seeded((nt, G, padn(P), K), seed + 1, (K * nt) ** -0.5)
    b = seeded((G, P), seed + 2, 0.1)
    keep = torch.arange(padn(P)) < P - dead
    if epi == GEGLU:
        keep[:P] = packing._geglu_rows(N - 11) >= 0
    w[:, :, ~keep] = 0
    b[:, ~keep[:P]] = 0
    c["live"] = N - 11 if epi == GEGLU else N - dead
    c["xs"], c["ws"], c["b"] = packing.split_rows(x), packing.split_rows(w, weight=True), b
    if epi in (FILM, RESADD):
        c["res"] = seeded((G, M, N), seed + 3)
    if epi == FILM and film:
        c["gb"] = seeded((B if film == "rows" else 1, G * 2 * N), seed + 4, 0.5)
        c["gb"][:, :N] += 1.0
    if epi == POSEMB:
        c["lengths"] = torch.tensor(lengths, dtype=torch.int32)
        c["tab"] = packing.sinusoidal_table(T + 1, N, N)
    return c


def subset(c, b):
    """the case of sequence b alone"""
    T, s = c["T"], dict(c)
    rows = slice(b * T, (b + 1) * T)
    s.update(B=1, M=T, xs=c["xs"][:, rows].contiguous())
    if "res" in c:
        s["res"] = c["res"][:, rows].contiguous()
    if "gb" in c and c["film"] == "rows":
        s["gb"] = c["gb"][b:b + 1].contiguous()
    if "lengths" in c:
        s["lengths"] = c["lengths"][b:b + 1].contiguous()
    return s


def reference(c):
    """(value, three products in float64, three products in fp32), each [G, M, N]"""
    epi, T, K, N, M, G = (c[k] for k in ("epi", "T", "K", "N", "M", "G"))
    seq = torch.arange(M) // T
    outs = [[], [], []]
    for g in range(G):
        terms = [(c["xs"][g if c["a_grouped"] else 0], c["ws"][j, g], sh * (1 << g) if c["shift_by_group"] else sh) for j, sh in enumerate(c["shifts"])]
        side = dict(bias=c["b"][g])
        if "res" in c:
            side["res"] = c["res"][g]
        if "gb" in c:
            rows = c["gb"][seq if c["film"] == "rows" else torch.zeros_like(seq)]
            side["ga"], side["be"] = rows[:, g * 2 * N: g * 2 * N + N], rows[:, g * 2 * N + N: (g + 1) * 2 * N]
        if epi == POSEMB:
            t = torch.arange(M) % T
            side["pos"] = c["tab"][torch.where(t < c["lengths"][seq], t + 1, torch.zeros_like(t))]
        for o, acc in zip(outs, contract(terms, T, K, c["P"])):
            o.append(epilogue(acc, epi, **side))
    return [torch.stack(o) for o in outs]


def launch(env, c, tile, split=False, pad=True):
    """One launch into a NaN-filled buffer with 3 rows and 4 (fp32) / 32 (split rows) columns to spare; asserts the route and that
    nothing outside [M, N] was written.  RESADD runs in place on the fp32 stream.  Returns the live [G, M, N] block on the CPU (fp32)."""
    _, packing, _ = env
    epi, T, N, M, G = (c[k] for k in ("epi", "T", "N", "M", "G"))
    rows, ldo = (M + 3, N + (32 if split else 4)) if pad else (M, N)
    out = torch.full((G, rows, 2 * ldo if split else ldo), NAN, dtype=torch.bfloat16 if split else torch.float32)
    if epi == RESADD:
        out[:, :M, :N] = c["res"]
    out = out.to(DEV)
    one = lambda t: t if G > 1 else t[0]
    xd, wd = c["xs"].to(DEV), c["ws"].to(DEV)
    terms = [(xd if c["a_grouped"] else xd[0], one(wd[j]), sh) for j, sh in enumerate(c["shifts"])]
    kw = dict(bias=one(c["b"]).contiguous().to(DEV), epilogue=epi, groups=G, a_grouped=c["a_grouped"], shift_by_group=c["shift_by_group"], tile=tile)
    if epi == FILM:
        kw.update(res=one(c["res"]).to(DEV))
        if "gb" in c:
            kw.update(gamma_beta=c["gb"].to(DEV), gb_half=N, gb_shared=c["film"] == "shared")
    if epi == RESADD:
        kw.update(res=one(out))
    if epi == POSEMB:
        kw.update(pos_table=c["tab"].to(DEV), lengths=c["lengths"].to(DEV))
    check_route(tile, epi, call(terms, one(out), T, N, **kw))
    got = out.cpu()
    if pad:
        assert all_nan(got[:, M:]) and all_nan(got[:, :M, (2 * N if split else N):]), "wrote outside [M, N]"
    return packing.unsplit_rows(got[:, :M, :2 * N]) if split else got[:, :M, :N]


def run_case(env, test, case, tile, epi, B, T, K, N, shifts, **kw):
    """Build, launch (fp32 output, then split rows where the epilogue writes them and N is whole 32-element groups), judge."""
    c = build(env, epi, B, T, K, N, shifts, **kw)
    got = launch(env, c, tile)
    val, p64, p32 = reference(c)
    judge(test, f"{case} tile {tile} {NAMES[epi]}", got, val, p64, p32, BAR[epi], K, len(shifts))
    if c["live"] < N:  # zero weight rows and zero bias: exact zeros (BIAS, RELU, SILU, GEGLU)
        assert got[..., c["live"]:].abs().max().item() == 0.0
    if epi != RESADD and N % 32 == 0:
        back = launch(env, c, tile, split=True)
        assert (back.double() - got.double()).abs().max().item() <= 2.0 ** -15 * got.abs().max().item(), case
    return got


EPILOGUES = [("bias", BIAS, {}), ("silu", SILU, {}), ("relu", RELU, {}), ("geglu", GEGLU, {}), ("film_rows", FILM, dict(film="rows")),
             ("film_shared", FILM, dict(film="shared")), ("film_none", FILM, dict(film=None)), ("resadd", RESADD, {}),
             ("posemb", POSEMB, dict(lengths=[0, 43, 17]))]


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name,epi,kw", EPILOGUES, ids=[e[0] for e in EPILOGUES])
def test_every_epilogue_on_every_tile(env, tile, name, epi, kw):
    """Three causal taps, M = 129 (3 x 43: sequence starts inside a slab, a ragged last slab), K = 128, N = 192 (two column tiles
    of 128, a ragged one of 256, one of 192); fp32 and split-row outputs, RESADD in place, POSEMB with lengths 0 / T / 17.
    Measured on an MI355X, worst of the test's cases: 0.028 of the value bar, 0.347 of the three-product bound."""
    run_case(env, "epilogues", name, tile, epi, 3, 43, 128, 192, [2, 1, 0], **kw)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, SILU], ids=["bias", "silu"])
@pytest.mark.parametrize("K", [32, 64, 128, 192, 320])
def test_k_tiles(env, tile, epi, K):
    """K of 1 (one 32-element group: a single (even, odd) pair on the 256 x 256 tile), 2, 4, 6 and 10 K-tiles of 128 bytes: the
    prologue and drain branches of both K loops, one term and three.
    Measured on an MI355X, worst of the test's cases: 0.033 of the value bar, 0.603 of the three-product bound (K = 320, three taps, SILU)."""
    run_case(env, "k_tiles", f"K {K} one term", tile, epi, 2, 50, K, 64, [0])
    run_case(env, "k_tiles", f"K {K} three taps", tile, epi, 2, 50, K, 64, [2, 1, 0], seed=7)


TERMS = {"one": [0], "taps_d1": [2, 1, 0], "taps_d4": [8, 4, 0], "tap_past_T": [40, 37, 0], "bwd_d1": [-2, -1, 0], "bwd_d4": [-8, -4, 0],
         "bwd_8_terms": [-7, -6, -5, -4, -3, -2, -1, 0], "mixed_8_terms": [36, 5, 3, 1, 0, -1, -3, -36]}


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, SILU], ids=["bias", "silu"])
@pytest.mark.parametrize("terms", list(TERMS), ids=list(TERMS))
def test_terms_and_shifts(env, tile, epi, terms):
    """Causal taps (dilation 1, 4), a tap whose shift is >= T (nothing), negative shifts (the backward-data form) and DN_MAX_TERMS
    terms, T = 37 with three sequences so that every shift crosses a sequence boundary inside a slab.
    Measured on an MI355X, worst of the test's cases: 0.032 of the value bar, 0.356 of the three-product bound."""
    run_case(env, "terms", terms, tile, epi, 3, 37, 64, 64, TERMS[terms])


def test_a_tap_past_the_sequence_contributes_nothing():
    """(CPU) the reference's own zero rows: a shift >= T, either sign, leaves nothing of the operand"""
    a = torch.ones(6, 2)
    assert shift_rows(a, 3, 3).abs().sum() == 0 and shift_rows(a, -3, 3).abs().sum() == 0
    assert shift_rows(a, 1, 3)[:, 0].tolist() == [0, 1, 1, 0, 1, 1] and shift_rows(a, -1, 3)[:, 0].tolist() == [1, 1, 0, 1, 1, 0]


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, FILM], ids=["bias", "film"])
@pytest.mark.parametrize("B,T", [(1, 37), (1, 127), (2, 64), (3, 43), (1, 255), (2, 128), (1, 257)])
def test_m_edges(env, tile, epi, B, T):
    """M below one slab, and one below, on and above the 128- and 256-row tiles: the full / !full slab variants of the epilogue.
    Measured on an MI355X, worst of the test's cases: 0.031 of the value bar, 0.175 of the three-product bound."""
    run_case(env, "m_edges", f"M {B}x{T}", tile, epi, B, T, 64, 64, [1, 0])


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [FILM, POSEMB], ids=["film", "posemb"])
@pytest.mark.parametrize("T", [1, 2, 3])
def test_sequences_shorter_than_four_frames(env, tile, epi, T):
    """T < 4: the per-lane (sequence, frame) advance of the FiLM and POSEMB epilogues divides instead of wrapping once.
    Measured on an MI355X, worst of the test's cases: 0.030 of the value bar, 0.278 of the three-product bound."""
    B = 70 // T
    kw = dict(lengths=[(i * 7) % (T + 1) for i in range(B)]) if epi == POSEMB else {}
    run_case(env, "short_T", f"T {T} B {B}", tile, epi, B, T, 64, 64, [1, 0], **kw)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, SILU], ids=["bias", "silu"])
def test_n_edges(env, tile, epi):
    """N % 4, fewer than 64 columns in a slab, each tile's column boundary; the last 4 columns are padded channels (exact zeros);
    split-row outputs at the multiples of 32 (run_case), every buffer with rows and columns to spare that must stay NaN.
    Measured on an MI355X, worst of the test's cases: 0.037 of the value bar, 0.400 of the three-product bound (N = 4)."""
    for N in (4, 60, 64, 68, 124, 128, 132, 192, 196, 256, 260, 32, 96, 160, 224, 288):
        run_case(env, "n_edges", f"N {N}", tile, epi, 1, 70, 64, N, [1, 0], dead=4 if N > 4 else 0)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, SILU], ids=["bias", "silu"])
def test_lda_beyond_k(env, tile, epi):
    """Row stride of the activations above K (a multiple of 32) with junk behind K: a projection reading the front of wider rows.
    Measured on an MI355X, worst of the test's cases: 0.028 of the value bar, 0.297 of the three-product bound."""
    run_case(env, "lda", "lda 160 K 64", tile, epi, 2, 50, 64, 64, [2, 0], lda=160)
    run_case(env, "lda", "lda 224 K 192", tile, epi, 2, 50, 192, 64, [2, 0], lda=224)


GROUPS = {"g2": dict(groups=2), "g3": dict(groups=3), "g3_shared_a": dict(groups=3, a_grouped=False),
          "g3_shift_by_group": dict(groups=3, a_grouped=False, shift_by_group=True)}


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi,film", [(BIAS, None), (FILM, "rows"), (FILM, "shared")], ids=["bias", "film_rows", "film_shared"])
@pytest.mark.parametrize("form", list(GROUPS), ids=list(GROUPS))
def test_groups(env, tile, epi, film, form):
    """Groups with every group stride set (activations, weights, bias, output, residual, FiLM rows), activations shared by the
    groups, and the WaveNet block form: shifts (2, 1, 0) << group.
    Measured on an MI355X, worst of the test's cases: 0.031 of the value bar, 0.257 of the three-product bound."""
    run_case(env, "groups", form, tile, epi, 2, 45, 64, 64, [2, 1, 0], film=film, **GROUPS[form])


@gpu
@pytest.mark.parametrize("epi,kw", [(BIAS, {}), (FILM, dict(film="rows")), (SILU, {}), (GEGLU, {}), (RESADD, {}), (POSEMB, dict(lengths=[5, 0, 43]))],
                         ids=["bias", "film", "silu", "geglu", "resadd", "posemb"])
def test_same_bits_on_every_tile(env, epi, kw):
    """All four tiles add one accumulator's MFMAs in the same order (module docstring): equal bits, fp32 and split-row outputs."""
    c = build(env, epi, 3, 43, 192, 192, [4, 2, 0], **kw)
    ref = launch(env, c, 1)
    for tile in (0, 2, 3, 8):
        assert torch.equal(launch(env, c, tile), ref), tile
    if epi != RESADD:
        refs = launch(env, c, 1, split=True)
        for tile in (2, 3, 8):
            assert torch.equal(launch(env, c, tile, split=True), refs), tile


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("epi", [BIAS, FILM], ids=["bias", "film"])
def test_a_sequence_alone_and_inside_a_batch(env, tile, epi):
    """Row m of the output depends on its own sequence only: the middle sequence of a batch, run alone, gives the same bits."""
    c = build(env, epi, 3, 50, 128, 64, [3, 1, 0])
    batch = launch(env, c, tile)
    alone = launch(env, subset(c, 1), tile)
    assert torch.equal(batch[:, 50:100], alone)


# ------------------------------------------------------------------------------------------ split norm: producer and consumers
PRODUCERS = [(e, g) for e in ("resadd", "posemb") for g in ("gamma", "gb_rows", "gb_shared")]


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("prod,gmode", PRODUCERS, ids=[f"{e}-{g}" for e, g in PRODUCERS])
def test_split_norm_producer_and_consumers(env, tile, prod, gmode):
    """RESADD / POSEMB with norm_split = 1: the stream, norm_out = row * gamma as split rows and as fp32, norm_ssq per 64 columns
    against float64 sums of squares of the row the device produced; then BIAS, SILU and GEGLU consumers fed that very norm_out and
    norm_ssq (row_ssq, row_D, row_bias per sample / shared / none), against float64 on what they were given.
    Measured on an MI355X, worst of the test's cases: 0.043 of the value bar, 0.278 of the three-product bound."""
    ops, packing, L = env
    B, T, K, D, N2 = 3, 43, 128, 128, 64
    M, epi = B * T, RESADD if prod == "resadd" else POSEMB
    c = build(env, epi, B, T, K, D, [1, 0], seed=11, lengths=[43, 0, 20])
    Bc = B if gmode == "gb_rows" else 1
    gvec = seeded((Bc, 2 * D), 21, 0.3)
    gvec[:, :D] += 1.0  # [gamma | beta]: the producer reads gamma only
    seq = torch.arange(M) // T
    grow = gvec[seq if gmode == "gb_rows" else torch.zeros_like(seq), :D]
    nkw = dict(norm_D=D, norm_gamma=gvec[0, :D].contiguous().to(DEV)) if gmode == "gamma" else \
        dict(norm_D=D, norm_gb=gvec.to(DEV), norm_gb_half=D, norm_gb_shared=gmode == "gb_shared")
    xd, wd = c["xs"].to(DEV), c["ws"].to(DEV)
    terms = [(xd[0], wd[j, 0], sh) for j, sh in enumerate(c["shifts"])]
    kw = dict(bias=c["b"][0].to(DEV), epilogue=epi, tile=tile)
    if epi == POSEMB:
        kw.update(pos_table=c["tab"].to(DEV), lengths=c["lengths"].to(DEV))
    produced = {}
    for kind in ("f32", "split"):
        stream = torch.full((M + 3, D + 4), NAN)
        if epi == RESADD:
            stream[:M, :D] = c["res"][0]
        stream = stream.to(DEV)
        xn = torch.full((M + 3, 2 * (D + 32)) if kind == "split" else (M + 3, D + 4), NAN, dtype=torch.bfloat16 if kind == "split" else torch.float32, device=DEV)
        ssq = torch.full((M + 3, D // 64), NAN, device=DEV)
        rkw = dict(res=stream) if epi == RESADD else {}
        check_route(tile, epi, call(terms, stream, T, D, norm_out=xn, norm_ssq=ssq, **nkw, **rkw, **kw))
        s, n, q = stream.cpu(), xn.cpu(), ssq.cpu()
        assert all_nan(s[M:]) and all_nan(s[:M, D:]) and all_nan(n[M:]) and all_nan(n[:M, (2 * D if kind == "split" else D):]) and all_nan(q[M:])
        produced[kind] = (s[:M, :D], packing.unsplit_rows(n[:M, :2 * D]) if kind == "split" else n[:M, :D], q[:M], xn, ssq)
    s, n32, q = produced["f32"][:3]
    val, p64, p32 = (t[0] for t in reference(c))
    judge("split_norm", f"{prod} {gmode} tile {tile} stream", s, val, p64, p32, BAR[epi], K, 2)
    judge("split_norm", f"{prod} {gmode} tile {tile} norm_out", n32, val * grow, p64 * grow, p32 * grow.float(), BAR[epi], K, 2)
    assert torch.equal(produced["split"][0], s) and torch.equal(produced["split"][2], q)
    assert (produced["split"][1].double() - n32.double()).abs().max().item() <= 2.0 ** -15 * n32.abs().max().item()
    want_q = s.double().pow(2).view(M, D // 64, 64).sum(-1)
    assert (q.double() - want_q).abs().max().item() <= 66 * 2.0 ** -24 * want_q.max().item()  # 64 squares, any fp32 summation order
    # ---- consumers of the split rows the device wrote: acc * sqrt(D) / |row| + beta . W^T, then the consumer's own epilogue
    xn, ssq = produced["split"][3][:M].contiguous(), produced["split"][4][:M].contiguous()
    xn_cpu = xn.cpu()[:, :2 * D].contiguous()
    scale = math.sqrt(D) / q.double().sum(-1).sqrt().clamp_min(1e-12)
    for cepi in (BIAS, SILU, GEGLU):
        for rb in ("rows", "shared", None):
            cc = build(env, cepi, B, T, D, N2, [0], seed=31)
            P = cc["P"]
            rbias = seeded((B if rb == "rows" else 1, P), 41, 0.2)
            ckw = dict(row_ssq=ssq, row_D=D)
            if rb:
                ckw.update(row_bias=rbias.to(DEV), row_bias_shared=rb == "shared")
            out = torch.full((M + 3, N2 + 4), NAN, device=DEV)
            xn_ld = xn  # the producer's rows are D + 32 wide: lda > K
            check_route(tile, cepi, call([(xn_ld, cc["ws"][0, 0].to(DEV), 0)], out, T, N2, bias=cc["b"][0].to(DEV), epilogue=cepi, tile=tile, **ckw))
            o = out.cpu()
            assert all_nan(o[M:]) and all_nan(o[:M, N2:])
            side = dict(bias=cc["b"][0], scale=scale, rbias=rbias[seq if rb == "rows" else torch.zeros_like(seq)] if rb else None)
            want = [epilogue(acc, cepi, **side) for acc in contract([(xn_cpu, cc["ws"][0, 0], 0)], T, D, P)]
            judge("split_norm", f"{prod} {gmode} tile {tile} consumer {NAMES[cepi]} row_bias {rb}", o[:M, :N2], *want, BAR[cepi], D, 1)


# ------------------------------------------------------------------------------------------ host only: routes and refusals
def host_case(env, epi, M, N, K=64, groups=1, n_terms=1):
    """CPU tensors of the right shapes for a call that is never launched"""
    _, packing, _ = env
    P = 2 * N if epi == GEGLU else N
    lead = (groups,) if groups > 1 else ()
    a = torch.empty(*lead, M, 2 * K, dtype=torch.bfloat16)
    w = torch.empty(*lead, padn(P), 2 * K, dtype=torch.bfloat16)
    kw = dict(bias=torch.empty(*lead, P), epilogue=epi, groups=groups)
    if epi in (FILM, RESADD):
        kw["res"] = torch.empty(*lead, M, N)
    if epi == POSEMB:
        kw.update(pos_table=torch.empty(8, N), lengths=torch.zeros(1, dtype=torch.int32))
    return [(a, w, n_terms - 1 - j) for j in range(n_terms)], torch.empty(*lead, M, N), kw


@pytest.mark.parametrize("M", [40, 300, 4096, 16384])
@pytest.mark.parametrize("N,groups", [(64, 1), (192, 1), (704, 1), (1408, 1), (512, 4), (2048, 1)])
def test_split_operands_route_to_three_tiles_only(env, M, N, groups):
    """Host only: whatever the shape, the epilogue and the forced tile, split operands run on 128 x 128, 256 x 128, 256 x 256 or
    (BIAS, forced) 256 x 192 -- never on DN_TILE_ROW (a split-norm producer included), 256 x 352, the two-workgroup tile or W4 / W8."""
    _, _, L = env
    for epi in (BIAS, SILU, GEGLU, FILM, RESADD, POSEMB, RELU):
        if groups > 1 and epi == POSEMB:
            continue
        for n_terms in (1, 3):
            terms, out, kw = host_case(env, epi, M, N, groups=groups, n_terms=n_terms)
            for force in range(0, 10):
                got = call(terms, out, M, N, tile=force, host=True, launch=False, **kw)
                allowed = {force} if force in (1, 2, 3) or (force == 8 and epi == BIAS) else {L.TILE_128X128, L.TILE_256X128, L.TILE_256X256}
                assert got in allowed, (epi, n_terms, force, got)
    if groups == 1 and N % 64 == 0:  # the producer of a split norm: the whole-row tile is for the other arithmetics
        terms, out, kw = host_case(env, RESADD, M, N)
        got = call(terms, out, M, N, host=True, launch=False, norm_out=torch.zeros(M, 2 * N, dtype=torch.bfloat16), norm_D=N,
                   norm_ssq=torch.zeros(M, N // 64), **kw)
        assert got in (1, 2, 3), got


def aligned(n, dtype, off_bytes=0):
    """CPU tensor of n elements whose base is 128-byte aligned plus off_bytes"""
    raw = torch.zeros(n + 128, dtype=dtype)
    es = raw.element_size()
    start = ((-raw.data_ptr()) % 128 + off_bytes) // es
    t = raw[start:start + n]
    assert t.data_ptr() % 128 == off_bytes
    return t


def test_host_refusals(env):
    """Every check of dn_conv_gemm that exists for split operands only answers DN_EINVAL before anything is launched (the calls carry
    CPU tensors and no stream: nothing here could run).  The unedited call passes the same checks (launch=False stops it there)."""
    ops, packing, L = env
    M, T, N, K = 64, 32, 64, 64

    def refused(match, terms=None, out=None, edit=None, backstop=True, **over):
        t0, o0, kw = host_case(env, over.pop("epi", BIAS), M, N, K=over.pop("K", K), groups=over.pop("groups", 1))
        kw.update(over)

        def edit_(p):  # + a K-blocked layout bit, refused by a later check: were the check under test gone, still nothing would be launched
            if edit:
                edit(p)
            if backstop:
                p.terms[p.n_terms - 1].layout |= L.LAYOUT_W_KBLOCKED

        with pytest.raises(L.DiffNormHipError, match=match) as e:
            call(terms or t0, o0 if out is None else out, T, N, host=True, edit=edit_, **kw)
        assert "failed (-1)" in str(e.value)  # DN_EINVAL

    call(*host_case(env, BIAS, M, N)[:2], T, N, host=True, launch=False, **host_case(env, BIAS, M, N)[2])
    a80 = torch.zeros(M, 2 * 80, dtype=torch.bfloat16)
    w = torch.zeros(128, 2 * K, dtype=torch.bfloat16)
    refused("multiples of 32", terms=[(a80, w, 0)])  # lda = 80
    refused("multiples of 32", groups=2, edit=lambda p: setattr(p.terms[0], "a_gstride", p.terms[0].a_gstride + 16))
    refused("multiples of 32", groups=2, edit=lambda p: setattr(p.terms[0], "w_gstride", p.terms[0].w_gstride + 16))
    refused("split-row output", out=aligned(M * 2 * N, torch.bfloat16).view(M, 2 * N), edit=lambda p: setattr(p, "ldo", N + 16))
    refused("split-row output", out=aligned(M * 2 * N, torch.bfloat16, 16).view(M, 2 * N))
    call(*host_case(env, BIAS, M, N)[:1], aligned(M * 2 * N, torch.bfloat16).view(M, 2 * N), T, N, host=True, launch=False, **host_case(env, BIAS, M, N)[2])
    xn, ssq = aligned(M * 2 * N, torch.bfloat16).view(M, 2 * N), torch.zeros(M, 1)
    refused("split-row norm_out", epi=RESADD, norm_out=xn, norm_D=N, norm_ssq=ssq, norm_kblocked=True)  # norm_split = 2
    refused("norm_split", epi=RESADD, norm_out=xn, norm_D=N)  # the whole-row fused norm
    refused("ldw", edit=lambda p: setattr(p.terms[0], "ldw", K))
    refused("K-blocked", edit=lambda p: setattr(p.terms[0], "layout", L.LAYOUT_A_KBLOCKED))
    refused("K-blocked", edit=lambda p: setattr(p.terms[0], "layout", L.LAYOUT_W_KBLOCKED))
    refused("pre_out", epi=GEGLU, pre_out=torch.zeros(M, 2 * N), backstop=False)  # (the last check of all)
    refused("residual input is fp32", epi=FILM, res=torch.zeros(M, N, dtype=torch.bfloat16))
    refused("K=16", edit=lambda p: setattr(p, "K", 16))  # K % 32 (gemm.hip: kt = 32 for split rows, one 128-byte group); K = 32 runs: test_k_tiles
