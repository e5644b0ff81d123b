"""Operator grid of dn_conv_gemm in the f16, bf16 and f32 modes against float64: every tile choose_tile honours when forced, every
epilogue, and the geometry edges of csrc/gemm_kernels.h, through ops.conv_gemm.  Operands are built on the CPU with
packing._arith / packing.kblock.  The split-operand mode has its own grid (tests/test_hip_x3_gemm_grid.py); the helpers that do not
depend on the arithmetic are shared (tests/gemm_grid_common.py).

Two float64 references per case, both on the CPU:
  * value: the operation on the numbers the device holds (operands rounded to the storage type, rows outside their sequence zero,
    the epilogue's formula in float64).  Bars of tests/test_hip_bf16x3.py, relative to max(1, max |want|): 1e-4 for the linear
    epilogues (BIAS, RELU, RESADD, POSEMB), 2e-4 where an activation follows (SILU, GEGLU, FILM_GATE); an output stored in a 2-byte
    type gets one unit roundoff of that format times |want| on top (2^-11 f16, 2^-8 bf16): the store's rounding and nothing else.
  * bound from the reference side: the same contraction with one torch float32 matmul per term, summed and finished in float32,
    is measured against the float64 value ("emulated"); the device is allowed max(8 x emulated, 2^-22 max |acc| sqrt(K n_terms / 64))
    plus the store's unit roundoff.  Products of 2-byte operands are exact in fp32, so the device differs by summation order only.
Every case prints one line "GEMMGRID <test> <mode> <tile> <case>: value err / bar | emulated, bound, measured, ratio".

Routes (`honoured`, restated from choose_tile, gemm_kernels.h:2350-2408): only (mode, tile, epilogue) triples the library honours
when forced are generated; every launch asserts through dn_conv_gemm_route (the Spy) that the forced tile runs, an unforced launch
that one of the honoured tiles does.  test_route_table_on_the_host holds the table against the library for every triple, on the CPU.

K order (read in gemm_kernels.h).  Term-outer: conv_gemm_kernel (tiles 1, 2: line 804), conv_gemm_mid2_kernel (9: line 1376),
conv_gemm_big_kernel<.., false, BNB> (3, 8) and conv_gemm_fat_kernel<.., false> (4, 6, 7) walk term 0's K, then term 1's, ...;
one accumulator sees the same MFMAs in the same order (16 elements of K per MFMA for 2-byte types), so these agree bit for bit
(tests/test_hip_ops.py asserts it for 1, 2, 3, 4, 6, 7 in bf16).  Tap-inner (DnGemmRoute.taps_inner: the taps of one causal conv on
tile 3 with BIAS / FILM_GATE, on 4, 6, 7 with any epilogue, on 10 always): per 32 elements of K all taps in turn; shared staged rows
change where a fragment is read from, not the order, so a call and the same call under DN_GEMM_NO_SHARED_ROWS agree bit for bit on
tiles 3, 4, 6, 7 (6 and 7 have no shared-row form at all: launch_fat instantiates it for NTW = 11 only).  Tile 10 under
DN_GEMM_NO_SHARED_ROWS is not tile 10 any more (sr_tile_ok needs big_taps_share_rows): the call is routed by shape to a term-outer
tile, so there the two results are each held to the float64 bound, not to each other's bits.

Out of scope: the split-operand mode, the weight-gradient kernels, the route heuristic's scores, timing; no test reads kernel
assembly; no sanitizer runs."""
import math

import pytest
import torch

from gemm_grid_common import BAR, BIAS, FILM, GEGLU, NAMES, NAN, POSEMB, RELU, RESADD, SILU, all_nan, call, epilogue, padn, seeded, shift_rows

gpu = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("f16", "bf16", "f32")
KT = {"f16": 64, "bf16": 64, "f32": 32}  # gemm.hip: K % kt
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "f32": 0.0}  # unit roundoff of a store in the operand type
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
# the emulated error's multiple the device is allowed, per epilogue (8: the x3 grid's rule)
FACTOR = {BIAS: 8, RELU: 8, RESADD: 8, POSEMB: 8, SILU: 8, GEGLU: 8, FILM: 8}


@pytest.fixture(scope="module")
def env():
    from diffnorm_amd import _lib, ops, packing

    _lib.load()
    assert [_lib.EPI_BIAS, _lib.EPI_SILU, _lib.EPI_GEGLU, _lib.EPI_FILM_GATE, _lib.EPI_RESADD, _lib.EPI_POSEMB, _lib.EPI_RELU] == list(range(7))
    assert (_lib.TILE_128X128, _lib.TILE_256X256, _lib.TILE_256X352, _lib.TILE_ROW, _lib.TILE_256X192, _lib.TILE_256X128_2WG, _lib.TILE_256X128_SR) == (1, 3, 4, 5, 8, 9, 10)
    return ops, packing, _lib


def code_of(L, mode):
    return {"f16": L.DN_F16, "bf16": L.DN_BF16, "f32": L.DN_F32}[mode]


# ------------------------------------------------------------------------------------------ the route table
def fold_taps(shifts, K, shift_by_group=False):
    """sr_tile_ok / big_taps_share_rows(p, 32), gemm_kernels.h:2288-2293 and 2344-2346: three taps (2d, d, 0), two 32-element chunks"""
    return len(shifts) == 3 and shifts[2] == 0 and shifts[1] >= 1 and shifts[0] == 2 * shifts[1] and K // 32 >= 2 and (shift_by_group or 2 * shifts[1] <= 128)


def honoured(mode, tile, epi, packed=0, fold=False, producer=False):
    """Does choose_tile (gemm_kernels.h:2350-2408; row-major operands, no ldw, no whole-row norm, option taps_inner != 2) return the
    forced `tile`?  packed: the packed output columns (2 N for GEGLU); fold: fold_taps() and tap-inner order allowed; producer:
    norm_split set.  RELU is asked about as RELU: routes_to_352 (:2320) knows BIAS and GEGLU only, mid2_ok (:2399) excludes RESADD
    and POSEMB only."""
    two = mode != "f32"  # dn_is16
    if tile == 4:  # :2390 routes_to_352, force == DN_TILE_256X352
        return two and epi in (BIAS, GEGLU) and packed % 352 == 0
    if tile == 10:  # :2391
        return two and epi == RESADD and fold
    if tile == 8:  # :2405
        return two and (epi == BIAS or (epi == RESADD and not producer))
    if tile == 9:  # :2406
        return two and epi not in (RESADD, POSEMB)
    if tile in (6, 7):  # :2407
        return mode == "bf16"
    return tile in (1, 2, 3)  # :2408; 5 (DN_TILE_ROW) is never forced: :2352 takes the whole-row norm there whatever is forced


def by_shape(mode, epi, packed):
    """the tiles choose_tile may name when nothing (honoured) is forced: :2390 (BIAS, a multiple of 352), :2455 (256 x 192), :2457-2458"""
    two = mode != "f32"
    return {1, 2, 3} | ({8} if two and epi in (BIAS, RESADD) else set()) | ({4} if two and epi == BIAS and packed % 352 == 0 else set())


TILES = {m: [t for t in range(11) if t == 0 or any(honoured(m, t, e, 352, True) for e in range(7))] for m in MODES}


def width(tile, epi, N):
    """N of a case on `tile`: the 256 x 352 tile takes packed columns that are a multiple of 352 (GEGLU: N a multiple of 64 too)"""
    return N if tile != 4 else 704 if epi == GEGLU else 352 * ((N + 351) // 352)


def grid(epis, modes=MODES, tiles=None, fold=True):
    """pytest params (mode, tile, epilogue name) for every honoured triple; `epis`: names of EPI below"""
    out = []
    for mode in modes:
        for tile in TILES[mode] if tiles is None else [t for t in tiles if t in TILES[mode]]:
            for name in epis:
                e = EPI[name][0]
                if tile == 0 or honoured(mode, tile, e, 2 * 704 if e == GEGLU else 352, fold):
                    if not (name == "film_res_op" and mode == "f32"):  # f32: the operand type is fp32, film_rows already
                        out.append(pytest.param(mode, tile, name, id=f"{mode}-t{tile}-{name}"))
    return out


# name -> (epilogue, build() arguments)
EPI = {"bias": (BIAS, {}), "silu": (SILU, {}), "relu": (RELU, {}), "geglu": (GEGLU, {}), "geglu_pre": (GEGLU, dict(pre=True)),
       "film_rows": (FILM, dict(film="rows")), "film_shared": (FILM, dict(film="shared")), "film_none": (FILM, dict(film=None)),
       "film_res_op": (FILM, dict(film="rows", res_op=True)), "resadd": (RESADD, {}), "posemb": (POSEMB, {})}


# ------------------------------------------------------------------------------------------ one contraction with an epilogue
def build(env, mode, epi, B, T, K, N, shifts, seed=1, groups=1, a_grouped=True, shift_by_group=False, lda=None, film="rows", lengths=None,
          dead=0, res_op=False, pre=False):
    """CPU side of a case.  dead: the last `dead` of the N columns have zero weight rows and zero bias (padded channels).  GEGLU: N
    packed output columns of which N - 11 are live (packing._geglu_rows).  lda > K: NaN behind K.  res_op: the FiLM residual in
    the operand type (else fp32)."""
    _, packing, L = env
    code, M, G, nt, lda = code_of(L, mode), B * T, groups, len(shifts), lda or K
    P = 2 * N if epi == GEGLU else N
    c = dict(mode=mode, epi=epi, B=B, T=T, K=K, N=N, M=M, G=G, P=P, shifts=list(shifts), a_grouped=a_grouped and G > 1, shift_by_group=shift_by_group,
             film=film, pre=pre)
    x = packing._arith(seeded((G if c["a_grouped"] else 1, M, lda), seed), code, weight=False)
    x[..., K:] = NAN
    w = seeded((nt, G, padn(P), K), seed + 1, (K * nt) ** -0.5)
    b = seeded((G, P), seed + 2, 0.1)
    keep = torch.arange(padn(P)) < P - dead
    if epi == GEGLU:
        keep[:P] = packing._geglu_rows(N - 11) >= 0
    w[:, :, ~keep] = 0
    b[:, ~keep[:P]] = 0
    c["live"] = N - 11 if epi == GEGLU else N - dead
    c["x"], c["w"], c["b"] = x, packing._arith(w, code, weight=True), b
    if epi in (FILM, RESADD):
        c["res"] = seeded((G, M, N), seed + 3)
        if res_op:
            c["res"] = c["res"].to(TORCH[mode])
    if epi == FILM and film:
        c["gb"] = seeded((B if film == "rows" else 1, G * 2 * N), seed + 4, 0.5)
        c["gb"][:, :N] += 1.0
    if epi == POSEMB:
        c["lengths"] = torch.tensor(lengths if lengths is not None else [(i * 7) % (T + 1) if i else T for i in range(B)], dtype=torch.int32)
        if B > 1 and lengths is None:
            c["lengths"][1] = 0
        c["tab"] = packing.sinusoidal_table(T + 1, N, N)
    return c


def subset(c, b):
    """the case of sequence b alone"""
    T, s = c["T"], dict(c)
    rows = slice(b * T, (b + 1) * T)
    s.update(B=1, M=T, x=c["x"][:, rows].contiguous())
    if "res" in c:
        s["res"] = c["res"][:, rows].contiguous()
    if "gb" in c and c["film"] == "rows":
        s["gb"] = c["gb"][b:b + 1].contiguous()
    if "lengths" in c:
        s["lengths"] = c["lengths"][b:b + 1].contiguous()
    return s


def reference(c):
    """(value in float64 [G, M, N], the same in fp32 arithmetic [G, M, N], max |accumulator|, pre-activation in float64 or None)"""
    epi, T, K, N, M, G, P = (c[k] for k in ("epi", "T", "K", "N", "M", "G", "P"))
    seq = torch.arange(M) // T
    v64, v32, pre64, accmax = [], [], [], 0.0
    for g in range(G):
        a64 = a32 = 0
        xg = c["x"][g if c["a_grouped"] else 0][:, :K]
        for j, sh in enumerate(c["shifts"]):
            sh = sh * (1 << g) if c["shift_by_group"] else sh
            wj = c["w"][j, g][:P]
            a64 = a64 + shift_rows(xg.double(), sh, T) @ wj.double().t()
            a32 = a32 + shift_rows(xg.float(), sh, T) @ wj.float().t()
        accmax = max(accmax, a64.abs().max().item())
        side = dict(bias=c["b"][g])
        if "res" in c:
            side["res"] = c["res"][g]
        if "gb" in c:
            rows = c["gb"][seq if c["film"] == "rows" else torch.zeros_like(seq)]
            side["ga"], side["be"] = rows[:, g * 2 * N: g * 2 * N + N], rows[:, g * 2 * N + N: (g + 1) * 2 * N]
        if epi == POSEMB:
            t = torch.arange(M) % T
            side["pos"] = c["tab"][torch.where(t < c["lengths"][seq], t + 1, torch.zeros_like(t))]
        v64.append(epilogue(a64, epi, **side))
        v32.append(epilogue(a32, epi, **side))
        pre64.append(a64 + c["b"][g].double())
    return torch.stack(v64), torch.stack(v32), accmax, torch.stack(pre64)


WORST = {}


def judge(test, mode, case, got, val, v32, accmax, epi, K, n_terms, unit):
    """Both references on one output (got: the device's values as fp32, CPU); unit: the unit roundoff of the output's storage type."""
    got = got.double()
    store = unit * val.abs()
    v_bar = BAR[epi] * max(1.0, val.abs().max().item())
    err = (got - val).abs()
    e_val = (err - store).clamp_min(0).max().item()
    emu = (v32.double() - val).abs().max().item()
    bound = max(FACTOR[epi] * emu, 2.0 ** -22 * accmax * math.sqrt(K * n_terms / 64))
    meas, ratio = err.max().item(), (err / (bound + store)).max().item()
    w = WORST.setdefault((test, mode), [0.0, 0.0])
    w[0], w[1] = max(w[0], e_val / v_bar), max(w[1], ratio)
    print(f"GEMMGRID {test} {mode} {case}: value err {e_val:.3e} / bar {v_bar:.3e} | emulated {emu:.3e} bound {bound:.3e} measured {meas:.3e} "
          f"ratio {ratio:.3f} | worst so far {w[0]:.3f} {w[1]:.3f}")
    assert not torch.isnan(got).any(), (case, "NaN in the output")
    assert e_val <= v_bar, (case, e_val, v_bar)
    assert ratio <= 1.0, (case, meas, bound, emu, ratio)


def launch(env, c, tile, out="f32", pad=12, frame=0, kb=False, out_kb=False, shared_rows=None, forced=True):
    """One launch into a NaN-filled buffer with 3 rows and `pad` columns to spare (ldo = N + pad); asserts the route and that nothing
    outside [M, N] was written.  RESADD runs in place on the fp32 stream.  frame: the activations sit inside a larger buffer with
    `frame` NaN rows in front of row 0 and behind row M.  kb: K-blocked activations and weights; out_kb: K-blocked output.
    forced=False: the forced tile need not run (the call is routed by shape).  Returns the live [G, M, N] block on the CPU as fp32
    (GEGLU with pre: and the pre-activation [M, 2 N]); the route is left in c["route"]."""
    _, packing, L = env
    mode, epi, T, N, M, G, P = (c[k] for k in ("mode", "epi", "T", "N", "M", "G", "P"))
    odt = torch.float32 if out == "f32" else TORCH[mode]
    if out_kb:
        buf = torch.full((G, N // 32, M, 32), NAN, dtype=odt)
    else:
        buf = torch.full((G, M + 3, N + pad) if pad else (G, M, N), NAN, dtype=odt)
    if epi == RESADD:
        buf[:, :M, :N] = c["res"]
    buf = buf.to(DEV)
    one = lambda t: t if G > 1 else t[0]
    x, wd = c["x"], c["w"].to(DEV)
    if frame:
        assert not c["a_grouped"]
        big = torch.full((M + 2 * frame, x.shape[-1]), NAN, dtype=x.dtype)
        big[frame:frame + M] = x[0]
        xd = big.to(DEV)[frame:frame + M]
        assert xd.is_contiguous()
    else:
        xd = x.to(DEV) if c["a_grouped"] else x[0].to(DEV)
    if kb:  # the taps' weights stay in arithmetic progression: slices of one K-blocked stack [n_terms, 1, K/32, rows, 32]
        assert G == 1 and x.shape[-1] == c["K"]
        xd, wd = packing.kblock(xd), packing.kblock(wd)
    terms = [(xd, one(wd[j]), sh) for j, sh in enumerate(c["shifts"])]
    kw = dict(bias=one(c["b"]).contiguous().to(DEV), epilogue=epi, groups=G, a_grouped=c["a_grouped"], shift_by_group=c["shift_by_group"], tile=tile,
              a_kblocked=kb, w_kblocked=kb, out_kblocked=out_kb, shared_rows=shared_rows)
    if epi == FILM:
        kw.update(res=one(c["res"]).to(DEV))
        if "gb" in c:
            kw.update(gamma_beta=c["gb"].to(DEV), gb_half=N, gb_shared=c["film"] == "shared")
    if epi == RESADD:
        kw.update(res=one(buf))
    if epi == POSEMB:
        kw.update(pos_table=c["tab"].to(DEV), lengths=c["lengths"].to(DEV))
    pre = None
    if c["pre"]:
        pre = torch.full((M + 3, P + 8), NAN, dtype=odt, device=DEV)
        kw.update(pre_out=pre)
    r = call(terms, one(buf), T, N, whole_route=True, **kw)
    c["route"] = r
    if tile == 0 or not forced:
        assert r.tile in by_shape(mode, epi, P), (tile, r.tile)
    else:
        assert r.tile == tile, (tile, r.tile)
    got = buf.cpu()
    if out_kb:
        return packing.unkblock(got).float()
    if pad:
        assert all_nan(got[:, M:]) and all_nan(got[:, :M, N:]), "wrote outside [M, N]"
    live = got[:, :M, :N].float()
    if pre is not None:
        pc = pre.cpu()
        assert all_nan(pc[M:]) and all_nan(pc[:M, P:]), "pre_out: wrote outside [M, 2 N]"
        return live, pc[:M, :P].float()
    return live


def kinds(c):
    """output types of a case: fp32 and the operand type; RESADD writes fp32 only, pre_out needs out_dtype == dtype (gemm.hip)"""
    if c["mode"] == "f32" or c["epi"] == RESADD:
        return ["f32"]
    return ["op"] if c["pre"] else ["f32", "op"]


def run_case(env, test, case, mode, tile, name, B, T, K, N, shifts, tight=False, frame=0, **kw):
    """Build, launch (fp32 output, then the operand type), judge.  tight: also with ldo = N and no spare rows (rows that are 16-byte
    aligned take the 8-column stores of wave_epilogue_wide)."""
    epi, ekw = EPI[name]
    N = width(tile, epi, N)
    c = build(env, mode, epi, B, T, K, N, shifts, **ekw, **kw)
    val, v32, accmax, pre64 = reference(c)
    outs = {}
    for kind in kinds(c):
        unit = UNIT[mode] if kind == "op" else 0.0
        for pad in (12, 0) if tight else (12,):
            got = launch(env, c, tile, out=kind, pad=pad, frame=frame)
            if c["pre"]:
                got, pre = got
                tol = BAR[BIAS] * max(1.0, pre64.abs().max().item()) + unit * pre64[0].abs()
                assert ((pre.double() - pre64[0]).abs() <= tol).all(), (case, "pre_out")
            judge(test, mode, f"t{tile} {case} {name} out {kind} pad {pad}", got, val, v32, accmax, epi, K, len(shifts), unit)
            if c["live"] < N and epi != FILM and epi != RESADD and epi != POSEMB:  # zero weight rows and zero bias: exact zeros
                assert got[..., c["live"]:].abs().max().item() == 0.0
            outs[kind, pad] = got
    return c, outs


# ------------------------------------------------------------------------------------------ host only: the table against the library
def test_route_table_on_the_host(env):
    """Every (mode, forced tile 0..10, epilogue), with the properties the table depends on (packed columns a multiple of 352 or not,
    the folded contraction's taps or one term, the split norm's producer, the whole-row norm): dn_conv_gemm_route names the forced
    tile exactly where `honoured` says so, else one of by_shape().  Nothing is launched and no device is touched."""
    _, _, L = env
    n = 0
    for mode in MODES:
        dt = TORCH[mode]
        for epi in range(7):
            for N in (64, 352, 704):
                for shifts in ([0], [2, 1, 0], [3, 1, 0]):
                    P = 2 * N if epi == GEGLU else N
                    M, K, nt = 300, 64, len(shifts)
                    a, w = torch.empty(M, K, dtype=dt), torch.empty(nt, padn(P), K, dtype=dt)
                    kw = dict(bias=torch.empty(P), epilogue=epi)
                    if epi in (FILM, RESADD):
                        kw["res"] = torch.empty(M, N)
                    if epi == POSEMB:
                        kw.update(pos_table=torch.empty(8, N), lengths=torch.zeros(3, dtype=torch.int32))
                    variants = [("plain", {})]
                    if epi in (RESADD, POSEMB):
                        variants.append(("producer", dict(norm_out=torch.empty(M, N), norm_D=N, norm_ssq=torch.empty(M, (N + 63) // 64))))
                        if N <= 512:
                            variants.append(("whole_row", dict(norm_out=torch.empty(M, N), norm_D=N)))
                    for vname, vkw in variants:
                        for force in range(11):
                            terms = [(a, w[j], sh) for j, sh in enumerate(shifts)]
                            got = call(terms, torch.empty(M, N), 100, N, tile=force, host=True, launch=False, **kw, **vkw)
                            key = (mode, NAMES[epi], N, shifts, vname, force, got)
                            n += 1
                            if vname == "whole_row":
                                assert got == L.TILE_ROW, key
                            elif force and honoured(mode, force, epi, P, fold_taps(shifts, K), vname == "producer"):
                                assert got == force, key
                            else:
                                assert got in by_shape(mode, epi, P) and got != force, key  # (by shape these sizes go to 1, 2 or 3)
    assert n == 3 * (7 * 9 + 2 * 3 * 3 + 2 * 2 * 3) * 11
    for m in MODES:  # the tile lists the device tests are generated from
        assert TILES[m] == {"f16": [0, 1, 2, 3, 4, 8, 9, 10], "bf16": [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], "f32": [0, 1, 2, 3]}[m]


def test_the_reference_rows_outside_a_sequence_are_zero():
    """(CPU) shift_rows: a shift >= T, either sign, leaves nothing; shift == t is the first frame that reads (shift_valid's >=)"""
    a = torch.ones(6, 2)
    assert shift_rows(a, 3, 3).abs().sum() == 0 and shift_rows(a, -3, 3).abs().sum() == 0
    assert shift_rows(a, 1, 3)[:, 0].tolist() == [0, 1, 1, 0, 1, 1] and shift_rows(a, 2, 3)[:, 0].tolist() == [0, 0, 1, 0, 0, 1]


# ------------------------------------------------------------------------------------------ device: epilogues, K, M, T, N, lda
@gpu
@pytest.mark.parametrize("mode,tile,name", grid(list(EPI)))
def test_every_epilogue_on_every_tile(env, mode, tile, name):
    """Three causal taps, M = 129 (3 x 43: sequence starts inside a tile, a ragged last tile), K = 128, N = 192 (352 / 704 on the
    256 x 352 tile); fp32 and operand-type outputs, each with ldo = N + 12 and ldo = N; RESADD in place; POSEMB with lengths 0 / T / 17;
    GEGLU with and without pre_out; FILM_GATE with gamma_beta per row, shared, absent and the residual in either type."""
    kw = dict(lengths=[0, 43, 17]) if name == "posemb" else {}
    run_case(env, "epilogues", "3x43", mode, tile, name, 3, 43, 128, 192, [2, 1, 0], tight=True, **kw)


def tiles_x(names):
    """pytest params (mode, tile, name): for every tile of every mode, each of `names` it is honoured for; tiles that take none of
    them (10) run resadd"""
    out = []
    for mode in MODES:
        for tile in TILES[mode]:
            ok = [n for n in names if tile == 0 or honoured(mode, tile, EPI[n][0], 352, True)] or ["resadd"]
            out += [pytest.param(mode, tile, n, id=f"{mode}-t{tile}-{n}") for n in ok]
    return out


@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["bias", "silu"]))
@pytest.mark.parametrize("kts", [1, 2, 3, 5])
def test_k_tiles(env, mode, tile, name, kts):
    """K of 1, 2, 3 and 5 K-tiles of the mode (64 elements, f32: 32): prologue and drain of every ring, one term and three taps
    (the shared-row tile: three taps only -- one term is not its contraction)."""
    K = kts * KT[mode]
    if tile != 10:
        run_case(env, "k_tiles", f"K {K} one term", mode, tile, name, 2, 50, K, 64, [0])
    run_case(env, "k_tiles", f"K {K} three taps", mode, tile, name, 2, 50, K, 64, [2, 1, 0], seed=7)


M_EDGES = [(1, 37), (1, 127), (2, 64), (3, 43), (1, 255), (2, 128), (1, 257), (3, 257)]


@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["bias", "film_rows"]))
def test_m_edges(env, mode, tile, name):
    """M below one tile, one below, on and above 128 and 256 rows, and 771 = 3 x 257: the full / ragged slab forms of the epilogue."""
    for B, T in M_EDGES:
        run_case(env, "m_edges", f"M {B}x{T}", mode, tile, name, B, T, 64, 64, [2, 1, 0])


@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["film_rows", "posemb", "bias"]))
@pytest.mark.parametrize("T", [1, 2, 3])
def test_sequences_shorter_than_the_shifts(env, mode, tile, name, T):
    """T = 1, 2, 3 under taps (8, 4, 0): both shifted taps lie before every sequence start and contribute nothing; a 256-row tile holds
    85 to 256 sequences, and the (sequence, frame) advance of the FiLM / POSEMB epilogues divides instead of wrapping once."""
    B = 258 // T
    kw = dict(lengths=[(i * 7) % (T + 1) for i in range(B)]) if name == "posemb" else {}
    run_case(env, "short_T", f"T {T} B {B}", mode, tile, name, B, T, 64, 64, [8, 4, 0], **kw)


@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["bias", "silu"]))
def test_n_edges(env, mode, tile, name):
    """N just past 64, 128, 192 and 256 columns (the 256 x 352 tile: 352 and 704), ldo = N + 12 with NaN behind N that must stay
    NaN, the last 4 columns padded channels (zero weight rows and bias: exact zeros where the epilogue keeps zero)."""
    for N in (352, 704) if tile == 4 else (68, 132, 196, 260):
        run_case(env, "n_edges", f"N {N}", mode, tile, name, 1, 70, 64, N, [2, 1, 0], dead=4)


@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["bias", "silu"]))
def test_lda_beyond_k(env, mode, tile, name):
    """Row stride of the activations above K with NaN behind K: a projection reading the front of wider rows."""
    run_case(env, "lda", "lda 160 K 64", mode, tile, name, 2, 50, 64, 64, [2, 1, 0], lda=160)
    run_case(env, "lda", "lda 224 K 192", mode, tile, name, 2, 50, 192, 64, [2, 1, 0], lda=224)


GROUPS = {"g2": dict(groups=2), "g3": dict(groups=3), "g3_shared_a": dict(groups=3, a_grouped=False),
          "g3_shift_by_group": dict(groups=3, a_grouped=False, shift_by_group=True)}


@gpu
@pytest.mark.parametrize("mode,tile,name", grid(["bias", "film_rows", "film_shared"]))
@pytest.mark.parametrize("form", list(GROUPS), ids=list(GROUPS))
def test_groups(env, mode, tile, name, form):
    """Groups with every group stride set (activations, weights, bias, output, residual, FiLM rows), activations shared by the
    groups, and the WaveNet block form: shifts (2, 1, 0) << group."""
    run_case(env, "groups", form, mode, tile, name, 2, 45, 64, 64, [2, 1, 0], **GROUPS[form])


BWD = {"bwd_d1": [-2, -1, 0], "bwd_d4": [-8, -4, 0], "bwd_8_terms": [-7, -6, -5, -4, -3, -2, -1, 0]}


@gpu
@pytest.mark.parametrize("mode,tile,name", grid(["bias", "silu"], modes=("f16",), tiles=[0, 1, 2, 3, 4]))
@pytest.mark.parametrize("terms", list(BWD), ids=list(BWD))
def test_negative_shifts_in_f16(env, mode, tile, name, terms):
    """The backward-data form (frames past the sequence end are zeros) in f16 on tiles 0-4: T = 37 with three sequences, so every
    shift crosses a sequence end inside a tile."""
    run_case(env, "bwd", terms, mode, tile, name, 3, 37, 64, 64, BWD[terms])


# ------------------------------------------------------------------------------------------ K-blocked operands and output
@gpu
@pytest.mark.parametrize("mode,tile,name", grid(["bias", "silu", "geglu", "film_rows", "resadd"], modes=("f16", "bf16"), tiles=[3, 4, 8, 9, 10]))
def test_kblocked_operands_and_output(env, mode, tile, name):
    """DN_LAYOUT_A_KBLOCKED | DN_LAYOUT_W_KBLOCKED on the tiles that take them: the layout changes addresses, not the K order, so the
    call equals the row-major call bit for bit; likewise a K-blocked output against packing.kblock of the row-major one (its
    unkblock here)."""
    epi, ekw = EPI[name]
    c = build(env, mode, epi, 3, 43, 128, width(tile, epi, 192), [2, 1, 0], **ekw)
    val, v32, accmax, _ = reference(c)
    for kind in kinds(c):
        ref = launch(env, c, tile, out=kind)
        judge("kblocked", mode, f"t{tile} {name} out {kind} row-major", ref, val, v32, accmax, epi, 128, 3, UNIT[mode] if kind == "op" else 0.0)
        kb_ok = tile != 8 or epi == BIAS  # choose_tile :2400-2404: K-blocked operands on the 192-column form for BIAS only (else refused)
        if kb_ok:
            assert torch.equal(launch(env, c, tile, out=kind, kb=True), ref), (kind, "K-blocked operands")
        if kind == "op" and epi != RESADD:
            assert torch.equal(launch(env, c, tile, out=kind, out_kb=True), ref), "K-blocked output"
            if kb_ok:
                assert torch.equal(launch(env, c, tile, out=kind, kb=True, out_kb=True), ref), "K-blocked operands and output"


# ------------------------------------------------------------------------------------------ shared rows and their fallback
def halo_cases():
    out = []
    for mode in MODES:
        for tile in (3, 4, 6, 7, 10):
            if tile not in TILES[mode]:
                continue
            for d in (1, 8) + ((64, 65) if tile == 3 else ()):
                for T in [255, 256, 257, 100] + ([2 * d - 1, 2 * d, 2 * d + 1] if d <= 8 else []):
                    out.append(pytest.param(mode, tile, d, T, id=f"{mode}-t{tile}-d{d}-T{T}"))
    return out


@gpu
@pytest.mark.parametrize("mode,tile,d,T", halo_cases())
def test_shared_rows_and_their_fallback(env, mode, tile, d, T):
    """Taps (2d, d, 0) on the tiles with a tap-inner order: T = 255 / 256 / 257 put the second sequence's start at the last row of
    the first tile, at the first row of the second (no start inside any tile) and at its second row, the third's in the middle;
    T = 100 puts three sequences in one tile; T = 2d - 1, 2d,
    2d + 1 makes a sequence shorter than, equal to and one longer than the halo.  d = 64 is the last shift that shares on the
    256 x 256 tile, d = 65 the first that does not (big_taps_share_rows: 2 d <= 128 ... per tap: d <= 64).  The activations lie
    between NaN rows: a halo read outside its own sequence's buffer shows.  Against float64, and against the same call under
    DN_GEMM_NO_SHARED_ROWS: equal bits on tiles 3, 4, 6, 7 (module docstring); tile 10 is then routed to a term-outer tile and held
    to the float64 bound."""
    name = "resadd" if tile == 10 else "bias"
    epi = EPI[name][0]
    B = max(1, 771 // T) if T > 17 else 720 // T
    K, N = 128, width(tile, epi, 64)
    c = build(env, mode, epi, B, T, K, N, [2 * d, d, 0], seed=3)
    val, v32, accmax, _ = reference(c)
    got = launch(env, c, tile, frame=8)
    judge("halo", mode, f"t{tile} d {d} T {T} B {B} shared {c['route'].shared_rows}", got, val, v32, accmax, epi, K, 3, 0.0)
    assert c["route"].taps_inner == 1, "the taps of one causal conv run innermost on this tile"
    off = launch(env, c, tile, frame=8, shared_rows=False, forced=tile != 10)
    assert c["route"].shared_rows == 0
    if tile == 10:
        judge("halo", mode, f"t{tile} d {d} T {T} B {B} no shared rows -> tile {c['route'].tile}", off, val, v32, accmax, epi, K, 3, 0.0)
    else:
        assert torch.equal(got, off), "shared rows changed the bits"


# ------------------------------------------------------------------------------------------ invariances
@gpu
@pytest.mark.parametrize("mode,tile,name", tiles_x(["bias", "film_rows"]))
def test_a_sequence_alone_and_inside_a_batch(env, mode, tile, name):
    """Row m of the output depends on its own sequence only: the middle sequence of a batch, run alone, gives the same bits."""
    epi, ekw = EPI[name]
    c = build(env, mode, epi, 3, 50, 128, width(tile, epi, 64), [2, 1, 0], **ekw)
    for kind in kinds(c):
        batch = launch(env, c, tile, out=kind)
        alone = launch(env, subset(c, 1), tile, out=kind)
        assert torch.equal(batch[:, 50:100], alone), kind


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["bias", "silu", "relu", "geglu", "film_rows", "resadd", "posemb"])
def test_same_bits_on_tiles_with_the_same_k_order(env, mode, name):
    """Every tile honoured for the epilogue, N = 352 (704 for GEGLU) so that the 256 x 352 tile takes part, taps (4, 2, 0): tiles whose
    DnGemmRoute reports the same taps_inner add one accumulator's MFMAs in the same order (module docstring) and agree bit for
    bit; the two orders are each held to the float64 bound."""
    epi, ekw = EPI[name]
    N = width(4, epi, 352)
    c = build(env, mode, epi, 3, 43, 192, N, [4, 2, 0], lengths=[5, 0, 43], **ekw)
    val, v32, accmax, _ = reference(c)
    for kind in kinds(c):
        first = {}
        for tile in TILES[mode]:
            if tile == 0 or not honoured(mode, tile, epi, c["P"], True):
                continue
            got = launch(env, c, tile, out=kind)
            order = c["route"].taps_inner
            if order not in first:
                first[order] = (tile, got)
                judge("same_bits", mode, f"t{tile} {name} out {kind} taps_inner {order}", got, val, v32, accmax, epi, 192, 3, UNIT[mode] if kind == "op" else 0.0)
            else:
                assert torch.equal(got, first[order][1]), (kind, "tile", tile, "against tile", first[order][0], "taps_inner", order)


# ------------------------------------------------------------------------------------------ split norm and the whole-row norm, f16
def norm_rows(env, c, tile, split, gamma):
    """RESADD / POSEMB with norm_out: split (norm_split = 1: row * gamma and the sums of squares per 64 columns) or the whole-row
    fused RMSNorm (DN_TILE_ROW).  Returns (stream, norm_out in fp32, norm_ssq or None, the device's norm_out and norm_ssq)."""
    _, packing, L = env
    mode, epi, T, N, M = (c[k] for k in ("mode", "epi", "T", "N", "M"))
    stream = torch.full((M + 3, N + 12), NAN)
    if epi == RESADD:
        stream[:M, :N] = c["res"][0]
    stream = stream.to(DEV)
    xn = torch.full((M + 3, N + 16 if split else N), NAN, dtype=TORCH[mode], device=DEV)  # (the whole-row norm: norm_ld <= 512)
    ssq = torch.full((M + 3, N // 64), NAN, device=DEV) if split else None
    xd, wd = c["x"][0].to(DEV), c["w"].to(DEV)
    terms = [(xd, wd[j, 0], sh) for j, sh in enumerate(c["shifts"])]
    kw = dict(bias=c["b"][0].to(DEV), epilogue=epi, tile=tile, norm_out=xn, norm_D=N, norm_gamma=gamma.to(DEV), norm_ssq=ssq)
    if epi == RESADD:
        kw.update(res=stream)
    else:
        kw.update(pos_table=c["tab"].to(DEV), lengths=c["lengths"].to(DEV))
    got = call(terms, stream, T, N, **kw)
    assert got == L.TILE_ROW if not split else got == tile if tile else got in (1, 2, 3), (tile, got)
    s, n = stream.cpu(), xn.cpu()
    assert all_nan(s[M:]) and all_nan(s[:M, N:]) and all_nan(n[M:]) and all_nan(n[:M, N:])
    q = None
    if split:
        q = ssq.cpu()
        assert all_nan(q[M:])
        q = q[:M]
    return s[:M, :N], n[:M, :N].float(), q, xn, ssq


def norm_producers():
    out = []
    for tile in TILES["f16"]:
        for name in ("resadd", "posemb"):
            if tile == 0 or honoured("f16", tile, EPI[name][0], 128, True, producer=True):
                out.append(pytest.param(tile, name, id=f"f16-t{tile}-{name}"))
    return out


@gpu
@pytest.mark.parametrize("tile,name", norm_producers())
def test_split_norm_producer_and_consumers_in_f16(env, tile, name):
    """f16: RESADD / POSEMB with norm_split = 1 on every tile honoured for a producer (8 is not: choose_tile :2405; 9 takes neither
    epilogue; 10 takes the folded taps): the stream, norm_out = row * gamma in f16, norm_ssq per 64 columns against float64 sums of
    squares of the row the device produced.  Then BIAS, SILU and GEGLU consumers on every tile honoured for them (2, 8 and 9
    included) fed that very norm_out and norm_ssq, with row_bias per sample, shared and absent, against float64 on what they were
    given."""
    ops, packing, L = env
    mode, B, T, K, D, N2 = "f16", 3, 43, 128, 128, 64
    M, epi = B * T, EPI[name][0]
    c = build(env, mode, epi, B, T, K, D, [2, 1, 0], seed=11, lengths=[43, 0, 20])
    gamma = seeded((D,), 21, 0.3) + 1.0
    s, n, q, xn, ssq = norm_rows(env, c, tile, True, gamma)
    val, v32, accmax, _ = (t[0] if torch.is_tensor(t) else t for t in reference(c))
    judge("split_norm", mode, f"t{tile} {name} stream", s, val, v32, accmax, epi, K, 3, 0.0)
    judge("split_norm", mode, f"t{tile} {name} norm_out", n, val * gamma.double(), v32 * gamma, accmax * gamma.max().item(), epi, K, 3, UNIT[mode])
    want_q = s.double().pow(2).view(M, D // 64, 64).sum(-1)
    assert (q.double() - want_q).abs().max().item() <= 66 * 2.0 ** -24 * want_q.max().item()  # 64 squares, any fp32 summation order
    seq = torch.arange(M) // T
    scale = math.sqrt(D) / q.double().sum(-1).sqrt().clamp_min(1e-12)
    xin = xn[:M].contiguous()  # rows D + 16 wide: lda > K
    x64 = xin.cpu()[:, :D].double()
    for ctile in TILES[mode]:
        for cname in ("bias", "silu", "geglu"):
            cepi = EPI[cname][0]
            if ctile == 4 or not (ctile == 0 or honoured(mode, ctile, cepi, 64, False)):
                continue
            for rb in ("rows", "shared", None):
                cc = build(env, mode, cepi, B, T, D, N2, [0], seed=31)
                P = cc["P"]
                rbias = seeded((B if rb == "rows" else 1, P), 41, 0.2)
                ckw = dict(row_ssq=ssq[:M].contiguous(), row_D=D)
                if rb:
                    ckw.update(row_bias=rbias.to(DEV), row_bias_shared=rb == "shared")
                out = torch.full((M + 3, N2 + 12), NAN, device=DEV)
                got = call([(xin, cc["w"][0, 0].to(DEV), 0)], out, T, N2, bias=cc["b"][0].to(DEV), epilogue=cepi, tile=ctile, **ckw)
                assert got == ctile or (ctile == 0 and got in by_shape(mode, cepi, P)), (ctile, got)
                o = out.cpu()
                assert all_nan(o[M:]) and all_nan(o[:M, N2:])
                wj = cc["w"][0, 0][:P]
                a64, a32 = x64 @ wj.double().t(), x64.float() @ wj.float().t()
                side = dict(bias=cc["b"][0], scale=scale, rbias=rbias[seq if rb == "rows" else torch.zeros_like(seq)] if rb else None)
                judge("split_norm", mode, f"producer t{tile} {name} consumer t{ctile} {cname} row_bias {rb}", o[:M, :N2], epilogue(a64, cepi, **side),
                      epilogue(a32, cepi, **side), (a64 * scale.unsqueeze(1)).abs().max().item(), cepi, D, 1, 0.0)


@gpu
@pytest.mark.parametrize("name", ["resadd", "posemb"])
@pytest.mark.parametrize("B,T,K,D", [(3, 43, 128, 128), (1, 130, 64, 64), (2, 100, 320, 512)])
def test_whole_row_fused_norm_in_f16(env, name, B, T, K, D):
    """f16 on DN_TILE_ROW (norm_out without norm_split, N <= 512; whatever tile is forced): the stream against both references, and
    norm_out = rmsnorm(row) * gamma in f16 against float64 on the stream the device wrote: sqrt(D) row / |row| * gamma, to 1e-4
    relative to max(1, max |want|) plus the f16 store."""
    mode, epi = "f16", EPI[name][0]
    c = build(env, mode, epi, B, T, K, D, [2, 1, 0], seed=13, lengths=[T, 0, 20][:B])
    gamma = seeded((D,), 23, 0.3) + 1.0
    for force in (0, 3):
        s, n, _, _, _ = norm_rows(env, c, force, False, gamma)
        val, v32, accmax, _ = (t[0] if torch.is_tensor(t) else t for t in reference(c))
        judge("row_norm", mode, f"t5 (forced {force}) {name} {B}x{T} K {K} D {D} stream", s, val, v32, accmax, epi, K, 3, 0.0)
        sd = s.double()
        want = sd * (math.sqrt(D) / sd.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)) * gamma.double()
        tol = 1e-4 * max(1.0, want.abs().max().item()) + UNIT[mode] * want.abs()
        err = (n.double() - want).abs()
        print(f"GEMMGRID row_norm f16 t5 {name} {B}x{T} D {D} norm_out: max err {err.max().item():.3e}, worst share of its tolerance {(err / tol).max().item():.3f}")
        assert (err <= tol).all()
