#!/usr/bin/env python3
"""Writes tests/golden/gemm_routes.npz: how dn_conv_gemm routes a deterministic sweep of contractions (dn_conv_gemm_route: tile,
K order, shared staged rows, band; and dn_conv_gemm_kblocked_ok), plus the contractions one step of the eps-predictor's sampling
chain issues at the bench and test configs.  tests/test_gemm_routes.py asserts that the library reproduces the table.

The params are stored beside the answers (P: one row per case, HEAD columns then MAX_TERMS x TERM columns); `to_params` turns a
row back into a DnGemmParams.  No GPU: the route is host logic.      python tools/gen_gemm_routes.py [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from diffnorm_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gemm_routes.npz")
HEAD = ("dtype", "epilogue", "M", "N", "K", "T", "groups", "n_terms", "flags", "norm_out", "norm_split", "opt_taps_inner", "opt_tile_192")
TERM = ("A", "W", "lda", "shift", "a_gstride", "w_gstride", "shift_by_group", "layout", "ldw")
MAX_TERMS = _lib.DN_MAX_TERMS
UNSET = -1  # an option column's "not set": applied as the library's default value (1 for both)
OPTIONS = (("taps_inner", HEAD.index("opt_taps_inner")), ("tile_192", HEAD.index("opt_tile_192")))
ANSWERS = ("tile", "taps_inner", "shared_rows", "band", "kblocked_ok")
KB = _lib.LAYOUT_A_KBLOCKED | _lib.LAYOUT_W_KBLOCKED


def to_params(row):
    """DnGemmParams of one stored row (operand addresses are synthetic: only their equality and spacing route)."""
    p = _lib.GemmParams()
    h = dict(zip(HEAD, (int(v) for v in row[:len(HEAD)])))
    p.dtype, p.epilogue, p.M, p.N, p.K, p.T = h["dtype"], h["epilogue"], h["M"], h["N"], h["K"], h["T"]
    p.groups, p.n_terms, p.flags, p.norm_split = h["groups"], h["n_terms"], h["flags"], h["norm_split"]
    p.norm_out = 1 << 40 if h["norm_out"] else None
    for i in range(MAX_TERMS):
        f = dict(zip(TERM, (int(v) for v in row[len(HEAD) + i * len(TERM):len(HEAD) + (i + 1) * len(TERM)])))
        t = p.terms[i]
        t.A, t.W = (1 + f["A"]) << 28, (1 << 44) + f["W"] * 256
        t.lda, t.shift, t.a_gstride, t.w_gstride = f["lda"], f["shift"], f["a_gstride"], f["w_gstride"]
        t.shift_by_group, t.layout, t.ldw = f["shift_by_group"], f["layout"], f["ldw"]
    return p


def query(lib, p, row=None, engine=False):
    """(tile, taps_inner, shared_rows, band, kblocked_ok) of params p (row / engine: the stored row it came from, unused here)."""
    r = _lib.GemmRoute()
    _lib.check(lib.dn_conv_gemm_route(C.byref(p), C.byref(r)), "dn_conv_gemm_route")
    return (r.tile, r.taps_inner, r.shared_rows, r.band, lib.dn_conv_gemm_kblocked_ok(C.byref(p)))


def answer_all(lib, P, engine, query=query):
    """Answers for every row, the stored options set around each query (and restored after)."""
    cur, out = {}, []
    try:
        for row, eng in zip(P, engine):
            for name, col in OPTIONS:
                v = 1 if int(row[col]) == UNSET else int(row[col])
                if cur.get(name) != v:
                    _lib.set_option(name, v)
                    cur[name] = v
            out.append(query(lib, to_params(row), row, bool(eng)))
    finally:
        for name, _ in OPTIONS:
            _lib.set_option(name, None)
    return np.array(out, dtype=np.int32)


def row_of(dtype, epi, M, N, K, T, terms, groups=1, flags=0, norm=(0, 0), opts=(UNSET, UNSET)):
    head = [dtype, epi, M, N, K, T, groups, len(terms), flags, norm[0], norm[1], opts[0], opts[1]]
    body = []
    for i in range(MAX_TERMS):
        body += list(terms[i]) if i < len(terms) else [0] * len(TERM)
    return head + body


def make_terms(kind, d, K, M, groups, layout=0, ldw=0):
    """(A, W, lda, shift, a_gstride, w_gstride, shift_by_group, layout, ldw) per term; A: an activation id, W: in 256-byte units."""
    ag = M * K if groups > 1 else 0
    wg = 3 * 4096 if groups > 1 else 0

    def term(j, shift, A=0, W=None, sbg=0):
        return (A, j * 4096 if W is None else W, K, shift, ag, wg, sbg, layout, ldw)

    taps = {"single": (0,), "taps2": (d, 0), "taps3": (2 * d, d, 0), "taps4": (3 * d, 2 * d, d, 0)}
    if kind in taps:
        return [term(j, s) for j, s in enumerate(taps[kind])]
    if kind == "taps3_by_group":  # dilation 2^group (the WaveNet blocks)
        return [term(j, s, sbg=1) for j, s in enumerate((2 * d, d, 0))]
    if kind == "negative3":  # the transposed conv of the backward data path
        return [term(j, s) for j, s in enumerate((0, -d, -2 * d))]
    if kind == "w_not_spaced":  # one activation, weights not in arithmetic progression: not the taps of one conv
        return [term(0, 2 * d, W=0), term(1, d, W=4096), term(2, 0, W=3 * 4096)]
    if kind in ("sum3", "sum8"):  # different activations (the WaveNet skip contraction)
        return [term(j, 0, A=j) for j in range(int(kind[3:]))]
    raise ValueError(kind)


KINDS = ("single", "single", "taps2", "taps3", "taps3", "taps4", "taps3_by_group", "negative3", "w_not_spaced", "sum3", "sum8")
DTYPES = (_lib.DN_F32, _lib.DN_BF16, _lib.DN_BF16X3, _lib.DN_F16)
EPIS = tuple(range(7))


def sweep():
    rng = np.random.RandomState(20261016)
    rows = []
    Ms = (16, 200, 1024, 4096, 8192, 12288, 16384, 32768)  # 8192: a half batch of [32,512]
    Ns = (512, 768, 1408, 1536, 2048, 57344)  # 57344: the eps-predictor's conditioning projection at dim 512
    Ks = (32, 64, 512, 768, 1408, 2048)
    for dtype in DTYPES:
        for epi in EPIS:
            for M in Ms:
                for N in Ns:
                    for K in Ks:
                        kind = KINDS[rng.randint(len(KINDS))]
                        d = (1, 2, 8, 64)[rng.randint(4)]
                        groups = (1, 8)[rng.randint(2)]
                        layout = KB if rng.rand() < 0.25 else 0
                        ldw = K + 64 if (layout == 0 and rng.rand() < 0.1) else 0
                        norm = (0, 0)
                        if epi in (_lib.EPI_RESADD, _lib.EPI_POSEMB):
                            norm = ((0, 0), (1, 0), (1, 1), (1, 2))[rng.randint(4)]
                        flags = 0
                        if rng.rand() < 0.3:
                            flags |= _lib.GEMM_TWIN
                        if rng.rand() < 0.3:
                            flags |= int(rng.randint(1, 10)) << _lib.GEMM_TILE_SHIFT
                        if rng.rand() < 0.1:
                            flags |= (1, 3, 7, 127)[rng.randint(4)] << _lib.GEMM_BAND_SHIFT
                        if rng.rand() < 0.1:
                            flags |= (_lib.GEMM_TAPS_INNER, _lib.GEMM_TERM_OUTER, _lib.GEMM_NO_SHARED_ROWS)[rng.randint(3)]
                        opts = ((UNSET, 0, 2)[rng.randint(3)], (UNSET, 0)[rng.randint(2)])
                        T = min(M, 512) if rng.rand() < 0.8 else 100
                        T = T if M % T == 0 else M
                        rows.append(row_of(dtype, epi, M, N, K, T, make_terms(kind, d, K, M, groups, layout, ldw), groups, flags, norm, opts))
    # every forced tile on shapes of one denoising step, both layouts, one term and three taps
    for tile in range(10):
        for dtype in DTYPES:
            for epi in EPIS:
                for (M, N, K) in ((16384, 1408, 1408), (8192, 1536, 512), (12288, 768, 768)):
                    for kind in ("single", "taps3"):
                        for layout in (0, KB):
                            rows.append(row_of(dtype, epi, M, N, K, 512, make_terms(kind, 1, K, M, 1, layout), 1, tile << _lib.GEMM_TILE_SHIFT))
    return rows


def eps_step(dim, B, T, dtype, flags, latent=128, heads=8, dim_head=64, wn_layers=8):
    """The contractions of one eps-predictor evaluation (engine.hip eps_core), both layouts where the engine may go K-blocked;
    `flags` is what the caller of eps_core passes down (DN_GEMM_TWIN from the two-stream sampler)."""
    padk = lambda c: (c + 63) // 64 * 64
    M, Dp, zp, hd, ip = B * T, padk(dim), padk(latent), heads * dim_head, padk(int(dim * 4 * 2 / 3))
    tag = lambda t: t << _lib.GEMM_TAG_SHIFT
    BIAS, FILM, RESADD, POSEMB, GEGLU = _lib.EPI_BIAS, _lib.EPI_FILM_GATE, _lib.EPI_RESADD, _lib.EPI_POSEMB, _lib.EPI_GEGLU
    rows = []

    def r(epi, N, K, terms, groups=1, f=0, norm=(0, 0)):
        rows.append(row_of(dtype, epi, M, N, K, T, terms, groups, flags | f, norm))

    for lay in (0, KB) if dtype in (_lib.DN_BF16, _lib.DN_F16) else (0,):
        r(BIAS, Dp, zp, make_terms("single", 0, zp, M, 1))                                        # init conv 1x1
        r(BIAS, Dp, Dp, make_terms("taps3", 1, Dp, M, 1))                                         # WaveNet init conv k = 3
        r(BIAS, Dp, Dp, make_terms("single", 0, Dp, M, wn_layers, lay), wn_layers)               # res convs
        r(FILM, Dp, Dp, make_terms("taps3_by_group", 1, Dp, M, wn_layers, lay), wn_layers, tag(_lib.TAG_WN_DILATED))
        r(BIAS, Dp, Dp, make_terms("sum8", 0, Dp, M, 1)[:wn_layers])                              # skip sum
        r(POSEMB, Dp, Dp, make_terms("single", 0, Dp, M, 1), norm=(1, 1))                         # final 1x1 + positions
        r(BIAS, 3 * hd, Dp, make_terms("single", 0, Dp, M, 1, lay))                               # q/kv
        r(RESADD, Dp, hd, make_terms("single", 0, hd, M, 1), norm=(1, 2 if lay else 1))           # attention out
        r(GEGLU, ip, Dp, make_terms("single", 0, Dp, M, 1, lay))                                  # GEGLU projection
        r(BIAS, ip, ip, make_terms("taps3", 1, ip, M, 1, lay), f=tag(_lib.TAG_FFN_CONV))          # FFN causal conv
        r(RESADD, Dp, ip, make_terms("single", 0, ip, M, 1), norm=(1, 2 if lay else 1))           # FFN out
        r(BIAS, Dp, Dp, make_terms("single", 0, Dp, M, 1))                                        # to_pred
        r(BIAS, latent, Dp, make_terms("single", 0, Dp, M, 1))                                    # final projection
    return rows


def engine_rows():
    rows = []
    for dim, B, T in ((512, 32, 512), (512, 16, 512), (512, 4, 256), (256, 8, 300), (64, 2, 40)):
        for dtype in DTYPES:
            rows += eps_step(dim, B, T, dtype, 0)                                    # one stream
            rows += eps_step(dim, B // 2, T, dtype, _lib.GEMM_TWIN)                  # the two-stream sampler's half batches
    return rows


def build():
    sw, en = sweep(), engine_rows()
    P = np.array(sw + en, dtype=np.int64)
    assert P.min() >= np.iinfo(np.int32).min and P.max() <= np.iinfo(np.int32).max
    return P.astype(np.int32), np.array([0] * len(sw) + [1] * len(en), dtype=np.int8)


def main(out=OUT):
    lib = _lib.load()
    P, engine = build()
    R = answer_all(lib, P, engine)
    np.savez_compressed(out, P=P, R=R, engine=engine)
    print(f"{out}: {len(P)} cases ({int(engine.sum())} engine contractions), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
