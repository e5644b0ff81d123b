"""The 256 x 128 shared-row tile (DN_TILE_256X128_SR) under the folded feed-forward contraction: three taps (shifts 2 / 1 / 0) of one
activation tensor, RESADD in place on an fp32 stream, with and without the split norm's producer -- as an operator against the
term-outer 128 x 128 route and float64, and in a tiny eps-predictor with the route forced (option ffn_fold = 4).

Bound of the operator test: both routes read the same 2-byte operands and accumulate in fp32, so the new route's error against a
float64 evaluation of those operands may be at most twice the term-outer route's error on the same inputs (a different summation
order moves an fp32 sum by a small multiple of its rounding error).  Measured max-abs errors, term-outer -> shared rows, largest
over K, N, norm layout and operand layout (the test prints every case):
  outputs f16 1.64e-6 -> 1.59e-6, bf16 1.44e-6 -> 1.56e-6 (worst single case 1.11 x) | frames 0 and 1: f16 6.04e-7 -> 7.02e-7, bf16 4.52e-7 -> 5.57e-7
  row * gamma f16 3.90e-3 -> 3.90e-3, bf16 3.12e-2 -> 3.12e-2 | sums of squares f16 1.07e-4 -> 1.02e-4, bf16 8.44e-5 -> 1.15e-4 (worst 1.64 x)
  tiny eps-predictor f16 against the float64 oracle: 4.398e-3 on either route."""
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, TINY_EPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FOLD_SR = 4  # option ffn_fold: the folded contraction forced to the shared-row tile


def seeded(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def mods():
    from diffnorm_amd import _lib, engine, ops, packing

    return _lib, engine, ops, packing


# ------------------------------------------------------------------------------------------ 1. the contraction as an operator
# T = 256: tiles start exactly at sequence starts; T = 128: a sequence start inside every tile (the shifted-copies fallback);
# T = 320: tile boundaries off the sequence grid (tile 1 has a start inside, tile 2 is partial in M)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(2, 256), (4, 128), (2, 320)])
def test_shared_row_tile_against_term_outer_and_float64(mods, dtype, B, T):
    _lib, engine, ops, packing = mods
    code = {"f16": _lib.DN_F16, "bf16": _lib.DN_BF16}[dtype]
    adt = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    M = B * T
    t = torch.arange(M) % T
    first2 = t < 2
    for K in (64, 192):  # one K-tile of the term-outer route (two 32-deep chunks here) and an odd count
        a_dev = packing._arith(seeded((M, K), 1), code, weight=False).to(DEV)
        a64 = a_dev.float().cpu().double()
        # the same activations with the last two frames of every sequence replaced: what frames 0 and 1 of the NEXT sequence would
        # pick up if causal padding leaked across a sequence start
        a_poison = a_dev.clone()
        a_poison[(t >= T - 2).to(DEV)] = 1000.0
        for N in (128, 256):  # one and two column tiles
            Ws = [packing._arith(seeded((N, K), 2 + j, (3 * K) ** -0.5), code, weight=True).to(DEV) for j in range(3)]
            Wall = torch.stack(Ws).contiguous()
            Wkb = packing.kblock(Wall)  # [3][K/32][N][32]
            akb, akb_poison = packing.kblock(a_dev), packing.kblock(a_poison)
            bias, x0, gamma = seeded((N,), 7, 0.1), seeded((M, N), 8, 2.0), seeded((N,), 9, 0.2) + 1.0
            want = x0.double() + bias.double()
            for j in range(3):
                src = torch.roll(a64, 2 - j, 0)
                src[t < 2 - j] = 0
                want = want + src @ Ws[j].float().cpu().double().T
            for norm in (0, 1, 2):  # no norm | split-norm producer, row-major | K-blocked

                def run(tile, kb, a=a_dev, a_kb=akb):
                    xd = x0.to(DEV).clone()
                    xg = torch.full((M, N), float("nan"), device=DEV, dtype=adt) if norm else None
                    ssq = torch.full((M, 8), float("nan"), device=DEV) if norm else None
                    terms = [(a_kb, Wkb[j], 2 - j) for j in range(3)] if kb else [(a, Wall[j], 2 - j) for j in range(3)]
                    ops.conv_gemm(terms, xd, T, N, bias=bias.to(DEV), epilogue=_lib.EPI_RESADD, res=xd, tile=tile, a_kblocked=kb, w_kblocked=kb,
                                  norm_out=xg, norm_D=N, norm_gamma=gamma.to(DEV) if norm else None, norm_ssq=ssq, norm_kblocked=norm == 2)
                    rows = None if not norm else (packing.unkblock(xg.view(N // 32, M, 32)) if norm == 2 else xg).float().cpu().double()
                    return xd.cpu(), rows, None if not norm else ssq[:, : N // 64].cpu().double().sum(1)

                old, old_rows, old_ssq = run(_lib.TILE_128X128, False)
                e_old = (old.double() - want).abs()
                for kb in (False, True):
                    new, new_rows, new_ssq = run(_lib.TILE_256X128_SR, kb)
                    e_new = (new.double() - want).abs()
                    print(f"{dtype} B={B} T={T} K={K} N={N} norm {norm} kblocked {kb}: max err term-outer {e_old.max().item():.3e}, shared rows {e_new.max().item():.3e}"
                          f" | first two frames {e_old[first2].max().item():.3e}, {e_new[first2].max().item():.3e}")
                    assert e_new.max() <= 2 * e_old.max(), (K, N, norm, kb)
                    assert e_new[first2].max() <= 2 * e_old[first2].max(), (K, N, norm, kb)  # causal padding: frames 0 and 1 of every sequence
                    if norm:
                        ref_g, ref_s = want * gamma.double(), (want ** 2).sum(1)
                        g_old, g_new = (old_rows - ref_g).abs().max(), (new_rows - ref_g).abs().max()
                        s_old, s_new = (old_ssq - ref_s).abs().max(), (new_ssq - ref_s).abs().max()
                        print(f"    row * gamma: {g_old.item():.3e}, {g_new.item():.3e} | sums of squares: {s_old.item():.3e}, {s_new.item():.3e}")
                        assert g_new <= 2 * g_old and s_new <= 2 * s_old, (K, N, norm, kb)
                    if kb:  # the operand layout does not change the K order: the same bits as from row-major operands
                        assert torch.equal(new, keep[0]) and (not norm or (torch.equal(new_rows, keep[1]) and torch.equal(new_ssq, keep[2])))
                    keep = (new, new_rows, new_ssq)
                    # frames 0 and 1 of a sequence read nothing of the sequence before it: exactly the same bits after its end changed
                    leak, _, _ = run(_lib.TILE_256X128_SR, kb, a_poison, akb_poison)
                    assert torch.equal(leak[first2], new[first2]), (K, N, norm, kb)
                    assert not torch.equal(leak[t == T - 1], new[t == T - 1])


def test_the_route_query_names_the_tile(mods):
    """dn_conv_gemm_route: the forced tile runs tap-inner with shared rows where it applies; term-outer keeps the contraction off it."""
    import ctypes as C

    _lib, engine, ops, packing = mods
    lib = _lib.load()

    def route(dtype, epilogue, flags, shifts=(2, 1, 0)):
        p = _lib.GemmParams()
        p.dtype, p.epilogue, p.M, p.N, p.K, p.T, p.groups, p.n_terms = dtype, epilogue, 8192, 512, 1408, 512, 1, 3
        p.flags = (_lib.TILE_256X128_SR << _lib.GEMM_TILE_SHIFT) | flags
        for j, s in enumerate(shifts):
            p.terms[j].A, p.terms[j].W, p.terms[j].lda, p.terms[j].shift = 1 << 30, (1 << 40) + j * 512 * 1408 * 2, 1408, s
        r = _lib.GemmRoute()
        _lib.check(lib.dn_conv_gemm_route(C.byref(p), C.byref(r)), "dn_conv_gemm_route")
        return r.tile, r.taps_inner, r.shared_rows

    for dtype in (_lib.DN_F16, _lib.DN_BF16):
        assert route(dtype, _lib.EPI_RESADD, 0) == (_lib.TILE_256X128_SR, 1, 1)
        assert route(dtype, _lib.EPI_RESADD, _lib.GEMM_TERM_OUTER)[0] != _lib.TILE_256X128_SR
        assert route(dtype, _lib.EPI_RESADD, 0, shifts=(0, 0, 0))[0] != _lib.TILE_256X128_SR
        assert route(dtype, _lib.EPI_BIAS, 0)[0] != _lib.TILE_256X128_SR
    assert route(_lib.DN_F32, _lib.EPI_RESADD, 0)[0] != _lib.TILE_256X128_SR


# ------------------------------------------------------------------------------------------ 2. a tiny eps-predictor on the new route
def test_eps_engine_on_the_shared_row_route(mods, hip_option, golden):
    """f16, the inputs and the bar of test_hip_ffn_fold.py's tiny case (t = 3, 500, 999; tests/test_hip_engine.py's 1e-2): the folded
    contraction forced to the shared-row tile with K-blocked operands; graph, eager and split chains agree bit for bit."""
    _lib, engine, ops, packing = mods
    sd = O.make_eps_state_dict(TINY_EPS, "tiny")
    sd64 = {k: v.double() for k, v in sd.items()}
    g = golden("eps_tiny")
    x, t, lens = (torch.from_numpy(g[k]) for k in ("x", "t", "lens"))
    assert t.tolist() == [3, 500, 999]
    mask = O.lengths_to_mask(lens, x.shape[1])
    want = O.eps_forward(sd64, TINY_EPS, x.double(), t, mask)
    e = engine.EpsEngine(sd, TINY_EPS, dtype="f16", device=DEV)
    assert e.fold_Wkb is not None and torch.equal(packing.unkblock(e.fold_Wkb), e.fold_W)  # the same bits in the other layout
    xd = x.to(DEV)
    hip_option("ffn_fold", 1)
    table = e.forward(xd, t, lens).cpu()
    hip_option("ffn_fold", FOLD_SR)
    on = e.forward(xd, t, lens).cpu()
    hip_option("kblock", 0)  # the same tile on row-major operands: the same K order, the same bits
    assert torch.equal(on, e.forward(xd, t, lens).cpu())
    hip_option("kblock", None)
    err_on, err_table = (on.double() - want)[mask].abs().max().item(), (table.double() - want)[mask].abs().max().item()
    print(f"eps tiny f16: max abs err vs float64 oracle: term-outer route {err_table:.3e}, shared-row route {err_on:.3e}")
    assert not torch.equal(on, table)  # another summation order: the route is really taken
    assert err_on < 1e-2
    from diffnorm_amd import scheduler

    coef = scheduler.DDPMScheduler(200).ddim_coef_table(DEV)
    l32 = lens.to(DEV).int()
    runs = {}
    for name, kw in (("graph", dict(use_graph=True, split=False)), ("eager", dict(use_graph=False, split=False)), ("split", dict(use_graph=True, split=True))):
        xs = xd.clone()
        e.ddim_loop(xs, l32, 6, coef, **kw)
        runs[name] = xs.cpu()
    assert torch.equal(runs["graph"], runs["eager"]) and torch.equal(runs["graph"], runs["split"]) and torch.isfinite(runs["graph"]).all()
    hip_option("ffn_fold", 1)  # the option is part of the captured step's key
    xs = xd.clone()
    e.ddim_loop(xs, l32, 6, coef, use_graph=True, split=False)
    assert not torch.equal(xs.cpu(), runs["graph"])


def test_refreshed_engine_equals_a_fresh_one_on_the_shared_row_route(mods, hip_option):
    _lib, engine, ops, packing = mods
    from diffnorm_amd import training

    c = CHAIN_VAE
    vae = training.VaeTrainEngine(O.make_vae_state_dict(c, "train"), dim=c.dim, latent_dim=c.latent_dim, dtype="f32", device=DEV, depth=c.depth,
                                  heads=c.heads, dim_head=c.dim_head, stacks=c.stacks, layers=c.layers)
    sd0 = O.make_eps_state_dict(CHAIN_EPS, "train")
    te = training.EpsTrainEngine(sd0, CHAIN_EPS, vae, timesteps=200, dtype="f32", device=DEV)
    e = engine.EpsEngine(sd0, CHAIN_EPS, dtype="f16", device=DEV)
    before = e.fold_Wkb.clone()
    te.master.mul_(1.0 + 0.25 * torch.sin(torch.arange(te.n_params, device=DEV, dtype=torch.float32)))  # changed master weights
    e.refresh_from(te)
    fresh = engine.EpsEngine(te.state_dict(), CHAIN_EPS, dtype="f16", device=DEV)
    same = lambda a, b: torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert not same(before, e.fold_Wkb)
    assert same(e.fold_W, fresh.fold_W) and same(e.fold_Wkb, fresh.fold_Wkb) and torch.equal(e.fold_b, fresh.fold_b)
    assert torch.equal(packing.unkblock(e.fold_Wkb), e.fold_W)
    hip_option("ffn_fold", FOLD_SR)
    x, lens, t = seeded((2, 40, CHAIN_EPS.latent_dim), 5).to(DEV), torch.tensor([40, 27]), torch.tensor([7, 400])
    got, want = e.forward(x, t, lens).cpu(), fresh.forward(x, t, lens).cpu()
    assert torch.isfinite(got).all() and torch.equal(got, want)
