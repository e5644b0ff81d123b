"""The folded feed-forward contraction on the GPU: dn_ffn_fold's weights against their float64 restatement, the three-tap RESADD
contraction as an operator on every tile, the engines with the fold on against the fold off and against the float64 oracle, the
refresh paths, the workspace plan and the launch tag.

Measured max-abs errors against the float64 oracle, fold off -> fold on (the test prints both per mode before it asserts the fold-on
figure at the mode's existing bar):
  tiny eps-predictor, t in {3, 500, 999}: f32 6.069e-5 -> 6.075e-5 | bf16x3 6.71e-5 -> 6.37e-5 | f16 4.32e-3 -> 4.40e-3 | bf16 3.34e-2 -> 3.23e-2
  small VAE decode:                       f32 1.52e-6 -> 1.94e-6   | bf16x3 2.03e-5 -> 2.09e-5 | f16 1.48e-3 -> 1.52e-3 | bf16 1.03e-2 -> 0.99e-2
  stored W' against float64 (|W'| <= 0.066): f32 3.1e-8 | bf16x3 2.5e-7 | f16 2.7e-5 | bf16 1.2e-4"""
import ctypes as C

import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_VAE, TINY_EPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["f32", "bf16x3", "f16", "bf16"]
# the engines' existing bars (tests/test_hip_engine.py); bf16 at t = 500 / 999: the measured-plus-15 % bar stated there
BAR = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 3.9e-2}
# unit roundoff of a mode's stored weight: fp32; hi + lo bf16 (16 significant bits); half; bf16
ULP = {"f32": 2.0 ** -24, "bf16x3": 2.0 ** -16, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}


def seeded(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def mods():
    from diffnorm_amd import _lib, engine, ops, packing

    return _lib, engine, ops, packing


def _stored(packing, _lib, t, dtype):
    """fp32 values of a tensor in a mode's weight storage."""
    if dtype == "bf16x3":
        return packing.unsplit_rows(t.cpu())
    return t.float().cpu()


def _tf_sd(sd, l, prefix="transformer."):
    p = f"{prefix}layers.{l}.5."
    return sd[p + "2.1.weight"], sd[p + "2.1.bias"], sd[p + "3.weight"], sd[p + "3.bias"]


# ------------------------------------------------------------------------------------------ 1. the fold entry
@pytest.mark.parametrize("dtype", MODES)
def test_fold_entry_against_float64(mods, dtype):
    _lib, engine, ops, packing = mods
    sd = O.make_eps_state_dict(TINY_EPS, "tiny")
    e = engine.EpsEngine(sd, TINY_EPS, dtype=dtype, device=DEV)
    D, inner = TINY_EPS.dim, int(TINY_EPS.dim * 4 * 2 / 3)
    W, b = _stored(packing, _lib, e.fold_W, dtype), e.fold_b.cpu()
    assert W.shape == (TINY_EPS.depth, 3, packing.padn(D), packing.padk(inner)) and b.shape == (TINY_EPS.depth, packing.padk(D))
    assert W[:, :, D:].abs().sum() == 0 and W[:, :, :, inner:].abs().sum() == 0 and b[:, D:].abs().sum() == 0
    for l in range(TINY_EPS.depth):
        cw, cb, ow, ob = _tf_sd(sd, l)
        Wf, bf = packing.ffn_fold_ref(cw, cb, ow, ob)
        # one rounding of the exact value into the format, plus the fp32 sum of `inner` products behind it (any order)
        S = torch.stack([ow.double().abs() @ cw[:, :, j].double().abs() for j in range(3)])
        err = (W[l, :, :D, :inner].double() - Wf).abs()
        bound = ULP[dtype] * Wf.abs() + inner * 2.0 ** -24 * S + (2.0 ** -25 if dtype == "f16" else 0.0)  # f16: subnormal spacing
        print(f"fold_W {dtype} layer {l}: max err {err.max().item():.3e}, max |W'| {Wf.abs().max().item():.3e}")
        assert (err <= bound).all(), (dtype, l, (err - bound).max().item())
        Sb = ow.double().abs() @ cb.double().abs() + ob.double().abs()
        assert ((b[l, :D].double() - bf).abs() <= (inner + 1) * 2.0 ** -24 * Sb).all()
    # two calls give identical bytes (a second engine: same sources, same entry)
    e2 = engine.EpsEngine(sd, TINY_EPS, dtype=dtype, device=DEV)
    assert torch.equal(e.fold_W.view(torch.uint8), e2.fold_W.view(torch.uint8)) and torch.equal(e.fold_b, e2.fold_b)


# ------------------------------------------------------------------------------------------ 2. the contraction as an operator
def _operands(packing, _lib, dtype, t, weight):
    code = {"f32": _lib.DN_F32, "bf16x3": _lib.DN_BF16X3, "f16": _lib.DN_F16, "bf16": _lib.DN_BF16}[dtype]
    dev = packing._arith(t, code, weight=weight).to(DEV)
    return dev, _stored(packing, _lib, dev, dtype).double()


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("B,T,K,N", [(3, 100, 128, 64), (2, 515, 192, 128), (2, 300, 1408, 512)])
def test_folded_contraction_operator(mods, dtype, B, T, K, N):
    """Three taps (shifts 2/1/0) of one activation tensor, RESADD in place on an fp32 stream, split-norm producer on: every tile,
    both norm layouts, against float64.  M = B T is ragged on every tile, sequences start inside tiles, and T = 100 is shorter than
    a tile."""
    _lib, engine, ops, packing = mods
    M, x3 = B * T, dtype == "bf16x3"
    adt = {"f32": torch.float32, "bf16x3": torch.bfloat16, "f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    a_dev, a64 = _operands(packing, _lib, dtype, seeded((M, K), 1), False)
    Ws = [_operands(packing, _lib, dtype, torch.nn.functional.pad(seeded((N, K), 2 + j, (3 * K) ** -0.5), (0, 0, 0, (N + 255) // 256 * 256 - N)), True) for j in range(3)]
    Wall = torch.stack([w for w, _ in Ws]).contiguous()
    bias, x0, gamma = seeded((N,), 7, 0.1), seeded((M, N), 8, 2.0), seeded((N,), 9, 0.2) + 1.0
    t = torch.arange(M) % T
    want, S = x0.double() + bias.double(), x0.double().abs() + bias.double().abs()
    for j in range(3):
        src = torch.roll(a64, 2 - j, 0)
        src[t < 2 - j] = 0
        want = want + src @ Ws[j][1][:N].T
        S = S + src.abs() @ Ws[j][1][:N].abs().T
    # fp32 accumulation of 3 K products and the epilogue's additions, any order; split operands drop the lo . lo products
    bound = ((3 * K + 2) * 2.0 ** -24 + (2.0 ** -16 if x3 else 0.0)) * S
    outs = {}
    for tile in (0, _lib.TILE_128X128, _lib.TILE_256X128, _lib.TILE_256X256):
        for kb in ((False, True) if dtype in ("f16", "bf16") else (False,)):
            xd = x0.to(DEV).clone()
            xg = torch.full((M, 2 * N if x3 else N), float("nan"), device=DEV, dtype=adt)
            ssq = torch.full((M, max(8, N // 64)), float("nan"), device=DEV)
            ops.conv_gemm([(a_dev, Wall[j], 2 - j) for j in range(3)], xd, T, N, bias=bias.to(DEV), epilogue=_lib.EPI_RESADD, res=xd, tile=tile,
                          norm_out=xg, norm_D=N, norm_gamma=gamma.to(DEV), norm_ssq=ssq, norm_kblocked=kb, x3=x3)
            got = xd.cpu().double()
            err = (got - want).abs()
            print(f"{dtype} M={M} K={K} N={N} tile {tile} kblocked {kb}: max err {err.max().item():.3e} (bound {bound.max().item():.3e})")
            assert (err <= bound).all(), (tile, kb, (err - bound).max().item())
            rows = packing.unkblock(xg.view(N // 32, M, 32)) if kb else xg
            g = _stored(packing, _lib, rows, dtype).double()
            ref_g = got * gamma.double()
            assert ((g - ref_g).abs() <= ULP[dtype] * ref_g.abs() + (2.0 ** -25 if dtype == "f16" else 1e-30)).all()  # (f16: subnormal spacing)
            assert ((ssq[:, : N // 64].cpu().double().sum(1) - (got ** 2).sum(1)).abs() <= 1e-5 * (got ** 2).sum(1)).all()
            outs[(tile, kb)] = (xd.cpu(), rows.cpu())
    # same K order (the 128-byte-K-tile kernel at two heights; either norm layout): the same bits
    for kb in (k for (tl, k) in outs if tl == 0):
        assert torch.equal(outs[(_lib.TILE_128X128, kb)][0], outs[(_lib.TILE_256X128, kb)][0])
        assert torch.equal(outs[(_lib.TILE_128X128, kb)][1], outs[(_lib.TILE_256X128, kb)][1])
    for tile in (0, _lib.TILE_128X128, _lib.TILE_256X128, _lib.TILE_256X256):
        if (tile, True) in outs:
            assert torch.equal(outs[(tile, False)][0], outs[(tile, True)][0]) and torch.equal(outs[(tile, False)][1], outs[(tile, True)][1])


# ------------------------------------------------------------------------------------------ 3. the engines, fold on against fold off
@pytest.mark.parametrize("dtype", MODES)
def test_eps_engine_fold_on_off(mods, dtype, hip_option, golden):
    """The inputs of test_hip_engine.py's tiny case (t = 3, 500, 999), whose bars these are.  DN_BF16 engines default to the
    two-stage form (the fold misses test_hip_bf16_model.py's 2e-3 engine-against-emulation bar by 3 %: DESIGN 11); the fold is
    still asserted there, switched on through the option."""
    _lib, engine, ops, packing = mods
    sd = O.make_eps_state_dict(TINY_EPS, "tiny")
    sd64 = {k: v.double() for k, v in sd.items()}
    g = golden("eps_tiny")
    x, t, lens = (torch.from_numpy(g[k]) for k in ("x", "t", "lens"))
    assert t.tolist() == [3, 500, 999]
    B, T = x.shape[0], x.shape[1]
    mask = O.lengths_to_mask(lens, T)
    want = O.eps_forward(sd64, TINY_EPS, x.double(), t, mask)
    e = engine.EpsEngine(sd, TINY_EPS, dtype=dtype, device=DEV)
    xd = x.to(DEV)
    if dtype == "bf16":
        dflt = e.forward(xd, t, lens).cpu()
        hip_option("ffn_fold", 0)
        assert torch.equal(dflt, e.forward(xd, t, lens).cpu())
    hip_option("ffn_fold", 1)
    on = e.forward(xd, t, lens).cpu()
    ws_on = e.workspace_bytes(B, T)
    hip_option("ffn_fold", 0)
    off = e.forward(xd, t, lens).cpu()  # same engine, same buffers: the option switches the form
    ws_off = e.workspace_bytes(B, T)
    hip_option("ffn_fold", 1)
    on2 = e.forward(xd, t, lens).cpu()
    err_on, err_off = (on.double() - want)[mask].abs().max().item(), (off.double() - want)[mask].abs().max().item()
    print(f"eps tiny {dtype}: max abs err vs float64 oracle: fold off {err_off:.3e}, fold on {err_on:.3e}, on vs off {(on - off).abs().max().item():.3e}")
    assert torch.equal(on, on2) and not torch.equal(on, off)
    assert err_on < BAR[dtype]
    # 5. workspace: the conv's output buffer leaves the plan (its 256-byte-aligned size)
    fc = (B * T * packing.padk(int(TINY_EPS.dim * 4 * 2 / 3)) * (2 if dtype in ("f16", "bf16") else 4) + 255) // 256 * 256
    assert ws_off - ws_on == fc
    # graph, eager and split chains with the fold on agree bit for bit; switching the option re-captures (the cache key)
    from diffnorm_amd import scheduler

    coef = scheduler.DDPMScheduler(200).ddim_coef_table(DEV)
    l32 = lens.to(DEV).int()
    runs = {}
    for name, kw in (("graph", dict(use_graph=True, split=False)), ("eager", dict(use_graph=False, split=False)), ("split", dict(use_graph=True, split=True))):
        xs = xd.clone()
        e.ddim_loop(xs, l32, 6, coef, **kw)
        runs[name] = xs.cpu()
    assert torch.equal(runs["graph"], runs["eager"]) and torch.equal(runs["graph"], runs["split"]) and torch.isfinite(runs["graph"]).all()
    hip_option("ffn_fold", 0)
    xs = xd.clone()
    e.ddim_loop(xs, l32, 6, coef, use_graph=True, split=False)
    xe = xd.clone()
    e.ddim_loop(xe, l32, 6, coef, use_graph=False, split=False)
    assert torch.equal(xs.cpu(), xe.cpu()) and not torch.equal(xs.cpu(), runs["graph"])
    hip_option("ffn_fold", 1)
    xs = xd.clone()
    e.ddim_loop(xs, l32, 6, coef, use_graph=True, split=False)
    assert torch.equal(xs.cpu(), runs["graph"])
    hip_option("ffn_fold", None)


@pytest.mark.parametrize("dtype", MODES)
def test_vae_engine_fold_on_off(mods, dtype, hip_option):
    _lib, engine, ops, packing = mods
    vsd = O.make_vae_state_dict(CHAIN_VAE, "chain")
    v64 = {k: v.double() for k, v in vsd.items()}
    B, T = 2, 40
    z, lens = seeded((B, T, CHAIN_VAE.z), 6), torch.tensor([40, 27])
    mask = O.lengths_to_mask(lens, T)
    r_ref, l_ref = O.vae_decode(v64, CHAIN_VAE, z.double(), mask)
    ve = engine.VaeEngine(vsd, dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype, device=DEV)
    errs = {}
    for fold in (1, 0):
        hip_option("ffn_fold", fold)  # (explicit in DN_BF16 too, whose engines default to the two-stage form)
        recon, logits, _ = ve.decode(z.to(DEV), lens)
        errs[fold] = max((recon.cpu().double() - r_ref)[mask].abs().max().item(), (logits.cpu().double() - l_ref)[mask].abs().max().item())
    print(f"vae small {dtype}: max abs err vs float64 oracle: fold off {errs[0]:.3e}, fold on {errs[1]:.3e}")
    assert errs[1] < {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 2e-2}[dtype]


# ------------------------------------------------------------------------------------------ 4. refresh
@pytest.mark.parametrize("source", ["model", "ema"])
def test_refresh_rebuilds_the_folded_weights(mods, source):
    _lib, engine, ops, packing = mods
    from diffnorm_amd import training

    vsd = O.make_vae_state_dict(CHAIN_VAE, "chain")
    te = training.VaeTrainEngine(vsd, dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32", device=DEV)
    if source == "ema":
        te.enable_ema()
    te.master.mul_(1.0 + 0.25 * torch.sin(torch.arange(te.n_params, device=DEV, dtype=torch.float32)))  # changed master weights
    if source == "ema":
        te.ema.copy_(te.master * 0.5)
    for dtype in ("f16", "bf16x3"):
        ve = engine.VaeEngine(vsd, dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype, device=DEV)
        before = ve.fold_W.clone()
        ve.refresh_from(te, source=source)
        new_sd = packing.unpack_flat(te.master if source == "model" else te.ema, te.entries, te.offsets)
        fresh = engine.VaeEngine(new_sd, dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype, device=DEV)
        assert not torch.equal(before.view(torch.uint8), ve.fold_W.view(torch.uint8))
        assert torch.equal(ve.fold_W.view(torch.uint8), fresh.fold_W.view(torch.uint8)) and torch.equal(ve.fold_b, fresh.fold_b)


# ------------------------------------------------------------------------------------------ 5. the launch tag
def test_folded_launches_carry_the_ffn_conv_tag(mods):
    _lib, engine, ops, packing = mods
    sd = O.make_eps_state_dict(TINY_EPS, "tiny")
    e = engine.EpsEngine(sd, TINY_EPS, dtype="f16", device=DEV)
    x, lens, t = seeded((2, 40, TINY_EPS.latent_dim), 5).to(DEV), torch.tensor([40, 27]), torch.tensor([7, 7])
    k = 3
    lib = _lib.load()
    _lib.check(lib.dn_profile_start(_lib.TAG_FFN_CONV, TINY_EPS.depth * k), "dn_profile_start")
    for _ in range(k):
        e.forward(x, t, lens)
    torch.cuda.synchronize()
    ms, n = C.c_float(), C.c_int32()
    _lib.check(lib.dn_profile_stop(C.byref(ms), C.byref(n)), "dn_profile_stop")
    assert n.value == TINY_EPS.depth * k and ms.value > 0
