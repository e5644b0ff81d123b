"""The engines past T = 1024, up to the end of the 2049-row positional table, against oracle/diffnorm_oracle.py evaluated in float64
here: EpsEngine.forward in every arithmetic mode, the VAE engines, the captured DDIM loops and the diffusion training engine.  The
eps-predictor is LONG_EPS: the tiny width with the recipe's eight WaveNet layers, so the dilated convs shift by up to 256 rows -- one
256-row tile -- and tiles carry sequence starts inside them.

Bars come from the reference side.  f32 / bf16x3: the project's flat 1e-3, and where the float32 oracle itself is further than 1e-3 / 8
from float64 (t = 500 / 999: random-init gains of 10-30 on the raw integer timestep) 8 x that distance -- the factor
tests/test_hip_vocoder.py and tests/test_hip_nar_widths.py grant another summation order plus the device transcendentals.  f16 / bf16: the
flat budget, and at t = 500 / 999 3 x the distance of the rounding-points model (oracle/bf16_emulation.py) from float64 where that is
larger (test_hip_vocoder.py's factor).  Every reference is computed once per module; every case prints what it measured.

Measured on an MI355X (max abs error on the valid frames; bar; reference-side error), [2, 2048] with lengths 2048 / 1337: DESIGN.md 3."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import bf16_emulation as E
import diffnorm_oracle as O
import train_oracle as TO
from gen_golden_configs import CHAIN_VAE, LONG_EPS, seeded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["f32", "bf16x3", "f16", "bf16"]
EXACT = ("f32", "bf16x3")
FLAT = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 1e-2}
VAE_BUDGET = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 2e-2}  # bf16: test_hip_engine.py's figure for the VAE goldens
F32_FACTOR, MODEL_FACTOR = 8, 3
SHAPES = {"full": (2, 2048, (2048, 1337)),        # the table's last row; 1337 ends inside a key tile and inside a 256-row tile
          "starts": (3, 2047, (2047, 1, 1100)),   # sequence starts inside tiles, a one-frame utterance
          "first": (2, 1025, (1025, 600))}        # the first length never run
TIMES = (3, 500, 999)
SEEDS = {"full": 11, "starts": 12, "first": 13}


def _double(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def _maxerr(a, b, mask):
    return float((a.double() - b.double())[mask].abs().max())


@functools.lru_cache(maxsize=None)
def _eps_weights():
    sd = O.make_eps_state_dict(LONG_EPS, "long")
    return sd, _double(sd)


@functools.lru_cache(maxsize=None)
def _eps_input(shape):
    B, T, lens = SHAPES[shape]
    lens = torch.tensor(lens)
    return seeded((B, T, LONG_EPS.latent_dim), SEEDS[shape]), lens, O.lengths_to_mask(lens, T)


def _eps_reference(x, t, mask, cfg=LONG_EPS):
    """float64 oracle and the distance from it of the float32 oracle and of the two rounding-points models, on the valid frames."""
    sd, sd64 = _eps_weights()
    times = torch.full((x.shape[0],), t)
    with torch.no_grad():
        ref = O.eps_forward(sd64, cfg, x.double(), times, mask)
        e32 = _maxerr(O.eps_forward(sd, cfg, x, times, mask), ref, mask)
        model = {k: _maxerr(E.eps_forward(sd, cfg, x, times, mask, R=E.Rounder(kind=k, count=False)), ref, mask) for k in ("f16", "bf16")}
    return dict(ref=ref, e32=e32, e_model=model, scale=float(ref[mask].abs().max()))


@functools.lru_cache(maxsize=None)
def _eps_ref(shape, t):
    x, _, mask = _eps_input(shape)
    return _eps_reference(x, t, mask)


@functools.lru_cache(maxsize=None)
def _eps_engine(dtype, max_pos=2048):
    from diffnorm_amd import engine

    return engine.EpsEngine(_eps_weights()[0], LONG_EPS, dtype=dtype, device=DEV, max_pos=max_pos)


def _eps_bar(dtype, t, r):
    """(bar, reference-side error) of a mode at timestep t."""
    side = r["e32"] if dtype in EXACT else r["e_model"][dtype]
    if t == 3:
        return FLAT[dtype], side
    return max(FLAT[dtype], (F32_FACTOR if dtype in EXACT else MODEL_FACTOR) * side), side


def _report(what, dtype, err, bar, side):
    name = "float32 oracle" if dtype in EXACT else "rounding-points model"
    print(f"{what} {dtype}: max abs err {err:.3e}  bar {bar:.3e}  {name} {side:.3e}  err / reference-side {err / max(side, 1e-300):.2f}")


def _forward(dtype, shape, t, x=None):
    xs, lens, _ = _eps_input(shape)
    x = xs if x is None else x
    return _eps_engine(dtype).forward(x.to(DEV), torch.full((x.shape[0],), t), lens).cpu()


# ----------------------------------------------------------------------------------------------------- 1. EpsEngine.forward at long T
@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_eps_forward_past_1024_frames(shape, t, dtype):
    """dn_eps_forward (per-sample timesteps) against O.eps_forward in float64 on the valid frames."""
    r = _eps_ref(shape, t)
    mask = _eps_input(shape)[2]
    got = _forward(dtype, shape, t)
    err = _maxerr(got, r["ref"], mask)
    bar, side = _eps_bar(dtype, t, r)
    B, T, lens = SHAPES[shape]
    _report(f"eps [{B}, {T}] lens {list(lens)} t = {t} (scale {r['scale']:.2f}),", dtype, err, bar, side)
    assert bool(torch.isfinite(got[mask]).all()) and err < bar


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_an_utterance_alone_and_inside_the_long_batch(dtype):
    """The 1337-frame utterance at T = 1337 on its own and as the second row of the [2, 2048] batch, at t = 3 -- where the gains are O(1)
    and test_eps_properties' absolute 1e-6 means what it means at T = 70.  f32: 1e-6; f16: bit-equal, or else within 3 x the
    rounding-points model's distance from float64 (printed)."""
    x, lens, mask = _eps_input("full")
    n = int(lens[1])
    batch = _forward(dtype, "full", 3)[1, :n]
    alone = _eps_engine(dtype).forward(x[1:2, :n].contiguous().to(DEV), torch.tensor([3]), lens[1:2]).cpu()[0]
    diff = float((alone.double() - batch.double()).abs().max())
    side = _eps_ref("full", 3)["e_model"]["f16"]
    print(f"alone (T = {n}) against row 1 of [2, 2048], {dtype}: max abs difference {diff:.3e}" +
          (f"  (3 x rounding-points model {MODEL_FACTOR * side:.3e})" if dtype == "f16" else ""))
    if dtype == "f32":
        assert diff < 1e-6
    elif not torch.equal(alone, batch):
        assert diff < MODEL_FACTOR * side


@pytest.mark.parametrize("dtype", MODES)
def test_padding_is_not_read_at_long_lengths(dtype):
    """1e3 in the padded frames of [3, 2047] (lengths 2047 / 1 / 1100): the valid frames do not change by a bit."""
    x, _, mask = _eps_input("starts")
    a = _forward(dtype, "starts", 500)
    x2 = x.clone()
    x2[~mask] = 1e3
    b = _forward(dtype, "starts", 500, x2)
    assert torch.equal(a[mask], b[mask])


def _dilated_route(dtype_code, B, T):
    """dn_conv_gemm_route of the WaveNet's grouped dilated contraction (engine.hip run_wavenet, K-blocked operands, stacks >= 1) at
    LONG_EPS: eight groups, group g shifted by (2, 1, 0) << g -- group 7 is the dilation-128 conv, a shift of 256 rows."""
    from diffnorm_amd import _lib

    cp, M, L = 64, B * T, LONG_EPS.wavenet_layers
    p = _lib.GemmParams()
    p.dtype, p.M, p.N, p.K, p.T, p.groups, p.n_terms, p.epilogue = dtype_code, M, cp, cp, T, L, 3, _lib.EPI_FILM_GATE
    p.flags = _lib.TAG_WN_DILATED << _lib.GEMM_TAG_SHIFT
    for j in range(3):
        t = p.terms[j]
        t.A, t.W, t.lda, t.shift, t.shift_by_group = 1 << 28, (1 << 44) + j * cp * cp * 2, cp, 2 - j, 1
        t.a_gstride, t.w_gstride, t.layout = M * cp, 3 * cp * cp, _lib.LAYOUT_A_KBLOCKED | _lib.LAYOUT_W_KBLOCKED
    r = _lib.GemmRoute()
    _lib.check(_lib.load().dn_conv_gemm_route(C.byref(p), C.byref(r)), "dn_conv_gemm_route")
    return r


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_kblocked_buffers_with_a_shift_of_one_whole_tile(dtype, hip_option):
    """test_kblocked_buffers_are_bit_identical's assertion at [3, 2047] with dilations 64 and 128 and sequence starts inside the 256-row
    tiles: term-outer K order everywhere (taps_inner = 0), row-major buffers (kblock = 0) against K-blocked ones on the 256 x 256 tile
    (kblock = 1), bit for bit.  The route of the grouped dilated contraction is pinned so that the case cannot move to another tile
    unnoticed: under kblock = 1 it is the 256 x 256 tile, with shared staged rows in the default K order -- and WITHOUT them under
    taps_inner = 0, which this bit comparison needs (rows are shared between taps only in the tap-inner order); the shared-row
    kernel itself runs in test_shared_row_tiles_with_a_shift_of_one_whole_tile."""
    from diffnorm_amd import _lib, engine

    B, T, _ = SHAPES["starts"]
    code = {"f16": _lib.DN_F16, "bf16": _lib.DN_BF16}[dtype]
    hip_option("taps_inner", 1)
    r = _dilated_route(code, B, T)
    assert (r.tile, r.taps_inner, r.shared_rows) == (_lib.TILE_256X256, 1, 1)
    hip_option("taps_inner", 0)
    r = _dilated_route(code, B, T)
    assert (r.tile, r.taps_inner, r.shared_rows) == (_lib.TILE_256X256, 0, 0)
    x, lens, mask = _eps_input("starts")
    times = torch.tensor(TIMES)
    outs = []
    for mode in (0, 1):
        hip_option("kblock", mode)
        e = engine.EpsEngine(_eps_weights()[0], LONG_EPS, dtype=dtype, device=DEV)
        outs.append(e.forward(x.to(DEV), times, lens).cpu())
    hip_option("kblock", None)
    hip_option("taps_inner", None)
    assert torch.equal(outs[0], outs[1])
    assert bool(torch.isfinite(outs[0][mask]).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_shared_row_tiles_with_a_shift_of_one_whole_tile(dtype, hip_option):
    """The kernel the route above names, run: default (tap-inner) K order and kblock = 1 put the grouped dilated conv of [3, 2047] on the
    256 x 256 tile with shared staged rows -- groups 0-6 share the rows of a tile and its halo (128 rows at dilation 64) unless a
    sequence starts inside the tile, group 7 (256 halo rows) and the tiles around frames 2047 and 2048 of the batch take the
    shifted-copies loop of the same kernel.  Another K order than the row-major run's, so no bit comparison: float64 parity at
    section 1's t = 3 bar."""
    from diffnorm_amd import engine

    hip_option("taps_inner", 1)
    hip_option("kblock", 1)
    x, lens, mask = _eps_input("starts")
    e = engine.EpsEngine(_eps_weights()[0], LONG_EPS, dtype=dtype, device=DEV)
    got = e.forward(x.to(DEV), torch.full((x.shape[0],), 3), lens).cpu()
    hip_option("kblock", None)
    hip_option("taps_inner", None)
    r = _eps_ref("starts", 3)
    err = _maxerr(got, r["ref"], mask)
    bar, side = _eps_bar(dtype, 3, r)
    _report("eps [3, 2047] t = 3, K-blocked, shared staged rows,", dtype, err, bar, side)
    assert err < bar


def test_the_end_of_the_positional_table():
    """T = max_pos reads row T of the (T + 1)-row table; T = max_pos + 1 is refused before anything is launched -- at the recipe's
    2048 and at a second table size, 300, where T = 300 also passes section 1's f32 bar at t = 3."""
    from diffnorm_amd import _lib

    e = _eps_engine("f32")
    x = seeded((1, 2049, LONG_EPS.latent_dim), 14).to(DEV)
    out = torch.full_like(x, 7.0)
    with pytest.raises(_lib.DiffNormHipError):
        e.forward(x, torch.tensor([3]), torch.tensor([2049]), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    short = _eps_engine("f32", 300)
    lens = torch.tensor([300, 123])
    x = seeded((2, 300, LONG_EPS.latent_dim), 15)
    mask = O.lengths_to_mask(lens, 300)
    r = _eps_reference(x, 3, mask)
    got = short.forward(x.to(DEV), torch.full((2,), 3), lens).cpu()
    err = _maxerr(got, r["ref"], mask)
    _report("eps [2, 300] on a 301-row table, t = 3,", "f32", err, FLAT["f32"], r["e32"])
    assert err < FLAT["f32"]
    x = seeded((1, 301, LONG_EPS.latent_dim), 16).to(DEV)
    out = torch.full_like(x, 7.0)
    with pytest.raises(_lib.DiffNormHipError):
        short.forward(x, torch.tensor([3]), torch.tensor([301]), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ----------------------------------------------------------------------------------------------------------- 2. VAE engines at long T
VAE_LENS = (2048, 1337)


@functools.lru_cache(maxsize=None)
def _vae_weights():
    sd = O.make_vae_state_dict(CHAIN_VAE, "chain")
    return sd, _double(sd)


@functools.lru_cache(maxsize=None)
def _vae_ref():
    """Posterior parameters, reconstruction and logits of [2, 2048, 192] in float64 (the decoder fed the float64 posterior mean), and
    the distances of the float32 oracle and of the rounding-points models from them -- once."""
    sd, sd64 = _vae_weights()
    cfg = CHAIN_VAE
    feat = seeded((2, 2048, cfg.dim), 31)
    lens = torch.tensor(VAE_LENS)
    mask = O.lengths_to_mask(lens, 2048)
    with torch.no_grad():
        params = O.vae_encode_params(sd64, cfg, feat.double())
        mean = params[..., :cfg.z].contiguous()
        recon, logits = O.vae_decode(sd64, cfg, mean, mask)
        ref = dict(params=params, recon=recon, logits=logits)
        m32 = mean.float()

        def dist(p, rl):
            return dict(params=_maxerr(p, params, mask), recon=_maxerr(rl[0], recon, mask), logits=_maxerr(rl[1], logits, mask))

        side = {"f32": dist(O.vae_encode_params(sd, cfg, feat), O.vae_decode(sd, cfg, m32, mask))}
        for kind in ("f16", "bf16"):
            side[kind] = dist(E.vae_encode_params(sd, cfg, feat, R=E.Rounder(kind=kind, count=False)),
                              E.vae_decode(sd, cfg, m32, mask, R=E.Rounder(kind=kind, count=False)))
    side["bf16x3"] = side["f32"]
    top2 = logits.topk(2, dim=-1).values
    return dict(feat=feat, lens=lens, mask=mask, mean=m32, ref=ref, side=side, margin=top2[..., 0] - top2[..., 1],
                units=(logits.argmax(-1) - 4).int())


def _vae_engine(dtype):
    from diffnorm_amd import engine

    c = CHAIN_VAE
    return engine.VaeEngine(_vae_weights()[0], dim=c.dim, latent_dim=c.latent_dim, dtype=dtype, device=DEV, depth=c.depth, heads=c.heads,
                            dim_head=c.dim_head, stacks=c.stacks, layers=c.layers, vocab=c.vocab)


def _vae_bar(dtype, ref, side, mask):
    scale = float(ref[mask].abs().max())
    if dtype in EXACT:
        return max(VAE_BUDGET[dtype] * max(1.0, scale / 4), F32_FACTOR * side), scale
    return max(VAE_BUDGET[dtype], MODEL_FACTOR * side), scale


@pytest.mark.parametrize("dtype", MODES)
def test_vae_engines_at_2048_frames(dtype):
    """dn_vae_encode_params and dn_vae_decode on [2, 2048, 192], lengths 2048 / 1337, against float64 on the valid frames; units equal
    to the oracle's argmax wherever its top-2 logit margin exceeds twice the mode's logit bar, which may exclude 2 % of the frames
    at the most (these inputs: none in f32 / bf16x3 / f16, 0.06 % in bf16)."""
    v = _vae_ref()
    ve = _vae_engine(dtype)
    mask = v["mask"]
    params = ve.encode_params(v["feat"].to(DEV)).cpu()
    recon, logits, units = ve.decode(v["mean"].to(DEV), v["lens"])
    got = dict(params=params, recon=recon.cpu(), logits=logits.cpu())
    bars = {}
    for k in ("params", "recon", "logits"):
        side = v["side"][dtype][k]
        bars[k], scale = _vae_bar(dtype, v["ref"][k], side, mask)
        err = _maxerr(got[k], v["ref"][k], mask)
        _report(f"VAE [2, 2048] {k} (scale {scale:.2f}),", dtype, err, bars[k], side)
        assert bool(torch.isfinite(got[k][mask]).all()) and err < bars[k], k
    safe = mask & (v["margin"] > 2 * bars["logits"])
    excluded = 1.0 - float(safe.sum()) / float(mask.sum())
    print(f"VAE [2, 2048] units {dtype}: {100 * excluded:.3f} % of the valid frames inside the margin of {2 * bars['logits']:.3e}")
    assert excluded <= 0.02
    assert bool((units.cpu()[safe] == v["units"][safe]).all())


def test_vae_engines_at_an_odd_length():
    """[1, 2051, 192] in f32: a length that is no multiple of 4, 64 or 256 and longer than any positional table in the project -- the VAE
    has none.  The flat part of the f32 bar alone (no wider than section 2's)."""
    sd, sd64 = _vae_weights()
    cfg = CHAIN_VAE
    feat = seeded((1, 2051, cfg.dim), 32)
    lens = torch.tensor([2051])
    mask = O.lengths_to_mask(lens, 2051)
    with torch.no_grad():
        params = O.vae_encode_params(sd64, cfg, feat.double())
        mean = params[..., :cfg.z].contiguous()
        recon, logits = O.vae_decode(sd64, cfg, mean, mask)
    ve = _vae_engine("f32")
    got_p = ve.encode_params(feat.to(DEV)).cpu()
    got_r, got_l, _ = ve.decode(mean.float().to(DEV), lens)
    for name, got, ref in (("params", got_p, params), ("recon", got_r.cpu(), recon), ("logits", got_l.cpu(), logits)):
        bar = VAE_BUDGET["f32"] * max(1.0, float(ref.abs().max()) / 4)
        err = _maxerr(got, ref, mask)
        print(f"VAE [1, 2051] {name} f32: max abs err {err:.3e}  bar {bar:.3e}")
        assert err < bar, name


# -------------------------------------------------------------------------------------------------------- 3. sampling loops at long T
@pytest.mark.parametrize("dtype", ["f16", "bf16x3"])
def test_ddim_loop_graph_and_split_at_2048_frames(dtype):
    """test_config3_chain_graph_and_split_are_bit_identical's assertion at [2, 2048], lengths 2048 / 1337: three evaluations from step
    999, eager == hipGraph replay (== the two half-batch streams, with and without the graph, in f16), finite, and not the input."""
    from diffnorm_amd import ops, scheduler

    e = _eps_engine(dtype)
    coef = scheduler.DDPMScheduler(1000).ddim_coef_table(DEV)
    x0 = ops.randn((2, 2048, LONG_EPS.latent_dim), seed=5, device=DEV)
    lens = torch.tensor(SHAPES["full"][2], dtype=torch.int32, device=DEV)
    ways = ((False, False), (True, False), (True, True), (False, True)) if dtype == "f16" else ((False, False), (True, False))
    outs = []
    for graph, split in ways:
        x = x0.clone()
        with torch.cuda.stream(torch.cuda.Stream()):
            n = e.ddim_loop(x, lens, 999, coef, use_graph=graph, max_evals=3, split=split)
        torch.cuda.synchronize()
        assert n == 3 and bool(torch.isfinite(x).all())
        outs.append(x)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert not torch.equal(outs[0], x0)


def test_one_ddim_step_at_2048_frames_against_float64():
    """dn_eps_forward at t = 3 and dn_ddim_step in f32 against O.ddim_update on section 1's float64 eps: the loop's step, tied to a
    float64 reference, under section 1's f32 bar."""
    from diffnorm_amd import ops, scheduler

    x, lens, mask = _eps_input("full")
    r = _eps_ref("full", 3)
    times = torch.full((2,), 3)
    want = O.ddim_update(O.ddpm_tables(1000), x.double(), r["ref"], times)
    coef = scheduler.DDPMScheduler(1000).ddim_coef_table(DEV)
    xd = x.to(DEV)
    eps = _eps_engine("f32").forward(xd, times, lens)
    got = ops.ddim_step(xd, eps, coef, times.to(DEV).int(), x.shape[1]).cpu()
    err = _maxerr(got, want, mask)
    _report("DDIM step [2, 2048] t = 3,", "f32", err, FLAT["f32"], r["e32"])
    assert err < FLAT["f32"]


# ------------------------------------------------------------------------------------------------ 4. diffusion training at T > 1024
TRAIN_T, TRAIN_LENS = 1536, (1536, 1030)
# CHAIN_VAE's latent is 8 wide (192 / (4 * 3) / 2): the training step runs LONG_EPS at that width
LONG_EPS_TRAIN = dataclasses.replace(LONG_EPS, latent_dim=CHAIN_VAE.z)


@functools.lru_cache(maxsize=None)
def _train_ref():
    """The batch, the frozen encoder's posterior sample and O.diffusion_train_forward's loss dict and autograd gradients in float64,
    laid out like the fixtures TO.compare_grads reads (names, [sum, l2, probe dot], whole tensors)."""
    ecfg, vcfg = LONG_EPS_TRAIN, CHAIN_VAE
    esd, vsd = O.make_eps_state_dict(ecfg, "long"), _vae_weights()[0]
    B, T = len(TRAIN_LENS), TRAIN_T
    lens = torch.tensor(TRAIN_LENS)
    mask = O.lengths_to_mask(lens, T)
    feat = seeded((B, T, vcfg.dim), 41)
    units = torch.randint(4, vcfg.vocab, (B, T), generator=torch.Generator().manual_seed(42)) * mask
    times = torch.tensor([37, 151])
    post, jitter, noise = (seeded((B, T, vcfg.z), s) for s in (43, 44, 45))
    args = (feat, units, mask, times, post, jitter, noise)
    d = lambda t: t.double() if t.is_floating_point() else t
    losses, grads = TO.eps_loss_and_grads(_double(esd), ecfg, _vae_weights()[1], vcfg, 200, *(d(a) for a in args))
    with torch.no_grad():
        z = O.vae_encode(_vae_weights()[1], vcfg, feat.double(), post.double()).float()
    fix = {"g/names": np.array(list(grads)), "g/total_norm": float(torch.sqrt(sum(g.pow(2).sum() for g in grads.values())))}
    for k, g in grads.items():
        fix["g/chk/" + k] = np.array([float(g.sum()), float(g.norm()), float((g.flatten() * TO.probe_vector(g.numel())).sum())])
        fix["g/full/" + k] = g.numpy()
    return dict(esd=esd, args=args, lens=lens, z=z, losses=losses, fix=fix)


@functools.lru_cache(maxsize=None)
def _train_f32_oracle():
    """The same gradients from the float32 oracle (only looked at when an f32 tensor misses the bar)."""
    r = _train_ref()
    return TO.eps_loss_and_grads(r["esd"], LONG_EPS_TRAIN, _vae_weights()[0], CHAIN_VAE, 200, *r["args"])[1]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_diffusion_training_step_at_1536_frames(dtype):
    """dn_eps_train_forward / _backward at B = 2, T = 1536 (lengths 1536 / 1030; LONG_EPS over the frozen CHAIN_VAE) against
    O.diffusion_train_forward and its autograd in float64.  f32: the loss dict within 2e-4 and every tensor under TO.compare_grads'
    1e-3, the bar of test_diffusion_loss_and_gradients_match_reference_f32 -- a tensor whose float32-oracle gradient is itself
    further than 1e-3 / 8 from float64 is held to 8 x that distance instead, and named.  bf16: every tensor's cosine >= 0.9985
    (test_hip_train.py's per-tensor rule)."""
    import test_hip_train as TT

    r = _train_ref()
    feat, units, mask, times, post, jitter, noise = r["args"]
    eps, vae, _, _, _ = TT._eps_setup(dtype, LONG_EPS_TRAIN, "long", "chain")
    stats = eps.forward(feat, units, r["lens"], r["z"], times, jitter, noise)
    vae.zero_grad()
    eps.zero_grad()
    eps.backward()
    s = stats.cpu().double().numpy()
    tol = 2e-4 if dtype == "f32" else 3e-2
    for i, k in enumerate(("total_loss", "nll_loss", "recon_mse_loss", "noise_loss")):
        ref = r["losses"][k]
        print(f"training [2, {TRAIN_T}] {dtype} {k}: {s[i]:.7f}  float64 {ref:.7f}  rel {abs(s[i] - ref) / max(1.0, abs(ref)):.2e}  bar {tol:.0e}")
        assert abs(s[i] - ref) <= tol * max(1.0, abs(ref)), (k, s[i], ref)
    assert float(vae.grads.abs().max()) == 0.0  # frozen
    got = eps.grad_dict()
    fix = r["fix"]
    if dtype == "bf16":
        TT._assert_bf16_gradient_per_tensor(TT._per_tensor_cosines(got, fix), f"diffusion bf16 (B = 2, T = {TRAIN_T})", min_cos=0.9985)
        return
    worst, widened = 0.0, []
    for name in fix["g/names"]:
        one = {**fix, "g/names": [name]}
        try:
            worst = max(worst, TO.compare_grads(got, one, "g/", rtol=1e-3))
        except AssertionError:
            e32 = TO.compare_grads(_train_f32_oracle(), one, "g/", rtol=float("inf"))
            if e32 <= 1e-3 / F32_FACTOR:
                raise
            widened.append((str(name), e32, TO.compare_grads(got, one, "g/", rtol=F32_FACTOR * e32)))
    print(f"training [2, {TRAIN_T}] f32: worst relative gradient error under the 1e-3 bar {worst:.3e}; held to 8 x the float32 oracle's "
          f"error instead (name, that error, measured): {widened}")
