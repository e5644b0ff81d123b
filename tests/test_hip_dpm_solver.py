"""dn_dpm_loop / dn_dpm2m_step on the GPU: the DPM-Solver++(2M) chain over a timestep schedule -- the update kernel alone against
float64, the device loop against the float64 host chain over the oracle's eps-predictor, eager == graph == split, the graph cache
against dn_ddim_sched_loop's, a dirty workspace, the mirror, and the refusals of the C entry.

Shapes: the CHAIN_EPS / CHAIN_VAE models (latent width 8), B = 3 (halves of 1 and 2 sequences), T = 24, lengths (24, 17, 9),
DDPMScheduler(200); chains of 5 evaluations from start_step = 50 (rows 1-3 second order) and the explicit list [40, 22, 7, 0] (its
last row goes to the clean level).  The parity bars are the flat per-mode bars test_hip_ddim_schedule.py holds its strided chains to."""
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, TINY_EPS_COND, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("f32", 1e-3), ("bf16x3", 1e-3), ("f16", 1e-2), ("bf16", 2e-2)]  # test_hip_ddim_schedule.py's
B, T, Z = 3, 24, CHAIN_VAE.z
LENS = torch.tensor([24, 17, 9])
EXPLICIT = [40, 22, 7, 0]
SELECTIONS = (dict(sampling_steps=5), dict(steps=EXPLICIT))
TIMESTEPS = 200
U = 2.0 ** -24
COMBOS = ((False, False), (True, False), (False, True), (True, True))  # (graph, split)


def maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


def on_stream(fn):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
    torch.cuda.synchronize()
    return out


def x_start():
    return seeded((B, T, Z), 271)


@pytest.fixture(scope="module")
def eng():
    from diffnorm_amd import engine, scheduler

    return engine, scheduler.DDPMScheduler(TIMESTEPS)


def new_engine(engine, dtype):
    return engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype=dtype, device=DEV)


_engines = {}


def eps_engine(engine, dtype):
    if dtype not in _engines:
        _engines[dtype] = new_engine(engine, dtype)
    return _engines[dtype]


_refs = {}


def reference_chain(sched, steps, order):
    """The float64 host chain (scheduler.dpm_chain_reference over float64 rows) stepping the oracle's eps-predictor.  Computed once
    per (schedule, order) and left unchanged."""
    from diffnorm_amd import scheduler

    key = (tuple(steps), order)
    if key not in _refs:
        sd = O.make_eps_state_dict(CHAIN_EPS, "chain")
        mask = O.lengths_to_mask(LENS.long(), T)

        def eps_fn(x, e):
            with torch.no_grad():
                return O.eps_forward(sd, CHAIN_EPS, x.float(), torch.full((B,), e, dtype=torch.long), mask).double()

        _refs[key] = scheduler.dpm_chain_reference(x_start().double(), eps_fn, steps, sched.dpm_rows64(steps, order))
    return _refs[key]


_runs = {}


def dpm_run(e, sched, graph, split, order=2, x0=None, **sel):
    st, rows = sched.dpm_schedule(50, order=order, device=DEV, **sel)
    x = (x_start() if x0 is None else x0).to(DEV).clone()
    n = on_stream(lambda: e.dpm_schedule_loop(x, LENS.to(DEV).int(), st, rows, use_graph=graph, split=split, timesteps=TIMESTEPS))
    assert n == st.shape[0]
    return x.cpu()


def cached_run(engine, sched, dtype, order, sel):
    key = (dtype, order, tuple(sorted((k, str(v)) for k, v in sel.items())))
    if key not in _runs:
        _runs[key] = dpm_run(eps_engine(engine, dtype), sched, False, False, order=order, **sel)
    return _runs[key]


# ------------------------------------------------------------------------------------------------------------------ kernel alone
GRID_CAP_ELEMS = 2048 * 256 * 4  # the element-wise grid is capped at 2048 blocks of 256 threads, a quad each


def step_alone(lib, x, eps, hist, n, rows, row):
    from diffnorm_amd import _lib

    idx = torch.tensor([row], dtype=torch.int32, device=DEV)
    rc = on_stream(lambda: lib.dn_dpm2m_step(x.data_ptr(), eps.data_ptr(), hist.data_ptr(), n, rows.data_ptr(), idx.data_ptr(),
                                            _lib.current_stream()))
    assert rc == 0, lib.dn_last_error()


@pytest.mark.parametrize("n", [4, 1020, 4100, GRID_CAP_ELEMS + 12])
def test_update_kernel_alone(eng, n):
    from diffnorm_amd import _lib

    _, sched = eng
    lib = _lib.load()
    _, rows = sched.dpm_schedule(50, sampling_steps=5)
    assert rows[0, 5] == 0 and rows[1, 5] != 0  # row 0 first order, row 1 second order
    r64 = rows.double()
    tail, sentinel = 64, 12345.0
    g = torch.Generator().manual_seed(n)
    x0, eps, h0 = (torch.randn(n, generator=g) for _ in range(3))

    def padded(v):
        return torch.cat([v, torch.full((tail,), sentinel)]).to(DEV)

    for row in (0, 1):
        x, hist, ev = padded(x0), padded(h0), padded(eps)
        step_alone(lib, x, ev, hist, n, rows.to(DEV), row)
        al, sg, a, b, c1, c0 = (r64[row, j].item() for j in range(6))
        xd, ed, hd = x0.double(), eps.double(), h0.double()
        p = (xd - sg * ed) / al
        want = a * xd + b * (c1 * p + c0 * hd)
        X = (xd.abs() + (sg * ed).abs()) / al
        bound = 8 * U * ((a * xd).abs() + abs(b) * (abs(c1) * X + abs(c0) * hd.abs()))
        err = (x[:n].cpu().double() - want).abs()
        herr = (hist[:n].cpu().double() - p).abs()
        print(f"n={n} row {row}: worst err / bound {(err / bound).max().item():.3f}, hist {(herr / (2 * U * X)).max().item():.3f}")
        assert (err <= bound).all() and (herr <= 2 * U * X).all()
        assert (x[n:] == sentinel).all() and (hist[n:] == sentinel).all() and torch.equal(ev.cpu()[:n], eps)  # nothing behind n
    # a first-order row never reads the history: NaN there changes nothing
    outs = []
    for fill in (float("nan"), 0.0):
        x, hist = padded(x0), padded(torch.full((n,), fill))
        step_alone(lib, x, padded(eps), hist, n, rows.to(DEV), 0)
        outs.append((x.cpu(), hist.cpu()))
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# The scheduled DDIM and generic Gaussian updates run the same kernel template as the 2M update, guided and unguided, so its launch
# geometry is pinned through their public single-step entries too, on the grid above: one quad, part of a block, across a block, a
# second grid-stride trip.  Every case draws or clips: (entry, keyword arguments of its launch).
PREFIX = 1020
SEED = 0x5EED0123456789AB
SCHED_CASES = [("ddim", dict(eta=0.0)), ("ddim", dict(eta=0.5, seed=SEED)),
               ("gaussian", dict(sampler=0, clip=0, eta=0.0, seed=SEED)), ("gaussian", dict(sampler=0, clip=1, eta=0.0, seed=SEED)),
               ("gaussian", dict(sampler=1, clip=0, eta=0.5, seed=SEED)), ("gaussian", dict(sampler=1, clip=1, eta=0.5, seed=SEED))]
KEYS = [0xE220A8397B1DCDAF, 1 << 63, 0x0123456789ABCDEF]
ROW = 1  # of 5: not the last row, its timestep is not 0 -- the row draws
_tables = {}


def sched_tables(sched, entry, eta):
    """-> (steps, coefficient rows) on the device: 5 rows of `scheduler.ddim_schedule` / of the cosine "ddim5" respacing."""
    key = (entry, eta if entry == "ddim" else None)
    if key not in _tables:
        if entry == "ddim":
            _tables[key] = sched.ddim_schedule(50, sampling_steps=5, eta=eta, device=DEV)
        else:
            from diffnorm_amd.diffusion import create_diffusion

            _tables[key] = create_diffusion("ddim5", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100).device_schedule(None, DEV)
    return _tables[key]


def sched_step_alone(lib, sched, entry, x, eps, n, eta=0.0, seed=0, sampler=0, clip=0, keys=None, shape=None):
    """dn_ddim_sched_step / dn_gaussian_sched_step (keys: the keyed entries on `shape` = (B, T, Z)) at row ROW, in place on x"""
    from diffnorm_amd import _lib

    steps, rows = sched_tables(sched, entry, eta)
    assert steps.shape[0] == 5 and int(steps[ROW]) != 0
    idx = torch.tensor([ROW], dtype=torch.int32, device=DEV)
    k64 = None if keys is None else torch.tensor([k - (1 << 64) if k >> 63 else k for k in keys], dtype=torch.int64, device=DEV)

    def run():
        s = _lib.current_stream()
        if entry == "ddim" and keys is None:
            return lib.dn_ddim_sched_step(x.data_ptr(), eps.data_ptr(), n, rows.data_ptr(), steps.data_ptr(), idx.data_ptr(), int(eta != 0), seed, None, s)
        if entry == "ddim":
            return lib.dn_ddim_sched_step_keyed(x.data_ptr(), eps.data_ptr(), k64.data_ptr(), *shape, rows.data_ptr(), steps.data_ptr(), idx.data_ptr(), s)
        if keys is None:
            return lib.dn_gaussian_sched_step(x.data_ptr(), eps.data_ptr(), n, rows.data_ptr(), idx.data_ptr(), 5, sampler, clip, eta, seed, None, s)
        return lib.dn_gaussian_sched_step_keyed(x.data_ptr(), eps.data_ptr(), k64.data_ptr(), *shape, rows.data_ptr(), steps.data_ptr(), idx.data_ptr(), 5,
                                                sampler, clip, eta, s)

    assert on_stream(run) == 0, lib.dn_last_error()


def sentinel_padded(v, tail=64, sentinel=12345.0):
    return torch.cat([v.reshape(-1), torch.full((tail,), sentinel)]).to(DEV)


@pytest.mark.parametrize("n", [4, 1020, 4100, GRID_CAP_ELEMS + 12])
def test_sched_step_kernels_alone(eng, n):
    """Nothing behind n is written and eps is not modified; and the prefix property, bit for bit: the first PREFIX elements of the
    n-element launch are the PREFIX-element launch on the same prefix (the update is element-wise and the draw counter is the quad
    index from 0, so this holds for the seeded rows too)."""
    from diffnorm_amd import _lib

    _, sched = eng
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    m = max(n, PREFIX)
    x0, eps = 2.0 * torch.randn(m, generator=g), torch.randn(m, generator=g)  # (|x0| up to ~10: the clip is reached)
    outs = {}
    for entry, kw in SCHED_CASES:
        got = {}
        for count in {n, PREFIX}:
            x, ev = sentinel_padded(x0[:count]), sentinel_padded(eps[:count])
            sched_step_alone(lib, sched, entry, x, ev, count, **kw)
            x, ev = x.cpu(), ev.cpu()
            assert (x[count:] == 12345.0).all() and (ev[count:] == 12345.0).all() and torch.equal(ev[:count], eps[:count]), (entry, kw, count)
            assert torch.isfinite(x).all() and not torch.equal(x[:count], x0[:count])
            got[count] = x[:count]
        k = min(n, PREFIX)
        assert torch.equal(got[n][:k], got[PREFIX][:k]), (entry, kw, n)
        outs[(entry, tuple(sorted(kw.items())))] = got[n]
    assert len({tuple(v[:4].tolist()) for v in outs.values()}) == len(SCHED_CASES)  # every case is an update of its own (eta, sampler, clip)


@pytest.mark.parametrize("B", [1, 3])
def test_keyed_sched_step_kernels_alone(eng, B):
    """The keyed entries along whole utterances: T = 5, Z = 4 -- an utterance of the B-row launch is the launch of that utterance
    alone under its key, bit for bit, and nothing behind the batch is written."""
    from diffnorm_amd import _lib

    _, sched = eng
    lib = _lib.load()
    Tk, Zk = 5, 4
    g = torch.Generator().manual_seed(40 + B)
    x0, eps = 2.0 * torch.randn(B, Tk, Zk, generator=g), torch.randn(B, Tk, Zk, generator=g)
    for entry, kw in (("ddim", dict(eta=0.5)), ("gaussian", dict(sampler=0, clip=1)), ("gaussian", dict(sampler=1, clip=0, eta=0.5))):
        x, ev = sentinel_padded(x0), sentinel_padded(eps)
        sched_step_alone(lib, sched, entry, x, ev, x0.numel(), keys=KEYS[:B], shape=(B, Tk, Zk), **kw)
        x, ev = x.cpu(), ev.cpu()
        assert (x[x0.numel():] == 12345.0).all() and torch.equal(ev[:x0.numel()], eps.reshape(-1)) and (ev[x0.numel():] == 12345.0).all()
        whole = x[:x0.numel()].view(B, Tk, Zk)
        for b in range(B):
            xb, eb = sentinel_padded(x0[b]), sentinel_padded(eps[b])
            sched_step_alone(lib, sched, entry, xb, eb, Tk * Zk, keys=[KEYS[b]], shape=(1, Tk, Zk), **kw)
            assert torch.equal(xb.cpu()[:Tk * Zk].view(Tk, Zk), whole[b]), (entry, kw, B, b)
        if B == 3:
            assert not torch.equal(whole[0] - x0[0], whole[1] - x0[1])  # (the utterances draw under their own keys)


def test_update_kernel_entry_refuses_bad_arguments():
    from diffnorm_amd import _lib

    lib = _lib.load()
    x = torch.zeros(16, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows = torch.zeros(1, 6, device=DEV)
    p = x.data_ptr()
    for args in ((None, p, p, 8), (p, p, p, 6), (p, p, p, 0), (p + 4, p, p, 8)):
        assert lib.dn_dpm2m_step(args[0], args[1], args[2], args[3], rows.data_ptr(), idx.data_ptr(), None) == -1
        assert b"dn_dpm2m_step" in lib.dn_last_error()


# ------------------------------------------------------------------------------------------------------------------ chain parity
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dtype,tol", MODES)
def test_chain_matches_the_float64_host_chain(eng, dtype, tol, order):
    engine, sched = eng
    mask = O.lengths_to_mask(LENS.long(), T)
    for sel in SELECTIONS:
        steps = sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        want = reference_chain(sched, steps, order)
        got = cached_run(engine, sched, dtype, order, sel)
        err = maxerr(got[mask], want[mask])
        print(f"dpm chain {steps} order {order} {dtype}: max abs err {err:.3e}")
        assert err < tol, (sel, err)


def test_the_order_matters(eng):
    """Order 2 and order 1 end far apart against the arithmetic's error: a kernel that ignored c0, or a loop that lost the history
    between steps, would give the order-1 end point."""
    engine, sched = eng
    mask = O.lengths_to_mask(LENS.long(), T)
    sel = dict(sampling_steps=5)
    steps = sched.ddim_steps(50, 5)
    two, one = cached_run(engine, sched, "f32", 2, sel), cached_run(engine, sched, "f32", 1, sel)
    parity = max(maxerr(two[mask], reference_chain(sched, steps, 2)[mask]), maxerr(one[mask], reference_chain(sched, steps, 1)[mask]))
    apart = maxerr(two[mask], one[mask])
    print(f"order 2 vs order 1: {apart:.3e} apart, f32 parity {parity:.3e}")
    assert apart > 100 * parity


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_eager_graph_and_split_agree_bit_for_bit(eng, dtype):
    engine, sched = eng
    e = eps_engine(engine, dtype)
    for order in (2, 1):
        for sel in SELECTIONS:
            outs = [dpm_run(e, sched, graph, split, order=order, **sel) for graph, split in COMBOS]
            assert all(torch.equal(o, outs[0]) for o in outs[1:]), (order, sel)
    # a cache hit: the same buffers, twice
    st, rows = sched.dpm_schedule(50, sampling_steps=5, device=DEV)
    lens = LENS.to(DEV).int()
    x = torch.empty(B, T, Z, device=DEV)
    got = []
    for _ in range(2):
        x.copy_(x_start())
        on_stream(lambda: e.dpm_schedule_loop(x, lens, st, rows, use_graph=True, split=True, timesteps=TIMESTEPS))
        got.append(x.cpu())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], dpm_run(e, sched, False, False, sampling_steps=5))


def test_graph_cache_keeps_the_two_loops_apart(eng):
    """ddim then dpm, and dpm then ddim, on one engine, one workspace, one x buffer, the same n_steps, each captured: every result
    is the one a freshly built engine gives."""
    engine, sched = eng
    lens = LENS.to(DEV).int()
    sd, cd = sched.ddim_schedule(50, sampling_steps=5, device=DEV)
    sp, cp = sched.dpm_schedule(50, sampling_steps=5, device=DEV)
    ddim = lambda e, x: e.ddim_schedule_loop(x, lens, sd, cd, use_graph=True, timesteps=TIMESTEPS)  # noqa: E731
    dpm = lambda e, x: e.dpm_schedule_loop(x, lens, sp, cp, use_graph=True, timesteps=TIMESTEPS)  # noqa: E731
    fresh = {}
    for name, chain in (("ddim", ddim), ("dpm", dpm)):
        x = x_start().to(DEV)
        on_stream(lambda: chain(new_engine(engine, "f16"), x))
        fresh[name] = x.cpu()
    assert not torch.equal(fresh["ddim"], fresh["dpm"])
    for order in ((("ddim", ddim), ("dpm", dpm)), (("dpm", dpm), ("ddim", ddim))):
        e = new_engine(engine, "f16")
        e._workspace(int(e.lib.dn_dpm_workspace_bytes(e.handle, B, T, 5)))  # one workspace for both
        ws_ptr = e._ws.data_ptr()
        x = torch.empty(B, T, Z, device=DEV)
        stream = torch.cuda.Stream()
        for name, chain in order + order[:1]:
            x.copy_(x_start())
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                chain(e, x)
            torch.cuda.synchronize()
            assert torch.equal(x.cpu(), fresh[name]), (name, [n for n, _ in order])
        assert e._ws.data_ptr() == ws_ptr


def test_a_dirty_workspace_changes_nothing(eng):
    engine, sched = eng
    e = new_engine(engine, "f32")
    ws = e._workspace(int(e.lib.dn_dpm_workspace_bytes(e.handle, B, T, 5)))
    outs = []
    for fill in (0, 0xFF):  # (0xFF bytes: NaN in every float the history buffer holds)
        for graph in (False, True):
            ws.fill_(fill)
            outs.append(dpm_run(e, sched, graph, True, sampling_steps=5))
            assert e._ws.data_ptr() == ws.data_ptr()
    assert torch.isfinite(outs[0]).all() and all(torch.equal(o, outs[0]) for o in outs[1:])


# ------------------------------------------------------------------------------------------------------------------ mirror
def _mirror(dtype):
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype)
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain"), strict=True)
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), CHAIN_EPS.dim, CHAIN_VAE.z, timesteps=TIMESTEPS, dtype=dtype)
    m.model.load_state_dict(dict(O.make_eps_state_dict(CHAIN_EPS, "chain"), **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    return m.to(DEV).eval()


def test_mirror_routes_the_solver_through_the_new_loop():
    from diffnorm_amd import ops

    m = _mirror("f16")
    feat = seeded((B, T, CHAIN_VAE.dim), 231).to(DEV)
    mask = O.lengths_to_mask(LENS.long(), T).to(DEV)
    post, start = seeded((B, T, Z), 232), seeded((B, T, Z), 233)
    lens = LENS.to(DEV).int()

    def by_hand(loop):
        z = m.speech_decoder.encode_feature(feat, noise=post).transpose(1, 2).contiguous()
        _, sa, s1 = m._tables()
        x = ops.q_sample(z, start.to(DEV).contiguous(), sa, s1, torch.full((B,), 50, dtype=torch.int32, device=DEV), T)
        loop(x)
        recon, _, units = m.speech_decoder.engine().decode(x, lens, want_logits=False)
        return units.long(), recon

    kw = dict(input_mask=mask, start_step=50, post_noise=post, start_noise=start, sampling_steps=5)
    for order in (2, 1):
        st, rows = m.scheduler.dpm_schedule(50, sampling_steps=5, order=order, device=DEV)
        units, recon = by_hand(lambda x: m.model.engine().dpm_schedule_loop(x, lens, st, rows, timesteps=TIMESTEPS))
        toks, _, total, got = m.ddim_sample(feat, solver="dpmpp_2m", solver_order=order, **kw)
        assert total == int(LENS.sum()) and torch.equal(got, recon)
        assert all(torch.equal(t, units[i, : LENS[i]]) for i, t in enumerate(toks))
    sd, cd = m.scheduler.ddim_schedule(50, sampling_steps=5, device=DEV)
    units, recon = by_hand(lambda x: m.model.engine().ddim_schedule_loop(x, lens, sd, cd, timesteps=TIMESTEPS))
    toks, _, _, got = m.ddim_sample(feat, solver=None, **kw)  # today's path, untouched
    assert torch.equal(got, recon) and all(torch.equal(t, units[i, : LENS[i]]) for i, t in enumerate(toks))
    toks2, _, _, got2 = m.ddim_sample(feat, **kw)
    assert torch.equal(got2, got)
    with pytest.raises(ValueError, match="eta"):
        m.ddim_sample(feat, solver="dpmpp_2m", eta=0.5, **kw)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_c_entry_refuses_and_leaves_x_untouched(eng):
    engine, sched = eng
    e = eps_engine(engine, "f32")
    lib = e.lib
    st, rows = sched.dpm_schedule(50, sampling_steps=5, device=DEV)
    lens = LENS.to(DEV).int()
    x = x_start().to(DEV)
    need = int(lib.dn_dpm_workspace_bytes(e.handle, B, T, 5))
    base = int(lib.dn_ddim_sched_workspace_bytes(e.handle, B, T, 5))
    assert need == base + (B * T * Z * 4 + 255) // 256 * 256
    assert lib.dn_dpm_workspace_bytes(None, B, T, 5) == 0 and lib.dn_dpm_workspace_bytes(e.handle, B, T, 0) == 0
    buf = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    wp = (buf.data_ptr() + 255) & ~255
    cond = engine.EpsEngine(O.make_eps_state_dict(TINY_EPS_COND, "cond"), TINY_EPS_COND, dtype="f32", device=DEV)
    xc = seeded((B, T, TINY_EPS_COND.latent_dim), 272).to(DEV)

    def call(m=e.handle, xp=x.data_ptr(), sp=st.data_ptr(), flags=0, wsn=need):
        return lib.dn_dpm_loop(m, xp, lens.data_ptr(), B, T, sp, rows.data_ptr(), 5, TIMESTEPS, flags, wp, wsn, None)

    assert call(m=cond.handle, xp=xc.data_ptr()) == -1 and "dn_guided_ddim_loop" in lib.dn_last_error().decode()
    assert call(flags=4) == -1 and "flags" in lib.dn_last_error().decode()
    assert call(flags=1 << 20) == -1 and "dn_dpm_loop" in lib.dn_last_error().decode()
    assert call(wsn=need - 1) == -3 and "dn_dpm_workspace_bytes" in lib.dn_last_error().decode()
    assert call(wsn=base) == -3  # the DDIM schedule's size is not enough
    assert call(sp=None) == -1 and "null schedule" in lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x_start()) and torch.equal(xc.cpu(), seeded((B, T, TINY_EPS_COND.latent_dim), 272))
    with pytest.raises(ValueError, match="dn_ddim_sched_check"):  # a host list is validated before it is uploaded
        e.dpm_schedule_loop(x, lens, [3, 30, 49], rows[:3].contiguous(), timesteps=TIMESTEPS)
    assert torch.equal(x.cpu(), x_start())
