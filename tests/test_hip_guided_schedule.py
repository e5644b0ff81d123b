"""dn_guided_ddim_loop on the GPU: the prompted, classifier-free-guided DDIM chain over a timestep schedule as a device loop --
against the existing host-driven chain (EpsEngine.guided_ddim_chain) bit for bit where the two coincide, against a CPU restatement
over the oracle's guided prediction where they do not, and through the mirror.

Model: TINY_EPS_COND (dim 64, z 16, depth 2, prompt dim 48, 8 latents), DDPMScheduler(200).  Shapes: B = 3 (odd), T = 40, Tp = 21,
ragged lengths (one sequence full length) and prompt lengths (one of a single frame).  Every call runs on a non-default stream.

Parity bar of a mode = max(project bar, 2 x baseline): the project bars are MODES of test_hip_ddim_schedule.py; the baseline is the
error of the EXISTING guided_ddim_chain at start_step = 6 (5 evaluations, same model, batch and scale) against the same restatement,
measured in the same run and printed -- guidance at scale 2 triples a prediction error, so the bar hangs on existing code and never
on the new loop."""
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, TINY_EPS_COND, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("f32", 1e-3), ("bf16x3", 1e-3), ("f16", 1e-2), ("bf16", 2e-2)]
DTYPES = [m for m, _ in MODES]
CFG = TINY_EPS_COND
B, T, TP, Z, P = 3, 40, 21, TINY_EPS_COND.latent_dim, TINY_EPS_COND.dim_prompt
LENS, PLENS = torch.tensor([40, 17, 29]), torch.tensor([21, 1, 13])
EXPLICIT = [49, 30, 29, 3, 0]
TIMESTEPS = 200


def maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


def on_stream(fn):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
    torch.cuda.synchronize()
    return out


def x_start():
    return seeded((B, T, Z), 171)


def prompt_cpu(seed=172):
    return seeded((B, TP, P), seed)


@pytest.fixture(scope="module")
def eng():
    from diffnorm_amd import engine, scheduler

    return engine, scheduler.DDPMScheduler(TIMESTEPS)


_engines = {}


def new_engine(engine, dtype):
    return engine.EpsEngine(O.make_eps_state_dict(CFG, "cond"), CFG, dtype=dtype, device=DEV)


def cond_engine(engine, dtype):
    if dtype not in _engines:
        _engines[dtype] = new_engine(engine, dtype)
    return _engines[dtype]


class Inputs:
    def __init__(self, prompt_seed=172):
        self.lens, self.plens = LENS.to(DEV).int(), PLENS.to(DEV).int()
        self.prompt = prompt_cpu(prompt_seed).to(DEV)


def loop_run(e, sched, inp, start, scale, use_graph, eta=0.0, x0=None, want_n=True, **kw):
    """The new loop from x_start() over the schedule (sampling_steps= / steps= select it) -> x on the CPU."""
    sel = {k: kw.pop(k) for k in ("sampling_steps", "steps") if k in kw}
    st, coef = sched.ddim_schedule(start, eta=eta, device=DEV, **sel)
    x = (x_start() if x0 is None else x0).to(DEV).clone()
    n = on_stream(lambda: e.guided_ddim_schedule_loop(x, inp.lens, inp.prompt, inp.plens, st, coef, cond_scale=scale, eta=eta, use_graph=use_graph,
                                                      timesteps=TIMESTEPS, **kw))
    assert n == st.shape[0]
    return x.cpu()


def chain_run(e, sched, inp, start, scale, use_graph=False):
    """The existing host-driven chain from x_start() -> (x on the CPU, evaluations)."""
    x = x_start().to(DEV).clone()
    coef = sched.ddim_coef_table(DEV)
    n = on_stream(lambda: e.guided_ddim_chain(x, inp.lens, inp.prompt, inp.plens, start, coef, cond_scale=scale, use_graph=use_graph))
    return x.cpu(), n


_refs = {}


def reference_chain(steps, scale, eta=0.0, noise=None):
    """The chain on the CPU: O.eps_forward_with_cond_scale and the fp32 update over O.ddpm_tables(200) (the restatement of
    test_hip_ddim_schedule.py with the guided predictor).  Computed once per (schedule, scale, eta) and left unchanged."""
    key = (tuple(steps), scale, eta)
    if key in _refs:
        return _refs[key]
    sd, tab = O.make_eps_state_dict(CFG, "cond"), O.ddpm_tables(TIMESTEPS)
    ab = tab.alphas_cumprod
    mask, pmask = O.lengths_to_mask(LENS, T), O.lengths_to_mask(PLENS, TP)
    prompt = prompt_cpu()
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)  # noqa: E731
    x = x_start()
    with torch.no_grad():
        for i, e in enumerate(steps):
            eps = O.eps_forward_with_cond_scale(sd, CFG, x, torch.full((B,), e, dtype=torch.long), mask, prompt, pmask, scale)
            tgt = ab[steps[i + 1]] if i + 1 < len(steps) else (ab[0] if e >= 1 else 1.0)
            sigma = eta * np.sqrt((1 - tgt) / (1 - ab[e])) * np.sqrt(1 - ab[e] / tgt)
            sa, s1 = f(np.sqrt(ab[e])), f(np.sqrt(1 - ab[e]))
            x1 = (x - s1 * eps) / sa.clamp(min=1e-10)
            pn = (x - sa * x1) / s1.clamp(min=1e-10)
            x = x1 * f(np.sqrt(tgt)) + f(np.sqrt(1 - tgt - sigma ** 2)) * pn
            if eta and e != 0:
                x = x + f(sigma) * noise[i]
    _refs[key] = x
    return x


def step_noise(n):
    return seeded((n, B, T, Z), 173)


# (selection, scale, eta): at most 5 evaluations each
CASES = [(dict(sampling_steps=1), 2.0, 0.0), (dict(sampling_steps=5), 2.0, 0.0), (dict(steps=EXPLICIT), 2.0, 0.0), (dict(steps=EXPLICIT), 2.0, 0.5),
         (dict(sampling_steps=5), 1.0, 0.0)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_time_table_of_a_step_list_is_rows_of_the_range_table(eng, dtype):
    engine, _ = eng
    e = cond_engine(engine, dtype)
    for steps, n_t in (([6, 5, 4, 3, 2, 1], 7), (EXPLICIT, 50)):
        full = on_stream(lambda: e.cond_time_table(0, n_t))
        got = on_stream(lambda: e.cond_time_table_steps(steps))
        assert got.shape == (len(steps), full.shape[1]) and got.dtype == torch.float32
        # both tables have fewer than 128 rows: the fp32 contraction takes the same route for either
        assert torch.equal(got, full[torch.tensor(steps, device=DEV)]), (steps, maxerr(got, full[torch.tensor(steps, device=DEV)]))
    assert torch.equal(on_stream(lambda: e.cond_time_table_steps(torch.tensor([3], dtype=torch.int64))), on_stream(lambda: e.cond_time_table(3, 1)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_timestep_schedule_is_the_existing_chain_bit_for_bit(eng, dtype):
    """start_step 1 / 2: no graph (one evaluation); 3: eager + capture + one replay; 7: eager + capture + replays."""
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    for start in (1, 2, 3, 7):
        for scale in (1.0, 2.0):
            want, n = chain_run(e, sched, inp, start, scale)
            assert n == max(1, start - 1)
            for graph in (False, True):
                got = loop_run(e, sched, inp, start, scale, graph)  # (asserts the evaluation count = len(schedule) = n)
                assert sched.ddim_steps(start) == ([0] if start == 1 else list(range(start - 1, 0, -1)))
                assert torch.equal(got, want), (start, scale, graph, maxerr(got, want))


_cases_out = {}


def case_outputs(e, sched, inp, dtype, i):
    """(eager, graph) results of CASES[i] in `dtype`, run once per module."""
    if (dtype, i) not in _cases_out:
        sel, scale, eta = CASES[i]
        kw = dict(sel)
        if eta:
            kw["noise"] = step_noise(len(sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))))
        _cases_out[(dtype, i)] = tuple(loop_run(e, sched, inp, 50, scale, graph, eta=eta, **kw) for graph in (False, True))
    return _cases_out[(dtype, i)]


@pytest.mark.parametrize("dtype,tol", MODES)
def test_strided_and_eta_chains_match_the_cpu_restatement(eng, dtype, tol):
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    mask = O.lengths_to_mask(LENS, T)
    bars = {}
    for scale in (2.0, 1.0):  # baseline: the existing chain at start_step = 6 (5 evaluations) against the same restatement
        base, n = chain_run(e, sched, inp, 6, scale)
        assert n == 5
        err = maxerr(base[mask], reference_chain([5, 4, 3, 2, 1], scale)[mask])
        bars[scale] = max(tol, 2 * err)
        print(f"baseline guided_ddim_chain start 6 scale {scale} {dtype}: max abs err {err:.3e} -> bar {bars[scale]:.3e}")
    for i, (sel, scale, eta) in enumerate(CASES):
        steps = sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        want = reference_chain(steps, scale, eta, step_noise(len(steps)) if eta else None)
        got = case_outputs(e, sched, inp, dtype, i)[0]
        err = maxerr(got[mask], want[mask])
        print(f"guided chain {steps} scale {scale} eta {eta} {dtype}: max abs err {err:.3e} (bar {bars[scale]:.3e})")
        assert err < bars[scale], (sel, scale, eta, err)


@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_equals_graph_and_in_kernel_noise(eng, dtype):
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    for i in range(len(CASES)):
        eager, graph = case_outputs(e, sched, inp, dtype, i)
        assert torch.equal(eager, graph), CASES[i]
    run = lambda seed, graph, scale=2.0: loop_run(e, sched, inp, 50, scale, graph, eta=0.5, seed=seed, sampling_steps=6)  # noqa: E731
    a = run(7, False)
    assert torch.equal(run(7, True), a) and torch.equal(run(7, False), a)  # eager == graph; a seed reproduces
    assert not torch.equal(run(8, False), a)  # another seed differs
    assert torch.equal(run(7, True, 1.0), run(7, False, 1.0)) and not torch.equal(run(7, False, 1.0), a)


def test_scale_one_draws_the_unconditional_loops_noise(eng):
    """One eta step from x = 0 with a coefficient row {sa, s1, 0, 0, 1}: the update is fmaf(1, z, 0 * x1 + 0 * pn) = z exactly (and
    exactly 0 with zero noise injected), so drawn - injected recovers the draw bit for bit -- from the guided loop at scale 1 and
    from dn_ddim_sched_loop on an unconditional model with as many latent elements: the same (seed, step index, element quad)."""
    engine, sched = eng
    e, inp = cond_engine(engine, "f32"), Inputs()
    u = engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype="f32", device=DEV)
    Tu = B * T * Z // (B * CHAIN_EPS.latent_dim)
    assert B * Tu * CHAIN_EPS.latent_dim == B * T * Z
    ulens = torch.full((B,), Tu, dtype=torch.int32, device=DEV)
    zs = {}
    for seed in (7, 8):
        for n_steps, steps in ((1, [49]), (2, [49, 41])):
            st, coef = sched.ddim_schedule(50, steps=steps, eta=0.5, device=DEV)
            coef[:, 2:4] = 0.0
            coef[:, 4] = 1.0
            outs = []
            for nz in (None, 0):
                xg, xu = torch.zeros(B, T, Z, device=DEV), torch.zeros(B, Tu, CHAIN_EPS.latent_dim, device=DEV)
                ng = None if nz is None else torch.zeros(n_steps, B, T, Z)
                nu = None if nz is None else torch.zeros(n_steps, B, Tu, CHAIN_EPS.latent_dim)
                on_stream(lambda: e.guided_ddim_schedule_loop(xg, inp.lens, inp.prompt, inp.plens, st, coef, cond_scale=1.0, eta=0.5, seed=seed,
                                                              noise=ng, use_graph=False, timesteps=TIMESTEPS))
                on_stream(lambda: u.ddim_schedule_loop(xu, ulens, st, coef, eta=0.5, seed=seed, noise=nu, use_graph=False, split=False,
                                                       timesteps=TIMESTEPS))
                outs.append((xg.cpu().flatten(), xu.cpu().flatten()))
            assert not outs[1][0].any() and not outs[1][1].any()  # zero noise injected: exactly 0
            zg, zu = outs[0][0] - outs[1][0], outs[0][1] - outs[1][1]
            assert torch.isfinite(zg).all() and zg.abs().max() > 1.0
            assert torch.equal(zg, zu), (seed, steps)
            zs[(seed, n_steps)] = zg
    assert not torch.equal(zs[(7, 1)], zs[(8, 1)]) and not torch.equal(zs[(7, 1)], zs[(7, 2)])  # per seed, per step index


def _raw_call(e, x, inp, st, coef, scale, wp, nbytes, flags=0):
    return e.lib.dn_guided_ddim_loop(e.handle, x.data_ptr(), inp.lens.data_ptr(), inp.prompt.data_ptr(), inp.plens.data_ptr(), B, T, TP, scale,
                                     st.data_ptr(), coef.data_ptr(), st.shape[0], TIMESTEPS, 0, 0, None, flags, wp, nbytes,
                                     torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("scale", [2.0, 1.0])
def test_nothing_is_read_before_it_is_written(eng, dtype, scale):
    """A 4-step chain on a workspace of exactly the reported size filled with 0xFF bytes (NaN) equals the clean (zeroed) run; at
    scale 1 that size is the guided = 0 one, which has no second halves at all.  One byte less is DN_EWORKSPACE."""
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    st, coef = sched.ddim_schedule(50, sampling_steps=4, device=DEV)
    need = int(e.lib.dn_guided_ddim_workspace_bytes(e.handle, B, T, TP, 4, int(scale != 1.0)))
    assert 0 < int(e.lib.dn_guided_ddim_workspace_bytes(e.handle, B, T, TP, 4, 0)) < int(e.lib.dn_guided_ddim_workspace_bytes(e.handle, B, T, TP, 4, 1))
    buf = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    wp = (buf.data_ptr() + 255) & ~255
    outs = []
    for fill in (0x00, 0xFF):
        for flags in (0, 1):
            buf.fill_(fill)
            x = x_start().to(DEV).clone()
            assert on_stream(lambda: _raw_call(e, x, inp, st, coef, scale, wp, need, flags)) == 4, e.lib.dn_last_error()
            outs.append(x.cpu())
    assert torch.isfinite(outs[0]).all()
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert torch.equal(outs[0], loop_run(e, sched, inp, 50, scale, False, sampling_steps=4))
    x = x_start().to(DEV).clone()
    assert _raw_call(e, x, inp, st, coef, scale, wp, need - 1) == -3 and "dn_guided_ddim_workspace_bytes" in e.lib.dn_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x_start())  # refused before anything ran


def test_graph_cache_serves_only_the_chain_it_captured(eng):
    """On one engine, one workspace and one x address, captured back to back: 6 steps, 4 steps, 6 steps again, 6 steps at scale 1.5,
    6 steps with another prompt tensor -- each equals the same chain run first on a fresh engine; the host-driven chain on that
    engine afterwards equals its fresh-engine result; an unconditional engine's dn_ddim_loop graph around it all is unaffected."""
    engine, sched = eng
    dtype = "f16"
    e, inp, other = new_engine(engine, dtype), Inputs(), Inputs(prompt_seed=174)
    u = engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype=dtype, device=DEV)
    ux0 = seeded((B, 48, CHAIN_EPS.latent_dim), 71)
    ulens, ucoef = torch.tensor([48, 30, 41], dtype=torch.int32, device=DEV), sched.ddim_coef_table(DEV)

    def uncond():
        x = ux0.to(DEV).clone()
        on_stream(lambda: u.ddim_loop(x, ulens, 8, ucoef, use_graph=True))
        return x.cpu()

    u_before = uncond()
    s6, c6 = sched.ddim_schedule(50, sampling_steps=6, device=DEV)
    s4, c4 = sched.ddim_schedule(50, sampling_steps=4, device=DEV)
    e._workspace(int(e.lib.dn_guided_ddim_workspace_bytes(e.handle, B, T, TP, 6, 1)))  # one workspace for all of them
    ws_ptr = e._ws.data_ptr()
    chains = [(inp, s6, c6, 2.0), (inp, s4, c4, 2.0), (inp, s6, c6, 2.0), (inp, s6, c6, 1.5), (other, s6, c6, 2.0)]
    x = torch.empty(B, T, Z, device=DEV)
    stream = torch.cuda.Stream()
    got = []
    for who, st, coef, scale in chains:
        x.copy_(x_start())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            assert e.guided_ddim_schedule_loop(x, who.lens, who.prompt, who.plens, st, coef, cond_scale=scale, use_graph=True, timesteps=TIMESTEPS) == st.shape[0]
        torch.cuda.synchronize()
        got.append(x.cpu())
    assert e._ws.data_ptr() == ws_ptr
    for i, (who, st, coef, scale) in enumerate(chains):
        fresh = new_engine(engine, dtype)
        ref = x_start().to(DEV)
        on_stream(lambda: fresh.guided_ddim_schedule_loop(ref, who.lens, who.prompt, who.plens, st, coef, cond_scale=scale, use_graph=True,
                                                          timesteps=TIMESTEPS))
        assert torch.equal(got[i], ref.cpu()), i
    assert torch.equal(got[0], got[2]) and not torch.equal(got[0], got[3]) and not torch.equal(got[0], got[4])
    after, _ = chain_run(e, sched, inp, 7, 2.0, use_graph=True)
    fresh_chain, _ = chain_run(new_engine(engine, dtype), sched, inp, 7, 2.0, use_graph=True)
    assert torch.equal(after, fresh_chain)
    assert torch.equal(uncond(), u_before)


def test_through_the_mirror():
    """LatentDiscreteModel(use_cond=True).prompted_ddim_sample: the every-timestep call is ddim_sample's prompted chain bit for bit, a
    2-evaluation schedule matches the CPU restatement through the decoder, and ddim_sample keeps refusing a schedule."""
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    def close(a, b, tol):
        assert maxerr(a, b) < tol, maxerr(a, b)

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32")
    vsd = O.make_vae_state_dict(CHAIN_VAE, "chain")
    vae.load_state_dict(vsd, strict=True)
    ldm = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 64, CHAIN_VAE.z, timesteps=TIMESTEPS, use_cond=True, dtype="f32").to(DEV).eval()
    ecfg = O.EpsConfig(dim=64, latent_dim=CHAIN_VAE.z, dim_prompt=CHAIN_VAE.dim, num_latents_m=64)
    esd = {k: v.detach().cpu() for k, v in ldm.model.state_dict().items() if not k.endswith("._float_tensor")}
    feat, src = seeded((2, 24, CHAIN_VAE.dim), 91), seeded((2, 30, CHAIN_VAE.dim), 92)
    flen, slen = torch.tensor([24, 15]), torch.tensor([30, 22])
    fmask, smask = O.lengths_to_mask(flen, 24), O.lengths_to_mask(slen, 30)
    post, start = seeded((2, 24, CHAIN_VAE.z), 93), seeded((2, 24, CHAIN_VAE.z), 94)
    kw = dict(prompt=src.to(DEV), prompt_mask=smask.to(DEV), input_mask=fmask.to(DEV), cond_scale=2.0, post_noise=post, start_noise=start)
    toks, match, total, recon = ldm.ddim_sample(feat.to(DEV), start_step=4, **kw)
    toks2, match2, total2, recon2 = ldm.prompted_ddim_sample(feat.to(DEV), start_step=4, **kw)
    assert (match2, total2) == (match, total) and torch.equal(recon, recon2) and all(torch.equal(a, b) for a, b in zip(toks, toks2))
    # sampling_steps = 2 from start_step = 50: evaluations at 49 and 1
    steps = ldm.scheduler.ddim_steps(50, 2)
    assert steps == [49, 1]
    evals = []
    eng_ = ldm.model.engine()
    orig = eng_.guided_ddim_schedule_loop
    eng_.guided_ddim_schedule_loop = lambda *a, **k: evals.append(orig(*a, **k)) or evals[-1]
    try:
        toks3, _, total3, recon3 = ldm.prompted_ddim_sample(feat.to(DEV), start_step=50, sampling_steps=2, **kw)
    finally:
        del eng_.guided_ddim_schedule_loop
    assert evals == [2]
    tab = O.ddpm_tables(TIMESTEPS)
    ab = tab.alphas_cumprod
    xx = O.vae_encode(vsd, CHAIN_VAE, feat, post)
    ts = torch.full((2,), 50, dtype=torch.long)
    xx = tab.at("sqrt_alphas_cumprod", ts, 3) * xx + tab.at("sqrt_one_minus_alphas_cumprod", ts, 3) * start
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)  # noqa: E731
    with torch.no_grad():
        for i, t_ in enumerate(steps):
            eps = O.eps_forward_with_cond_scale(esd, ecfg, xx, torch.full((2,), t_, dtype=torch.long), fmask, src, smask, 2.0)
            tgt = ab[steps[i + 1]] if i + 1 < len(steps) else ab[0]
            sa, s1 = f(np.sqrt(ab[t_])), f(np.sqrt(1 - ab[t_]))
            x1 = (xx - s1 * eps) / sa.clamp(min=1e-10)
            pn = (xx - sa * x1) / s1.clamp(min=1e-10)
            xx = x1 * f(np.sqrt(tgt)) + f(np.sqrt(1 - tgt)) * pn
    want, _ = O.vae_decode(vsd, CHAIN_VAE, xx, fmask)
    close(recon3.cpu()[fmask], want[fmask], 2e-3)
    assert total3 == int(flen.sum()) and [t_.shape[0] for t_ in toks3] == flen.tolist()
    with pytest.raises(ValueError, match="unconditional"):
        ldm.ddim_sample(feat.to(DEV), start_step=50, sampling_steps=2, **kw)
