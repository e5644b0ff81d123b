"""dn_ddim_sched_loop on the GPU: the DDIM chain over a timestep schedule (strided steps, eta) against dn_ddim_loop where the two
coincide, against a CPU restatement over the oracle's eps-predictor where they do not, and through the mirror and normalize().

Shapes: the CHAIN_EPS / CHAIN_VAE models, B = 3, T = 48, the ragged lengths of chain_small.npz, DDPMScheduler(200).  The parity
bars are the flat bars test_ddpm_loop_matches_reference_p_sample_steps holds on this model, schedule and batch; chains compared
against the CPU stay at <= 7 evaluations, the regime those bars were set for."""
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("f32", 1e-3), ("bf16x3", 1e-3), ("f16", 1e-2), ("bf16", 2e-2)]
B, T = 3, 48
EXPLICIT = [49, 30, 29, 3, 0]


def T_(a):
    return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
    return (a.double() - b.double()).abs().max().item()


@pytest.fixture(scope="module")
def eng():
    from diffnorm_amd import engine, scheduler

    return engine, scheduler


_engines = {}


def eps_engine(engine, dtype):
    if dtype not in _engines:
        _engines[dtype] = engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype=dtype, device=DEV)
    return _engines[dtype]


def on_stream(fn):
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        out = fn()
    torch.cuda.synchronize()
    return out


def x_start():
    return seeded((B, T, CHAIN_VAE.z), 71)


_refs = {}


def reference_chain(lens, steps, eta=0.0, noise=None):
    """The chain of section "Schedule semantics" on the CPU: O.eps_forward and the fp32 update over O.ddpm_tables(200)."""
    key = (tuple(steps), eta)
    if key in _refs:
        return _refs[key]
    sd, tab = O.make_eps_state_dict(CHAIN_EPS, "chain"), O.ddpm_tables(200)
    ab = tab.alphas_cumprod
    mask = O.lengths_to_mask(lens.long(), T)
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)  # noqa: E731
    x = x_start()
    with torch.no_grad():
        for i, e in enumerate(steps):
            eps = O.eps_forward(sd, CHAIN_EPS, x, torch.full((B,), e, dtype=torch.long), mask)
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


def sched_run(e, sched, lens, start, x0, use_graph, split, eta=0.0, **kw):
    sel = {k: kw.pop(k) for k in ("sampling_steps", "steps") if k in kw}
    st, coef = sched.ddim_schedule(start, eta=eta, device=DEV, **sel)
    x = x0.to(DEV).clone()
    n = on_stream(lambda: e.ddim_schedule_loop(x, lens, st, coef, eta=eta, use_graph=use_graph, split=split, timesteps=200, **kw))
    assert n == st.shape[0]
    return x.cpu()


COMBOS = ((False, False), (True, False), (False, True), (True, True))  # (graph, split)


@pytest.mark.parametrize("dtype", [m for m, _ in MODES])
def test_every_timestep_schedule_is_the_existing_chain(eng, golden, dtype):
    engine, scheduler = eng
    e, sched = eps_engine(engine, dtype), scheduler.DDPMScheduler(200)
    lens = T_(golden("chain_small")["lens"]).to(DEV).int()
    coef = sched.ddim_coef_table(DEV)
    for start in (1, 2, 5, 50):
        for graph, split in COMBOS:
            want = x_start().to(DEV).clone()
            n = on_stream(lambda: e.ddim_loop(want, lens, start, coef, use_graph=graph, split=split))
            got = sched_run(e, sched, lens, start, x_start(), graph, split)
            assert n == max(1, start - 1)
            assert torch.equal(got, want.cpu()), (start, graph, split)
            if start > 1:
                assert torch.equal(sched_run(e, sched, lens, start, x_start(), graph, split, sampling_steps=start - 1), got)


def _mirror(dtype):
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype)
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain"), strict=True)
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), CHAIN_EPS.dim, CHAIN_VAE.z, timesteps=200, dtype=dtype)
    m.model.load_state_dict(dict(O.make_eps_state_dict(CHAIN_EPS, "chain"), **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    return m.to(DEV).eval()


@pytest.mark.parametrize("dtype", [m for m, _ in MODES])
def test_mirror_every_timestep_schedule_is_the_default_call(golden, dtype):
    g = golden("chain_small")
    m = _mirror(dtype)
    feat = seeded((B, T, CHAIN_VAE.dim), 31).to(DEV)
    mask = O.lengths_to_mask(T_(g["lens"]), T).to(DEV)
    for start in (5, 50):
        kw = dict(input_mask=mask, ref_units=(T_(g["units"]) - 4).to(DEV), start_step=start, post_noise=T_(g[f"s{start}_post_noise"]),
                  start_noise=T_(g[f"s{start}_start_noise"]))
        toks, match, total, recon = m.ddim_sample(feat, **kw)
        toks2, match2, total2, recon2 = m.ddim_sample(feat, sampling_steps=start - 1, **kw)
        assert (match2, total2) == (match, total) and all(torch.equal(a, b) for a, b in zip(toks, toks2)) and torch.equal(recon, recon2)
        toks3, _, _, recon3 = m.ddim_sample(feat, timestep_schedule=list(range(start - 1, 0, -1)), **kw)
        assert all(torch.equal(a, b) for a, b in zip(toks, toks3)) and torch.equal(recon, recon3)


def test_mirror_refuses_a_schedule_for_the_prompted_model():
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32")
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 64, CHAIN_VAE.z, timesteps=200, use_cond=True, dtype="f32").to(DEV).eval()
    feat = seeded((2, 24, CHAIN_VAE.dim), 91).to(DEV)
    for kw in (dict(sampling_steps=5), dict(timestep_schedule=[49, 3]), dict(eta=0.5)):
        with pytest.raises(ValueError, match="unconditional"):
            m.ddim_sample(feat, prompt=feat, prompt_mask=torch.ones(2, 24, dtype=torch.bool), start_step=50, **kw)


@pytest.mark.parametrize("dtype,tol", MODES)
def test_strided_chain_matches_the_cpu_restatement(eng, golden, dtype, tol):
    engine, scheduler = eng
    e, sched = eps_engine(engine, dtype), scheduler.DDPMScheduler(200)
    lens_cpu = T_(golden("chain_small")["lens"])
    lens, mask = lens_cpu.to(DEV).int(), O.lengths_to_mask(lens_cpu, T)
    for sel in (dict(sampling_steps=1), dict(sampling_steps=5), dict(sampling_steps=7), dict(steps=EXPLICIT)):
        steps = sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        want = reference_chain(lens_cpu, steps)
        outs = [sched_run(e, sched, lens, 50, x_start(), graph, split, **sel) for graph, split in COMBOS]
        err = maxerr(outs[0][mask], want[mask])
        print(f"strided chain {steps} {dtype}: max abs err {err:.3e}")
        assert err < tol, (sel, err)
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), sel  # eager == graph == split


@pytest.mark.parametrize("dtype,tol", MODES)
@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_eta_with_injected_noise_matches_the_cpu_restatement(eng, golden, dtype, tol, eta):
    engine, scheduler = eng
    e, sched = eps_engine(engine, dtype), scheduler.DDPMScheduler(200)
    lens_cpu = T_(golden("chain_small")["lens"])
    lens, mask = lens_cpu.to(DEV).int(), O.lengths_to_mask(lens_cpu, T)
    for sel in (dict(sampling_steps=5), dict(steps=EXPLICIT)):
        steps = sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        noise = seeded((len(steps), B, T, CHAIN_VAE.z), 72)
        want = reference_chain(lens_cpu, steps, eta, noise)
        outs = [sched_run(e, sched, lens, 50, x_start(), graph, split, eta=eta, noise=noise, **sel) for graph, split in COMBOS]
        err = maxerr(outs[0][mask], want[mask])
        print(f"eta={eta} chain {steps} {dtype}: max abs err {err:.3e}")
        assert err < tol, (sel, err)
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), sel


@pytest.mark.parametrize("dtype", [m for m, _ in MODES])
def test_eta_with_in_kernel_noise(eng, golden, dtype):
    engine, scheduler = eng
    e, sched = eps_engine(engine, dtype), scheduler.DDPMScheduler(200)
    lens = T_(golden("chain_small")["lens"]).to(DEV).int()
    z = CHAIN_VAE.z
    run = lambda seed, graph, split, **sel: sched_run(e, sched, lens, 50, x_start(), graph, split, eta=1.0, seed=seed, **sel)  # noqa: E731
    a = run(7, False, False, sampling_steps=5)
    assert torch.equal(run(7, False, False, sampling_steps=5), a)  # a seed reproduces
    assert not torch.equal(run(8, False, False, sampling_steps=5), a)  # another seed differs
    for graph, split in COMBOS[1:]:  # the draw depends on (seed, step, element of the whole batch) only
        assert torch.equal(run(7, graph, split, sampling_steps=5), a), (graph, split)
    # one step from a fixed x: (x_out - x_zero_noise) / sigma is standard normal (1152 samples: standard errors 0.03 and 0.02)
    sig = lambda steps: sched.ddim_schedule(50, steps=steps, eta=1.0)[1][:, 4].tolist()  # noqa: E731
    inject = lambda steps, noise, **kw: sched_run(e, sched, lens, 50, x_start(), False, False, eta=1.0, noise=noise, steps=steps, **kw)  # noqa: E731
    first = (run(7, False, False, steps=[49]) - inject([49], torch.zeros(1, B, T, z))) / sig([49])[0]  # the draw of step 0
    zed = first.flatten()
    assert abs(zed.mean().item()) < 0.15 and abs(zed.std().item() - 1.0) < 0.1, (zed.mean().item(), zed.std().item())
    # the second step's draw differs from the first's: against the chain whose step 0 is given that draw and whose step 1 gets none
    both = run(7, False, False, steps=[49, 41])
    noise = torch.zeros(2, B, T, z)
    noise[0] = first
    second = (both - inject([49, 41], noise)) / sig([49, 41])[1]
    assert not torch.allclose(second.flatten()[:64], first.flatten()[:64], atol=0.1)
    # a last step at e = 0 adds no noise: the schedule's own sigma vanishes there, so give the kernel a row whose sigma does not
    st0, c0 = sched.ddim_schedule(1, steps=[0], eta=1.0, device=DEV)
    c0[0, 4] = 0.3
    outs = []
    for nz in (None, torch.zeros(1, B, T, z)):
        x = x_start().to(DEV).clone()
        assert on_stream(lambda: e.ddim_schedule_loop(x, lens, st0, c0, eta=1.0, seed=7, noise=nz, use_graph=False, split=False)) == 1
        outs.append(x.cpu())
    assert torch.equal(outs[0], outs[1])
    st3, c3 = sched.ddim_schedule(4, steps=[3], eta=1.0, device=DEV)  # (and the same row at a step other than 0 does draw)
    c3[0, 4] = 0.3
    outs = []
    for nz in (None, torch.zeros(1, B, T, z)):
        x = x_start().to(DEV).clone()
        on_stream(lambda: e.ddim_schedule_loop(x, lens, st3, c3, eta=1.0, seed=7, noise=nz, use_graph=False, split=False))
        outs.append(x.cpu())
    assert not torch.equal(outs[0], outs[1])


def test_workspace_scales_with_the_evaluations(eng):
    from diffnorm_amd import _lib

    engine, scheduler = eng
    e, sched = eps_engine(engine, "f16"), scheduler.DDPMScheduler(200)
    lib = e.lib
    ws = lambda n: int(lib.dn_ddim_sched_workspace_bytes(e.handle, B, T, n))  # noqa: E731
    full = lambda s: int(lib.dn_ddim_workspace_bytes(e.handle, B, T, s))  # noqa: E731
    for start in (1, 5, 50, 199):
        for n in sorted(n for n in {1, 2, start // 2, start - 1, start} if 1 <= n <= start):
            assert 0 < ws(n) <= full(start), (n, start)
    assert ws(1) < ws(5) < ws(7) < ws(50) < ws(199)  # it grows with n, not with the start step
    st, coef = sched.ddim_schedule(50, sampling_steps=7, device=DEV)
    x = x_start().to(DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    buf = torch.empty(ws(7) + 256, dtype=torch.uint8, device=DEV)
    wp = (buf.data_ptr() + 255) & ~255
    call = lambda nbytes: lib.dn_ddim_sched_loop(e.handle, x.data_ptr(), lens.data_ptr(), B, T, st.data_ptr(), coef.data_ptr(), 7, 200, 0, 0,  # noqa: E731
                                                 None, 0, wp, nbytes, None)
    assert call(ws(7) - 1) == -3 and "dn_ddim_sched_workspace_bytes" in lib.dn_last_error().decode()
    assert call(ws(7)) == 7
    torch.cuda.synchronize()
    assert _lib.DDIM_SCHED_COLS == coef.shape[1]


def test_graph_cache_keeps_the_loops_apart(eng, golden):
    """ddim, schedule, ddim, ddpm, schedule (another list of the same length) on one engine, one workspace and one x address,
    each captured: every one equals its eager run."""
    engine, scheduler = eng
    e = engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype="f16", device=DEV)
    sched = scheduler.DDPMScheduler(200)
    lens = T_(golden("chain_small")["lens"]).to(DEV).int()
    coef, table = sched.ddim_coef_table(DEV), sched.gaussian_table(DEV)
    sa, ca = sched.ddim_schedule(50, sampling_steps=7, device=DEV)
    sb, cb = sched.ddim_schedule(50, steps=[44, 40, 31, 22, 9, 2, 0], device=DEV)
    e._workspace(int(e.lib.dn_ddim_workspace_bytes(e.handle, B, T, 50)))  # one workspace for all of them
    chains = [lambda x, g: e.ddim_loop(x, lens, 50, coef, use_graph=g),
              lambda x, g: e.ddim_schedule_loop(x, lens, sa, ca, use_graph=g, timesteps=200),
              lambda x, g: e.ddim_loop(x, lens, 50, coef, use_graph=g),
              lambda x, g: e.ddpm_loop(x, lens, 8, table, seed=3, use_graph=g),
              lambda x, g: e.ddim_schedule_loop(x, lens, sb, cb, use_graph=g, timesteps=200),
              lambda x, g: e.ddim_schedule_loop(x, lens, sa, ca, eta=0.0, use_graph=g, timesteps=200)]
    x = torch.empty(B, T, CHAIN_VAE.z, device=DEV)
    ws_ptr = e._ws.data_ptr()
    got = []
    stream = torch.cuda.Stream()
    for chain in chains:  # captured, back to back, on one stream (the cache is keyed by the stream-independent arguments)
        x.copy_(x_start())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            chain(x, True)
        torch.cuda.synchronize()
        got.append(x.cpu())
    assert e._ws.data_ptr() == ws_ptr
    for i, chain in enumerate(chains):
        ref = x_start().to(DEV)
        on_stream(lambda: chain(ref, False))
        assert torch.equal(got[i], ref.cpu()), i
    assert not torch.equal(got[1], got[4]) and torch.equal(got[1], got[5])


def test_graph_cache_serves_a_repeated_chain(eng, golden):
    """A served hit of the unconditional loops' graph slot: every loop captured twice back to back on one stream, one workspace and
    one x address (reset to the same start) -- the second call replays the first call's graph, and both equal the eager run bit for
    bit.  Then what the benchmark does, a kept-table continuation from a smaller start step served by the same graph, and a chain
    with another seed, which must not be."""
    engine, scheduler = eng
    e = engine.EpsEngine(O.make_eps_state_dict(CHAIN_EPS, "chain"), CHAIN_EPS, dtype="f16", device=DEV)
    sched = scheduler.DDPMScheduler(200)
    lens = T_(golden("chain_small")["lens"]).to(DEV).int()
    coef, table = sched.ddim_coef_table(DEV), sched.gaussian_table(DEV)
    s0, c0 = sched.ddim_schedule(50, sampling_steps=7, device=DEV)
    s1, c1 = sched.ddim_schedule(50, sampling_steps=7, eta=1.0, device=DEV)
    sd, cd = sched.dpm_schedule(50, sampling_steps=7, device=DEV)
    e._workspace(max(int(e.lib.dn_ddim_workspace_bytes(e.handle, B, T, 50)), int(e.lib.dn_dpm_workspace_bytes(e.handle, B, T, 7))))
    ws_ptr = e._ws.data_ptr()
    chains = [lambda x, g: e.ddpm_loop(x, lens, 8, table, seed=3, use_graph=g),
              lambda x, g: e.ddim_schedule_loop(x, lens, s0, c0, eta=0.0, use_graph=g, timesteps=200),
              lambda x, g: e.ddim_schedule_loop(x, lens, s1, c1, eta=1.0, seed=7, use_graph=g, timesteps=200),
              lambda x, g: e.dpm_schedule_loop(x, lens, sd, cd, use_graph=g, timesteps=200),
              lambda x, g: e.ddim_loop(x, lens, 50, coef, use_graph=g, max_evals=4)]  # (last: the continuation follows it)
    evals = [8, 7, 7, 7, 4]  # each of 3 .. 8 evaluations: long enough to be captured
    x = torch.empty(B, T, CHAIN_VAE.z, device=DEV)
    stream = torch.cuda.Stream()

    def captured(chain, start=None):
        if start is not None:
            x.copy_(start)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            n = chain(x, True)
        torch.cuda.synchronize()
        return n, x.cpu()

    got = []
    for chain, n in zip(chains, evals):
        (n1, first), (n2, second) = captured(chain, x_start()), captured(chain, x_start())
        assert n1 == n2 == n
        assert torch.equal(first, second), len(got)
        got.append(second)
    # x now stands at step 46 of the DDIM chain: continue on the kept table, from the graph captured at start step 50
    n, cont = captured(lambda xx, g: e.ddim_loop(xx, lens, 46, coef, use_graph=g, max_evals=4, keep_table=True))
    assert n == 4
    n, other_seed = captured(lambda xx, g: e.ddpm_loop(xx, lens, 8, table, seed=4, use_graph=g), x_start())
    assert n == 8 and e._ws.data_ptr() == ws_ptr

    def eager(chain, start):
        ref = start.to(DEV).clone()
        on_stream(lambda: chain(ref, False))
        return ref.cpu()

    for i, chain in enumerate(chains):
        assert torch.equal(got[i], eager(chain, x_start())), i
    assert torch.equal(cont, eager(lambda xx, g: e.ddim_loop(xx, lens, 46, coef, use_graph=g, max_evals=4), got[4]))
    assert not torch.equal(other_seed, got[0])
    assert torch.equal(other_seed, eager(lambda xx, g: e.ddpm_loop(xx, lens, 8, table, seed=4, use_graph=g), x_start()))


def test_schedule_graph_observes_run_time_options(eng):
    """As test_sampling_graph_observes_run_time_options asks of dn_ddim_loop: a schedule chain captured under the default K order
    is not replayed after taps_inner changed."""
    from diffnorm_amd import _lib

    engine, scheduler = eng
    cfg = O.EpsConfig(dim=512, latent_dim=128, depth=1, wavenet_layers=2, wavenet_stacks=1)
    e = engine.EpsEngine(O.make_eps_state_dict(cfg, "graph_opts"), cfg, dtype="bf16", device=DEV)
    Bb, Tt = 32, 512
    st, coef = scheduler.DDPMScheduler(200).ddim_schedule(50, sampling_steps=4, device=DEV)
    lens = torch.full((Bb,), Tt, dtype=torch.int32, device=DEV)
    x0 = seeded((Bb, Tt, cfg.latent_dim), 5).to(DEV)
    x = x0.clone()
    loop = lambda xx, g: on_stream(lambda: e.ddim_schedule_loop(xx, lens, st, coef, use_graph=g, timesteps=200))  # noqa: E731
    with _lib.option("taps_inner", 1):
        assert loop(x, True) == 4
    first = x.clone()
    x.copy_(x0)
    with _lib.option("taps_inner", 0):
        loop(x, True)
        ref = x0.clone()
        loop(ref, False)
    assert not torch.equal(first, ref)  # the two K orders differ in the last bits here: the check below can tell them apart
    assert torch.equal(x, ref)


def test_normalize_forwards_the_schedule(golden):
    from diffnorm_amd import normalize as N

    m = _mirror("f32")
    rng = np.random.RandomState(5)
    utts = []
    for i, n in enumerate((11, 17, 9)):
        units = rng.permutation(1000)[:n]  # all different: de-duplication keeps every frame
        utts.append(N.Utterance(f"utt{i}", f"src{i}.wav", 100 + i, torch.from_numpy(rng.randn(n, CHAIN_VAE.dim).astype(np.float32)),
                                units.tolist(), units.tolist()))
    seen = []

    def sample(feat, **kw):
        g = torch.Generator().manual_seed(900 + feat.shape[0] * 100 + feat.shape[1])
        post = torch.randn(feat.shape[0], feat.shape[1], CHAIN_VAE.z, generator=g)
        start = torch.randn(feat.shape[0], feat.shape[1], CHAIN_VAE.z, generator=g)
        seen.append(dict(kw))
        return m.ddim_sample(feat, post_noise=post, start_noise=start, **kw)

    lines = N.normalize(sample, utts, start_step=50, batch_size=2, device=DEV, sampling_steps=5)
    assert [k.get("sampling_steps") for k in seen] == [5, 5] and all("eta" not in k and "seed" not in k for k in seen)
    want = []
    from diffnorm_amd import _lib
    with _lib.option("taps_inner", 2 if _lib.get_option("taps_inner") is None else _lib.get_option("taps_inner")):
        for items in (utts[:2], utts[2:]):
            feat, ref, lens = N.assemble_batch(items, DEV)
            mask = torch.arange(feat.shape[1], device=DEV).view(1, -1) < lens.view(-1, 1)
            pred, _, _, _ = sample(feat, input_mask=mask, cond_scale=1.0, ref_units=ref, start_step=50, sampling_steps=5)
            want += [N.tsv_line(it, p.tolist()) for it, p in zip(items, pred)]
    assert lines == want
    seen.clear()
    plain = N.normalize(sample, utts, start_step=5, batch_size=2, device=DEV)
    assert all(set(k) == {"input_mask", "cond_scale", "ref_units", "start_step"} for k in seen)  # today's call
    every = N.normalize(sample, utts, start_step=5, batch_size=2, device=DEV, sampling_steps=4)
    assert plain == every and len(plain) == 3
    seen.clear()
    N.normalize(sample, utts, start_step=5, batch_size=2, device=DEV, eta=0.5, seed=11)
    assert all(k["eta"] == 0.5 and k["seed"] == 11 and "sampling_steps" not in k for k in seen)
