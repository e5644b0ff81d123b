"""dn_guided_dpm_loop on the GPU: DPM-Solver++(2M) on the prompted, classifier-free-guided prediction as a device loop -- bit for bit
against a host-stepped chain (the model pass of the loop, the existing combine op, the existing dn_dpm2m_step), against the float64
restatement over the oracle's guided prediction, order 1 against dn_guided_ddim_loop, eager against graph, a dirty workspace, the
graph cache shared with dn_guided_ddim_loop, the workspace size and the mirror.

Model, batch, prompt and stream handling are test_hip_guided_schedule.py's: TINY_EPS_COND, DDPMScheduler(200), B = 3, T = 40 (480
latent quads: one block, not a multiple of 256), Tp = 21, ragged lengths.  Schedules from start_step = 50: sampling_steps 1 (a lone
first-order row), 2 (no capture), 3 (the first captured step is second order, the last is lower_order_final), 5, and the explicit
lists [49,37,25,13,0] and [49,30,29,3,0] (a last step to the clean level: a = 0, b = 1; the second with c1 = 28.5).

Host-stepped chain: stepped through forward_with_cond_scale with a per-call time vector AND through the table-row pass (HOST_PASSES);
the two are bitwise equal here, and the loop equals both."""
import types

import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_VAE, seeded
from test_hip_guided_schedule import (B, CFG, DEV, LENS, PLENS, T, TIMESTEPS, TP, Z, Inputs, cond_engine, loop_run, maxerr, new_engine, on_stream,
                                      prompt_cpu, x_start)

pytestmark = pytest.mark.gpu
MODES = [("f32", 1e-3), ("bf16x3", 1e-3), ("f16", 1e-2), ("bf16", 2e-2)]  # test_hip_dpm_solver.py's bars for the same solver
DTYPES = [m for m, _ in MODES]
SCALES = (2.0, 1.0)
SMOOTH = [49, 37, 25, 13, 0]
STEEP = [49, 30, 29, 3, 0]
SELECTIONS = [dict(sampling_steps=1), dict(sampling_steps=2), dict(sampling_steps=3), dict(sampling_steps=5), dict(steps=SMOOTH), dict(steps=STEEP)]
PARITY_SELECTIONS = [dict(sampling_steps=3), dict(sampling_steps=5), dict(steps=SMOOTH)]  # max c1 = 2.62 / 2.35 / 2.74 on this table
# the model pass of the host-stepped chain: "times" = forward_with_cond_scale with a per-call time vector (it is bitwise the table-row pass
# on this model in all four modes, so it is the chain the loop is held to), "table" = forward_cond with the rows of
# cond_time_table_steps, the loop's own form of the pass, and dn_cfg_combine (held to the same bits)
HOST_PASSES = ("times", "table")


@pytest.fixture(scope="module")
def eng():
    from diffnorm_amd import engine, scheduler

    return engine, scheduler.DDPMScheduler(TIMESTEPS)


def sel_key(sel):
    return tuple(sorted((k, str(v)) for k, v in sel.items()))


def dpm_run(e, sched, inp, scale, graph, order=2, **sel):
    """The new loop from x_start() over the schedule -> x on the CPU."""
    st, rows = sched.dpm_schedule(50, order=order, device=DEV, **sel)
    x = x_start().to(DEV).clone()
    n = on_stream(lambda: e.guided_dpm_schedule_loop(x, inp.lens, inp.prompt, inp.plens, st, rows, cond_scale=scale, use_graph=graph, timesteps=TIMESTEPS))
    assert n == st.shape[0]
    return x.cpu()


_runs = {}


def cached_run(engine, sched, dtype, scale, graph, order, sel):
    key = (dtype, scale, graph, order, sel_key(sel))
    if key not in _runs:
        _runs[key] = dpm_run(cond_engine(engine, dtype), sched, Inputs(), scale, graph, order=order, **sel)
    return _runs[key]


def host_chain(e, sched, inp, scale, via, order=2, **sel):
    """The chain stepped from the host: one model pass per step, the guidance combination, then the existing dn_dpm2m_step on the
    guided eps with its own history buffer.  via = "times": `forward_with_cond_scale` at steps[i]; via = "table": `forward_cond` over
    [x ; x] with row i of `cond_time_table_steps` and `dn_cfg_combine` (B rows and no combination at scale 1)."""
    from diffnorm_amd import _lib

    st, rows = sched.dpm_schedule(50, order=order, device=DEV, **sel)
    steps = st.tolist()
    x = x_start().to(DEV).clone()
    hist = torch.full_like(x, float("nan"))  # (row 0 is first order: never read)
    guided = scale != 1.0
    l2, p2, pl2, drop2 = e._guided_inputs(inp.lens, inp.prompt, inp.plens)
    both = torch.empty(2 * B if guided else B, T, Z, device=DEV)
    eps = torch.empty_like(x)

    def run():
        table = e.cond_time_table_steps(steps) if via == "table" else None
        for i, t in enumerate(steps):
            if via == "times":
                ev = e.forward_with_cond_scale(x, torch.full((B,), t, dtype=torch.int32), inp.lens, inp.prompt, inp.plens, cond_scale=scale)
            elif guided:
                tv = torch.full((2 * B,), i, dtype=torch.int32, device=DEV)
                e.forward_cond(torch.cat([x, x]).contiguous(), tv, l2, p2, pl2, drop2, out=both, reuse_prompt=i > 0, time_table=table, table_t0=0)
                _lib.check(e.lib.dn_cfg_combine(both.data_ptr(), float(scale), x.numel(), eps.data_ptr(), _lib.current_stream()), "dn_cfg_combine")
                ev = eps
            else:
                tv = torch.full((B,), i, dtype=torch.int32, device=DEV)
                ev = e.forward_cond(x, tv, inp.lens, inp.prompt, inp.plens, torch.zeros(B, dtype=torch.int32, device=DEV), out=both, reuse_prompt=i > 0,
                                    time_table=table, table_t0=0)
            idx = torch.tensor([i], dtype=torch.int32, device=DEV)
            _lib.check(e.lib.dn_dpm2m_step(x.data_ptr(), ev.data_ptr(), hist.data_ptr(), x.numel(), rows.data_ptr(), idx.data_ptr(), _lib.current_stream()),
                       "dn_dpm2m_step")

    on_stream(run)
    return x.cpu()


# ------------------------------------------------------------------------------------------------------------------ 1: host-stepped chain
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_loop_is_the_host_stepped_chain_bit_for_bit(eng, dtype):
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    for sel in SELECTIONS:
        for scale in SCALES:
            want, table = (host_chain(e, sched, inp, scale, via, **sel) for via in HOST_PASSES)
            assert torch.isfinite(want).all() and torch.equal(want, table), (sel, scale, maxerr(want, table))
            for graph in (False, True):
                got = cached_run(engine, sched, dtype, scale, graph, 2, sel)
                assert torch.equal(got, want), (sel, scale, graph, maxerr(got, want))
    _, rows = sched.dpm_schedule(50, steps=STEEP)
    assert rows[:, 4].max() > 28 and rows[1, 5] != 0 and rows[-1, 2] == 0 and rows[-1, 3] == 1  # what the steep list is here for


# ------------------------------------------------------------------------------------------------------------------ 2: float64 restatement
_refs = {}


def reference_chain(sched, steps, scale, order):
    """scheduler.dpm_chain_reference over float64 rows, stepping the oracle's guided prediction.  Computed once and left unchanged."""
    from diffnorm_amd import scheduler

    key = (tuple(steps), scale, order)
    if key not in _refs:
        sd = O.make_eps_state_dict(CFG, "cond")
        mask, pmask = O.lengths_to_mask(LENS, T), O.lengths_to_mask(PLENS, TP)
        prompt = prompt_cpu()

        def eps_fn(x, t):
            with torch.no_grad():
                return O.eps_forward_with_cond_scale(sd, CFG, x.float(), torch.full((B,), t, dtype=torch.long), mask, prompt, pmask, scale).double()

        _refs[key] = scheduler.dpm_chain_reference(x_start().double(), eps_fn, steps, sched.dpm_rows64(steps, order))
    return _refs[key]


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("dtype,tol", MODES)
def test_chain_matches_the_float64_restatement(eng, dtype, tol, order):
    """Measured on MI355X, worst max abs err on valid frames over the three schedules and both scales, order 2 / order 1: f32 1.2e-6 /
    7.0e-7, bf16x3 9.2e-6 / 5.8e-6, f16 5.4e-4 / 3.9e-4, bf16 4.1e-3 / 2.3e-3 (DESIGN 6 has the table)."""
    engine, sched = eng
    mask = O.lengths_to_mask(LENS, T)
    worst = 0.0
    for sel in PARITY_SELECTIONS:
        steps = sched.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        c1 = float(sched.dpm_rows64(steps, order)[:, 4].max())
        assert c1 <= 3.0, (sel, c1)  # a bar is never asked to absorb an amplified coefficient
        for scale in SCALES:
            want = reference_chain(sched, steps, scale, order)
            got = cached_run(engine, sched, dtype, scale, False, order, sel)
            err = maxerr(got[mask], want[mask])
            worst = max(worst, err)
            print(f"guided dpm chain {steps} order {order} scale {scale} {dtype}: max c1 {c1:.2f}, max abs err {err:.3e} (bar {tol:.0e})")
            assert err < tol, (sel, scale, err)
    print(f"guided dpm worst case order {order} {dtype}: {worst:.3e} (bar {tol:.0e})")


# ------------------------------------------------------------------------------------------------------------------ 3: order 1 is DDIM
@pytest.mark.parametrize("dtype,tol", MODES)
def test_order_one_equals_guided_ddim_at_eta_zero(eng, dtype, tol):
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    mask = O.lengths_to_mask(LENS, T)
    for scale in SCALES:
        ddim = loop_run(e, sched, inp, 50, scale, False, sampling_steps=5)
        one = cached_run(engine, sched, dtype, scale, False, 1, dict(sampling_steps=5))
        err = maxerr(one[mask], ddim[mask])
        print(f"guided dpm order 1 vs guided ddim eta 0, scale {scale} {dtype}: {err:.3e} (bar {tol:.0e})")
        assert err < tol
        two = cached_run(engine, sched, dtype, scale, False, 2, dict(sampling_steps=5))
        assert not torch.equal(two, one)  # (the order reaches the kernel)


# ------------------------------------------------------------------------------------------------------------------ 4: eager, graph, repeats
@pytest.mark.parametrize("dtype", DTYPES)
def test_eager_equals_graph_and_a_repeated_graph_chain_equals_itself(eng, dtype):
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    for sel in SELECTIONS:
        for scale in SCALES:
            eager, graph = (cached_run(engine, sched, dtype, scale, g, 2, sel) for g in (False, True))
            assert torch.equal(eager, graph), (sel, scale)
    # the same buffers twice: the second chain replays the first one's graph over the history the first one left
    for scale in SCALES:
        st, rows = sched.dpm_schedule(50, sampling_steps=5, device=DEV)
        x = torch.empty(B, T, Z, device=DEV)
        got = []
        for _ in range(2):
            x.copy_(x_start())
            on_stream(lambda: e.guided_dpm_schedule_loop(x, inp.lens, inp.prompt, inp.plens, st, rows, cond_scale=scale, use_graph=True, timesteps=TIMESTEPS))
            got.append(x.cpu())
        assert torch.equal(got[0], got[1]) and torch.equal(got[0], cached_run(engine, sched, dtype, scale, False, 2, dict(sampling_steps=5)))


# ------------------------------------------------------------------------------------------------------------------ 5: dirty workspace, refusals
def _raw_call(e, x, inp, st, rows, scale, wp, nbytes, flags=0):
    return e.lib.dn_guided_dpm_loop(e.handle, x.data_ptr(), inp.lens.data_ptr(), inp.prompt.data_ptr(), inp.plens.data_ptr(), B, T, TP, scale,
                                    st.data_ptr(), rows.data_ptr(), st.shape[0], TIMESTEPS, flags, wp, nbytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("scale", [2.0, 1.0])
def test_nothing_is_read_before_it_is_written(eng, dtype, scale):
    """A 4-step chain on a workspace of exactly the reported size filled with 0xFF bytes (NaN in every float `hist` holds) equals the
    zero-filled run, eager and graph.  Refused calls -- DN_LOOP_SPLIT2, an unknown flag, one byte too few, an ascending host list --
    leave x untouched."""
    engine, sched = eng
    e, inp = cond_engine(engine, dtype), Inputs()
    st, rows = sched.dpm_schedule(50, sampling_steps=4, device=DEV)
    assert (rows[1:3, 5] != 0).all()  # rows 1 and 2 read the history
    need = int(e.lib.dn_guided_dpm_workspace_bytes(e.handle, B, T, TP, 4, int(scale != 1.0)))
    assert need > 0
    buf = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    wp = (buf.data_ptr() + 255) & ~255
    outs = []
    for fill in (0x00, 0xFF):
        for flags in (0, 1):
            buf.fill_(fill)
            x = x_start().to(DEV).clone()
            assert on_stream(lambda: _raw_call(e, x, inp, st, rows, scale, wp, need, flags)) == 4, e.lib.dn_last_error()
            outs.append(x.cpu())
    assert torch.isfinite(outs[0]).all()
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    assert torch.equal(outs[0], dpm_run(e, sched, inp, scale, False, sampling_steps=4))
    x = x_start().to(DEV).clone()
    err = lambda: e.lib.dn_last_error().decode()  # noqa: E731
    assert _raw_call(e, x, inp, st, rows, scale, wp, need, flags=2) == -1 and "dn_guided_dpm_loop: DN_LOOP_SPLIT2 is not offered" in err()
    assert _raw_call(e, x, inp, st, rows, scale, wp, need, flags=3) == -1 and "DN_LOOP_SPLIT2" in err()
    assert _raw_call(e, x, inp, st, rows, scale, wp, need, flags=4) == -1 and "dn_guided_dpm_loop: flags=4 (DN_LOOP_GRAPH only)" in err()
    assert _raw_call(e, x, inp, st, rows, scale, wp, need - 1) == -3 and "dn_guided_dpm_workspace_bytes" in err()
    with pytest.raises(ValueError, match="dn_ddim_sched_check"):  # a host list is validated before it is uploaded
        e.guided_dpm_schedule_loop(x, inp.lens, inp.prompt, inp.plens, [3, 30, 49, 50], rows, cond_scale=scale, timesteps=TIMESTEPS)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), x_start())  # refused before anything ran


# ------------------------------------------------------------------------------------------------------------------ 6: graph cache
def test_graph_cache_keeps_the_two_guided_loops_apart(eng):
    """DDIM, DPM, DPM again (served from the cache: the same key), DDIM, DPM on one engine, one workspace, one x address, one prompt and
    one n_steps, each captured: every result equals the same chain run eagerly and captured on a freshly built engine -- observed as
    test_graph_cache_serves_only_the_chain_it_captured observes it."""
    engine, sched = eng
    dtype = "f16"
    e, inp = new_engine(engine, dtype), Inputs()
    sd, cd = sched.ddim_schedule(50, sampling_steps=5, device=DEV)
    sp, cp = sched.dpm_schedule(50, sampling_steps=5, device=DEV)
    ddim = lambda en, x, g: en.guided_ddim_schedule_loop(x, inp.lens, inp.prompt, inp.plens, sd, cd, cond_scale=2.0, use_graph=g, timesteps=TIMESTEPS)  # noqa: E731
    dpm = lambda en, x, g: en.guided_dpm_schedule_loop(x, inp.lens, inp.prompt, inp.plens, sp, cp, cond_scale=2.0, use_graph=g, timesteps=TIMESTEPS)  # noqa: E731
    fresh = {}
    for name, chain in (("ddim", ddim), ("dpm", dpm)):
        for graph in (False, True):
            x = x_start().to(DEV)
            on_stream(lambda: chain(new_engine(engine, dtype), x, graph))
            fresh[name, graph] = x.cpu()
        assert torch.equal(fresh[name, False], fresh[name, True])
    assert not torch.equal(fresh["ddim", True], fresh["dpm", True])
    e._workspace(int(e.lib.dn_guided_dpm_workspace_bytes(e.handle, B, T, TP, 5, 1)))  # one workspace for both (the larger figure)
    ws_ptr = e._ws.data_ptr()
    x = torch.empty(B, T, Z, device=DEV)
    stream = torch.cuda.Stream()
    for name, chain in (("ddim", ddim), ("dpm", dpm), ("dpm", dpm), ("ddim", ddim), ("dpm", dpm)):
        x.copy_(x_start())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            assert chain(e, x, True) == 5
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), fresh[name, True]), name
    assert e._ws.data_ptr() == ws_ptr


# ------------------------------------------------------------------------------------------------------------------ 7: workspace size
def _take(off, nbytes):
    return ((off + 255) & ~255) + nbytes


def guided_ddim_plan_bytes(e, n_steps, guided):
    """dn_guided_ddim_loop's workspace as its header comment lays it out, from the two sizes the model pass and the time table report
    themselves: the pass's own bytes, the prediction, the index vector, the counter, the drop mask, (guided) the 2B-row input, doubled
    lengths, prompt lengths and prompt, the steps, the time table, DN_DDIM_SCHED_COLS coefficient columns, the table's workspace."""
    n = 2 * B if guided else B
    n_cond = e.cond_time_table_steps([0]).shape[1]
    core = int(e.lib.dn_eps_cond_workspace_bytes(e.handle, n, T, TP)) - 256
    off = _take(0, (core + 255) & ~255)
    off = _take(off, n * T * Z * 4)
    off = _take(off, n * 4)
    off = _take(off, 64)
    off = _take(off, n * 4)
    if guided:
        off = _take(off, 2 * B * T * Z * 4)
        off = _take(off, n * 4)
        off = _take(off, n * 4)
        off = _take(off, n * TP * CFG.dim_prompt * 4)
    off = _take(off, n_steps * 4)
    off = _take(off, n_steps * n_cond * 4)
    off = _take(off, n_steps * 5 * 4)
    off = _take(off, int(e.lib.dn_eps_cond_time_table_workspace_bytes(e.handle, n_steps)))
    return off + 256


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_workspace_sizes(eng, dtype):
    engine, _ = eng
    e = cond_engine(engine, dtype)
    for n_steps in (1, 5, 49):
        for guided in (0, 1):
            ddim = int(e.lib.dn_guided_ddim_workspace_bytes(e.handle, B, T, TP, n_steps, guided))
            dpm = int(e.lib.dn_guided_dpm_workspace_bytes(e.handle, B, T, TP, n_steps, guided))
            assert ddim == guided_ddim_plan_bytes(e, n_steps, bool(guided)), (n_steps, guided)  # unchanged by the second entry
            assert dpm >= ddim + B * T * Z * 4
            assert dpm <= ddim + B * T * Z * 4 + n_steps * 4 + 512  # hist, one more coefficient column, alignment
    assert e.lib.dn_guided_dpm_workspace_bytes(None, B, T, TP, 5, 1) == 0 and e.lib.dn_guided_dpm_workspace_bytes(e.handle, B, T, TP, 0, 1) == 0


# ------------------------------------------------------------------------------------------------------------------ 8: mirror
def test_through_the_mirror():
    """LatentDiscreteModel(use_cond=True).prompted_ddim_sample(solver="dpmpp_2m", sampling_steps=5) returns units, counts and recon,
    and equals encode + q_sample + the engine-level loop + decode by hand; solver=None stays the DDIM chain."""
    from diffnorm_amd import ops
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32")
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain"), strict=True)
    ldm = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 64, CHAIN_VAE.z, timesteps=TIMESTEPS, use_cond=True, dtype="f32").to(DEV).eval()
    feat, src = seeded((2, 24, CHAIN_VAE.dim), 91).to(DEV), seeded((2, 30, CHAIN_VAE.dim), 92).to(DEV)
    flen, slen = torch.tensor([24, 15]), torch.tensor([30, 22])
    fmask, smask = O.lengths_to_mask(flen, 24).to(DEV), O.lengths_to_mask(slen, 30).to(DEV)
    post, start = seeded((2, 24, CHAIN_VAE.z), 93), seeded((2, 24, CHAIN_VAE.z), 94)
    lens, plens = flen.to(DEV).int(), slen.to(DEV).int()
    kw = dict(prompt=src, prompt_mask=smask, input_mask=fmask, cond_scale=2.0, post_noise=post, start_noise=start, start_step=50, sampling_steps=5)

    def by_hand(loop):
        z = ldm.speech_decoder.encode_feature(feat, noise=post).transpose(1, 2).contiguous()
        _, sa, s1 = ldm._tables()
        x = ops.q_sample(z, start.to(DEV).contiguous(), sa, s1, torch.full((2,), 50, dtype=torch.int32, device=DEV), 24)
        assert loop(x) == 5
        recon, _, units = ldm.speech_decoder.engine().decode(x, lens, want_logits=False)
        return units.long(), recon

    outs = {}
    for order in (2, 1):
        st, rows = ldm.scheduler.dpm_schedule(50, sampling_steps=5, order=order, device=DEV)
        units, recon = by_hand(lambda x: ldm.model.engine().guided_dpm_schedule_loop(x, lens, src, plens, st, rows, cond_scale=2.0, timesteps=TIMESTEPS))
        toks, match, total, got = ldm.prompted_ddim_sample(feat, solver="dpmpp_2m", solver_order=order, ref_units=units, **kw)
        assert total == int(flen.sum()) and match == total and [t.shape[0] for t in toks] == flen.tolist()
        assert torch.isfinite(got).all() and torch.equal(got, recon)
        assert all(torch.equal(t, units[i, : flen[i]]) for i, t in enumerate(toks))
        outs[order] = got
    assert not torch.equal(outs[1], outs[2])
    sd, cd = ldm.scheduler.ddim_schedule(50, sampling_steps=5, device=DEV)
    units, recon = by_hand(lambda x: ldm.model.engine().guided_ddim_schedule_loop(x, lens, src, plens, sd, cd, cond_scale=2.0, timesteps=TIMESTEPS))
    toks, _, _, got = ldm.prompted_ddim_sample(feat, solver=None, **kw)  # today's path
    assert torch.equal(got, recon) and all(torch.equal(t, units[i, : flen[i]]) for i, t in enumerate(toks))
    with pytest.raises(ValueError, match="eta"):
        ldm.prompted_ddim_sample(feat, solver="dpmpp_2m", eta=0.5, **kw)
