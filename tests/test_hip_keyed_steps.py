"""Keyed per-step noise (`keyed_steps=True`): stochastic chains whose draws do not depend on the batch.

The update that leaves timestep t adds dn_randn_keyed's stream 2 + t of the utterance's key, drawn inside the update kernel.  Because
`ops.randn_keyed(keys, T, Z, 2 + t)` materialises exactly those numbers, everything here but the draws themselves is BIT FOR BIT: a
keyed update / chain against the same update / chain with those numbers injected (tests/test_hip_mirror.py holds the injected path
to the reference), a batch against its utterances run alone, normalize() across batch plans.  The draws are held to the host
restatement of tests/test_hip_chain_start.py (oracle/philox_normal.py's Philox4x32-10 and Box-Muller, third counter word 2 + t,
fourth "STRT") at the bar of tests/test_hip_philox.py.

Across DIFFERENT padded lengths (test_normalize_stochastic_across_padded_lengths) the unit lines must be identical and the
valid-frame reconstructions within twice the bar tests/test_hip_mirror.py holds the mode to against the oracle (1e-3 outside plain
bf16); measured on an MI355X the difference is 0 in f32, bf16x3 and f16 (MEASURED_ACROSS_T), so bit-identity is asserted."""
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, seeded
from test_hip_chain_start import (DEV, EDGE_KEYS, KEYS, LENGTHS, PASS_QUADS, SENTINEL, TIMESTEPS, bits, corpus, device_keyed, host_keyed, i64,
                                  keys_for, ldm_for, same, same_result, sampler_inputs)
from test_hip_philox import BAR, UNIT

pytestmark = pytest.mark.gpu
STEP_TS = [0, 1, 199, 999]
DRAW_SHAPES = [(3, 5, 4), (2, 37, 16)]
STEP_SHAPES = [(3, 7, 4), (1, 1, 128), (5, 3, 8), (2, 1025, 1024)]  # the last: 524 800 quads, a second grid-stride pass over the row boundary
assert STEP_SHAPES[3][0] * STEP_SHAPES[3][1] * STEP_SHAPES[3][2] // 4 > PASS_QUADS > STEP_SHAPES[3][1] * STEP_SHAPES[3][2] // 4
SCHEDULE = [49, 37, 25, 13, 0]
ETA = 0.7
Z = CHAIN_VAE.z


def step_noise(keys, T, steps, z=Z):
    """What a keyed chain over the timesteps `steps` draws, as injected noise [n, B, T, z]."""
    from diffnorm_amd import ops

    return torch.stack([ops.randn_keyed(keys, T, z, 2 + int(t), DEV) for t in steps])


# ------------------------------------------------------------------------------------------ 1. the draws
@pytest.fixture(scope="module")
def step_draws():
    out = {}
    for B, T, Zs in DRAW_SHAPES:
        for t in STEP_TS:
            dev, intact = device_keyed(keys_for(B), T, Zs, 2 + t)
            host, rad = host_keyed(keys_for(B), T, Zs, 2 + t)
            r = float((np.abs(dev.double().numpy() - host) / (UNIT * np.maximum(rad, 1.0))).max())
            print(f"dn_randn_keyed {(B, T, Zs)} stream 2 + {t}: worst {r:.3f} units (bar {BAR})")
            out[((B, T, Zs), t)] = (dev, r, intact)
    return out


@pytest.mark.parametrize("shape", DRAW_SHAPES)
def test_step_streams_draw_the_host_numbers(step_draws, shape):
    for t in STEP_TS:
        dev, r, intact = step_draws[(shape, t)]
        assert intact and dev.shape == shape and torch.isfinite(dev).all() and r <= BAR, (shape, t, r)


def test_step_streams_are_apart(step_draws):
    B, T, Zs = DRAW_SHAPES[1]
    streams = [device_keyed(keys_for(B), T, Zs, s)[0] for s in (0, 1)] + [step_draws[(DRAW_SHAPES[1], t)][0] for t in STEP_TS]
    for i in range(len(streams)):
        for j in range(i):
            assert (streams[i] != streams[j]).float().mean() > 0.99, (i, j)


# ------------------------------------------------------------------------------------------ 2. one keyed update
def schedule(steps=SCHEDULE, eta=ETA):
    from diffnorm_amd import scheduler

    return scheduler.DDPMScheduler(TIMESTEPS).ddim_schedule(50, steps=steps, eta=eta, device=DEV)


def tailed(t):
    """A copy of `t` on the device in a buffer 8 floats longer, the tail a sentinel -> (the view like t, the buffer)."""
    buf = torch.full((t.numel() + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    buf[: t.numel()] = t.reshape(-1).to(DEV)
    return buf[: t.numel()].view(t.shape), buf


def tail_intact(buf):
    return torch.equal(bits(buf[-8:].cpu()), bits(torch.full((8,), SENTINEL)))


def step_keys(B):
    return (KEYS * 2)[:B]


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_keyed_update_is_the_update_on_the_injected_draws(shape):
    from diffnorm_amd import ops

    B, T, Zs = shape
    steps, coef = schedule()
    keys = i64(step_keys(B))
    x0, eps = seeded(shape, 11), seeded(shape, 12).to(DEV)
    for i in (0, 3, 4):
        idx = torch.tensor([i], dtype=torch.int32, device=DEV)
        x, buf = tailed(x0)
        assert ops.ddim_sched_step_keyed(x, eps, keys, coef, steps, idx) is x
        want = ops.ddim_sched_step(x0.to(DEV), eps, coef, steps, idx, noise=ops.randn_keyed(keys, T, Zs, 2 + SCHEDULE[i], DEV))
        torch.cuda.synchronize()
        assert tail_intact(buf) and torch.isfinite(x).all() and same(x, want), (shape, i)
        plain = ops.ddim_sched_step(x0.to(DEV), eps, coef, steps, idx, eta_on=False)
        assert torch.equal(x, plain) == (SCHEDULE[i] == 0), (shape, i)  # timestep 0 applies no noise; every other one does


def test_a_keyed_update_depends_on_key_timestep_frame_and_channel_only():
    from diffnorm_amd import ops

    steps, coef = schedule()
    for shape in STEP_SHAPES[:3]:
        B, T, Zs = shape
        keys = step_keys(B)
        x0, eps = seeded(shape, 11), seeded(shape, 12)
        idx = torch.tensor([1], dtype=torch.int32, device=DEV)
        batch = ops.ddim_sched_step_keyed(x0.to(DEV), eps.to(DEV), i64(keys), coef, steps, idx).cpu()
        pad = lambda t, b: torch.cat([t[b:b + 1], seeded((1, 5, Zs), 13 + b)], dim=1).to(DEV).contiguous()  # another padded length
        for b in range(B):  # the row alone
            alone = ops.ddim_sched_step_keyed(pad(x0, b), pad(eps, b), i64([keys[b]]), coef, steps, idx)
            assert same(alone[0, :T], batch[b]), (shape, b)
        rev = ops.ddim_sched_step_keyed(x0.flip(0).to(DEV).contiguous(), eps.flip(0).to(DEV).contiguous(), i64(keys[::-1]), coef, steps, idx)
        assert same(rev.flip(0), batch), shape  # reversed key order: every row moves, no row changes
        # the timestep is the stream, not the step index: the same timestep at another index of another schedule
        steps2, coef2 = schedule([45, SCHEDULE[1], 7])
        assert int(steps2[1]) == SCHEDULE[1]
        coef2[1] = coef[1]
        other = ops.ddim_sched_step_keyed(x0.to(DEV), eps.to(DEV), i64(keys), coef2, steps2, idx)
        assert same(other, batch), shape
    # across the pass boundary of the big case: row 1 alone
    B, T, Zs = STEP_SHAPES[3]
    x0, eps, keys = seeded(STEP_SHAPES[3], 11), seeded(STEP_SHAPES[3], 12), step_keys(B)
    idx = torch.tensor([0], dtype=torch.int32, device=DEV)
    big = ops.ddim_sched_step_keyed(x0.to(DEV), eps.to(DEV), i64(keys), coef, steps, idx)
    alone = ops.ddim_sched_step_keyed(x0[1:, :40].contiguous().to(DEV), eps[1:, :40].contiguous().to(DEV), i64(keys[1:]), coef, steps, idx)
    assert same(alone[0], big[1, :40])


# ------------------------------------------------------------------------------------------ 3. the scheduled loop
def loop_inputs(m, T=48):
    """-> (engine, x0 [3, T, z] on the device, lengths int32 on the device, keys on the device)."""
    x0 = seeded((3, T, Z), 41).to(DEV)
    return m.model.engine(), x0, torch.tensor([48, 31, 40], dtype=torch.int32, device=DEV), i64(EDGE_KEYS).to(DEV)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16", "bf16"])
def test_keyed_ddim_chain_is_the_injected_path(dtype):
    m = ldm_for(dtype)
    feat, mask, keys, n0, n1 = sampler_inputs()
    eng, x0, lens, kdev = loop_inputs(m)
    for sched_kw in (dict(sampling_steps=4), dict(timestep_schedule=SCHEDULE)):
        ts = m.scheduler.ddim_steps(50, sched_kw.get("sampling_steps"), sched_kw.get("timestep_schedule"))
        assert len(ts) >= 4 and (ts[-1] == 0) == ("timestep_schedule" in sched_kw)
        sn = step_noise(keys, 48, ts)
        kw = dict(input_mask=mask, start_step=50, eta=ETA, **sched_kw)
        for use_graph in (True, False):
            keyed = m.ddim_sample(feat, noise_keys=keys, keyed_steps=True, use_graph=use_graph, **kw)
            want = m.ddim_sample(feat, post_noise=n0, start_noise=n1, step_noise=sn, use_graph=use_graph, **kw)
            assert torch.isfinite(keyed[3]).all() and same_result(keyed, want), (dtype, sched_kw, use_graph)
        # the engine's loop, with and without the two half-batch streams (odd B: the halves are rows 0 | 1 2)
        steps, rows = m.scheduler.ddim_schedule(50, sched_kw.get("sampling_steps"), sched_kw.get("timestep_schedule"), eta=ETA, device=DEV)
        outs = []
        for use_graph in (True, False):
            for split in (True, False):
                xk, xi = x0.clone(), x0.clone()
                assert eng.ddim_schedule_loop(xk, lens, steps, rows, eta=ETA, keys=kdev, use_graph=use_graph, split=split, timesteps=TIMESTEPS) == len(ts)
                eng.ddim_schedule_loop(xi, lens, steps, rows, eta=ETA, noise=sn, use_graph=use_graph, split=split, timesteps=TIMESTEPS)
                torch.cuda.synchronize()
                assert torch.isfinite(xk).all() and same(xk, xi), (dtype, sched_kw, use_graph, split)
                outs.append(xk)
        assert same(outs[0], outs[2]) and same(outs[1], outs[3])  # graph and eager
        assert not same(outs[0], x0)


# ------------------------------------------------------------------------------------------ 4. the other two samplers
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("fixed_large", [False, True])
def test_keyed_ddpm_chain_is_the_injected_path(clip, fixed_large):
    m = ldm_for("f32")
    feat, mask, keys, n0, n1 = sampler_inputs()
    sn = step_noise(keys, 48, range(4, -1, -1))  # row start_step-1-t for step t
    kw = dict(input_mask=mask, start_step=5, clip_denoised=clip, fixed_large=fixed_large)
    for use_graph in (True, False):
        keyed = m.ddpm_sample(feat, noise_keys=keys, keyed_steps=True, use_graph=use_graph, **kw)
        want = m.ddpm_sample(feat, post_noise=n0, start_noise=n1, step_noise=sn, use_graph=use_graph, **kw)
        assert torch.isfinite(keyed[3]).all() and same_result(keyed, want), (clip, fixed_large, use_graph)
    assert not same_result(keyed, m.ddpm_sample(feat, noise_keys=keys, seed=3, **kw))  # (today's seed-drawn chain is another chain)


def test_keyed_ddpm_chain_is_split_invariant():
    """Both half batches draw under the keys.  The seed-drawn chain's second half draws under another seed: it is not."""
    m = ldm_for("f32")
    eng, x0, lens, kdev = loop_inputs(m)
    table = m.scheduler.gaussian_table(DEV)
    outs = {}
    for split in (True, False):
        for use_graph in (True, False):
            x = x0.clone()
            assert eng.ddpm_loop(x, lens, 5, table, keys=kdev, use_graph=use_graph, split=split) == 5
            outs[(split, use_graph)] = x
    torch.cuda.synchronize()
    assert all(same(v, outs[(True, True)]) for v in outs.values()) and torch.isfinite(outs[(True, True)]).all()
    xs, xu = x0.clone(), x0.clone()
    eng.ddpm_loop(xs, lens, 5, table, seed=3, split=True)
    eng.ddpm_loop(xu, lens, 5, table, seed=3, split=False)
    assert same(xs[:1], xu[:1]) and not same(xs[1:], xu[1:])  # the control: rows of the second half change with the split


def test_keyed_prompted_ddim_chain_is_the_injected_path():
    """The tiny conditional model of tests/test_hip_chain_start.py::test_prompted_ddim_sample_with_keys_is_the_injected_path."""
    from diffnorm_amd import ops
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32")
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain"), strict=True)
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 64, Z, timesteps=TIMESTEPS, use_cond=True, dtype="f32").to(DEV).eval()
    feat, src = seeded((2, 24, CHAIN_VAE.dim), 91).to(DEV), seeded((2, 30, CHAIN_VAE.dim), 92).to(DEV)
    fmask, smask = O.lengths_to_mask(torch.tensor([24, 15]), 24).to(DEV), O.lengths_to_mask(torch.tensor([30, 22]), 30).to(DEV)
    keys = i64(KEYS[1:3])
    n0, n1 = ops.randn_keyed(keys, 24, Z, 0, DEV), ops.randn_keyed(keys, 24, Z, 1, DEV)
    sn = step_noise(keys, 24, m.scheduler.ddim_steps(50, 3))
    for scale in (2.0, 1.0):
        kw = dict(input_mask=fmask, cond_scale=scale, start_step=50, sampling_steps=3, eta=ETA)
        for use_graph in (True, False):
            keyed = m.prompted_ddim_sample(feat, src, smask, noise_keys=keys, keyed_steps=True, use_graph=use_graph, **kw)
            want = m.prompted_ddim_sample(feat, src, smask, post_noise=n0, start_noise=n1, step_noise=sn, use_graph=use_graph, **kw)
            assert torch.isfinite(keyed[3]).all() and same_result(keyed, want), (scale, use_graph)
    assert not same_result(keyed, m.prompted_ddim_sample(feat, src, smask, noise_keys=keys, seed=3, **kw))
    for bad in (dict(keyed_steps=True), dict(keyed_steps=True, noise_keys=keys, step_noise=sn), dict(keyed_steps=True, noise_keys=keys, seed=3)):
        with pytest.raises(ValueError, match="keyed_steps"):
            m.prompted_ddim_sample(feat, src, smask, **bad, **kw)
    kw0 = dict(kw, eta=0.0)
    assert same_result(m.prompted_ddim_sample(feat, src, smask, noise_keys=keys, keyed_steps=True, **kw0),
                       m.prompted_ddim_sample(feat, src, smask, noise_keys=keys, **kw0))


# ------------------------------------------------------------------------------------------ 5. batch independence of the samplers
@pytest.mark.parametrize("sampler", ["ddim", "ddpm"])
def test_an_utterance_alone_reproduces_its_rows_of_the_batch(sampler):
    from diffnorm_amd import _lib

    m = ldm_for("f32")
    feat, mask, keys, _, _ = sampler_inputs()
    lens = [48, 31, 40]

    def run(feat, mask, keys, **noise):
        if sampler == "ddim":
            return m.ddim_sample(feat, input_mask=mask, noise_keys=keys, eta=ETA, start_step=50, sampling_steps=4, **noise)
        return m.ddpm_sample(feat, input_mask=mask, noise_keys=keys, start_step=5, **noise)

    with _lib.option("taps_inner", 2):  # routing by shape, as normalize() sets it
        for noise, independent in ((dict(keyed_steps=True), True), (dict(seed=3), False)):
            batch = run(feat, mask, keys, **noise)
            agree = []
            for b, n in enumerate(lens):
                Tb = (n + 7) // 8 * 8  # its own padded length: 48, 32, 40
                alone = run(feat[b:b + 1, :Tb].contiguous(), mask[b:b + 1, :Tb].contiguous(), keys[b:b + 1], **noise)
                agree.append(same(alone[3][0, :n], batch[3][b, :n]) and torch.equal(alone[0][0], batch[0][b]))
            if independent:
                assert agree == [True, True, True], (sampler, agree)
            else:  # the control: seed-drawn step noise is indexed by position in the batch (row 0 at the batch's own T keeps its index)
                assert agree[1:] == [False, False], (sampler, agree)


# ------------------------------------------------------------------------------------------ 6. normalize() with a stochastic chain
def run_plan(dtype, utts, **plan):
    """tests/test_hip_chain_start.py::run_plan with a stochastic chain -> (TSV lines, {utterance: valid-frame reconstruction}, shapes)."""
    from diffnorm_amd import normalize as N
    from diffnorm_amd import sharding

    m = ldm_for(dtype)
    index = {k: i for i, k in enumerate(sharding.utterance_keys(5, range(len(utts))).tolist())}
    recons, shapes = {}, []

    def sample(feat, **kw):
        assert kw["keyed_steps"] is True and kw["eta"] == 0.5 and "seed" not in kw
        out = m.ddim_sample(feat, **kw)
        shapes.append(tuple(feat.shape[:2]))
        for b, (k, n) in enumerate(zip(kw["noise_keys"].tolist(), kw["input_mask"].sum(1).tolist())):
            recons[index[k]] = out[3][b, :n].cpu()
        return out

    lines = N.normalize(sample, utts, start_step=50, device=DEV, noise_seed=5, eta=0.5, sampling_steps=3, keyed_steps=True, **plan)
    assert sorted(recons) == list(range(len(utts))) and all(recons[i].shape[0] == n for i, n in enumerate(LENGTHS))
    return lines, recons, shapes


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16"])
def test_normalize_stochastic_does_not_depend_on_the_batches_at_one_padded_length(dtype):
    utts = corpus()
    lines_a, rec_a, shapes_a = run_plan(dtype, utts, batch_size=4, pad_multiple=64)
    lines_b, rec_b, shapes_b = run_plan(dtype, utts, max_tokens=192, pad_multiple=64)
    assert shapes_a == [(4, 64), (4, 64), (3, 64)] and shapes_b == [(3, 64), (3, 64), (3, 64), (2, 64)]
    assert lines_a == lines_b and len(lines_a) == len(utts)
    worst = max((rec_a[i].double() - rec_b[i].double()).abs().max().item() for i in rec_a)
    print(f"{dtype}: eta 0.5, largest valid-frame reconstruction difference across batch compositions at T = 64: {worst:.3e}")
    assert all(same(rec_a[i], rec_b[i]) for i in rec_a), worst


# largest valid-frame reconstruction difference between the two plans below, measured on an MI355X: 0 in every mode, so the assertion is
# bit-identity
MEASURED_ACROSS_T = {"f32": 0.0, "bf16x3": 0.0, "f16": 0.0}


@pytest.mark.parametrize("dtype", ["f32", "bf16x3", "f16"])
def test_normalize_stochastic_across_padded_lengths(dtype):
    utts = corpus()
    lines_a, rec_a, shapes_a = run_plan(dtype, utts, batch_size=4, pad_multiple=8)
    lines_b, rec_b, shapes_b = run_plan(dtype, utts, max_tokens=192, pad_multiple=8)
    assert shapes_a == [(4, 64), (4, 56), (3, 56)] and shapes_b == [(3, 64), (3, 56), (3, 56), (2, 40)]
    worst = max((rec_a[i].double() - rec_b[i].double()).abs().max().item() for i in rec_a)
    print(f"{dtype}: eta 0.5, largest valid-frame reconstruction difference across padded lengths: {worst:.3e} "
          f"(recorded {MEASURED_ACROSS_T[dtype]})")
    assert lines_a == lines_b
    assert worst <= 2 * 1e-3
    assert worst == MEASURED_ACROSS_T[dtype] == 0.0 and all(same(rec_a[i], rec_b[i]) for i in rec_a), worst


# ------------------------------------------------------------------------------------------ 7. the graph cache
def test_a_captured_step_reads_the_keys_from_memory():
    m = ldm_for("f32")
    eng, x0, lens, _ = loop_inputs(m)
    steps, rows = m.scheduler.ddim_schedule(50, 4, eta=ETA, device=DEV)
    table = m.scheduler.gaussian_table(DEV)
    x = torch.empty_like(x0)  # one latent buffer for every chain: its address is part of the graph key

    def sched(use_graph, **noise):
        x.copy_(x0)
        eng.ddim_schedule_loop(x, lens, steps, rows, eta=ETA, use_graph=use_graph, timesteps=TIMESTEPS, **noise)
        return x.clone()

    def ddpm(use_graph, **noise):
        x.copy_(x0)
        eng.ddpm_loop(x, lens, 5, table, use_graph=use_graph, **noise)
        return x.clone()

    for run in (sched, ddpm):
        ka, kb, kc = (i64(k).to(DEV) for k in (EDGE_KEYS, KEYS[3:6], KEYS[4:7]))
        want = {name: run(False, keys=k.clone()) for name, k in (("a", ka), ("b", kb), ("c", kc))}
        assert not same(want["a"], want["b"]) and not same(want["b"], want["c"])
        assert same(run(True, keys=ka), want["a"])  # captured under ka's address
        ka.copy_(kc)  # the same address, new contents: a hit whose replays must draw the new numbers
        assert same(run(True, keys=ka), want["c"])
        assert same(run(True, keys=kb), want["b"])  # another tensor: a miss
        # a keyed chain behind a seed-drawn one on the same buffers, and the other way round
        seeded_want = run(False, seed=3)
        assert same(run(True, seed=3), seeded_want) and same(run(True, keys=kb), want["b"]) and same(run(True, seed=3), seeded_want)
        assert not same(seeded_want, want["b"])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 8. refusals
def test_refused_arguments_write_nothing():
    from diffnorm_amd import _lib

    lib = _lib.load()
    m = ldm_for("f32")
    eng, x0, lens, _ = loop_inputs(m)
    steps, coef = schedule()
    table = m.scheduler.gaussian_table(DEV)
    B, T, Zs = 2, 3, 8
    n = 3 * 48 * Z  # (the loops' latent; the single update uses its first B T Zs floats)
    xbuf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    eps = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
    keys = torch.zeros(4, dtype=torch.int64, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = _lib.current_stream()
    X_, E_, K_, C_, S_, I_ = (v.data_ptr() for v in (xbuf, eps, keys, coef, steps, idx))

    def step(x=X_, eps=E_, keys=K_, B=B, T=T, Z=Zs, coef=C_, steps=S_, idx=I_):
        return lib.dn_ddim_sched_step_keyed(x, eps, keys, B, T, Z, coef, steps, idx, s)

    wp, wn = eng._aligned_workspace(lib.dn_ddim_sched_workspace_bytes(eng.handle, 3, 48, len(SCHEDULE)))

    def loop(keys=K_, flags=0, x=X_):
        return lib.dn_ddim_sched_loop_keyed(eng.handle, x, lens.data_ptr(), 3, 48, S_, C_, len(SCHEDULE), TIMESTEPS, keys, flags, wp, wn, s)

    def ancestral(keys=K_):
        return lib.dn_ddpm_loop_keyed(eng.handle, X_, lens.data_ptr(), 3, 48, 5, 0, table.data_ptr(), TIMESTEPS, 0, keys, 0, wp, wn, s)

    def guided(keys=K_, flags=0):  # (an unconditional model is refused whatever else is passed: the keys are looked at first)
        return lib.dn_guided_ddim_loop_keyed(eng.handle, X_, lens.data_ptr(), E_, lens.data_ptr(), 3, 48, 4, 2.0, S_, C_, len(SCHEDULE), TIMESTEPS,
                                             keys, flags, wp, wn, s)

    bad = [lambda: step(keys=None), lambda: step(keys=K_ + 4), lambda: step(Z=6), lambda: step(Z=0), lambda: step(x=None), lambda: step(eps=None),
           lambda: step(x=X_ + 4), lambda: step(eps=E_ + 8), lambda: step(B=0), lambda: step(T=0), lambda: step(coef=None),
           lambda: step(steps=None), lambda: step(idx=None),
           lambda: loop(keys=None), lambda: loop(keys=K_ + 4), lambda: loop(flags=64), lambda: loop(flags=4), lambda: loop(x=None),
           lambda: ancestral(keys=None), lambda: ancestral(keys=K_ + 4),
           lambda: guided(keys=None), lambda: guided(keys=K_ + 4), lambda: guided(flags=64), lambda: guided()]
    for i, call in enumerate(bad):
        with pytest.raises(_lib.DiffNormHipError):
            _lib.check(call(), f"case {i}")
    torch.cuda.synchronize()
    assert torch.equal(bits(xbuf.cpu()), bits(torch.full((n + 8,), SENTINEL)))
    xbuf[:n] = x0.reshape(-1)
    assert step() == 0 and loop() == len(SCHEDULE) and ancestral() == 5  # and the good calls are taken
    torch.cuda.synchronize()
    assert torch.isfinite(xbuf[:n]).all() and tail_intact(xbuf)


def test_keyed_steps_refusals_and_chains_with_nothing_to_draw():
    m = ldm_for("f32")
    feat, mask, keys, n0, n1 = sampler_inputs()
    kw = dict(input_mask=mask, start_step=50, sampling_steps=4)
    sn = step_noise(keys, 48, m.scheduler.ddim_steps(50, 4))
    for bad in (dict(), dict(noise_keys=keys, step_noise=sn), dict(noise_keys=keys, seed=3)):
        with pytest.raises(ValueError, match="keyed_steps"):
            m.ddim_sample(feat, keyed_steps=True, eta=ETA, **bad, **kw)
    for bad in (dict(), dict(noise_keys=keys, step_noise=step_noise(keys, 48, range(4, -1, -1))), dict(noise_keys=keys, seed=3)):
        with pytest.raises(ValueError, match="keyed_steps"):
            m.ddpm_sample(feat, keyed_steps=True, input_mask=mask, start_step=5, **bad)
    eng, x0, lens, kdev = loop_inputs(m)
    steps, rows = m.scheduler.ddim_schedule(50, 4, eta=ETA, device=DEV)
    for bad in (dict(noise=sn), dict(seed=3), dict(eta=0.0)):
        with pytest.raises(ValueError):
            eng.ddim_schedule_loop(x0.clone(), lens, steps, rows, **dict(dict(eta=ETA, keys=kdev), **bad))
    for extra in (dict(eta=0.0), dict(solver="dpmpp_2m"), dict(eta=0.0, sampling_steps=None, start_step=5)):
        kw2 = dict(kw, **extra)
        assert same_result(m.ddim_sample(feat, noise_keys=keys, keyed_steps=True, **kw2), m.ddim_sample(feat, noise_keys=keys, **kw2)), extra
    # and without the switch, keys leave the per-step noise where it was: drawn from `seed`
    a = m.ddim_sample(feat, noise_keys=keys, eta=ETA, seed=3, **kw)
    assert same_result(a, m.ddim_sample(feat, post_noise=n0, start_noise=n1, eta=ETA, seed=3, **kw))
    assert not same_result(a, m.ddim_sample(feat, noise_keys=keys, keyed_steps=True, eta=ETA, **kw))
