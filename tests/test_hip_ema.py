"""GPU: the EMA of the trained parameters.  dn_ema_update / dn_adam_step_ema (csrc/optim.hip) against each other bit for bit and
against the reference's real EMA class (tests/golden/ema.npz, tools/gen_golden_ema.py); the trainers with an optim.EmaSchedule
(updates unchanged, the EMA the float64 recurrence over the recorded parameters); sampling from the EMA (`sample_from="ema"`:
packed tensors bit-identical to an engine built from ema_state_dict(), same device addresses); the plugin's two optimizer paths;
checkpoints.

The value bound is derived, not measured: an applied update is e' = fl(p * b + fl(e * a)) with a + b = 1 up to their own rounding --
two fp32 roundings of values no larger than max(|e|, |p|), i.e. at most 2 * 2^-24 * max(|e|, |p|) of new error, while the old error is
multiplied by a < 1.  After k applied updates: |error| <= k * 2^-23 * max(|e|, |p|) elementwise, the maximum taken over the trajectory."""
import ctypes as C
import logging
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, seeded
from test_hip_train import _FairseqAdamThroughData, _batch
from test_hip_train import _sample as _plugin_sample
from test_hip_train_sample import B, LENS, T, _units, same_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_BIG = 4 * (2 * 2048 * 256 + 300) + 3  # at 8 workgroups per CU: one paired grid-stride iteration, the single tail, the scalar tail
SIZES = [3, 4, 1027, N_BIG]
EPS23 = 2.0 ** -23


def _stream():
    from diffnorm_amd import _lib

    return _lib.current_stream()


# ------------------------------------------------------------------------------------------ 1. operators, bits
@pytest.fixture(scope="module")
def adam_inputs():
    """n -> (param, grad, exp_avg, exp_avg_sq, ema) on the device: made once, only ever cloned."""
    out = {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        p, gr, e = (torch.randn(n, generator=g) for _ in range(3))
        m, v = 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
        out[n] = tuple(t.to(DEV) for t in (p, gr, m, v, e))
    return out


def _adam(n, inputs, fused, full, decay=0.97, ema_fill=None):
    """One Adam step on copies of `inputs`; fused: dn_adam_step_ema.  full: clipping, weight decay and a device gradient scale on.
    -> (param, exp_avg, exp_avg_sq, bf16 copy, ema)."""
    from diffnorm_amd import _lib

    lib = _lib.load()
    p, gr, m, v, e = (t.clone() for t in inputs)
    if ema_fill is not None:
        e.fill_(ema_fill)
    bf = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    scratch = torch.empty(1025, device=DEV)
    scale_dev = torch.tensor([0.25], device=DEV) if full else None
    _lib.check(lib.dn_grad_sumsq(gr.data_ptr(), n, scratch.data_ptr(), scratch[1024:].data_ptr(), 0, _stream()), "sumsq")
    hp = _lib.AdamParams(lr=3e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01 if full else 0.0, max_norm=0.5 if full else 0.0, step=3,
                         grad_scale=0.5 if full else 1.0, grad_scale_dev=_lib.ptr(scale_dev))
    head = (p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, C.byref(hp), scratch[1024:].data_ptr(), bf.data_ptr())
    if fused:
        _lib.check(lib.dn_adam_step_ema(*head, e.data_ptr(), decay, _stream()), "dn_adam_step_ema")
    else:
        _lib.check(lib.dn_adam_step(*head, _stream()), "dn_adam_step")
    torch.cuda.synchronize()
    return p, m, v, bf, e


@pytest.mark.parametrize("full", [False, True], ids=["plain", "clip+wd+scale"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_is_the_adam_step_plus_the_ema_pass(adam_inputs, n, full):
    from diffnorm_amd import optim

    want = _adam(n, adam_inputs[n], False, full)
    got = _adam(n, adam_inputs[n], True, full)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "bf16 copy"), got, want):
        assert torch.equal(a, b), (n, name)
    assert not torch.equal(got[0], adam_inputs[n][0])
    ema = adam_inputs[n][4].clone()
    optim.ema_update(ema, got[0], 0.97)
    assert torch.equal(got[4], ema), n
    assert not torch.equal(ema, adam_inputs[n][4]) and not torch.equal(ema, got[0])


@pytest.mark.parametrize("n", SIZES)
def test_decay_zero_is_an_exact_copy_that_does_not_read_the_ema(adam_inputs, n):
    from diffnorm_amd import optim

    p, _, _, _, e = _adam(n, adam_inputs[n], True, True, decay=0.0, ema_fill=float("nan"))
    assert torch.equal(e, p) and bool(torch.isfinite(e).all())
    e2 = torch.full((n,), float("nan"), device=DEV)
    optim.ema_update(e2, p, 0.0)
    assert torch.equal(e2, p)


def test_arguments_are_checked_on_the_host():
    from diffnorm_amd import _lib, optim

    lib = _lib.load()
    a, b = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    for args in ((None, b.data_ptr(), 16, 0.9), (a.data_ptr(), None, 16, 0.9), (a.data_ptr(), b.data_ptr(), 0, 0.9), (a.data_ptr(), b.data_ptr(), 16, 1.0),
                 (a.data_ptr(), b.data_ptr(), 16, -0.1), (a.data_ptr() + 4, b.data_ptr(), 8, 0.9)):
        assert lib.dn_ema_update(*args, None) == -1 and b"dn_ema_update" in lib.dn_last_error(), args
    hp = _lib.AdamParams(lr=1e-3, beta1=0.9, beta2=0.98, eps=1e-8, step=1)
    bufs = [torch.zeros(16, device=DEV) for _ in range(4)]
    head = tuple(t.data_ptr() for t in bufs) + (16, C.byref(hp), None, None)
    assert lib.dn_adam_step_ema(*head, None, 0.9, None) == -1 and b"dn_adam_step_ema" in lib.dn_last_error()  # no EMA: use dn_adam_step
    assert lib.dn_adam_step_ema(*head, a.data_ptr(), 1.0, None) == -1
    assert lib.dn_adam_step_ema(*head, a.data_ptr() + 4, 0.9, None) == -1
    with pytest.raises(ValueError):
        optim.ema_update(a, torch.zeros(8, device=DEV), 0.9)


# ------------------------------------------------------------------------------------------ 2. operator, values
def _recurrence(params, schedule, e0):
    """The float64 recurrence with the kernel's fp32-rounded scalars over `params` (update 1 ..), from e0.
    -> (EMA after every update, applied updates so far, elementwise max(|e|, |p|) so far)."""
    e = e0.double().clone()
    big = e.abs()
    out, k = [], 0
    for u, p in enumerate(params, start=1):
        apply, decay = schedule(u)
        p = p.double()
        big = torch.maximum(big, p.abs())
        if apply:
            a, b = float(np.float32(decay)), float(np.float32(1.0 - decay))
            e = p.clone() if decay == 0.0 else p * b + e * a
            k += 1
        out.append((e.clone(), k, big.clone()))
    return out


@pytest.mark.parametrize("i", range(3))
def test_ema_update_follows_the_reference_class(golden, i):
    from diffnorm_amd import optim

    g = golden("ema")
    decay, start, freq = g["configs"][i]
    params = torch.from_numpy(g["params"])
    make = lambda: optim.EmaSchedule(float(decay), int(start), int(freq))
    want64 = _recurrence(params[1:], make(), params[0])
    sched = make()
    ema = params[0].clone().to(DEV)  # the reference deep-copies the model
    for u in range(1, 8):
        apply, d = sched(u)
        assert apply == bool(g[f"c{i}/applied"][u - 1])
        if apply:
            optim.ema_update(ema, params[u].to(DEV), d)
        got = ema.cpu().double()
        e64, k, big = want64[u - 1]
        bound = k * EPS23 * big
        ref = torch.from_numpy(g[f"c{i}/ema"][u - 1]).double()
        err_ref, err_64 = (got - ref).abs(), (got - e64).abs()
        print(f"config {i} update {u}: k={k} worst error / bound vs the reference {float((err_ref / bound.clamp(min=1e-30)).max()):.3f}, "
              f"vs float64 {float((err_64 / bound.clamp(min=1e-30)).max()):.3f}")
        assert bool((err_ref <= bound).all()), (i, u)
        assert bool((err_64 <= bound).all()), (i, u)


# ------------------------------------------------------------------------------------------ 3. trainers
def _vae_engine(dtype):
    from diffnorm_amd import training

    c = CHAIN_VAE
    return training.VaeTrainEngine(O.make_vae_state_dict(c, "train"), dim=c.dim, latent_dim=c.latent_dim, dtype=dtype, device=DEV, depth=c.depth,
                                   heads=c.heads, dim_head=c.dim_head, stacks=c.stacks, layers=c.layers)


def _run_vae(g, dtype, ema_cfg, updates=5):
    """-> (engine, trainer, master snapshots [initial, after update 1, ..], logged losses)."""
    from diffnorm_amd import optim, training

    eng = _vae_engine(dtype)
    feat, units, lens = _batch(g)
    sched = None if ema_cfg is None else optim.EmaSchedule(*ema_cfg)
    tr = training.VaeTrainer(eng, lr=3e-3, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0, ema=sched)
    sample = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": lens, "ntokens": int(lens.sum()), "nsentences": 3}
    snaps, logs = [eng.master.clone()], []
    for it in range(updates):
        logged, norm = tr.train_step([sample], noises=[torch.from_numpy(g[f"traj_noise{it}"])])
        snaps.append(eng.master.clone())
        logs.append(torch.cat([logged, norm.reshape(1)]).clone())
    torch.cuda.synchronize()
    return eng, tr, snaps, logs


def _ldm(dtype, sample_dtype=None, sample_from="model"):
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype, sample_dtype=sample_dtype)
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain"), strict=True)
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), CHAIN_EPS.dim, CHAIN_VAE.z, timesteps=200, dtype=dtype, sample_dtype=sample_dtype,
                            sample_from=sample_from)
    m.model.load_state_dict(dict(O.make_eps_state_dict(CHAIN_EPS, "chain"), **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    return m.to(DEV).eval()


def _eps_step(tr, it):
    z = CHAIN_VAE.z
    batch = {"reduce_target": seeded((B, T, CHAIN_VAE.dim), 31), "reduce_target_unit": _units(), "reduce_target_lengths": LENS,
             "ntokens": int(LENS.sum()), "nsentences": B}
    draws = {"times": torch.tensor([20 + 50 * it, 140 - 30 * it]), "post_noise": seeded((B, T, z), 50 + it),
             "jitter_noise": seeded((B, T, z), 60 + it).to(DEV), "true_noise": seeded((B, T, z), 70 + it).to(DEV)}
    return tr.train_step([batch], noises=[draws])


def _run_eps(dtype, ema_cfg, updates=3, sample_dtype=None, sample_from="model"):
    from diffnorm_amd import optim, training

    m = _ldm(dtype, sample_dtype, sample_from)
    sched = None if ema_cfg is None else optim.EmaSchedule(*ema_cfg)
    tr = training.DiffusionTrainer(m, lr=3e-3, clip_norm=2.0, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0, ema=sched)
    eng = m._train_engine
    snaps, logs = [eng.master.clone()], []
    for it in range(updates):
        logged, norm = _eps_step(tr, it)
        snaps.append(eng.master.clone())
        logs.append(torch.cat([logged, norm.reshape(1)]).clone())
    torch.cuda.synchronize()
    return eng, tr, snaps, logs, m


def _check_ema_run(plain, run, ema_cfg, what):
    from diffnorm_amd import optim

    eng0, tr0, snaps0, logs0 = plain[:4]
    eng, tr, snaps, logs = run[:4]
    assert eng0.ema is None and eng.ema is not None and eng.ema.dtype == torch.float32 and eng.ema.numel() == eng.n_params
    assert eng.ema.data_ptr() % 256 == 0
    for u, (a, b) in enumerate(zip(snaps, snaps0)):
        assert torch.equal(a, b), (what, "master after update", u)
    assert torch.equal(tr.adam.exp_avg, tr0.adam.exp_avg) and torch.equal(tr.adam.exp_avg_sq, tr0.adam.exp_avg_sq), what
    for u, (a, b) in enumerate(zip(logs, logs0)):
        assert torch.equal(a, b), (what, "logged losses of update", u + 1)
    if eng.work is not eng.master:
        assert torch.equal(eng.work, eng0.work), what
    e64, k, big = _recurrence([s.cpu() for s in snaps[1:]], optim.EmaSchedule(*ema_cfg), snaps[0].cpu())[-1]
    assert eng.ema_count == k and k > 0, (what, eng.ema_count, k)
    err, bound = (eng.ema.cpu().double() - e64).abs(), k * EPS23 * big
    print(f"{what} {ema_cfg}: k={k}, worst error / bound {float((err / bound.clamp(min=1e-30)).max()):.3f}")
    assert bool((err <= bound).all()), what
    assert not torch.equal(eng.ema, eng.master)


EMA_CFGS = [(0.999, 0, 1), (0.9, 2, 2)]


@pytest.mark.parametrize("dtype", ["bf16", "f32", "bf16x3"])
def test_vae_trainer_with_ema(golden, dtype):
    from diffnorm_amd import packing

    g = golden("vae_train")
    plain = _run_vae(g, dtype, None)
    for cfg in EMA_CFGS:
        run = _run_vae(g, dtype, cfg)
        _check_ema_run(plain, run, cfg, f"VaeTrainer {dtype}")
        if dtype == "bf16x3":  # the split work copy is still made from master (dn_vae_train_refresh), whatever the EMA does
            eng = run[0]
            assert same_bytes(eng.work, packing.split_rows(eng.master.cpu(), weight=True).to(DEV))


def test_diffusion_trainer_with_ema():
    plain = _run_eps("bf16", None)
    for cfg in EMA_CFGS:
        _check_ema_run(plain, _run_eps("bf16", cfg), cfg, "DiffusionTrainer bf16")


# ------------------------------------------------------------------------------------------ 4. sampling from the EMA
def _count_refreshes(e):
    calls = []
    inner = e.refresh_from

    def counted(*a, **kw):
        calls.append(kw.get("source", a[1] if len(a) > 1 else "model"))
        return inner(*a, **kw)

    e.refresh_from = counted
    return calls


def test_model_samples_from_the_ema():
    from diffnorm_amd import engine, optim, training

    m = _ldm("bf16", "f16", "ema")
    tr = training.DiffusionTrainer(m, lr=3e-3, clip_norm=2.0, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0, ema=optim.EmaSchedule(0.9))
    eng = m._train_engine
    e = m.model.engine()
    assert e.dtype == 3  # DN_F16
    ptrs = [t.data_ptr() for t in e.tensors]
    calls = _count_refreshes(e)
    for it in range(3):
        _eps_step(tr, it)
    assert m.model.engine() is e and calls == ["ema"] and [t.data_ptr() for t in e.tensors] == ptrs
    fresh = engine.EpsEngine(eng.ema_state_dict(), CHAIN_EPS, dtype="f16", device=DEV)
    for i, (a, b) in enumerate(zip(e.tensors, fresh.tensors)):
        assert same_bytes(a, b), f"packed tensor {i}"
    x, t = seeded((B, T, CHAIN_VAE.z), 35).to(DEV), torch.tensor([3, 120])
    from_model = engine.EpsEngine(eng.state_dict(), CHAIN_EPS, dtype="f16", device=DEV).forward(x, t, LENS).clone()
    got = e.forward(x, t, LENS).clone()
    assert torch.equal(got, fresh.forward(x, t, LENS)) and not torch.equal(got, from_model)


@pytest.mark.parametrize("sample_dtype", ["f16", "bf16x3"])
def test_vae_samples_from_the_ema(golden, sample_dtype):
    from diffnorm_amd import engine, optim, training
    from diffnorm_amd.latent_module import SpeechVAEEncoderDecoder

    g = golden("vae_train")
    c = CHAIN_VAE
    vae = SpeechVAEEncoderDecoder(dim=c.dim, latent_dim=c.latent_dim, dtype="bf16", sample_dtype=sample_dtype, sample_from="ema")
    vae.load_state_dict(O.make_vae_state_dict(c, "train"), strict=True)
    vae.to(DEV)
    eng = vae.enable_training()
    with pytest.raises(ValueError, match="store-ema"):  # sampling from an EMA nobody keeps
        vae.engine()
    tr = training.VaeTrainer(eng, lr=3e-3, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0, ema=optim.EmaSchedule(0.9, 0, 2))
    e = vae.engine()
    ptrs = [t.data_ptr() for t in e.tensors]
    calls = _count_refreshes(e)
    feat, units, lens = _batch(g)
    sample = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": lens, "ntokens": int(lens.sum()), "nsentences": 3}
    tr.train_step([sample], noises=[torch.from_numpy(g["traj_noise0"])])
    assert vae.engine() is e and calls == [] and eng.ema_count == 0  # update_freq 2: the update that skips the EMA repacks nothing
    tr.train_step([sample], noises=[torch.from_numpy(g["traj_noise1"])])
    tr.train_step([sample], noises=[torch.from_numpy(g["traj_noise2"])])
    assert vae.engine() is e and calls == ["ema"] and eng.ema_count == 1 and [t.data_ptr() for t in e.tensors] == ptrs
    build = lambda sd: engine.VaeEngine(sd, dim=c.dim, latent_dim=c.latent_dim, dtype=sample_dtype, device=DEV)
    fresh = build(eng.ema_state_dict())
    for i, (a, b) in enumerate(zip(e.tensors, fresh.tensors)):
        assert same_bytes(a, b), (sample_dtype, f"packed tensor {i}")
    got, want, other = e.encode_params(feat).clone(), fresh.encode_params(feat).clone(), build(eng.state_dict()).encode_params(feat).clone()
    assert torch.equal(got, want) and not torch.equal(got, other)
    with pytest.raises(ValueError):
        SpeechVAEEncoderDecoder(dim=c.dim, latent_dim=c.latent_dim, sample_from="average")


# ------------------------------------------------------------------------------------------ 5. plugin, checkpoints
def _plugin(**flags):
    from diffnorm_amd import fairseq_plugin  # noqa: F401  (registers the names)
    from diffnorm_amd.fairseq_plugin import registry

    c = CHAIN_VAE
    args = types.SimpleNamespace(arch="speech_vae_decoder", criterion="speech_vae_decoder_loss", latent_dim=c.latent_dim, feature_dim=c.dim,
                                 hip_dtype="f32", target_code_size=1000, data="", optimizer="adam", lr=[1e-3], **flags)
    task = registry.TASK_REGISTRY["speech_decoder"].setup_task(args)
    model = task.build_model(args)
    model.load_state_dict({"encoder." + k: v for k, v in O.make_vae_state_dict(c, "train").items()}, strict=True)
    model.to(DEV)
    model.encoder.attn_dropout = 0.0
    return task, model, task.build_criterion(args)


EMA_FLAGS = dict(store_ema=True, ema_decay=0.9, ema_start_update=0, ema_update_freq=1, hip_sample_from="ema")


def test_plugin_steps_the_ema_under_both_optimizers(golden, tmp_path):
    from diffnorm_amd import checkpoint, optim

    g = golden("vae_train")
    task, model, criterion = _plugin(**EMA_FLAGS)
    task2, model2, criterion2 = _plugin(**EMA_FLAGS)
    eng, eng2 = model.encoder._train_engine, model2.encoder._train_engine
    assert eng.ema is not None and torch.equal(eng.ema, eng.master) and model.encoder.sample_from == "ema"
    flat = optim.FlatOptimizer(eng, lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
    ext = _FairseqAdamThroughData(model2, lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
    for it in range(3):
        sample = _plugin_sample(g, torch.from_numpy(g[f"traj_noise{it}"]))
        for t, mdl, crit, opt in ((task, model, criterion, flat), (task2, model2, criterion2, ext)):
            opt.zero_grad()
            _, n, _ = t.train_step(sample, mdl, crit, opt, it)
            opt.multiply_grads(1.0 / n)
            t.optimizer_step(opt, mdl, it)
        rel = float((eng.ema - eng2.ema).norm() / eng.ema.norm())
        assert rel < 1e-6, (it, rel)
        assert not torch.equal(eng.ema, eng.master) and not torch.equal(eng2.ema, eng2.master)
    assert eng.ema_count == 3 and eng2.ema_count == 3 and flat.ema is task.ema_schedule and task.ema_decay == 0.9
    assert model.encoder.engine().dtype == 0 and len(model.encoder.engine().tensors) > 0  # the inference engine comes up from the EMA
    # extra_state["ema"] under the model's key names, next to the schedule's state
    path = str(tmp_path / "plugin.pt")
    state = checkpoint.save_checkpoint(path, model, optimizer=flat, num_updates=3)
    assert set(state["extra_state"]["ema"]) == set(model.state_dict()) and all(k.startswith("encoder.") for k in state["extra_state"]["ema"])
    assert state["extra_state"]["ema_schedule"] == task.ema_schedule.state_dict()
    task3, model3, _ = _plugin(**EMA_FLAGS)
    flat3 = optim.FlatOptimizer(model3.encoder._train_engine, lr=1e-3, betas=(0.9, 0.98), eps=1e-8, ema=task3.ema_schedule)
    checkpoint.load_checkpoint(path, model3, optimizer=flat3)
    eng3 = model3.encoder._train_engine
    assert torch.equal(eng3.ema, eng.ema) and torch.equal(eng3.master, eng.master) and not torch.equal(eng3.ema, eng3.master)
    # without --store-ema the task's optimizer_step is today's: no EMA anywhere
    task4, model4, _ = _plugin()
    assert task4.ema_schedule is None and model4.encoder._train_engine.ema is None and task4.ema_decay is None


def test_checkpoint_round_trip_of_the_ema(golden, tmp_path, caplog):
    from diffnorm_amd import checkpoint, optim, training
    from diffnorm_amd.latent_module import SpeechVAEEncoderDecoder

    g = golden("vae_train")
    c = CHAIN_VAE

    def trainer(ema_cfg, seed_sd=True):
        vae = SpeechVAEEncoderDecoder(dim=c.dim, latent_dim=c.latent_dim, dtype="bf16")
        if seed_sd:
            vae.load_state_dict(O.make_vae_state_dict(c, "train"), strict=True)
        vae.to(DEV)
        sched = None if ema_cfg is None else optim.EmaSchedule(*ema_cfg)
        return vae, training.VaeTrainer(vae.enable_training(), lr=3e-3, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0, ema=sched)

    feat, units, lens = _batch(g)
    sample = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": lens, "ntokens": int(lens.sum()), "nsentences": 3}
    vae, tr = trainer((0.9, 0, 2))
    for it in range(3):
        tr.train_step([sample], noises=[torch.from_numpy(g[f"traj_noise{it}"])])
    assert tr.ema.counter == 1 and tr.engine.ema_count == 1
    path = str(tmp_path / "ema.pt")
    state = checkpoint.save_checkpoint(path, vae, ema=tr.ema, num_updates=3)
    assert set(state["extra_state"]["ema"]) == set(vae.state_dict())
    vae2, tr2 = trainer((0.9, 0, 2), seed_sd=False)
    checkpoint.load_checkpoint(path, vae2, ema=tr2.ema)
    assert torch.equal(tr2.engine.master, tr.engine.master) and torch.equal(tr2.engine.ema, tr.engine.ema)
    assert not torch.equal(tr2.engine.ema, tr2.engine.master)
    assert tr2.ema.state_dict() == tr.ema.state_dict() and tr2.ema.counter == 1
    # a checkpoint written without an EMA: the EMA starts from the loaded model, with a warning
    vae3, tr3 = trainer(None)
    tr3.train_step([sample], noises=[torch.from_numpy(g["traj_noise0"])])
    plain = str(tmp_path / "plain.pt")
    assert "ema" not in checkpoint.save_checkpoint(plain, vae3)["extra_state"]
    vae4, tr4 = trainer((0.9, 0, 1), seed_sd=False)
    tr4.engine.ema.fill_(7.0)
    with caplog.at_level(logging.WARNING):
        checkpoint.load_checkpoint(plain, vae4, ema=tr4.ema)
    assert torch.equal(tr4.engine.master, tr3.engine.master) and torch.equal(tr4.engine.ema, tr4.engine.master)
    assert any("ema" in r.getMessage().lower() for r in caplog.records)
