"""GPU: sampling from a model in training.  dn_repack_weights (csrc/repack.hip) writes the inference engines' packed tensors from a
training engine's flat fp32 master buffer; EpsEngine / VaeEngine.refresh_from launch it into the engine's existing tensors and
forget what the engine derived from the old weights; the module layer's engine() refreshes instead of rebuilding, in a sampling
arithmetic (`sample_dtype`) of its own.  The contract everywhere: bit-identical to an engine built afresh from state_dict()."""
import types

import pytest
import torch

import diffnorm_oracle as O
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, seeded
from test_repack_plan import AWKWARD_EPS, CASES, DTYPES, packed, state_dict_with_specials, train_layout

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T = 2, 48
LENS = torch.tensor([48, 31])  # ragged


def same_bytes(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu())


# ------------------------------------------------------------------------------------------ 1. the kernel against the host packer
@pytest.fixture(scope="module")
def masters():
    """case -> (state dict, entries, offsets, n_params, flat master on the device): built once, read by every dtype."""
    from diffnorm_amd import _lib, packing

    lib = _lib.load()
    out = {}
    for name, (kind, cfg) in CASES.items():
        sd = state_dict_with_specials(kind, cfg)  # one row of hand-picked values: f16 saturation, bf16 / f16 ties, subnormals
        entries, offsets, n = train_layout(lib, kind, cfg)
        out[name] = (sd, entries, offsets, n, packing.pack_flat(sd, entries, offsets, n).to(DEV))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(CASES))
def test_repack_kernel_equals_the_host_packer(masters, case, dtype):
    from diffnorm_amd import _lib, engine, packing

    kind, cfg = CASES[case]
    code = engine._dtype_code(dtype)
    sd, entries, offsets, n, master = masters[case]
    want = packed(kind, sd, cfg, code)
    plan = packing.repack_plan(entries, offsets, code, kind=kind)
    esize = lambda dt: torch.empty(0, dtype=dt).element_size()
    # destinations pre-filled with 0xFF bytes: a tensor, a layer slice or a pad region the kernel skips shows
    dests = [torch.zeros(4, device=DEV) if s is None else
             torch.full((max(1, torch.Size(s[0]).numel()) * esize(s[1]),), 0xFF, dtype=torch.uint8, device=DEV).view(s[1]).view(s[0]) for s in plan.shapes]
    dest = engine._Engine.__new__(engine._Engine)  # the engines' own descriptor builder and launch, over bare tensors
    dest.device, dest.lib, dest.tensors, dest.dtype, dest._kind = torch.device(DEV), _lib.load(), dests, code, kind
    dest._refresh_from(types.SimpleNamespace(entries=entries, offsets=offsets, n_params=n, master=master))
    torch.cuda.synchronize()
    assert len(dests) == len(want)
    for i, (g, w, s) in enumerate(zip(dests, want, plan.shapes)):
        if s is None:
            assert float(g.abs().max()) == 0.0, f"tensor {i} is not in the plan and was written"
        else:
            assert same_bytes(g, w), f"tensor {i} differs from the host packer ({dtype})"
    if kind == "eps":  # the pad regions spelled out once: final_proj's rows beyond latent_dim and its K pad
        fw = dests[7 + 12 + 15].view(torch.uint8).cpu()
        per_row = fw.numel() // packing.padn(cfg.latent_dim)
        assert int(fw.view(-1, per_row)[cfg.latent_dim:].max()) == 0
    assert dest.refresh_bytes() > 4 * sum(e_n for e_n in (torch.Size(e.shape).numel() for e in entries))


def test_repack_rejects_bad_arguments_and_foreign_layouts(masters):
    import ctypes as C

    from diffnorm_amd import _lib, engine

    lib = _lib.load()
    assert lib.dn_repack_weights(None, None, 1, _lib.DN_BF16, None) == -1 and b"dn_repack_weights" in lib.dn_last_error()
    sd, entries, offsets, n, master = masters["chain_eps"]
    d = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert lib.dn_repack_weights(master.data_ptr(), d.data_ptr(), 0, _lib.DN_BF16, None) == -1
    assert lib.dn_repack_weights(master.data_ptr(), d.data_ptr(), 1, 7, None) == -1
    assert C.sizeof(_lib.RepackDesc) == 48
    eng = engine.EpsEngine(O.make_eps_state_dict(AWKWARD_EPS, "x"), AWKWARD_EPS, dtype="f16", device=DEV)
    with pytest.raises(ValueError, match="refresh_from"):  # CHAIN_EPS's training layout does not fit AWKWARD_EPS's engine
        eng.refresh_from(types.SimpleNamespace(entries=entries, offsets=offsets, n_params=n, master=master))


# ------------------------------------------------------------------------------------------ 2. / 3. refresh_from against a rebuild
def _vae_train(dtype):
    from diffnorm_amd import training

    c = CHAIN_VAE
    return training.VaeTrainEngine(O.make_vae_state_dict(c, "train"), dim=c.dim, latent_dim=c.latent_dim, dtype=dtype, device=DEV, depth=c.depth,
                                   heads=c.heads, dim_head=c.dim_head, stacks=c.stacks, layers=c.layers)


def _vae_infer(sd, dtype):
    from diffnorm_amd import engine

    c = CHAIN_VAE
    return engine.VaeEngine(sd, dim=c.dim, latent_dim=c.latent_dim, dtype=dtype, device=DEV, depth=c.depth, heads=c.heads, dim_head=c.dim_head,
                            stacks=c.stacks, layers=c.layers)


def _update(eng, adam, run_forward):
    run_forward()
    eng.zero_grad()
    eng.backward()
    adam.step(eng.grads)
    eng.refresh()


def _units():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(4, 1004, (B, T), generator=g)
    return u.masked_fill(~O.lengths_to_mask(LENS, T), 0)


class _EpsRig:
    """An EpsTrainEngine (with its frozen VAE) and the inputs of its update and of the sampling checks."""

    def __init__(self, dtype):
        from diffnorm_amd import optim, scheduler, training

        self.vae = _vae_train(dtype)
        self.eng = training.EpsTrainEngine(O.make_eps_state_dict(CHAIN_EPS, "train"), CHAIN_EPS, self.vae, timesteps=200, dtype=dtype, device=DEV)
        self.adam = optim.Adam(self.eng.master, lr=3e-3, betas=(0.9, 0.98), bf16_copy=self.eng.adam_copy)
        z = CHAIN_VAE.z
        self.feat, self.units = seeded((B, T, CHAIN_VAE.dim), 31), _units()
        self.z, self.jitter, self.noise = seeded((B, T, z), 32), seeded((B, T, z), 33), seeded((B, T, z), 34)
        self.x0 = seeded((B, T, z), 35).to(DEV)
        self.coef = scheduler.DDPMScheduler(200).ddim_coef_table(torch.device(DEV))
        self.lens = LENS.to(DEV, torch.int32)
        self.n = 0

    def update(self):
        times = torch.tensor([17 + 40 * self.n, 150 - 30 * self.n])
        self.n += 1
        _update(self.eng, self.adam, lambda: self.eng.forward(self.feat, self.units, LENS, self.z, times, self.jitter, self.noise))

    def chain(self, e, x=None, **loop):
        """The end of a 5-step graph-captured DDIM chain of the inference engine `e` (in the caller's buffer `x`, if given)."""
        x = self.x0.clone() if x is None else x.copy_(self.x0)
        e.ddim_loop(x, self.lens, 5, self.coef, use_graph=True, **loop)
        torch.cuda.synchronize()
        return x.clone()

    def outputs(self, e):
        """(eps_hat at per-sample timesteps, the end of the chain) of the inference engine `e`."""
        return e.forward(self.x0, torch.tensor([3, 120]), LENS).clone(), self.chain(e)


@pytest.mark.parametrize("train_dtype", ["f32", "bf16"])
def test_eps_refresh_equals_a_rebuild(train_dtype):
    from diffnorm_amd import engine

    rig = _EpsRig(train_dtype)
    live = {d: engine.EpsEngine(rig.eng.state_dict(), CHAIN_EPS, dtype=d, device=DEV) for d in DTYPES}
    ptrs = {d: [t.data_ptr() for t in e.tensors] for d, e in live.items()}
    for update in range(2):
        rig.update()
        sd = rig.eng.state_dict()
        for d, e in live.items():
            e.refresh_from(rig.eng)
            fresh = engine.EpsEngine(sd, CHAIN_EPS, dtype=d, device=DEV)
            for i, (a, b) in enumerate(zip(e.tensors, fresh.tensors)):
                assert same_bytes(a, b), (train_dtype, d, update, f"packed tensor {i}")
            got, want = rig.outputs(e), rig.outputs(fresh)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (train_dtype, d, update)
            assert [t.data_ptr() for t in e.tensors] == ptrs[d]


@pytest.mark.parametrize("train_dtype", ["f32", "bf16", "bf16x3"])
def test_vae_refresh_equals_a_rebuild(train_dtype):
    from diffnorm_amd import optim

    eng = _vae_train(train_dtype)
    adam = optim.Adam(eng.master, lr=3e-3, betas=(0.9, 0.98), bf16_copy=eng.adam_copy)
    feat, units, post, lat = seeded((B, T, CHAIN_VAE.dim), 31), _units(), seeded((B, T, CHAIN_VAE.z), 36), seeded((B, T, CHAIN_VAE.z), 37)
    live = {d: _vae_infer(eng.state_dict(), d) for d in DTYPES}
    for update in range(2):
        _update(eng, adam, lambda: eng.forward(feat, units, LENS, noise=post, ntokens=int(LENS.sum())))
        sd = eng.state_dict()
        for d, e in live.items():
            e.refresh_from(eng)
            fresh = _vae_infer(sd, d)
            for i, (a, b) in enumerate(zip(e.tensors, fresh.tensors)):
                assert same_bytes(a, b), (train_dtype, d, update, f"packed tensor {i}")
            got, want = e.decode(lat, LENS), fresh.decode(lat, LENS)
            for a, b in zip(got, want):
                assert torch.equal(a, b), (train_dtype, d, update)
            assert torch.equal(e.encode_params(feat), fresh.encode_params(feat))


def test_nothing_derived_from_the_old_weights_survives_a_refresh():
    """The same graph-captured chain, same buffers (so the loop's hipGraph is served from its cache), before and after an update:
    the second result differs from the first and equals a fresh engine's -- also when the caller asks for the conditioning table
    of the previous call (keep_table), which was built from the old weights."""
    from diffnorm_amd import engine

    rig = _EpsRig("bf16")
    e = engine.EpsEngine(rig.eng.state_dict(), CHAIN_EPS, dtype="f16", device=DEV)
    x = rig.x0.clone()
    before = rig.chain(e, x)
    again = rig.chain(e, x, keep_table=True)  # (nothing else used the engine in between: the flag's contract)
    assert torch.equal(before, again)  # the cached graph and the kept table reproduce the chain
    rig.update()
    e.refresh_from(rig.eng)
    after = rig.chain(e, x, keep_table=True)
    fresh = engine.EpsEngine(rig.eng.state_dict(), CHAIN_EPS, dtype="f16", device=DEV)
    want = rig.chain(fresh)
    assert not torch.equal(after, before)
    assert torch.equal(after, want)
    assert torch.equal(rig.chain(e, x), want)


# ------------------------------------------------------------------------------------------ 4. / 5. through the mirror
def _ldm(dtype, sample_dtype=None, esd=None, vsd=None):
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype=dtype, sample_dtype=sample_dtype)
    vae.load_state_dict(O.make_vae_state_dict(CHAIN_VAE, "chain") if vsd is None else vsd, strict=True)
    m = LatentDiscreteModel(types.SimpleNamespace(encoder=vae), CHAIN_EPS.dim, CHAIN_VAE.z, timesteps=200, dtype=dtype, sample_dtype=sample_dtype)
    esd = O.make_eps_state_dict(CHAIN_EPS, "chain") if esd is None else {k: v for k, v in esd.items() if not k.startswith("pos_embed")}
    m.model.load_state_dict(dict(esd, **{"pos_embed._float_tensor": torch.zeros(1)}), strict=True)
    return m.to(DEV).eval()


def _sample(m):
    toks, _, total, recon = m.ddim_sample(seeded((B, T, CHAIN_VAE.dim), 41).to(DEV), input_mask=O.lengths_to_mask(LENS, T).to(DEV), start_step=5,
                                          post_noise=seeded((B, T, CHAIN_VAE.z), 42), start_noise=seeded((B, T, CHAIN_VAE.z), 43))
    return torch.cat(toks).cpu(), recon.cpu()


def _train_and_sample(dtype, sample_dtype, sample=True, force_rebuild=False, updates=3):
    """`updates` DiffusionTrainer updates with injected draws, a ddim_sample after each but the last.  -> (master buffer, samples,
    state dicts at the samples, (engine id, packed tensors' addresses) at every sample)."""
    from diffnorm_amd import training

    m = _ldm(dtype, sample_dtype)
    tr = training.DiffusionTrainer(m, lr=3e-3, clip_norm=2.0, warmup_updates=1, warmup_init_lr=3e-3, attn_dropout=0.0)
    feat, units = seeded((B, T, CHAIN_VAE.dim), 31), _units()
    batch = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": LENS, "ntokens": int(LENS.sum()), "nsentences": B}
    samples, sds, ids = [], [], []
    for it in range(updates):
        z = CHAIN_VAE.z
        draws = {"times": torch.tensor([20 + 50 * it, 140 - 30 * it]), "post_noise": seeded((B, T, z), 50 + it),
                 "jitter_noise": seeded((B, T, z), 60 + it).to(DEV), "true_noise": seeded((B, T, z), 70 + it).to(DEV)}
        tr.train_step([batch], noises=[draws])
        if sample and it + 1 < updates:
            if force_rebuild:
                m.model._engine = None
            samples.append(_sample(m))
            sds.append(m.model.state_dict())
            e = m.model.engine()
            ids.append((id(e), [t.data_ptr() for t in e.tensors]))
    torch.cuda.synchronize()
    return m._train_engine.master.clone(), samples, sds, ids


def test_train_sample_train_in_two_arithmetics():
    """A bf16 model in training samples in f16 between its updates: the updates are those of a run that never sampled, every sample
    is that of a fresh f16 model loaded from state_dict() at that point, and the engine and its tensors' addresses stay."""
    master, samples, sds, ids = _train_and_sample("bf16", "f16")
    quiet, _, _, _ = _train_and_sample("bf16", "f16", sample=False)
    assert torch.equal(master, quiet)
    assert len(samples) == 2 and not torch.equal(samples[0][1], samples[1][1])
    assert ids[0] == ids[1]
    for (toks, recon), sd in zip(samples, sds):
        fresh = _ldm("f16", esd=sd)
        assert fresh.model.engine().dtype == 3 and fresh.speech_decoder.engine().dtype == 3  # DN_F16
        want_toks, want_recon = _sample(fresh)
        assert torch.equal(toks, want_toks) and torch.equal(recon, want_recon)


def test_sample_dtype_pairs_are_checked():
    from diffnorm_amd.latent_module import Model, SpeechVAEEncoderDecoder

    with pytest.raises(ValueError):
        Model(CHAIN_EPS.dim, CHAIN_VAE.z, sample_dtype="int8")
    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="bf16x3", sample_dtype="f16").to(DEV)
    vae.enable_training()
    assert vae._train_engine.dtype == 2 and vae.engine().dtype == 3  # trains in bf16x3, samples in f16


def test_default_sampling_arithmetic_is_unchanged():
    """sample_dtype=None: the refresh path gives what the rebuild it replaces gave (the engine dropped before every sample)."""
    master, samples, _, ids = _train_and_sample("bf16", None)
    master_rb, samples_rb, _, ids_rb = _train_and_sample("bf16", None, force_rebuild=True)
    assert torch.equal(master, master_rb)
    assert ids[0][0] == ids[1][0] and len(samples) == len(samples_rb) == 2
    for (a, b), (c, d) in zip(samples, samples_rb):
        assert torch.equal(a, c) and torch.equal(b, d)
