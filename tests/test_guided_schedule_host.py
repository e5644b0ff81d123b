"""Host side of the guided (prompted) DDIM chain over a timestep schedule: the argument validation of
LatentDiscreteModel.prompted_ddim_sample, the refusals of dn_guided_ddim_loop and the sizes dn_guided_ddim_workspace_bytes reports
-- none of it needs a GPU, and every refusal comes before any device work."""
import ctypes as C
import types

import pytest
import torch

import diffnorm_oracle as O
from diffnorm_amd import _lib, packing
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE, TINY_EPS_COND, seeded

DN_EINVAL, DN_EWORKSPACE = -1, -3
DN_LOOP_GRAPH, DN_LOOP_SPLIT2, DN_LOOP_KEEP_TABLE = 1, 2, 4


def _last_error(lib):
    return (lib.dn_last_error() or b"").decode()


def _ldm(use_cond):
    from diffnorm_amd.latent_module import LatentDiscreteModel, SpeechVAEEncoderDecoder

    vae = SpeechVAEEncoderDecoder(dim=CHAIN_VAE.dim, latent_dim=CHAIN_VAE.latent_dim, dtype="f32")
    return LatentDiscreteModel(types.SimpleNamespace(encoder=vae), 64, CHAIN_VAE.z, timesteps=200, use_cond=use_cond, dtype="f32").eval()


def test_prompted_ddim_sample_validates_before_any_device_work():
    """The models live on the CPU: a call that got past its validation would fail on the missing device, not with ValueError."""
    feat, src = seeded((2, 24, CHAIN_VAE.dim), 91), seeded((2, 30, CHAIN_VAE.dim), 92)
    pmask = torch.ones(2, 30, dtype=torch.bool)
    with pytest.raises(ValueError, match="use_cond"):
        _ldm(False).prompted_ddim_sample(feat, src, pmask, start_step=50)
    m = _ldm(True)
    assert hasattr(m, "prompted_ddim_sample")
    with pytest.raises(ValueError, match="prompt"):
        m.prompted_ddim_sample(feat, None, pmask, start_step=50)
    with pytest.raises(ValueError, match="prompt"):
        m.prompted_ddim_sample(feat, src, None, start_step=50)
    with pytest.raises(ValueError, match="not both"):
        m.prompted_ddim_sample(feat, src, pmask, start_step=50, sampling_steps=5, timestep_schedule=[49, 3])
    with pytest.raises(ValueError, match="does not descend"):
        m.prompted_ddim_sample(feat, src, pmask, start_step=50, timestep_schedule=[3, 30, 49])
    with pytest.raises(ValueError, match="eta"):
        m.prompted_ddim_sample(feat, src, pmask, start_step=50, sampling_steps=5, eta=-0.5)
    with pytest.raises(ValueError, match="sampling_steps"):
        m.prompted_ddim_sample(feat, src, pmask, start_step=50, sampling_steps=50)


@pytest.fixture(scope="module")
def host_handles():
    """DnEps objects over HOST copies of the packed tensors (a prompted and an unconditional model): dn_eps_create only keeps the
    pointers, and an entry that refuses its arguments returns before anything reads them."""
    lib = _lib.load()
    made = []

    def create(cfg, seed, cond):
        tensors = [t.contiguous() for t in packing.pack_eps(O.make_eps_state_dict(cfg, seed), cfg, _lib.DN_F32, 2048)]
        table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
        c = _lib.EpsConfig(cfg.dim, cfg.latent_dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.wavenet_layers, cfg.wavenet_stacks, cfg.dim_cond_mult,
                           _lib.DN_F32, 2048, cfg.dim_prompt if cond else 0, cfg.num_latents_m if cond else 0, cfg.resampler_depth if cond else 0)
        h = C.c_void_p()
        assert lib.dn_eps_create(C.byref(c), table, len(tensors), C.byref(h)) == 0, _last_error(lib)
        made.append((h, tensors))
        return h

    yield lib, create(TINY_EPS_COND, "cond", True), create(CHAIN_EPS, "chain", False)
    for h, _ in made:
        lib.dn_eps_destroy(h)


B, T, TP, N = 3, 40, 21, 5


def test_workspace_size_is_positive_and_monotonic(host_handles):
    lib, h, h_uncond = host_handles
    ws = lambda n, guided: int(lib.dn_guided_ddim_workspace_bytes(h, B, T, TP, n, guided))  # noqa: E731
    sizes = [ws(n, 1) for n in (1, 2, 5, 20, 100, 199)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    for n in (1, 5, 199):
        assert 0 < ws(n, 0) <= ws(n, 1)
        assert ws(n, 0) >= int(lib.dn_eps_cond_workspace_bytes(h, B, T, TP)) - 256  # (it holds the pass's own workspace)
        assert ws(n, 1) >= int(lib.dn_eps_cond_workspace_bytes(h, 2 * B, T, TP)) - 256
    assert ws(0, 1) == 0 and int(lib.dn_guided_ddim_workspace_bytes(None, B, T, TP, N, 1)) == 0
    assert int(lib.dn_guided_ddim_workspace_bytes(h, 0, T, TP, N, 1)) == 0 and int(lib.dn_guided_ddim_workspace_bytes(h, B, T, 0, N, 1)) == 0
    assert int(lib.dn_guided_ddim_workspace_bytes(h_uncond, B, T, TP, N, 1)) == 0  # no prompt branch


def test_loop_entry_checks_its_arguments_before_any_device_call(host_handles):
    lib, h, h_uncond = host_handles
    z, P = TINY_EPS_COND.latent_dim, TINY_EPS_COND.dim_prompt
    x = torch.zeros(B, T, z)
    lens, plens = torch.full((B,), T, dtype=torch.int32), torch.full((B,), TP, dtype=torch.int32)
    prompt = torch.zeros(B, TP, P)
    steps = torch.tensor([49, 30, 29, 3, 0], dtype=torch.int32)
    coef = torch.zeros(N, _lib.DDIM_SCHED_COLS)
    need = int(lib.dn_guided_ddim_workspace_bytes(h, B, T, TP, N, 1))
    need1 = int(lib.dn_guided_ddim_workspace_bytes(h, B, T, TP, N, 0))
    ws = torch.zeros(need + 256, dtype=torch.uint8)
    wp = (ws.data_ptr() + 255) & ~255

    def call(m=h, xp=x.data_ptr(), lp=lens.data_ptr(), pp=prompt.data_ptr(), plp=plens.data_ptr(), Bc=B, Tc=T, Tpc=TP, scale=2.0,
             sp=steps.data_ptr(), cp=coef.data_ptr(), nc=N, timesteps=200, eta_on=0, noise=None, flags=0, wsp=wp, wsn=need):
        return lib.dn_guided_ddim_loop(m, xp, lp, pp, plp, Bc, Tc, Tpc, scale, sp, cp, nc, timesteps, eta_on, 0, noise, flags, wsp, wsn, None)

    for what, kw in (("null engine", dict(m=None)), ("null x", dict(xp=None)), ("null lengths", dict(lp=None)), ("null prompt", dict(pp=None)),
                     ("null prompt lengths", dict(plp=None)), ("null schedule", dict(sp=None)), ("null coef", dict(cp=None)),
                     ("null workspace", dict(wsp=None)), ("empty", dict(nc=0)), ("negative", dict(nc=-1)),
                     ("more steps than timesteps", dict(nc=5, timesteps=4)), ("B = 0", dict(Bc=0)), ("Tp = 0", dict(Tpc=0)),
                     ("T beyond the positional table", dict(Tc=4096)), ("noise without eta", dict(noise=x.data_ptr())),
                     ("split", dict(flags=DN_LOOP_SPLIT2)), ("split + graph", dict(flags=DN_LOOP_GRAPH | DN_LOOP_SPLIT2)),
                     ("keep table", dict(flags=DN_LOOP_KEEP_TABLE)), ("misaligned workspace", dict(wsp=wp + 4)),
                     ("unconditional model", dict(m=h_uncond))):
        assert call(**kw) == DN_EINVAL, what
        assert "dn_guided_ddim_loop" in _last_error(lib), (what, _last_error(lib))
    assert call(flags=DN_LOOP_SPLIT2) == DN_EINVAL and "DN_LOOP_SPLIT2" in _last_error(lib)
    assert call(wsn=need - 1) == DN_EWORKSPACE and "dn_guided_ddim_workspace_bytes" in _last_error(lib)
    assert call(scale=1.0, wsn=need1 - 1) == DN_EWORKSPACE and "dn_guided_ddim_loop" in _last_error(lib)
    if need1 < need:  # a guided chain does not fit into the scale-1 size
        assert call(scale=2.0, wsn=need1) == DN_EWORKSPACE


def test_time_table_steps_checks_its_arguments(host_handles):
    lib, h, h_uncond = host_handles
    steps = torch.tensor([6, 5, 4], dtype=torch.int32)
    table = torch.zeros(8)
    ws = torch.zeros(4096, dtype=torch.uint8)
    wp = (ws.data_ptr() + 255) & ~255
    big = int(lib.dn_eps_cond_time_table_workspace_bytes(h, 3))
    for kw in (dict(m=None), dict(sp=None), dict(tp=None), dict(wsp=None), dict(n=0), dict(m=h_uncond), dict(wsn=16), dict(wsp=wp + 8)):
        a = dict(m=h, sp=steps.data_ptr(), n=3, tp=table.data_ptr(), wsp=wp, wsn=big)
        a.update(kw)
        assert lib.dn_eps_cond_time_table_steps(a["m"], a["sp"], a["n"], a["tp"], a["wsp"], a["wsn"], None) == DN_EINVAL, kw
        assert "dn_eps_cond_time_table_steps" in _last_error(lib)
