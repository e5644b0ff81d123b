"""Host side of the DDIM chain over a timestep schedule (scheduler.ddim_schedule, dn_ddim_sched_check, the argument checks of
dn_ddim_sched_loop): the selection rule, the coefficient rows and the update they drive against the oracle's pinned generic
scheduler, and the schedules that are refused -- none of it needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from diffnorm_amd import _lib, packing, scheduler
from gen_golden_configs import CHAIN_EPS, seeded

DN_EINVAL, DN_EWORKSPACE = -1, -3


def test_selection_rule_known_answers():
    s = scheduler.DDPMScheduler(1000)
    e = s.ddim_steps(999, 50)
    assert e[0] == 998 and e[-1] == 1 and len(e) == 50 and all(a > b for a, b in zip(e, e[1:]))
    for start in (2, 5, 50, 999):
        assert s.ddim_steps(start, start - 1) == list(range(start - 1, 0, -1)) == s.ddim_steps(start)
    assert s.ddim_steps(999, 1) == [998] and s.ddim_steps(2, 1) == [1] and s.ddim_steps(1) == [0]
    # e_i = 49 - floor((2 i 48 + 6) / 12) = 49 - floor(8 i + 1/2)
    assert s.ddim_steps(50, 7) == [49, 41, 33, 25, 17, 9, 1]
    # halves round up: start 8, N 3: 7 - floor((12 i + 2) / 4) = 7 - floor(3 i + 1/2); start 9, N 3: 8 - floor((14 i + 2) / 4) -> 3.5 i + .5
    assert s.ddim_steps(8, 3) == [7, 4, 1] and s.ddim_steps(9, 3) == [8, 4, 1]
    for start in (3, 17, 200, 999):  # every N: strictly descending from start-1 to 1
        for n in sorted(n for n in {2, 3, (start - 1) // 2, start - 2, start - 1} if 2 <= n <= start - 1):
            e = s.ddim_steps(start, n)
            assert len(e) == n and e[0] == start - 1 and e[-1] == 1 and all(a > b for a, b in zip(e, e[1:])), (start, n)
    st, coef = s.ddim_schedule(999, 50)
    assert st.dtype == torch.int32 and st.tolist() == s.ddim_steps(999, 50) and coef.shape == (50, _lib.DDIM_SCHED_COLS) and coef.dtype == torch.float32


@pytest.mark.parametrize("timesteps,start", [(200, 1), (200, 2), (200, 50), (200, 199), (1000, 999)])
def test_every_timestep_rows_are_the_coef_table_rows(timesteps, start):
    s = scheduler.DDPMScheduler(timesteps)
    table = s.ddim_coef_table()
    for kw in ({}, {"sampling_steps": start - 1}) if start > 1 else ({}, {"steps": [0]}):
        st, coef = s.ddim_schedule(start, **kw)
        assert torch.equal(coef[:, :4], table[st.long()])  # bit for bit
        assert (coef[:, 4] == 0).all()


def test_target_level_of_the_last_update():
    s = scheduler.DDPMScheduler(200)
    _, c1 = s.ddim_schedule(50, steps=[49, 30, 29, 3])   # ends above 0: to abar[0]
    _, c0 = s.ddim_schedule(50, steps=[49, 30, 29, 3, 0])  # ends at 0: to 1
    assert c1[-1, 2].item() == np.sqrt(np.float32(s.alphas_cumprod[0])) and c0[-1, 2].item() == 1.0 and c0[-1, 3].item() == 0.0
    assert c0[3, 2].item() == c1[3, 2].item() and torch.equal(c0[:3], c1[:3])
    assert c0[1, 2].item() == np.sqrt(np.float32(s.alphas_cumprod[29]))
    _, ce = s.ddim_schedule(50, steps=[49, 30, 29, 3, 0], eta=1.0)
    assert ce[-1, 4].item() == 0.0 and (ce[:-1, 4] > 0).all()  # sigma vanishes with the target level 1


def sched_update(row, x, eps, z, e_i):
    """The update of one row, fp32, in the safe-div form of the model's own eta = 0 update."""
    sa, s1, ct, cd, sg = (row[j] for j in range(5))
    x1 = (x - s1 * eps) / sa.clamp(min=1e-10)
    pn = (x - sa * x1) / s1.clamp(min=1e-10)
    return x1 * ct + cd * pn + (sg * z if e_i != 0 else 0.0)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("respacing", ["ddim10", "ddim25"])
def test_update_matches_the_oracles_generic_scheduler(eta, respacing):
    """Every update of the chain over the respaced timesteps against GaussianDiffusionOracle.ddim_sample (clipping off) on the same
    cosine schedule: the two differ only in how x0 is divided out -- fp32 round-off, the 5e-5 test_oracle_golden.py holds the
    oracle itself to."""
    diff = O.create_diffusion_oracle(respacing, noise_schedule="cosine", learn_sigma=False, sigma_small=True, diffusion_steps=200)
    steps = sorted(diff.timestep_map, reverse=True)
    assert steps[-1] == 0 and len(steps) == int(respacing[4:])
    st, coef = scheduler.DDPMScheduler(200).ddim_schedule(steps[0] + 1, steps=steps, eta=eta)
    x, eps, z = seeded((3, 16, 48), 11), seeded((3, 16, 48), 12), seeded((3, 16, 48), 13)
    worst = 0.0
    for i, e_i in enumerate(steps):
        t = torch.full((3,), len(steps) - 1 - i, dtype=torch.long)  # the respaced index of e_i
        want = diff.ddim_sample(lambda xx, tt: eps, x, t, z, clip_denoised=False, eta=eta)["sample"]
        got = sched_update(coef[i], x, eps, z, e_i)
        worst = max(worst, (got - want).abs().max().item())
    print(f"{respacing} eta={eta}: worst update error {worst:.3e}")
    assert worst <= 5e-5


BAD = {"ascending": [3, 30, 49], "repeated": [49, 30, 30, 3], "above": [200, 49, 3], "below": [49, 3, -1], "empty": []}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_schedules_raise_on_the_host(name):
    s = scheduler.DDPMScheduler(200)
    with pytest.raises(ValueError, match="ddim_schedule"):
        s.ddim_schedule(50, steps=BAD[name])
    with pytest.raises(ValueError, match="ddim_schedule"):
        s.ddim_schedule(50, steps=torch.tensor(BAD[name], dtype=torch.int32))


def test_bad_step_counts_raise_on_the_host():
    s = scheduler.DDPMScheduler(200)
    for start, n in ((50, 50), (50, 0), (50, -3), (1, 1), (200, 5), (0, 1)):
        with pytest.raises(ValueError, match="ddim_schedule"):
            s.ddim_schedule(start, sampling_steps=n)
    with pytest.raises(ValueError, match="not both"):
        s.ddim_schedule(50, sampling_steps=5, steps=[49, 3])
    with pytest.raises(ValueError, match="eta"):
        s.ddim_schedule(50, sampling_steps=5, eta=-0.5)
    with pytest.raises(ValueError, match="eta"):
        s.ddim_schedule(50, sampling_steps=5, eta=1.5)


def _last_error(lib):
    return (lib.dn_last_error() or b"").decode()


@pytest.mark.parametrize("name", sorted(BAD))
def test_c_check_refuses_the_same_schedules(name):
    lib = _lib.load()
    arr = (C.c_int32 * max(1, len(BAD[name])))(*BAD[name])
    assert lib.dn_ddim_sched_check(arr, len(BAD[name]), 200) == DN_EINVAL
    assert "dn_ddim_sched_check" in _last_error(lib)
    good = (C.c_int32 * 5)(49, 30, 29, 3, 0)
    assert lib.dn_ddim_sched_check(good, 5, 200) == 0
    assert lib.dn_ddim_sched_check(good, 5, 49) == DN_EINVAL and lib.dn_ddim_sched_check(None, 5, 200) == DN_EINVAL


@pytest.fixture(scope="module")
def host_handle():
    """A DnEps over HOST copies of the packed tensors: dn_eps_create only keeps the pointers, and an entry that refuses its
    arguments returns before anything reads them."""
    lib = _lib.load()
    cfg = CHAIN_EPS
    tensors = [t.contiguous() for t in packing.pack_eps(O.make_eps_state_dict(cfg, "chain"), cfg, _lib.DN_F32, 2048)]
    table = (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    c = _lib.EpsConfig(cfg.dim, cfg.latent_dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.wavenet_layers, cfg.wavenet_stacks, cfg.dim_cond_mult,
                       _lib.DN_F32, 2048, 0, 0, 0)
    h = C.c_void_p()
    assert lib.dn_eps_create(C.byref(c), table, len(tensors), C.byref(h)) == 0
    yield lib, h, tensors
    lib.dn_eps_destroy(h)


def test_loop_entry_checks_its_arguments_before_any_device_call(host_handle):
    lib, h, _ = host_handle
    B, T, n = 3, 48, 5
    z = CHAIN_EPS.latent_dim
    x = torch.zeros(B, T, z)
    lens = torch.full((B,), T, dtype=torch.int32)
    steps = torch.tensor([49, 30, 29, 3, 0], dtype=torch.int32)
    coef = torch.zeros(n, _lib.DDIM_SCHED_COLS)
    need = lib.dn_ddim_sched_workspace_bytes(h, B, T, n)
    assert need > 0 and need == lib.dn_ddim_workspace_bytes(h, B, T, n)
    assert lib.dn_ddim_sched_workspace_bytes(h, B, T, 0) == 0 and lib.dn_ddim_sched_workspace_bytes(None, B, T, n) == 0
    ws = torch.zeros(need + 256, dtype=torch.uint8)
    wp = (ws.data_ptr() + 255) & ~255

    def call(m=h, xp=x.data_ptr(), lp=lens.data_ptr(), Bc=B, Tc=T, sp=steps.data_ptr(), cp=coef.data_ptr(), nc=n, timesteps=200, eta_on=0,
             noise=None, flags=0, wsp=wp, wsn=need):
        return lib.dn_ddim_sched_loop(m, xp, lp, Bc, Tc, sp, cp, nc, timesteps, eta_on, 0, noise, flags, wsp, wsn, None)

    for what, kw in (("empty", dict(nc=0)), ("negative", dict(nc=-1)), ("more steps than timesteps", dict(nc=5, timesteps=4)),
                     ("null schedule", dict(sp=None)), ("null coef", dict(cp=None)), ("null x", dict(xp=None)), ("null engine", dict(m=None)),
                     ("B = 0", dict(Bc=0)), ("T beyond the positional table", dict(Tc=4096)), ("noise without eta", dict(noise=x.data_ptr())),
                     ("unknown flag", dict(flags=4)), ("misaligned workspace", dict(wsp=wp + 4))):
        assert call(**kw) == DN_EINVAL, what
        assert _last_error(lib), what
    assert call(wsn=need - 1) == DN_EWORKSPACE and "dn_ddim_sched_workspace_bytes" in _last_error(lib)
    assert call(flags=2, wsn=need - 1) == DN_EWORKSPACE
