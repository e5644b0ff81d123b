"""Host side of the generic Gaussian scheduler's device loop (dn_gaussian_loop): the chain's steps and table rows against the float64
tables of the oracle's create_diffusion, the start_index tails, every refusal of p_sample_loop_device / ddim_sample_loop_device and
gaussian_sample raised before any library call (against recording stand-ins), and the new entries in the header and the binding
table -- none of it needs a GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
from diffnorm_amd import _lib
from diffnorm_amd.diffusion import SpacedDiffusion, create_diffusion
from diffnorm_amd.diffusion import gaussian_diffusion as gd
from diffnorm_amd.latent_module import LatentDiscreteModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ZERO = [3, 11, 40, 77, 99]  # an explicit use_timesteps without 0, of 100


def oracle_rows(orc, fixed_large):
    """The DN_GD_COLS columns from the oracle's float64 tables, cast to fp32: [num_timesteps, 12] in index order."""
    t = orc.tab
    large_var = np.append(t.posterior_variance[1], t.betas[1:])
    fixed_var = large_var if fixed_large else t.posterior_variance
    fixed_log = np.log(large_var) if fixed_large else t.posterior_log_variance_clipped
    cols = [t.sqrt_recip_alphas_cumprod, t.sqrt_recipm1_alphas_cumprod, t.posterior_mean_coef1, t.posterior_mean_coef2, fixed_log,
            t.posterior_log_variance_clipped, np.log(t.betas), t.alphas_cumprod, t.alphas_cumprod_prev, t.alphas_cumprod_next,
            t.posterior_variance, fixed_var]
    return torch.from_numpy(np.stack(cols, axis=1).astype(np.float32))


CASES = [("", 100, True), ("ddim5", 100, False), ("10,15,20", 300, True), ("", 300, False)]


@pytest.mark.parametrize("respacing,n,small", CASES)
def test_steps_and_rows_match_the_oracles_tables(respacing, n, small):
    diff = create_diffusion(respacing, noise_schedule="cosine", learn_sigma=False, sigma_small=small, diffusion_steps=n)
    orc = O.create_diffusion_oracle(respacing, noise_schedule="cosine", learn_sigma=False, sigma_small=small, diffusion_steps=n)
    steps, table = diff.device_schedule()
    assert steps.dtype == torch.int32 and steps.tolist() == orc.timestep_map[::-1]
    assert (np.diff(steps.numpy()) < 0).all()  # strictly descending: what dn_ddim_sched_check asks for
    want = oracle_rows(orc, not small)
    assert table.dtype == torch.float32 and table.shape == (orc.num_timesteps, _lib.GD_COLS) and table.is_contiguous()
    assert torch.equal(table, want.flip(0))
    assert table[-1, 8] == 1.0  # the last row is respaced index 0: abar_prev = 1
    if respacing == "ddim5":
        assert steps.tolist() == [80, 60, 40, 20, 0]
    if respacing == "10,15,20":
        assert len(steps) == 45 and steps[0] == 299 and steps[-1] == 0


def test_a_use_timesteps_without_zero_keeps_its_own_last_step():
    betas = gd.get_named_beta_schedule("cosine", 100)
    diff = SpacedDiffusion(NO_ZERO, betas=betas, model_mean_type=gd.ModelMeanType.EPSILON, model_var_type=gd.ModelVarType.FIXED_LARGE,
                           loss_type=gd.LossType.MSE)
    orc = O.GaussianDiffusionOracle(O.cosine_betas(100), "fixed_large", NO_ZERO)
    steps, table = diff.device_schedule()
    assert steps.tolist() == NO_ZERO[::-1] and steps[-1] != 0
    assert torch.equal(table, oracle_rows(orc, True).flip(0))
    assert table[-1, 8] == 1.0 and table[-1, 4] != 0  # respaced index 0 has a variance of its own: the kernel masks its noise by the row


def test_start_index_keeps_the_tail():
    diff = create_diffusion("", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100)
    full_s, full_t = diff.device_schedule()
    s6, t6 = diff.device_schedule(6)
    assert s6.tolist() == [5, 4, 3, 2, 1, 0] and torch.equal(s6, full_s[-6:]) and torch.equal(t6, full_t[-6:])
    d5 = create_diffusion("ddim5", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100)
    s2, t2 = d5.device_schedule(2)
    assert s2.tolist() == [20, 0] and torch.equal(t2, d5.device_schedule()[1][-2:])
    assert d5.device_schedule(5)[0].tolist() == d5.device_schedule()[0].tolist()
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="start_index"):
            d5.device_schedule(bad)


class _Recorder:
    """Stands in for EpsEngine: records gaussian_loop calls and answers nothing else (no library handle, no device work)."""

    def __init__(self, conditional=False):
        self.calls, self.conditional, self.device = [], conditional, torch.device("cpu")

    def gaussian_loop(self, *a, **k):
        self.calls.append((a, k))
        return int(a[2].shape[0])


@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library fails the test."""
    def boom():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("entry", ["p_sample_loop_device", "ddim_sample_loop_device"])
def test_the_device_entries_refuse_with_the_way_out(no_library, entry):
    x, lens = torch.zeros(2, 4, 8), torch.tensor([4, 3])
    host = entry[:-len("_device")]
    learned = create_diffusion("ddim5", diffusion_steps=100)  # learn_sigma=True: LEARNED_RANGE
    rec = _Recorder()
    with pytest.raises(ValueError, match=rf"{entry}: .*learn_sigma=False.*{host}"):
        getattr(learned, entry)(rec, x, lens)
    start_x = create_diffusion("ddim5", learn_sigma=False, predict_xstart=True, diffusion_steps=100)
    with pytest.raises(ValueError, match=rf"{entry}: .*START_X.*predict_xstart=False"):
        getattr(start_x, entry)(rec, x, lens)
    ok = create_diffusion("ddim5", learn_sigma=False, diffusion_steps=100)
    with pytest.raises(ValueError, match=rf"{entry}: .*unconditional.*prompted_ddim_sample"):
        getattr(ok, entry)(_Recorder(conditional=True), x, lens)
    with pytest.raises(ValueError, match="start_index"):
        getattr(ok, entry)(rec, x, lens, start_index=6)
    assert not rec.calls


def test_the_device_entries_reach_the_loop_with_the_schedule(no_library):
    diff = create_diffusion("ddim5", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100)
    x, lens = torch.randn(2, 4, 8), torch.tensor([4, 3])
    noise = torch.zeros(3, 2, 4, 8)
    rec = _Recorder()
    out = diff.ddim_sample_loop_device(rec, x, lens, clip_denoised=False, start_index=3, noise=noise, eta=0.5)
    (a, k), = rec.calls
    steps, table = diff.device_schedule(3)
    assert torch.equal(a[0], x) and a[0] is not x and out is a[0] and a[1] is lens  # the loop works in place on a copy
    assert torch.equal(a[2], steps) and torch.equal(a[3], table)
    assert k == dict(sampler="ddim", clip_denoised=False, eta=0.5, seed=0, noise=noise, keys=None, timesteps=100)
    rec.calls.clear()
    keys = torch.tensor([5, 6])
    diff.p_sample_loop_device(rec, x, lens, keys=keys)
    (a, k), = rec.calls
    assert torch.equal(a[2], diff.device_schedule()[0])
    assert k["sampler"] == "p_sample" and k["clip_denoised"] is True and k["eta"] == 0.0 and k["keys"] is keys and k["noise"] is None


def test_gaussian_sample_refuses_bad_arguments_before_touching_an_engine(no_library):
    diff = create_diffusion("ddim5", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100)
    feat = torch.zeros(2, 4, 16)

    def boom():
        raise AssertionError("an engine was asked for")

    def model(use_cond=False):
        return types.SimpleNamespace(use_cond=use_cond, device=torch.device("cpu"), model=types.SimpleNamespace(engine=boom),
                                     speech_decoder=types.SimpleNamespace(engine=boom, encode_feature=boom))

    call = lambda m=None, **k: LatentDiscreteModel.gaussian_sample(m or model(), feat, diff, **k)  # noqa: E731
    with pytest.raises(ValueError, match="gaussian_sample: unknown sampler"):
        call(sampler="dpm")
    with pytest.raises(ValueError, match="gaussian_sample: .*unconditional"):
        call(model(use_cond=True))
    with pytest.raises(ValueError, match="gaussian_sample: keyed_steps .*needs noise_keys"):
        call(keyed_steps=True)
    keys = torch.tensor([1, 2])
    with pytest.raises(ValueError, match="gaussian_sample: keyed_steps .*step_noise"):
        call(keyed_steps=True, noise_keys=keys, step_noise=torch.zeros(5, 2, 4, 8))
    with pytest.raises(ValueError, match="gaussian_sample: keyed_steps .*seed"):
        call(keyed_steps=True, noise_keys=keys, seed=3)
    with pytest.raises(ValueError, match="gaussian_sample: start_index"):
        call(start_index=6)
    with pytest.raises(ValueError, match="noise_keys draws the posterior and the start noise"):
        call(noise_keys=keys, start_noise=torch.zeros(2, 4, 8))


NEW = ("dn_gaussian_workspace_bytes", "dn_gaussian_loop", "dn_gaussian_loop_keyed", "dn_gaussian_sched_step", "dn_gaussian_sched_step_keyed")


def test_the_new_entries_are_bound_and_declared():
    text = open(os.path.join(ROOT, "include", "diffnorm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NEW:
        assert n in _lib.SYMBOLS
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} is not declared in include/diffnorm_hip.h"
    assert _lib.SYMBOLS["dn_gaussian_workspace_bytes"] == _lib.SYMBOLS["dn_ddim_sched_workspace_bytes"]
    # the keyed loop takes `keys` where the twin takes seed and noise
    assert len(_lib.SYMBOLS["dn_gaussian_loop_keyed"][1]) == len(_lib.SYMBOLS["dn_gaussian_loop"][1]) - 1
    # the header entry cites the reference lines it replaces
    entry = text[text.index("The generic Gaussian scheduler as a device loop"):text.index("size_t dn_gaussian_workspace_bytes")]
    assert "gaussian_diffusion.py" in entry and "419-511" in entry and "600-680" in entry and "respace.py" in entry


def test_the_oracle_reproduces_the_reference_loops(golden):
    """tests/golden/gaussian_loop.npz (tools/gen_golden_gaussian_loop.py: the REAL SpacedDiffusion "ddim5" of 100 cosine steps over the
    real tiny Model, p_sample_loop and ddim_sample_loop at eta = 0.5, recorded draws) against the oracle's create_diffusion on the
    same arrays, at the bound test_oracle_golden.py holds loop5_out to."""
    from gen_golden_configs import CHAIN_EPS

    g = golden("gaussian_loop")
    T_ = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    x, lens = T_(g["x_T"]), T_(g["lens"])
    orc = O.create_diffusion_oracle("ddim5", noise_schedule="cosine", learn_sigma=False, diffusion_steps=100)
    assert orc.timestep_map == g["timestep_map"].tolist()
    sd, mask = O.make_eps_state_dict(CHAIN_EPS, "chain"), O.lengths_to_mask(lens, x.shape[1])
    model = lambda xx, t: O.eps_forward(sd, CHAIN_EPS, xx, t, mask)  # noqa: E731
    for name, step in (("p_sample", lambda xx, t, nz: orc.p_sample(model, xx, t, nz, clip_denoised=False)),
                       ("ddim", lambda xx, t, nz: orc.ddim_sample(model, xx, t, nz, clip_denoised=False, eta=float(g["eta"])))):
        xx = x
        with torch.no_grad():
            for k, i in enumerate(range(orc.num_timesteps - 1, -1, -1)):
                xx = step(xx, torch.full((x.shape[0],), i, dtype=torch.long), T_(g[f"{name}_noise"][k]))["sample"]
        err = (xx.double() - T_(g[f"{name}_out"]).double())[mask].abs().max().item()
        print(f"oracle {name} loop against the reference: max abs err {err:.3e} (output scale {np.abs(g[f'{name}_out']).max():.2f})")
        assert err <= 5e-6, (name, err)
