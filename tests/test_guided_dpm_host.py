"""Host side of the prompted, guided DPM-Solver++(2M) chain: the keyword handling of prompted_ddim_sample(solver=...) against
stand-ins for the model's engines (what reaches which loop, with which steps and rows), the refusals, ddim_sample's own refusal for a
prompted model, and the two C entries in the binding table and the header -- none of it needs a GPU."""
import os
import re
import types

import pytest
import torch

from diffnorm_amd import _lib, latent_module, scheduler
from diffnorm_amd.latent_module import LatentDiscreteModel

from test_dpm_schedule_host import _NoEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMESTEPS = 200
B, T, TP, D, Z = 2, 8, 6, 16, 4
EXPLICIT = [49, 37, 25, 13, 0]


def test_prompted_ddim_sample_refuses_bad_solver_arguments_before_touching_an_engine():
    feat = torch.zeros(B, T, D)
    kw = dict(prompt=feat, prompt_mask=torch.ones(B, T, dtype=torch.bool), start_step=50)
    call = lambda **k: LatentDiscreteModel.prompted_ddim_sample(_NoEngine(True), feat, **kw, **k)  # noqa: E731
    with pytest.raises(ValueError, match=r"prompted_ddim_sample: .*eta"):
        call(solver="dpmpp_2m", eta=0.5)
    with pytest.raises(ValueError, match=r"prompted_ddim_sample: .*step_noise"):
        call(solver="dpmpp_2m", step_noise=torch.zeros(5, B, T, Z))
    with pytest.raises(ValueError, match=r"prompted_ddim_sample: unknown solver"):
        call(solver="x")
    for order in (0, 3):
        with pytest.raises(ValueError, match=r"prompted_ddim_sample: solver_order"):
            call(solver="dpmpp_2m", solver_order=order)


def test_ddim_sample_still_sends_a_prompted_model_away():
    feat = torch.zeros(B, T, D)
    with pytest.raises(ValueError, match="unconditional"):
        LatentDiscreteModel.ddim_sample(_NoEngine(True), feat, start_step=50, solver="dpmpp_2m", prompt=feat,
                                        prompt_mask=torch.ones(B, T, dtype=torch.bool))


class _Recorder:
    """Stands in for EpsEngine: records the call of either guided loop, and answers nothing else."""

    def __init__(self):
        self.calls = []

    def guided_ddim_schedule_loop(self, *a, **k):
        self.calls.append(("ddim", a, k))
        return int(a[4].shape[0])

    def guided_dpm_schedule_loop(self, *a, **k):
        self.calls.append(("dpm", a, k))
        return int(a[4].shape[0])


def _stub(monkeypatch):
    """A LatentDiscreteModel's attributes as prompted_ddim_sample reads them, on the CPU: the real scheduler, a latent that is a
    slice of the features, q_sample restated in torch, a decoder that returns the latent."""
    sched = scheduler.DDPMScheduler(TIMESTEPS)
    rec = _Recorder()
    cpu = torch.device("cpu")
    vae = types.SimpleNamespace(
        encode_feature=lambda feat, noise=None: feat[..., :Z].transpose(1, 2),
        engine=lambda: types.SimpleNamespace(decode=lambda x, lengths, want_logits=False: (x.clone(), None, torch.zeros(x.shape[:2], dtype=torch.int32))))
    stub = types.SimpleNamespace(use_cond=True, scheduler=sched, device=cpu, timesteps=TIMESTEPS, speech_decoder=vae,
                                 model=types.SimpleNamespace(engine=lambda: rec),
                                 _tables=lambda: (None, sched.f32("sqrt_alphas_cumprod", cpu), sched.f32("sqrt_one_minus_alphas_cumprod", cpu)))
    monkeypatch.setattr(latent_module.ops, "q_sample",
                        lambda z, noise, sa, s1, t, T_: sa[t.long()].view(-1, 1, 1) * z + s1[t.long()].view(-1, 1, 1) * noise)
    return stub, rec, sched


def _inputs():
    g = torch.Generator().manual_seed(3)
    feat, prompt = torch.randn(B, T, D, generator=g), torch.randn(B, TP, D, generator=g)
    pmask = torch.arange(TP)[None, :] < torch.tensor([TP, 2])[:, None]
    imask = torch.arange(T)[None, :] < torch.tensor([T, 5])[:, None]
    return feat, prompt, pmask, imask, torch.randn(B, T, Z, generator=g)


def test_solver_none_reaches_the_ddim_loop_with_unchanged_arguments(monkeypatch):
    stub, rec, sched = _stub(monkeypatch)
    feat, prompt, pmask, imask, start = _inputs()
    noise = torch.zeros(5, B, T, Z)
    for extra in (dict(), dict(solver=None, solver_order=2)):
        rec.calls.clear()
        toks, match, total, recon = LatentDiscreteModel.prompted_ddim_sample(stub, feat, prompt, pmask, input_mask=imask, cond_scale=2.0, start_step=50,
                                                                             sampling_steps=5, eta=0.5, seed=11, step_noise=noise, start_noise=start,
                                                                             use_graph=False, **extra)
        assert len(rec.calls) == 1
        name, a, k = rec.calls[0]
        st, coef = sched.ddim_schedule(50, 5, None, eta=0.5)
        sa, s1 = sched.f32("sqrt_alphas_cumprod"), sched.f32("sqrt_one_minus_alphas_cumprod")
        assert name == "ddim" and len(a) == 6
        assert torch.equal(a[0], sa[50] * feat[..., :Z] + s1[50] * start)  # x: q_sample at start_step
        assert a[1].tolist() == [T, 5] and a[2] is prompt and a[3].tolist() == [TP, 2]
        assert torch.equal(a[4], st) and torch.equal(a[5], coef)
        assert set(k) == {"cond_scale", "eta", "seed", "noise", "use_graph", "timesteps"}
        assert (k["cond_scale"], k["eta"], k["seed"], k["use_graph"], k["timesteps"]) == (2.0, 0.5, 11, False, TIMESTEPS) and k["noise"] is noise
        assert total == T + 5 and [t.shape[0] for t in toks] == [T, 5] and recon.shape == (B, T, Z)


@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("sel", [dict(sampling_steps=5), dict(timestep_schedule=EXPLICIT)], ids=["n5", "explicit"])
def test_solver_reaches_the_dpm_loop_with_dpm_schedules_rows(monkeypatch, sel, order):
    stub, rec, sched = _stub(monkeypatch)
    feat, prompt, pmask, imask, start = _inputs()
    toks, match, total, recon = LatentDiscreteModel.prompted_ddim_sample(stub, feat, prompt, pmask, input_mask=imask, cond_scale=2.0, start_step=50,
                                                                         start_noise=start, solver="dpmpp_2m", solver_order=order, **sel)
    assert len(rec.calls) == 1
    name, a, k = rec.calls[0]
    st, rows = sched.dpm_schedule(50, sel.get("sampling_steps"), sel.get("timestep_schedule"), order=order)
    assert name == "dpm" and len(a) == 6
    assert a[1].tolist() == [T, 5] and a[2] is prompt and a[3].tolist() == [TP, 2]
    assert a[4].dtype == torch.int32 and torch.equal(a[4], st) and a[5].shape == (5, _lib.DPM_COLS) and torch.equal(a[5], rows)
    assert (rows[1:-1, 5] != 0).all() if order == 2 else (rows[:, 5] == 0).all()  # (the order reached the rows)
    assert k == dict(cond_scale=2.0, use_graph=True, timesteps=TIMESTEPS)
    assert total == T + 5 and [t.shape[0] for t in toks] == [T, 5]
    assert torch.equal(recon, a[0])  # decode saw the loop's x


def test_a_bad_schedule_raises_under_the_solvers_name(monkeypatch):
    stub, rec, _ = _stub(monkeypatch)
    feat, prompt, pmask, imask, start = _inputs()
    with pytest.raises(ValueError, match="dpm_schedule"):
        LatentDiscreteModel.prompted_ddim_sample(stub, feat, prompt, pmask, start_step=50, timestep_schedule=[3, 30, 49], solver="dpmpp_2m")
    assert not rec.calls


def test_the_new_entries_are_bound_and_declared():
    names = ("dn_guided_dpm_workspace_bytes", "dn_guided_dpm_loop")
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffnorm_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib.SYMBOLS
        assert re.search(r"\b" + n + r"\s*\(", src), f"{n} is not declared in include/diffnorm_hip.h"
    # the loop takes dn_guided_ddim_loop's arguments without eta_on / seed / noise
    assert len(_lib.SYMBOLS["dn_guided_dpm_loop"][1]) == len(_lib.SYMBOLS["dn_guided_ddim_loop"][1]) - 3
    assert _lib.SYMBOLS["dn_guided_dpm_workspace_bytes"] == _lib.SYMBOLS["dn_guided_ddim_workspace_bytes"]


def test_the_update_kernels_of_pointwise_compile_without_scratch():
    """tools/check_resources.py on csrc/pointwise.hip (hipcc cross-compiles: no GPU needed): no kernel of the unit, the guided and
    unguided forms of the 2M update (sched_step_kernel under Dpm2mRule) among them, spills or keeps a stack object."""
    import importlib.util
    import shutil

    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    src = open(os.path.join(ROOT, "diffnorm_amd", "csrc", "pointwise.hip")).read()
    assert "sched_step_kernel" in src and "sched_launch_source<Dpm2mRule, false>" in src
    spec = importlib.util.spec_from_file_location("check_resources", os.path.join(ROOT, "tools", "check_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.check(["pointwise.hip"]) == []
