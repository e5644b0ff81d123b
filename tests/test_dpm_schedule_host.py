"""Host side of the DPM-Solver++(2M) chain (scheduler.dpm_schedule, the keyword checks of ddim_sample(solver=...) and
normalize(solver=...)): the coefficient rows against a float64 evaluation of their formulas, order 1 against the DDIM statements, and
the solver's order on an analytic model whose probability-flow solution is known in closed form -- none of it needs a GPU.

The analytic model: data i.i.d. N(0, s^2), so the exact eps-predictor is eps*(x, t) = sigma_t x / (alpha_t^2 s^2 + sigma_t^2) and the
exact solution is x_t = x_s sqrt((alpha_t^2 s^2 + sigma_t^2) / (alpha_s^2 s^2 + sigma_s^2))."""
import math

import numpy as np
import pytest
import torch

from diffnorm_amd import _lib, scheduler

EXPLICIT = [40, 22, 7, 0]
SELECTIONS = [dict(sampling_steps=n) for n in (1, 2, 5, 10, 49)] + [dict(steps=EXPLICIT)]


def rows_by_formula(s, e, order, lower_order_final):
    """The rows of the issue's definition, one scalar at a time, in float64."""
    ab = s.alphas_cumprod
    lam = lambda a: math.log(math.sqrt(a) / math.sqrt(1.0 - a))  # noqa: E731
    n, out = len(e), []
    for i in range(n):
        tgt = ab[e[i + 1]] if i + 1 < n else (ab[0] if e[i] >= 1 else 1.0)
        al_s, sg_s = math.sqrt(ab[e[i]]), math.sqrt(1.0 - ab[e[i]])
        first = i == 0 or order == 1 or (lower_order_final and i == n - 1) or tgt == 1.0
        if tgt == 1.0:
            a, b = 0.0, 1.0
        else:
            h = lam(tgt) - lam(ab[e[i]])
            a, b = math.sqrt(1.0 - tgt) / sg_s, -math.sqrt(tgt) * math.expm1(-h)
        if first:
            c1, c0 = 1.0, 0.0
        else:
            r = (lam(ab[e[i]]) - lam(ab[e[i - 1]])) / h
            c1, c0 = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
        out.append((al_s, sg_s, a, b, c1, c0))
    return np.array(out, dtype=np.float64)


@pytest.mark.parametrize("timesteps", [1000, 200])
@pytest.mark.parametrize("sel", SELECTIONS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_rows_match_their_formulas(timesteps, sel):
    s = scheduler.DDPMScheduler(timesteps)
    e = s.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
    for order in (2, 1):
        for lof in (True, False):
            st, coef = s.dpm_schedule(50, order=order, lower_order_final=lof, **sel)
            assert st.dtype == torch.int32 and st.tolist() == e and coef.dtype == torch.float32 and coef.shape == (len(e), _lib.DPM_COLS)
            want = rows_by_formula(s, e, order, lof)
            got = coef.double().numpy()
            rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
            assert (rel[want != 0] <= 1.2e-7).all(), (order, lof, rel.max())  # one fp32 rounding
            assert (got[want == 0] == 0).all()
            first = want[:, 5] == 0
            assert (got[first, 5] == 0).all() and (got[first, 4] == 1).all()  # c0 exactly 0, c1 exactly 1 on first-order rows
            assert first[0]  # row 0 is first order
            if lof or order == 1:
                assert first[-1]
            if order == 2 and len(e) >= 3:
                assert not first[1:-1].any()  # the rows in between are second order
                if not lof and e[-1] >= 1:
                    assert not first[-1]
            if e[-1] == 0:  # a chain that ends at step 0 ends at the clean level: x <- x0
                assert got[-1, 2] == 0.0 and got[-1, 3] == 1.0 and first[-1]
            assert np.array_equal(s.dpm_rows64(e, order, lof).astype(np.float32), coef.numpy())


def analytic(s, s2):
    ab = s.alphas_cumprod
    eps_fn = lambda x, t: math.sqrt(1.0 - ab[t]) * x / (ab[t] * s2 + (1.0 - ab[t]))  # noqa: E731
    exact = lambda e0, tgt: math.sqrt((tgt * s2 + (1.0 - tgt)) / (ab[e0] * s2 + (1.0 - ab[e0])))  # noqa: E731  (from x = 1)
    return eps_fn, exact


def ddim_chain64(s, e, eps_fn, x=1.0):
    """The eta = 0 statements of the scheduled DDIM update, in float64."""
    ab = s.alphas_cumprod
    for i, t in enumerate(e):
        tgt = ab[e[i + 1]] if i + 1 < len(e) else (ab[0] if t >= 1 else 1.0)
        sa, s1 = math.sqrt(ab[t]), math.sqrt(1.0 - ab[t])
        x1 = (x - s1 * eps_fn(x, t)) / max(sa, 1e-10)
        pn = (x - sa * x1) / max(s1, 1e-10)
        x = x1 * math.sqrt(tgt) + math.sqrt(1.0 - tgt) * pn
    return x


@pytest.mark.parametrize("timesteps", [1000, 200])
@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_order_one_is_ddim(timesteps, s2):
    s = scheduler.DDPMScheduler(timesteps)
    eps_fn, _ = analytic(s, s2)
    for sel in SELECTIONS:
        e = s.ddim_steps(50, sel.get("sampling_steps"), sel.get("steps"))
        got = scheduler.dpm_chain_reference(1.0, eps_fn, e, s.dpm_rows64(e, order=1))
        want = ddim_chain64(s, e, eps_fn)
        assert abs(got - want) <= 1e-12 * abs(want), (sel, got, want)


@pytest.mark.parametrize("timesteps", [200, 1000])
@pytest.mark.parametrize("s2", [0.25, 4.0])
def test_second_order_on_the_analytic_model(timesteps, s2):
    s = scheduler.DDPMScheduler(timesteps)
    eps_fn, exact = analytic(s, s2)
    err = {}
    for n in (10, 20):
        e = s.ddim_steps(50, n)
        want = exact(e[0], s.alphas_cumprod[0])
        for order in (1, 2):
            got = scheduler.dpm_chain_reference(1.0, eps_fn, e, s.dpm_rows64(e, order=order))
            err[order, n] = abs(got - want) / abs(want)
        err["ddim", n] = abs(ddim_chain64(s, e, eps_fn) - want) / abs(want)
    print(f"T={timesteps} s2={s2}: " + "  ".join(f"{k}: {v:.3e}" for k, v in err.items()))
    assert err[2, 10] <= 0.6 * err["ddim", 10]
    assert err[2, 20] <= 0.25 * err["ddim", 20]
    assert err[2, 10] / err[2, 20] >= 4.0
    assert 1.8 <= err[1, 10] / err[1, 20] <= 2.3


BAD = {"ascending": [3, 30, 49], "repeated": [49, 30, 30, 3], "above": [200, 49, 3], "below": [49, 3, -1], "empty": []}


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_schedules_raise_on_the_host(name):
    s = scheduler.DDPMScheduler(200)
    with pytest.raises(ValueError, match="dpm_schedule"):
        s.dpm_schedule(50, steps=BAD[name])
    with pytest.raises(ValueError, match="dpm_schedule"):
        s.dpm_schedule(50, steps=torch.tensor(BAD[name], dtype=torch.int32))


def test_bad_orders_and_counts_raise_on_the_host():
    s = scheduler.DDPMScheduler(200)
    for order in (0, 3, -1):
        with pytest.raises(ValueError, match="order"):
            s.dpm_schedule(50, sampling_steps=5, order=order)
    for start, n in ((50, 50), (50, 0), (1, 1), (200, 5)):
        with pytest.raises(ValueError, match="dpm_schedule"):
            s.dpm_schedule(start, sampling_steps=n)
    with pytest.raises(ValueError, match="not both"):
        s.dpm_schedule(50, sampling_steps=5, steps=[49, 3])


class _NoEngine:
    """Stands in for the model: answers `use_cond` and nothing else, so a check that passes would be seen reaching for an engine."""

    def __init__(self, use_cond):
        self.use_cond = use_cond

    def __getattr__(self, name):
        raise AssertionError(f"ddim_sample touched self.{name} before refusing its arguments")


def test_ddim_sample_refuses_bad_solver_arguments_before_touching_an_engine():
    from diffnorm_amd.latent_module import LatentDiscreteModel

    feat = torch.zeros(2, 8, 16)
    call = lambda stub, **kw: LatentDiscreteModel.ddim_sample(stub, feat, start_step=50, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="eta"):
        call(_NoEngine(False), solver="dpmpp_2m", eta=0.5)
    with pytest.raises(ValueError, match="step_noise"):
        call(_NoEngine(False), solver="dpmpp_2m", step_noise=torch.zeros(5, 2, 8, 4))
    with pytest.raises(ValueError, match="unknown solver"):
        call(_NoEngine(False), solver="x")
    with pytest.raises(ValueError, match="unconditional"):
        call(_NoEngine(True), solver="dpmpp_2m", prompt=feat, prompt_mask=torch.ones(2, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="solver_order"):
        call(_NoEngine(False), solver="dpmpp_2m", solver_order=3)


def test_normalize_forwards_the_solver_only_when_set():
    from diffnorm_amd import normalize as N

    rng = np.random.RandomState(5)
    utts = []
    for i, n in enumerate((11, 17, 9)):
        units = rng.permutation(1000)[:n]  # all different: de-duplication keeps every frame
        utts.append(N.Utterance(f"utt{i}", f"src{i}.wav", 100 + i, torch.from_numpy(rng.randn(n, 8).astype(np.float32)), units.tolist(),
                                units.tolist()))
    seen = []

    def sample(feat, input_mask=None, ref_units=None, **kw):
        seen.append(dict(kw))
        lens = input_mask.sum(1).tolist()
        return [ref_units[i, : lens[i]] for i in range(feat.shape[0])], 0, 0, None

    plain = N.normalize(sample, utts, start_step=50, batch_size=2, device="cpu")
    assert len(plain) == 3 and all(set(k) == {"cond_scale", "start_step"} for k in seen)  # today's call
    seen.clear()
    N.normalize(sample, utts, start_step=50, batch_size=2, device="cpu", solver="dpmpp_2m", sampling_steps=10)
    assert len(seen) == 2 and all(k["solver"] == "dpmpp_2m" and k["sampling_steps"] == 10 and "eta" not in k and "seed" not in k for k in seen)
    seen.clear()
    N.normalize(sample, utts, start_step=50, batch_size=2, device="cpu", sampling_steps=10)
    assert all("solver" not in k for k in seen)
