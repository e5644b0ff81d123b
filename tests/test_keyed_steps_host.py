"""Host logic of keyed per-step noise (no GPU): normalize()'s `keyed_steps=` over the stand-in sampler of
tests/test_batch_plan_host.py -- which keywords reach the sampler with and without the switch, and what is refused."""
import pytest

from test_batch_plan_host import PLANS, corpus, lib, run  # noqa: F401  (lib: the fixture that builds the library when it is missing)

BASE = {"input_mask", "cond_scale", "ref_units", "start_step"}


def test_normalize_passes_keyed_steps_next_to_the_keys_and_no_seed(lib, monkeypatch):
    utts = corpus()
    want, fake = run(monkeypatch, utts, noise_seed=7, eta=0.5, keyed_steps=True, max_tokens=64)
    assert len(want) == len(utts) and len(fake.calls) > 1
    assert all(set(kw) == BASE | {"eta", "noise_keys", "keyed_steps"} for _, kw in fake.calls)
    assert all(kw["keyed_steps"] is True and kw["eta"] == 0.5 for _, kw in fake.calls)
    _, fake = run(monkeypatch, utts, noise_seed=7, eta=0.5, seed=9, keyed_steps=True, sampling_steps=3, batch_size=4)
    assert all(set(kw) == BASE | {"eta", "noise_keys", "keyed_steps", "sampling_steps"} for _, kw in fake.calls)  # `seed` is not passed on
    for plan in PLANS:  # the lines of a stochastic chain do not depend on the plan either
        assert run(monkeypatch, utts, noise_seed=7, eta=0.5, keyed_steps=True, **plan)[0] == want, plan


def test_keyed_steps_at_eta_zero_is_passed_on_too(lib, monkeypatch):
    _, fake = run(monkeypatch, corpus(), noise_seed=7, keyed_steps=True, batch_size=4)
    assert all(set(kw) == BASE | {"noise_keys", "keyed_steps"} for _, kw in fake.calls)


def test_without_keyed_steps_the_keyword_sets_are_the_earlier_ones(lib, monkeypatch):
    utts = corpus()
    _, fake = run(monkeypatch, utts, batch_size=4)
    assert all(set(kw) == BASE for _, kw in fake.calls)
    _, fake = run(monkeypatch, utts, batch_size=4, sampling_steps=3, eta=0.5, seed=9)
    assert all(set(kw) == BASE | {"sampling_steps", "eta", "seed"} for _, kw in fake.calls)
    _, fake = run(monkeypatch, utts, noise_seed=7, max_tokens=64)
    assert all(set(kw) == BASE | {"noise_keys"} for _, kw in fake.calls)
    _, fake = run(monkeypatch, utts, noise_seed=7, max_tokens=64, keyed_steps=False)
    assert all(set(kw) == BASE | {"noise_keys"} for _, kw in fake.calls)


def test_refusals(lib, monkeypatch):
    utts = corpus()
    with pytest.raises(ValueError, match="eta") as e:
        run(monkeypatch, utts, noise_seed=1, eta=0.5)
    assert "keyed_steps" in str(e.value)  # the message names the way out
    with pytest.raises(ValueError, match="eta"):
        run(monkeypatch, utts, noise_seed=1, max_tokens=64, eta=1.0, keyed_steps=False)
    with pytest.raises(ValueError, match="noise_seed"):
        run(monkeypatch, utts, eta=0.5, keyed_steps=True)
    with pytest.raises(ValueError, match="noise_seed"):
        run(monkeypatch, utts, keyed_steps=True, batch_size=4)
