"""CPU: the schedule of the EMA of the parameters (optim.EmaSchedule) against the fixture taken from the reference's real EMA class
(tools/gen_golden_ema.py -> tests/golden/ema.npz: per update, EMA.get_decay() and whether _step_internal ran)."""
import pytest

CONFIGS = range(3)


def _schedule(g, i):
    from diffnorm_amd import optim

    decay, start, freq = g["configs"][i]
    return optim.EmaSchedule(decay=float(decay), start_update=int(start), update_freq=int(freq))


@pytest.mark.parametrize("i", CONFIGS)
def test_schedule_reproduces_the_reference_update_by_update(golden, i):
    g = golden("ema")
    sched = _schedule(g, i)
    want_applied, want_decay = g[f"c{i}/applied"], g[f"c{i}/decay"]
    assert len(want_applied) == 7
    for u in range(1, 8):  # the number of updates AFTER the increment (fairseq/trainer.py:1018-1025)
        apply, decay = sched(u)
        assert apply == bool(want_applied[u - 1]), (i, u)
        assert decay == float(want_decay[u - 1]) and sched.get_decay() == decay, (i, u, decay)


def test_fixture_covers_the_three_regimes(golden):
    g = golden("ema")
    assert [tuple(c) for c in g["configs"].tolist()] == [(0.999, 0.0, 1.0), (0.9, 3.0, 1.0), (0.9, 2.0, 3.0)]
    assert g["c0/applied"].all() and (g["c1/decay"][:2] == 0).all() and g["c1/decay"][2] == 0.9
    assert g["c2/applied"].tolist() == [False, False, True, False, False, True, False]
    assert g["params"].shape == (8, 68) and g["c2/ema"].shape == (7, 68)


@pytest.mark.parametrize("i", CONFIGS)
def test_a_restored_schedule_continues_identically(golden, i):
    g = golden("ema")
    whole = _schedule(g, i)
    first = _schedule(g, i)
    for u in range(1, 5):
        assert first(u) == whole(u)
    resumed = _schedule(g, i)  # a fresh process: same flags, state from the checkpoint
    resumed.load_state_dict(dict(first.state_dict()))
    for u in range(5, 8):
        assert resumed(u) == whole(u) == (bool(g[f"c{i}/applied"][u - 1]), float(g[f"c{i}/decay"][u - 1])), (i, u)
    assert resumed.state_dict() == whole.state_dict()


def test_schedule_arguments_and_engine_contract():
    from diffnorm_amd import optim

    with pytest.raises(ValueError):
        optim.EmaSchedule(decay=1.0)
    with pytest.raises(ValueError):
        optim.EmaSchedule(decay=-0.1)
    calls = []
    # no schedule: exactly the caller's call, no new keywords (the exchange tests' recorder takes none)
    assert optim.step_engine_ema(object(), None, 1, lambda **kw: calls.append(kw) or "norm") == "norm" and calls == [{}]

    class Eng:
        ema, ema_count = None, 0

    with pytest.raises(ValueError, match="enable_ema"):
        optim.step_engine_ema(Eng(), optim.EmaSchedule(0.9), 1, lambda **kw: None)
    eng = Eng()
    eng.ema = "buffer"
    sched = optim.EmaSchedule(0.9, start_update=2, update_freq=2)
    for u in (1, 2, 3, 4):
        optim.step_engine_ema(eng, sched, u, lambda **kw: calls.append(kw))
    assert calls[1:] == [{}, {"ema": "buffer", "ema_decay": 0.9}, {}, {"ema": "buffer", "ema_decay": 0.9}] and eng.ema_count == 2
