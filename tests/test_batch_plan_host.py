"""Host logic of batch-independent normalisation (no GPU): the per-utterance noise keys (splitmix64 known answers), the frame-budget
planner and the cost balancer of diffnorm_amd/sharding.py, and normalize() over a stand-in sampler whose prediction is a pure
function of (the utterance's key, its own valid frames) -- so any way of forming and sharding batches must give the same lines."""
import os
import random

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
WORKED = [40, 9, 33, 17, 40, 5, 28, 12, 36, 21, 7]


@pytest.fixture(scope="module")
def lib():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    return _lib.load()


def rows(lengths, batches, pad_multiple=1):
    from diffnorm_amd import sharding

    return sum(len(b) * sharding.padded_length(max(lengths[i] for i in b), pad_multiple) for b in batches)


# ------------------------------------------------------------------------------------------ keys
def test_splitmix64_known_answers_and_int64_round_trip():
    from diffnorm_amd import sharding

    k = sharding.utterance_keys(0, [0, 1])
    assert k.dtype == torch.int64 and k.shape == (2,)
    assert [int(v) & M64 for v in k.tolist()] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]
    assert sharding.key_bits(sharding.utterance_keys(1234567, [0])) == [0x599ED017FB08FC85]
    assert k[0].item() < 0 < k[1].item()  # bit 63 set: the int64 is negative, the bit pattern is kept
    # a key depends on (seed, index) only: any subset, any order
    idx = [7, 0, 3, 1 << 40]
    full = sharding.key_bits(sharding.utterance_keys(99, range(8)))
    assert sharding.key_bits(sharding.utterance_keys(99, idx))[:3] == [full[7], full[0], full[3]]
    assert sharding.key_bits(sharding.utterance_keys((1 << 64) + 99, idx)) == sharding.key_bits(sharding.utterance_keys(99, idx))  # mod 2^64
    assert len(set(sharding.key_bits(sharding.utterance_keys(5, range(1000))))) == 1000
    assert sharding.utterance_keys(0, []).shape == (0,)


# ------------------------------------------------------------------------------------------ planner
def check_plan(lengths, max_tokens, max_sentences, pad_multiple):
    from diffnorm_amd import sharding

    plan = sharding.plan_batches(lengths, max_tokens, max_sentences, pad_multiple)
    assert plan == sharding.plan_batches(list(lengths), max_tokens, max_sentences, pad_multiple)  # deterministic
    assert sorted(i for b in plan for i in b) == list(range(len(lengths)))  # every index exactly once
    order = [i for b in plan for i in b]
    assert order == sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    for b in plan:
        T = sharding.padded_length(lengths[b[0]], pad_multiple)
        assert T % pad_multiple == 0 and T >= max(lengths[i] for i in b) and T - lengths[b[0]] < pad_multiple
        assert len(b) * T <= max_tokens or (len(b) == 1 and T > max_tokens)
        assert max_sentences is None or len(b) <= max_sentences
    for b, nxt in zip(plan, plan[1:]):  # greedy: the next utterance did not fit
        T = sharding.padded_length(lengths[b[0]], pad_multiple)
        assert (len(b) + 1) * T > max_tokens or (max_sentences is not None and len(b) == max_sentences)
    return plan


def test_plan_batches_worked_example():
    plan = check_plan(WORKED, 96, None, 8)
    assert plan == [[0, 4], [8, 2], [6, 9, 3], [7, 1, 10, 5]]
    consecutive = [list(range(s, min(s + 4, len(WORKED)))) for s in range(0, len(WORKED), 4)]
    assert rows(WORKED, plan, 8) == 320 and rows(WORKED, consecutive) == 428


def test_plan_batches_hand_cases():
    from diffnorm_amd import sharding

    assert sharding.plan_batches([], 10) == []
    assert check_plan([5], 10, None, 1) == [[0]]
    assert check_plan([50, 3, 3], 10, None, 1) == [[0], [1, 2]]  # longer than the budget: alone
    assert check_plan([50, 60, 3], 10, None, 1) == [[1], [0], [2]]
    assert check_plan([4, 4, 4, 4, 4], 8, None, 1) == [[0, 1], [2, 3], [4]]  # ties by index
    assert check_plan([4, 4, 4, 4, 4], 100, 2, 1) == [[0, 1], [2, 3], [4]]  # the sentence cap
    assert check_plan([4, 4, 4, 4, 4], 100, None, 1) == [[0, 1, 2, 3, 4]]
    assert check_plan([5, 3], 8, None, 8) == [[0], [1]] and check_plan([5, 3], 16, None, 8) == [[0, 1]]  # T counts padded
    assert check_plan([9, 8], 16, None, 8) == [[0], [1]]  # 9 pads to 16
    for bad in (dict(max_tokens=0), dict(max_tokens=8, max_sentences=0), dict(max_tokens=8, pad_multiple=0)):
        with pytest.raises(ValueError):
            sharding.plan_batches([1, 2], **bad)


@pytest.mark.parametrize("seed", range(6))
def test_plan_batches_properties_on_random_lengths(seed):
    rng = random.Random(seed)
    lengths = [rng.choice([1, 2, 7, 31, 32, 33]) if rng.random() < 0.2 else int(rng.lognormvariate(5.5, 0.6)) + 1 for _ in range(rng.randint(1, 300))]
    for max_tokens in (64, 1000, 16384):
        for max_sentences in (None, 1, 7):
            for pad_multiple in (1, 8, 32):
                check_plan(lengths, max_tokens, max_sentences, pad_multiple)


def test_budget_plans_compute_fewer_rows_than_consecutive_hundreds():
    """The padding argument on a synthetic log-normal corpus: sorted batches under a frame budget compute fewer frame-rows."""
    rng = random.Random(0)
    lengths = [min(1024, max(58, int(rng.lognormvariate(5.55, 0.55)))) for _ in range(400)]
    consecutive = [list(range(s, min(s + 100, 400))) for s in range(0, 400, 100)]
    valid = sum(lengths)
    for budget in (16384, 49152):
        assert valid <= rows(lengths, check_plan(lengths, budget, None, 1)) < rows(lengths, consecutive)


# ------------------------------------------------------------------------------------------ balancer
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_balanced_batches(world):
    from diffnorm_amd import sharding

    rng = random.Random(world)
    for costs in ([], [5], [3, 3, 3, 3], [10, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [rng.randint(1, 20000) for _ in range(57)]):
        parts = [sharding.balanced_batches(costs, r, world) for r in range(world)]
        assert parts == [sharding.balanced_batches(list(costs), r, world) for r in range(world)]  # deterministic
        assert sorted(b for p in parts for b in p) == list(range(len(costs)))  # a partition
        assert all(p == sorted(p) for p in parts)
        loads = [sum(costs[b] for b in p) for p in parts]
        if costs:
            assert max(loads) <= sum(costs) / world + max(costs)
    assert sharding.balanced_batches([3, 3, 3, 3], 0, 2) == [0, 2] and sharding.balanced_batches([3, 3, 3, 3], 1, 2) == [1, 3]
    if world == 2:  # the largest first, then the lightest rank, the lowest on ties
        assert sharding.balanced_batches([1, 9, 4, 4], 0, 2) == [1] and sharding.balanced_batches([1, 9, 4, 4], 1, 2) == [0, 2, 3]


# ------------------------------------------------------------------------------------------ normalize() over a stand-in sampler
def corpus():
    from diffnorm_amd import normalize as N

    g = torch.Generator().manual_seed(3)
    utts = []
    for i in range(23):
        n = int(torch.randint(3, 40, (1,), generator=g))
        units = (torch.randint(0, 25, (n,), generator=g) * 2 + torch.arange(n) % 2).tolist()  # neighbours differ: nothing to de-duplicate
        utts.append(N.Utterance(f"u{i}", f"s{i}.wav", 100 + i, torch.randn(n, 16, generator=g), units, units))
    return utts


class FakeSampler:
    """Prediction of frame (b, t) = f(noise_keys[b], feat[b, t]) for the valid frames: nothing of the batch's shape or neighbours."""

    def __init__(self):
        self.calls = []

    def __call__(self, feat, **kw):
        self.calls.append((tuple(feat.shape), dict(kw)))
        lens = kw["input_mask"].sum(1).tolist()
        assert kw["input_mask"].shape == feat.shape[:2] and kw["ref_units"].shape == feat.shape[:2]
        keys = kw["noise_keys"].tolist() if "noise_keys" in kw else [0] * feat.shape[0]
        pred = [((feat[b, : lens[b]].abs().sum(-1) * 7).long() + ((keys[b] & M64) % 1009)) % 50 for b in range(feat.shape[0])]
        return pred, 0, int(sum(lens)), None


def run(monkeypatch, utts, rank_world=(0, 1), **kw):
    """normalize() as rank `rank` of `world` without a process group: the gather returns this rank's batches only (the others empty)."""
    from diffnorm_amd import normalize as N
    from diffnorm_amd import sharding

    def gather(local, ids, n_total, group=None):
        out = [[] for _ in range(n_total)]
        for i, r in zip(ids, local):
            out[i] = r
        return out

    monkeypatch.setattr(sharding, "rank_world", lambda group=None: rank_world)
    monkeypatch.setattr(sharding, "gather_in_order", gather)
    fake = FakeSampler()
    return N.normalize(fake, utts, start_step=5, device="cpu", **kw), fake


PLANS = [dict(batch_size=4), dict(batch_size=100), dict(batch_size=4, pad_multiple=8), dict(max_tokens=64), dict(max_tokens=200, pad_multiple=8),
         dict(max_tokens=4096, max_sentences=5), dict(max_tokens=1)]


def test_normalize_lines_do_not_depend_on_the_plan_or_the_world(lib, monkeypatch):
    utts = corpus()
    want, fake = run(monkeypatch, utts, noise_seed=7, **PLANS[0])
    assert len(want) == len(utts) and [l.split("\t")[0] for l in want] == [u.audio_id for u in utts]
    assert all(set(kw) == {"input_mask", "cond_scale", "ref_units", "start_step", "noise_keys"} for _, kw in fake.calls)
    shapes = set()
    for plan in PLANS:
        got, fake = run(monkeypatch, utts, noise_seed=7, **plan)
        assert got == want, plan
        pm = plan.get("pad_multiple", 1)
        assert all(shape[1] % pm == 0 for shape, _ in fake.calls)
        if "max_tokens" in plan:
            assert all(s[0] * s[1] <= plan["max_tokens"] or s[0] == 1 for s, _ in fake.calls)
            assert all(s[0] <= plan.get("max_sentences", 1 << 30) for s, _ in fake.calls)
        shapes.add(tuple(s for s, _ in fake.calls))
        parts = [run(monkeypatch, utts, rank_world=(r, 2), noise_seed=7, **plan)[0] for r in range(2)]
        assert all((a is None) != (b is None) for a, b in zip(*parts)), plan  # every utterance on exactly one rank
        assert [a if a is not None else b for a, b in zip(*parts)] == want, plan
    assert len(shapes) == len(PLANS)  # the plans did form different batches
    other, _ = run(monkeypatch, utts, noise_seed=8, **PLANS[0])
    assert other != want  # the seed reaches the sampler


def test_normalize_keys_are_the_utterances_positions(lib, monkeypatch):
    from diffnorm_amd import sharding

    utts = corpus()
    _, fake = run(monkeypatch, utts, noise_seed=11, max_tokens=128, pad_multiple=8)
    lengths = [len(u.reduce_tgt_unit) for u in utts]
    plan = sharding.plan_batches(lengths, 128, None, 8)
    assert len(fake.calls) == len(plan)
    for ids, (shape, kw) in zip(plan, fake.calls):
        assert torch.equal(kw["noise_keys"], sharding.utterance_keys(11, ids)) and shape[0] == len(ids)
        assert kw["input_mask"].sum(1).tolist() == [lengths[i] for i in ids]


def test_normalize_with_the_new_arguments_unset_calls_the_sampler_as_before(lib, monkeypatch):
    utts = corpus()
    lines, fake = run(monkeypatch, utts, batch_size=4)
    assert len(lines) == len(utts) and len(fake.calls) == 6
    assert all(set(kw) == {"input_mask", "cond_scale", "ref_units", "start_step"} for _, kw in fake.calls)
    assert [s for s, _ in fake.calls] == [(len(utts[s:s + 4]), max(len(u.reduce_tgt_unit) for u in utts[s:s + 4]), 16) for s in range(0, 23, 4)]
    _, fake = run(monkeypatch, utts, batch_size=4, sampling_steps=3, eta=0.5, seed=9, solver=None)
    assert all(set(kw) == {"input_mask", "cond_scale", "ref_units", "start_step", "sampling_steps", "eta", "seed"} for _, kw in fake.calls)
    _, fake = run(monkeypatch, utts, batch_size=4, noise_seed=1, sampling_steps=3, solver="dpmpp_2m")
    assert all(set(kw) == {"input_mask", "cond_scale", "ref_units", "start_step", "sampling_steps", "solver", "noise_keys"} for _, kw in fake.calls)


def test_normalize_refusals(lib, monkeypatch):
    utts = corpus()
    with pytest.raises(ValueError, match="noise_seed"):
        run(monkeypatch, utts, max_tokens=64)
    with pytest.raises(ValueError, match="eta"):
        run(monkeypatch, utts, noise_seed=1, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        run(monkeypatch, utts, noise_seed=1, max_tokens=64, eta=1.0)


def test_assemble_batch_pad_to():
    from diffnorm_amd import normalize as N

    utts = corpus()[:3]
    feat, unit, lens = N.assemble_batch(utts, "cpu")
    wide, wunit, wlens = N.assemble_batch(utts, "cpu", pad_to=feat.shape[1] + 5)
    assert wide.shape[1] == feat.shape[1] + 5 and torch.equal(wide[:, : feat.shape[1]], feat) and not wide[:, feat.shape[1]:].any()
    assert torch.equal(wunit[:, : feat.shape[1]], unit) and torch.equal(wlens, lens)
    with pytest.raises(AssertionError):
        N.assemble_batch(utts, "cpu", pad_to=feat.shape[1] - 1)
