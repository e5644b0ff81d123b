"""The device normal generators against their host restatement (oracle/philox_normal.py): dn_randn element for element, and the
in-kernel draws of dn_ddpm_loop, dn_ddim_sched_loop (eta > 0) and dn_guided_ddim_loop (eta > 0) through the loops' own `noise=`
argument -- a seeded run against the same run with the restatement's numbers injected.

Bar for "device equals host".  The integer core (Philox4x32-10, counter and key layout) and the float32 uniforms / angle are exact in
both; the device then takes logf, sqrtf and sincosf in float32, the restatement log, sqrt, sin and cos in float64.  unit =
2^-23 max(rad, 1) per element, rad the Box-Muller radius from the restatement.  A structurally wrong draw (another counter, key,
round count, lane) is off by about 10^6 units; glibc's float32 functions measured 1.43 units worst over 2^20 quads.  Measured on an
MI355X over the dn_randn cases of this file: 1.680 units worst (at n = 2098179; MEASURED); BAR = ceil(2 x 1.680) = 4 units (it may never
exceed 16: a device that needs more has swapped in fast intrinsics, which is a finding, not a reason for a wider bar).  The lowest bits of the
24-bit uniforms lie below this resolution (flipping the last kept bit of u1 moves the radius by 2^-24 / (u1 rad), under a unit for
all but the smallest u1; of u2, the angle by 2^-24 * 2 pi = 0.4 units of the radius): the known-answer vectors of
tests/test_philox_host.py cover the integer core, and every word of a wrong core changes the top bits of half the draws.

One update: |seeded - injected| <= sigma_step BAR unit + 2^-23 |x| elementwise, sigma_step from the loop's own table (DDPM:
exp(log-variance / 2) of the timestep's row) or coefficient row (column 4), and the timesteps chosen so that sigma_step is at least
100 x the largest such tolerance (asserted): DDPM at t = 199 of the 200-step cosine schedule (sigma 0.9995, |x| up to 400: tolerance
5e-5), the scheduled loops at the one-step schedule [49] (sigma 0.01596, |x| < 5: tolerance 6e-7) -- the one-step schedule [199]
would not do (x1 = x / sqrt abar_199 = 4058 x leaves 2^-23 |x| at a tenth of its sigma).

Short chains (three evaluations: one eager step, one captured, two replays): seeded against injected within the flat f32 chain bar
1e-3 of test_ddpm_loop_matches_reference_p_sample_steps and DESIGN section 6; a step counter that does not advance under replay feeds step
i + 1 the draw of step i, which tests/test_philox_host.py shows to miss that bar by more than 100 x on the CPU oracle chains."""
import math

import numpy as np
import pytest
import torch

import philox_normal as P
from gen_golden_configs import CHAIN_VAE
from test_hip_ddim_schedule import COMBOS, eps_engine, on_stream, sched_run
from test_hip_ddim_schedule import B as BU, T as TU, x_start as x_start_u
from test_hip_guided_schedule import B as BG, T as TG, Z as ZG, Inputs, cond_engine, loop_run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x123456789ABCDEF0
MEASURED = 1.680  # worst |device - host| / unit over the dn_randn cases below, on an MI355X
BAR = 4  # units: ceil(2 * MEASURED), never above 16
UNIT = 2.0 ** -23
CHAIN_BAR = 1e-3  # the f32 chain bar of test_hip_engine.py / test_hip_ddim_schedule.py / test_hip_guided_schedule.py
SENTINEL = -12345.678
PASS_QUADS = 2048 * 256  # quads of one grid-stride pass of randn_kernel (the grid is capped at 2048 blocks of 256 threads)
N_BIG = PASS_QUADS * 4 + 256 * 4 + 3  # a second pass of 257 quads, the last one ragged
SIZES = (1, 2, 3, 4, 5, 1023, 4096)
OFFSETS = (((1 << 32) - 3, 32), ((1 << 40) + 5, 64), ((1 << 64) - 2, 16))  # carry into the second counter word; the bench's range; wrap
K_CUT = PASS_QUADS - 100  # quads: randn(1000, offset = K_CUT) = elements 4 K_CUT .. 4 K_CUT + 999 of the big draw, across its pass boundary
SCHED = [49, 41, 33]
UZ = CHAIN_VAE.z


def device_randn(n, seed, offset=0):
    """dn_randn into a buffer 8 floats longer, prefilled with a sentinel -> (float32 [n] on the CPU, whether the 8 floats past n kept
    the sentinel bit for bit)."""
    from diffnorm_amd import _lib

    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device=DEV)
    on_stream(lambda: _lib.check(_lib.load().dn_randn(buf.data_ptr(), n, seed, offset, _lib.current_stream()), "dn_randn"))
    out = buf.cpu()
    return out[:n], torch.equal(out[n:].view(torch.int32), torch.full((8,), SENTINEL).view(torch.int32))


def ratio(dev, host, rad):
    """Worst |device - host| in units of 2^-23 max(rad, 1)."""
    return float((np.abs(dev.double().numpy().ravel() - host.ravel()) / (UNIT * np.maximum(rad.ravel(), 1.0))).max())


@pytest.fixture(scope="module")
def draws():
    """Every dn_randn case once: {(n, seed, offset): (device float32 [n], worst ratio against the restatement, tail intact)}."""
    cases = [(n, SEED, 0) for n in SIZES] + [(N_BIG, SEED, 0)] + [(n, SEED, off) for off, n in OFFSETS] + [(4096, SEED ^ (1 << 40), 0)]
    out = {}
    for n, seed, off in cases:
        dev, intact = device_randn(n, seed, off)
        host, rad = P.randn(n, seed, off)
        out[(n, seed, off)] = (dev, ratio(dev, host, rad), intact)
        print(f"dn_randn n={n} seed={seed:#x} offset={off:#x}: worst {out[(n, seed, off)][1]:.3f} units")
    return out


def test_bar_is_twice_the_measured_device_error(draws):
    worst = max(r for _, r, _ in draws.values())
    print(f"dn_randn against the float64 restatement, worst of {len(draws)} cases: {worst:.3f} units (recorded {MEASURED}, bar {BAR})")
    assert BAR <= 16 and BAR == math.ceil(2 * MEASURED)
    assert worst <= BAR


@pytest.mark.parametrize("n", SIZES + (N_BIG,))
def test_randn_sizes_and_tails(draws, n):
    dev, r, intact = draws[(n, SEED, 0)]
    assert intact, n  # nothing past n was written
    assert dev.shape == (n,) and torch.isfinite(dev).all() and r <= BAR, (n, r)


@pytest.mark.parametrize("offset,n", OFFSETS)
def test_randn_offsets(draws, offset, n):
    dev, r, intact = draws[(n, SEED, offset)]
    assert intact and r <= BAR, (offset, r)
    if offset == (1 << 64) - 2:  # quads 2^64 - 2, 2^64 - 1, 0, 1: the second half is the start of the offset-0 stream
        assert torch.equal(dev[8:], draws[(4096, SEED, 0)][0][:8])


def test_randn_offset_is_a_quad_index_across_the_pass_boundary(draws):
    big = draws[(N_BIG, SEED, 0)][0]
    assert 4 * K_CUT < 4 * PASS_QUADS < 4 * K_CUT + 1000 <= N_BIG
    cut, intact = device_randn(1000, SEED, K_CUT)
    assert intact and torch.equal(cut, big[4 * K_CUT:4 * K_CUT + 1000])
    assert torch.equal(draws[(4096, SEED, 0)][0], big[:4096]) and torch.equal(draws[(1023, SEED, 0)][0], big[:1023])


def test_randn_high_seed_word(draws):
    a, b = draws[(4096, SEED, 0)], draws[(4096, SEED ^ (1 << 40), 0)]
    assert a[1] <= BAR and b[1] <= BAR and not torch.equal(a[0], b[0])


# ------------------------------------------------------------------------------------------ in-kernel draws
@pytest.fixture(scope="module")
def eng():
    from diffnorm_amd import engine, scheduler

    return engine, scheduler.DDPMScheduler(200)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float()


def assert_one_update(seeded, injected, rad, sigma, what):
    tol = sigma * BAR * UNIT * np.maximum(rad, 1.0) + UNIT * injected.double().abs().numpy()
    err = (seeded.double() - injected.double()).abs().numpy()
    print(f"{what}: sigma {sigma:.4e}, worst tolerance {tol.max():.3e}, worst error {err.max():.3e} ({(err / tol).max():.3f} of its tolerance)")
    assert sigma >= 100 * tol.max(), (what, sigma, tol.max())  # a wrong draw (off by about sigma) cannot hide
    assert (err <= tol).all(), (what, float((err / tol).max()))


def ddpm_run(e, lens, table, start, evals, graph, split, **kw):
    x = x_start_u().to(DEV).clone()
    assert on_stream(lambda: e.ddpm_loop(x, lens, start, table, use_graph=graph, split=split, max_evals=evals, **kw)) == evals
    return x.cpu()


def ddpm_rows(start, evals, split):
    """Injected noise of a chain from `start`: row k for t = start - 1 - k (the rows past `evals` are never read)."""
    shape = (BU, TU, UZ)
    noise, rads = torch.zeros(start, *shape), []
    for k in range(evals):
        z, rad = P.ddpm_loop_noise(shape, SEED, start - 1 - k, split=split)
        noise[k] = f32(z)
        rads.append(rad)
    return noise, rads


@pytest.mark.parametrize("graph,split", [(False, False), (True, False), (True, True)])
def test_ddpm_one_update_draws_the_host_numbers(eng, golden, graph, split):
    """t = 199.  B = 3: a split chain's halves are rows [0, 1) under the seed and [1, 3) under seed ^ SPLIT_KEY, quads from 0 in
    each.  (One evaluation is never captured, whatever the flag says: the chains below replay.)"""
    engine, sched = eng
    e, lens = eps_engine(engine, "f32"), torch.from_numpy(golden("chain_small")["lens"]).to(DEV).int()
    table = sched.gaussian_table(DEV)
    noise, rads = ddpm_rows(200, 1, split)
    sigma = float(np.exp(0.5 * np.float64(sched.gaussian_table()[199, 4].item())))
    seeded = ddpm_run(e, lens, table, 200, 1, graph, split, seed=SEED)
    injected = ddpm_run(e, lens, table, 200, 1, graph, split, noise=noise)
    assert_one_update(seeded, injected, rads[0], sigma, f"ddpm t=199 graph={graph} split={split}")
    if split:  # the unsplit stream in the second half is a different draw
        other = ddpm_run(e, lens, table, 200, 1, graph, split, noise=ddpm_rows(200, 1, False)[0])
        assert (seeded - other)[1:].abs().max() > 1.0 and torch.equal(other[:1], injected[:1])


def sched_rows(shape, steps):
    zs, rads = zip(*(P.sched_loop_noise(shape, SEED, i, step=s) for i, s in enumerate(steps)))
    return torch.stack([f32(z) for z in zs]), rads


@pytest.mark.parametrize("graph,split", COMBOS)
def test_sched_one_update_draws_the_host_numbers(eng, golden, graph, split):
    """The one-step schedule [49] at eta = 1: eager, graph and split against the same host noise of the whole batch."""
    engine, sched = eng
    e, lens = eps_engine(engine, "f32"), torch.from_numpy(golden("chain_small")["lens"]).to(DEV).int()
    noise, rads = sched_rows((BU, TU, UZ), [49])
    sigma = float(sched.ddim_schedule(50, steps=[49], eta=1.0)[1][0, 4])
    seeded = sched_run(e, sched, lens, 50, x_start_u(), graph, split, eta=1.0, seed=SEED, steps=[49])
    injected = sched_run(e, sched, lens, 50, x_start_u(), graph, split, eta=1.0, noise=noise, steps=[49])
    assert_one_update(seeded, injected, rads[0], sigma, f"sched [49] graph={graph} split={split}")


def test_sched_last_step_at_zero_draws_nothing(eng, golden):
    """steps = [0] with a coefficient row whose sigma is not 0 (the schedule's own vanishes there): seeded = the restatement's row
    (zeros) injected = the eta = 0 update of that step, bit for bit; the same row at timestep 3 does draw."""
    engine, sched = eng
    e, lens = eps_engine(engine, "f32"), torch.from_numpy(golden("chain_small")["lens"]).to(DEV).int()
    shape = (BU, TU, UZ)

    def run(step, eta, **kw):
        st, coef = sched.ddim_schedule(step + 1, steps=[step], eta=eta, device=DEV)
        plain = coef.clone()
        if eta:
            coef[0, 4] = 0.3
        x = x_start_u().to(DEV).clone()
        assert on_stream(lambda: e.ddim_schedule_loop(x, lens, st, coef, eta=eta, use_graph=False, split=True, timesteps=200, **kw)) == 1
        return x.cpu(), plain

    (seeded, c1), (plain, c0) = run(0, 1.0, seed=SEED), run(0, 0.0)
    assert torch.equal(c1[:, :4], c0[:, :4])  # (the same first four columns: only the noise term could differ)
    assert torch.equal(seeded, plain)
    assert torch.equal(run(0, 1.0, noise=sched_rows(shape, [0])[0])[0], plain)
    drawn, _ = run(3, 1.0, seed=SEED)
    noise, rads = sched_rows(shape, [3])
    assert_one_update(drawn, run(3, 1.0, noise=noise)[0], rads[0], 0.3, "sched [3] with sigma 0.3")


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_guided_one_update_draws_the_scheduled_loops_stream(eng, scale):
    engine, sched = eng
    e, inp = cond_engine(engine, "f32"), Inputs()
    noise, rads = sched_rows((BG, TG, ZG), [49])
    sigma = float(sched.ddim_schedule(50, steps=[49], eta=1.0)[1][0, 4])
    seeded = loop_run(e, sched, inp, 50, scale, False, eta=1.0, seed=SEED, steps=[49])
    injected = loop_run(e, sched, inp, 50, scale, False, eta=1.0, noise=noise, steps=[49])
    assert_one_update(seeded, injected, rads[0], sigma, f"guided [49] scale {scale}")


def chain_close(seeded, injected, what):
    err = (seeded.double() - injected.double()).abs().max().item()
    print(f"{what}: seeded against injected, max abs err {err:.3e}")
    assert torch.isfinite(seeded).all() and err < CHAIN_BAR, (what, err)


@pytest.mark.parametrize("graph,split", [(False, False), (True, False), (True, True)])
def test_ddpm_chain_advances_its_step(eng, golden, graph, split):
    """t = 49, 48, 47 from start 50."""
    engine, sched = eng
    e, lens = eps_engine(engine, "f32"), torch.from_numpy(golden("chain_small")["lens"]).to(DEV).int()
    table = sched.gaussian_table(DEV)
    seeded = ddpm_run(e, lens, table, 50, 3, graph, split, seed=SEED)
    chain_close(seeded, ddpm_run(e, lens, table, 50, 3, graph, split, noise=ddpm_rows(50, 3, split)[0]), f"ddpm chain graph={graph} split={split}")


@pytest.mark.parametrize("graph,split", COMBOS)
def test_sched_chain_advances_its_step(eng, golden, graph, split):
    engine, sched = eng
    e, lens = eps_engine(engine, "f32"), torch.from_numpy(golden("chain_small")["lens"]).to(DEV).int()
    noise, _ = sched_rows((BU, TU, UZ), SCHED)
    seeded = sched_run(e, sched, lens, 50, x_start_u(), graph, split, eta=1.0, seed=SEED, steps=SCHED)
    chain_close(seeded, sched_run(e, sched, lens, 50, x_start_u(), graph, split, eta=1.0, noise=noise, steps=SCHED), f"sched chain graph={graph} split={split}")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_guided_chain_advances_its_step(eng, scale, graph):
    engine, sched = eng
    e, inp = cond_engine(engine, "f32"), Inputs()
    noise, _ = sched_rows((BG, TG, ZG), SCHED)
    seeded = loop_run(e, sched, inp, 50, scale, graph, eta=1.0, seed=SEED, steps=SCHED)
    chain_close(seeded, loop_run(e, sched, inp, 50, scale, graph, eta=1.0, noise=noise, steps=SCHED), f"guided chain scale {scale} graph={graph}")
