"""oracle/philox_normal.py, the host restatement the device normal generators are held to (tests/test_hip_philox.py): the Random123
known-answer vectors of Philox4x32-10, the ends of the (0, 1] uniform map, moments and lane correlations of each stream, the
distinctness the counter / key layouts promise, and -- on the CPU oracle chains -- that a step fed the next step's noise row misses
the chain bars by a wide margin, so the short seeded chains of the GPU test can tell a counter that does not advance."""
import numpy as np
import pytest
import torch

import diffnorm_oracle as O
import philox_normal as P
from gen_golden_configs import CHAIN_EPS, CHAIN_VAE

SEED = 0x123456789ABCDEF0
NQ = 1 << 20

KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def test_random123_known_answer_vectors():
    for ctr, key, want in KAT:
        assert " ".join("%08x" % int(w) for w in P.philox4x32_10(*ctr, *key)) == want
    # vectorised: the three at once give the same words
    cols = [np.array([c[j] for c, _, _ in KAT], dtype=np.uint64) for j in range(4)]
    keys = [np.array([k[j] for _, k, _ in KAT], dtype=np.uint64) for j in range(2)]
    out = P.philox4x32_10(*cols, *keys)
    for i, (_, _, want) in enumerate(KAT):
        assert " ".join("%08x" % int(w[i]) for w in out) == want


def test_uniform_map_is_half_open_at_zero():
    top = np.array([0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64)  # the 24 kept bits all ones: 16777215 + 0.5 ties to 2^24 in float32
    u = P.uniform_from_word(top)
    assert u.dtype == np.float32 and (u == np.float32(1.0)).all()
    zero = np.zeros(2, dtype=np.uint64)
    assert (P.uniform_from_word(zero) == np.float32(2.0 ** -25)).all()
    assert (P.uniform_from_word(np.array([0xFFFFFE00], dtype=np.uint64)) < 1.0).all()  # one below: (2^24 - 1.5) 2^-24, exact
    # u1 = 1: radius 0, a finite draw of 0 whatever the angle; u1 = 2^-25: the largest radius, sqrt(50 ln 2)
    z, rad = P.normals_from_words((top, np.array([0x12345678, 0xFFFFFFFF], dtype=np.uint64), zero, zero))
    assert np.isfinite(z).all() and (z[:, :2] == 0).all() and (rad[:, :2] == 0).all()
    assert np.allclose(rad[:, 2:], np.sqrt(50 * np.log(2.0)), rtol=1e-15) and np.isfinite(rad).all()
    assert np.allclose(z[:, 2], np.sqrt(50 * np.log(2.0)) * np.cos(np.float64(np.float32(6.28318530717958647692) * np.float32(2.0 ** -25))))


# measured on the restatement, 2^20 quads each (mean, std, fourth moment); the bars are test_randn_statistics's
STREAMS = {"randn": (lambda: P.randn(4 * NQ, SEED), (-8.912e-05, 1.000481, 3.005355)),
           "ddpm t=199": (lambda: P.step_noise(NQ, SEED, 199), (-6.843e-05, 1.000345, 3.006144)),
           "sched i=0": (lambda: P.step_noise(NQ, SEED, 0), (3.646e-04, 1.000132, 3.004109))}


@pytest.mark.parametrize("name", list(STREAMS))
def test_moments_and_lane_correlations(name):
    draw, (mean, std, m4) = STREAMS[name]
    z, rad = draw()
    assert z.shape == rad.shape == (4 * NQ,) and np.isfinite(z).all() and rad.max() <= np.sqrt(50 * np.log(2.0))
    got = (z.mean(), z.std(), (z ** 4).mean())
    print(f"{name}: mean {got[0]:.3e} std {got[1]:.6f} fourth moment {got[2]:.6f}")
    assert abs(got[0] - mean) < 1e-6 and abs(got[1] - std) < 1e-6 and abs(got[2] - m4) < 1e-6  # the recorded values
    assert abs(got[0]) < 5e-3 and abs(got[1] - 1) < 5e-3 and abs(got[2] - 3) < 5e-2
    corr = np.corrcoef(z.reshape(NQ, 4).T)
    off = np.abs(corr - np.eye(4)).max()
    print(f"{name}: largest lane correlation {off:.3e} (bar {4 / np.sqrt(NQ):.3e})")
    assert off < 4 / np.sqrt(NQ)


def test_streams_are_distinct():
    n = 64
    shape = (3, 4, 16)
    plain, _ = P.randn(4 * n, SEED, 0)
    tagged, _ = P.step_noise(n, SEED, 0)  # the same key and first three counter words: only the tag differs
    assert not np.any(plain == tagged)
    assert not np.any(P.step_noise(n, SEED, 1)[0] == tagged)  # steps i and i + 1
    assert not np.any(P.sched_loop_noise(shape, SEED, 1)[0] == P.sched_loop_noise(shape, SEED, 2)[0])
    assert not np.any(P.ddpm_loop_noise(shape, SEED, 199)[0] == P.ddpm_loop_noise(shape, SEED, 198)[0])
    # the DDPM halves: rows [0, 1) and [1, 3) of a split chain; the second half is not the first half's stream continued, restarted
    # or re-keyed by the low word alone
    whole, split = P.ddpm_loop_noise(shape, SEED, 7)[0], P.ddpm_loop_noise(shape, SEED, 7, split=True)[0]
    assert np.array_equal(split[:1], whole[:1]) and not np.any(split[1:] == whole[1:])
    assert not np.any(split[1].ravel() == split[0].ravel())
    assert np.array_equal(split[1:].ravel(), P.step_noise(2 * 4 * 16 // 4, SEED ^ P.SPLIT_KEY, 7)[0])
    # the scheduled loops' halves continue one stream: q0 = the first quad of the second half
    assert np.array_equal(P.sched_loop_noise(shape, SEED, 2)[0][1:].ravel(), P.step_noise(2 * 16, SEED, 2, q0=16)[0])
    assert not np.any(P.step_noise(16, SEED, 2, q0=16)[0] == P.step_noise(16, SEED, 2, q0=0)[0])
    # the high seed word reaches the key
    assert not np.any(P.randn(4 * n, SEED ^ (1 << 40))[0] == plain) and not np.any(P.step_noise(n, SEED ^ (1 << 40), 0)[0] == tagged)
    # the counter: offset = quad index, with the carry into the second word and modulo 2^64
    long_, _ = P.randn(4 * n, SEED, (1 << 32) - 3)
    assert np.array_equal(long_[12:], P.randn(4 * n - 12, SEED, 1 << 32)[0]) and not np.any(long_[12:] == plain[:4 * n - 12])
    wrap, _ = P.randn(16, SEED, (1 << 64) - 2)
    assert np.array_equal(wrap[8:], plain[:8]) and not np.any(wrap[:8] == plain[:8])
    assert np.array_equal(P.randn(5, SEED)[0], plain[:5])  # the tail: the first n of the last quad
    assert not P.sched_loop_noise(shape, SEED, 3, step=0)[0].any()  # timestep 0 applies no draw


def _ddpm_chain(rows, start, mask):
    from test_hip_ddim_schedule import x_start

    sd = O.make_eps_state_dict(CHAIN_EPS, "chain")
    diff = O.GaussianDiffusionOracle(O.cosine_betas(200), "fixed_small")
    x = x_start()
    with torch.no_grad():
        for k, row in enumerate(rows):
            t = torch.full((x.shape[0],), start - 1 - k, dtype=torch.long)
            x = diff.p_sample(lambda xx, tt: O.eps_forward(sd, CHAIN_EPS, xx, tt, mask), x, t, row, False)["sample"]
    return x


def test_a_shifted_noise_row_breaks_the_chain_bars(golden):
    """The three-evaluation chains of tests/test_hip_philox.py on the CPU oracle, once with rows i = 0, 1, 2 and once with rows
    1, 2, 3 (every step fed its successor's draw): the results differ by more than 100 x the 1e-3 chain bar (measured: DDPM from
    start 50 0.44, scheduled [49, 41, 33] at eta = 1 0.94, guided at scale 2 0.96)."""
    import test_hip_ddim_schedule as S
    import test_hip_guided_schedule as G

    f = lambda a: torch.from_numpy(a).float()  # noqa: E731
    lens = torch.from_numpy(golden("chain_small")["lens"])
    mask = O.lengths_to_mask(lens.long(), S.T)
    shape = (S.B, S.T, CHAIN_VAE.z)
    rows = [f(P.ddpm_loop_noise(shape, SEED, 49 - k)[0]) for k in range(4)]
    d = (_ddpm_chain(rows[:3], 50, mask) - _ddpm_chain(rows[1:], 50, mask)).abs().max().item()
    print(f"ddpm chain, shifted rows: {d:.3e}")
    assert d > 0.1
    steps = [49, 41, 33]
    saved = dict(S._refs), dict(G._refs)  # (the modules' caches are keyed without the noise: keep these runs out of them)
    try:
        rows = torch.stack([f(P.sched_loop_noise(shape, SEED, i)[0]) for i in range(4)])
        S._refs.clear()
        a = S.reference_chain(lens, steps, 1.0, rows[:3])
        S._refs.clear()
        d = (a - S.reference_chain(lens, steps, 1.0, rows[1:])).abs().max().item()
        print(f"scheduled chain, shifted rows: {d:.3e}")
        assert d > 0.1
        rows = torch.stack([f(P.sched_loop_noise((G.B, G.T, G.Z), SEED, i)[0]) for i in range(4)])
        G._refs.clear()
        a = G.reference_chain(steps, 2.0, 1.0, rows[:3])
        G._refs.clear()
        d = (a - G.reference_chain(steps, 2.0, 1.0, rows[1:])).abs().max().item()
        print(f"guided chain, shifted rows: {d:.3e}")
        assert d > 0.1
    finally:
        for mod, keep in zip((S, G), saved):
            mod._refs.clear()
            mod._refs.update(keep)
