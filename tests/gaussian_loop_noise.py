"""TEST INFRASTRUCTURE ONLY: the counter / key layout of dn_gaussian_loop's in-kernel draws, restated on the host with
oracle/philox_normal.py (imported, never edited).  the generic Gaussian update (sched_step_kernel under GaussRule) draws through the scheduled loops' sched_normal4:

* seed-drawn:  Philox4x32-10 under key (seed low, seed high), counter (quad low, quad high, chain position i, "DPMP"), the quad of
               the WHOLE [B, T, Z] batch -- philox_normal.step_noise, as dn_ddim_sched_loop;
* keyed:       under key keys[b], counter (q low, q high, 2 + t, "STRT"), q = the quad WITHIN utterance b and t = steps[i], the
               ORIGINAL timestep -- the stream dn_randn_keyed materialises for stream_id = 2 + t.

The update at the last row (respaced index 0) applies no draw; the callers below restate that by not asking for it."""
import numpy as np

import philox_normal as P

STRT = 0x53545254  # fourth counter word of the keyed streams


def seed_noise(shape, seed, i):
    """The seed-drawn normals of update `i` for x of `shape` = (B, T, Z) -> (normals, radius) float64 of `shape`."""
    B, T, Z = shape
    assert Z % 4 == 0
    z, rad = P.step_noise(B * T * Z // 4, seed, i)
    return z.reshape(shape), rad.reshape(shape)


def keyed_noise(keys, T, Z, timestep):
    """The keyed normals of the update that leaves ORIGINAL timestep `timestep`, for utterances under `keys` (Python ints, uint64)
    -> (normals, radius) float64 [len(keys), T, Z]."""
    assert Z % 4 == 0
    nq = T * (Z // 4)
    q = np.arange(nq, dtype=np.uint64)
    one = np.ones(nq, dtype=np.uint64)
    zs, rads = [], []
    for k in keys:
        k = int(k) & P.MASK64
        words = P.philox4x32_10(q & P.M32, q >> P.S32, one * np.uint64(2 + int(timestep)), one * np.uint64(STRT), k & 0xFFFFFFFF, k >> 32)
        z, rad = P.normals_from_words(words)
        zs.append(z.reshape(T, Z))
        rads.append(rad.reshape(T, Z))
    return np.stack(zs), np.stack(rads)
