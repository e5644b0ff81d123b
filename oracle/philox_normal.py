"""TEST INFRASTRUCTURE ONLY -- never imported by the product path (diffnorm_amd/).  NumPy only.

Host restatement of the device normal generators of diffnorm_amd/csrc/pointwise.hip: Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11; the Random123 known-answer vectors pin `philox4x32_10`) followed by Box-Muller on two 24-bit
uniforms per pair.  Four kernels draw with it:

* randn_kernel (dn_randn):           counter (ctr low, ctr high, 0, 0), ctr = (offset + quad) mod 2^64;   key (seed low, seed high)
* ddpm_step_kernel (dn_ddpm_loop):   counter (quad low, quad high, timestep t, TAG), quad within the LAUNCH; key (seed low, seed high),
                                     a split chain's second half-batch under seed ^ SPLIT_KEY with its quads restarting at 0
* ddim_sched_step_kernel (dn_ddim_sched_loop, eta > 0) and guided_sched_step_kernel (dn_guided_ddim_loop, eta > 0):
                                     counter (quad low, quad high, step index i, TAG), quad of the WHOLE B-row batch -- a split
                                     chain's halves continue one stream under one key; no draw is applied where steps[i] == 0

A quad is four consecutive floats; the four output words of one Philox call become its four normals.

Uniform map: u = (float32(w >> 8) + 0.5f) * 2^-24 in float32.  For the 24-bit value 2^24 - 1 the sum ties to even, 2^24, so u lies
in (0, 1]: u1 = 1 gives radius 0 (a finite 0 draw), u1 = 2^-25 the largest radius sqrt(50 ln 2) = 5.887.  The angle is the float32
product 6.28318530717958647692f * u2.  Both are exactly reproducible; log, sqrt, sin and cos are evaluated here in float64, so a
device draw differs from this restatement by the error of the device's float32 logf / sqrtf / sincosf only, a few units of
2^-23 max(radius, 1)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MUL0, MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
KEY0, KEY1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)  # the key schedule (Weyl constants: golden ratio, sqrt 3 - 1)
TAG = 0x44504D50  # "DPMP": fourth counter word of the update kernels, a stream apart from dn_randn's
SPLIT_KEY = 0x9E3779B97F4A7C15  # dn_ddpm_loop: key of the second half-batch = seed ^ SPLIT_KEY
MASK64 = (1 << 64) - 1


def _u64(v):
    return np.asarray(v, dtype=np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32 with ten rounds, vectorised over uint64 arrays holding 32-bit words.  -> four uint64 arrays of 32-bit output
    words."""
    c0, c1, c2, c3, k0, k1 = (_u64(v) for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL1 * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> S32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + KEY0) & M32, (k1 + KEY1) & M32
    return c0, c1, c2, c3


def uniform_from_word(w):
    """The kernels' 24-bit uniform in (0, 1], float32 arithmetic throughout."""
    return ((_u64(w) >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def normals_from_words(words):
    """Box-Muller as the kernels spell it, on the four output words of one call each: -> (normals float64 [..., 4] =
    [rad0 cos0, rad0 sin0, rad1 cos1, rad1 sin1], rad float64 [..., 4] = the radius each element was scaled by)."""
    u = [uniform_from_word(w) for w in words]
    out, rads = [], []
    for h in range(2):
        u1, u2 = u[2 * h], u[2 * h + 1]
        ang = (np.float32(6.28318530717958647692) * u2).astype(np.float32).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        out += [rad * np.cos(ang), rad * np.sin(ang)]
        rads += [rad, rad]
    return np.stack(out, axis=-1), np.stack(rads, axis=-1)


def _key(seed):
    seed = int(seed) & MASK64
    return seed & 0xFFFFFFFF, seed >> 32


def _quads(first, n_quads):
    """(first + 0 .. n_quads-1) mod 2^64 as (low, high) 32-bit words, for any Python int `first`."""
    first = int(first) & MASK64
    with np.errstate(over="ignore"):
        q = np.uint64(first) + np.arange(n_quads, dtype=np.uint64)  # uint64 addition wraps modulo 2^64
    return q & M32, q >> S32


def randn(n, seed, offset=0):
    """dn_randn(out[n], seed, offset): -> (normals float64 [n], rad float64 [n])."""
    nq = (int(n) + 3) // 4
    lo, hi = _quads(offset, nq)
    zero = np.zeros(nq, dtype=np.uint64)
    z, rad = normals_from_words(philox4x32_10(lo, hi, zero, zero, *_key(seed)))
    return z.reshape(-1)[:n], rad.reshape(-1)[:n]


def step_noise(n_quads, seed, ctr_hi, q0=0):
    """The update kernels' draw for quads q0 .. q0 + n_quads - 1 under third counter word `ctr_hi`:
    -> (normals float64 [4 n_quads], rad float64 [4 n_quads])."""
    lo, hi = _quads(q0, int(n_quads))
    full = np.ones(int(n_quads), dtype=np.uint64)
    z, rad = normals_from_words(philox4x32_10(lo, hi, full * np.uint64(int(ctr_hi) & 0xFFFFFFFF), full * np.uint64(TAG), *_key(seed)))
    return z.reshape(-1), rad.reshape(-1)


def ddpm_loop_noise(shape, seed, t, split=False):
    """dn_ddpm_loop's draw at timestep `t` for x of `shape` = (B, T, z), z a multiple of 4: ctr_hi = t, quad within the launch.
    split (and B >= 2): rows [0, B // 2) under `seed`, rows [B // 2, B) under seed ^ SPLIT_KEY with the quads restarting at 0.
    -> (normals, rad) float64 of `shape`."""
    B, T, z = shape
    assert z % 4 == 0
    row = T * z // 4
    if not (split and B >= 2):
        zz, rad = step_noise(B * row, seed, t)
    else:
        B0 = B // 2
        a, b = step_noise(B0 * row, seed, t), step_noise((B - B0) * row, int(seed) ^ SPLIT_KEY, t)
        zz, rad = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    return zz.reshape(shape), rad.reshape(shape)


def sched_loop_noise(shape, seed, i, step=1):
    """dn_ddim_sched_loop's and dn_guided_ddim_loop's draw at step index `i` (eta > 0) for x of `shape` = (B, T, z), z a multiple of
    4: ctr_hi = i, quad of the whole batch -- split or not, guided or not.  `step` = steps[i]: at timestep 0 the kernels apply no
    draw, which an injected row of zeros restates.  -> (normals, rad) float64 of `shape`."""
    B, T, z = shape
    assert z % 4 == 0
    zz, rad = step_noise(B * T * z // 4, seed, i)
    if step == 0:
        zz = np.zeros_like(zz)
    return zz.reshape(shape), rad.reshape(shape)
