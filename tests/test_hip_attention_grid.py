"""dn_attention / dn_attention_backward over their whole accepted domain against oracle/attention_ref.py in float64.

Every arithmetic mode (f32, bf16, f16, x3 = DN_BF16X3), every padded head size, query counts on both sides of every tile edge
(16 queries per MFMA tile, 64 keys per LDS tile, 128 queries per workgroup), ragged key lengths incl. 1, 0 and "no mask",
cross-attention, peaked and moving softmaxes, dropout, the XCD workgroup remap at awkward grid sizes.  The reference is fed the
operands as the kernel sees them (rounded to the 2-byte type; plain fp32 for f32 and x3); errors are max-abs over the reference's
max-abs (`relerr`).

What the kernels must NOT do is checked too: every q / k / v / O / dO buffer has its own row stride and NaN in the columns behind
the last head (a fragment that reads past dim_head inside its padded template would carry it into the result); every output
(out, lse, dq, dk, dv, delta) has a row stride wider than heads * dim_head and two guard rows on either side, all filled with a NaN
bit pattern that must still be there afterwards, while every element in range must have been written (finite).

Bounds: the project's own for the same kernel and mode (forward f32 2e-5, bf16 2e-2, f16 3e-3; backward f32 1e-4, bf16 2e-2, with
dropout 2.5e-2; lse f32 1e-4, bf16 3e-2).  Those were set on N(0,1) scores; for T >= 1024, for the score-dynamics cases and for x3
(which has no operator bound of its own) the bound is max(project bound, 4 x the error the FORMAT alone costs), the latter
computed here on the CPU by attention_ref with the mode's roundings applied in float64 (attention_ref.mode_rounders) -- never
from what a kernel returns.  x3 is floored at the exact-fp32 bound: its accumulators are fp32.  DESIGN.md ("attention operator
grid") tabulates emulated error, bound and measured error of those cases."""
import functools
import math

import pytest
import torch

from attention_ref import attention_grads_stored_out, attention_ref, mode_rounders, round_to
from dropout_mask import dropout_keep_mask

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("f32", "bf16", "f16", "x3")
STORE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32}     # q / k / v / O / dO in memory
OUT_STORE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.bfloat16}  # x3: split rows
FILL = {torch.float32: (torch.int32, 0x7FC00BAD), torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01)}  # NaNs
FWD_TOL = {"f32": 2e-5, "bf16": 2e-2, "f16": 3e-3, "x3": 2e-5}
BWD_TOL = {"f32": 1e-4, "bf16": 2e-2, "x3": 1e-4}  # x3 backward = the exact-fp32 kernels with a split store (2^-16 per element)
LSE_TOL = {"f32": 1e-4, "bf16": 3e-2, "x3": 1e-4}


@pytest.fixture(scope="module")
def ops():
    from diffnorm_amd import _lib, ops, packing

    _lib.load()
    return ops, packing, _lib


def code(_lib, mode):
    return {"f32": _lib.DN_F32, "bf16": _lib.DN_BF16, "f16": _lib.DN_F16, "x3": _lib.DN_BF16X3}[mode]


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def seen(mode, t):
    """fp32 values as the kernel of `mode` sees them."""
    return t.float().to(STORE[mode]).float()


@functools.lru_cache(maxsize=None)
def seeded(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def wide(cols):
    return (cols + 31) // 32 * 32 + 32


def nan_padded(x2d, dt, ld):
    """[rows, cols] -> device [rows, ld] of dtype dt, NaN behind the last head."""
    buf = torch.full((x2d.shape[0], ld), float("nan"), dtype=dt)
    buf[:, :x2d.shape[1]] = x2d.to(dt)
    return buf.to(DEV)


class Guarded:
    """An output of `rows` x `cols` values with row stride wide(cols), two guard rows before and after, everything a NaN pattern."""

    def __init__(self, rows, cols, dt, split=False, ld=None):
        self.rows, self.cols, self.split, self.ld = rows, cols, split, ld or wide(cols)
        w = self.ld * (2 if split else 1)  # split rows: every 32 elements as 32 hi + 32 lo bf16 entries
        self.full = torch.empty(rows + 4, w, dtype=dt, device=DEV)
        self.itype, pat = FILL[dt]
        self.full.view(self.itype).fill_(pat)
        self.pat = pat
        self.t = self.full[2:2 + rows]
        e = torch.arange(w)
        self.valid = ((e // 64) * 32 + e % 32 < cols) if split else (e < cols)

    def values(self, packing=None):
        """Asserts guards intact and every value written; -> fp32 [rows, cols] on the host."""
        torch.cuda.synchronize()
        bits = self.full.view(self.itype).cpu()
        assert (bits[:2] == self.pat).all() and (bits[-2:] == self.pat).all(), "guard rows overwritten"
        assert (bits[2:-2][:, ~self.valid] == self.pat).all(), "columns behind heads * dim_head overwritten"
        body = self.t.cpu()
        assert torch.isfinite(body[:, self.valid].float()).all(), "an element in range was not written (or is not finite)"
        if self.split:
            body[:, ~self.valid] = 0
            return packing.unsplit_rows(body)[:, :self.cols]
        return body[:, :self.cols].float()


def lens_for(T):
    """T, T - 1, a value strictly inside a key tile, 1, 0."""
    inside = max(1, (T * 5) // 8)
    if inside % 64 == 0:
        inside -= 3
    return (T, max(T - 1, 0), inside, 1, 0)


REF_CACHE = {}


def reference(key, q, k, v, heads, lens, keep=None, p=0.0, grad=None):
    """(out, lse[, dq, dk, dv]) of attention_ref on exactly these operands, cached per `key` (shape, inputs as seen)."""
    key = key + (lens, p, None if keep is None else int(keep.sum()), tuple(q.shape), tuple(k.shape))  # what the caller's key must not forget
    if key not in REF_CACHE or (grad is not None and len(REF_CACHE[key]) == 2):
        lt = None if lens is None else torch.tensor(lens)
        if grad is None:
            REF_CACHE[key] = attention_ref(q, k, v, heads, lt, keep=keep, p=p)
        else:
            qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
            o, lse = attention_ref(qd, kd, vd, heads, lt, keep=keep, p=p)
            o.backward(grad.double())
            REF_CACHE[key] = (o.detach(), lse, qd.grad, kd.grad, vd.grad)
    return REF_CACHE[key]


def emulated(mode, key, q, k, v, heads, lens, keep=None, p=0.0):
    """(relerr of out, max abs lse difference) that the formats of `mode` alone cost on these operands (no kernel involved)."""
    ekey = ("emu", mode, lens, p) + key
    if ekey not in REF_CACHE:
        lt = None if lens is None else torch.tensor(lens)
        want, wl = reference(key, q, k, v, heads, lens, keep=keep, p=p)[:2]
        got, gl = attention_ref(q, k, v, heads, lt, keep=keep, p=p, rounders=mode_rounders(mode))
        REF_CACHE[ekey] = (relerr(got, want), (gl - wl).abs().max().item())
    return REF_CACHE[ekey]


def fwd_bound(mode, derive, key, q, k, v, heads, lens, keep=None, p=0.0):
    """-> (bound on out, bound on lse, emulated out error or None)."""
    if not (derive or mode == "x3"):
        return FWD_TOL[mode], LSE_TOL.get(mode), None
    e_out, e_lse = emulated(mode, key, q, k, v, heads, lens, keep=keep, p=p)
    return max(FWD_TOL[mode], 4 * e_out), max(LSE_TOL.get(mode, 0.0), 4 * e_lse), e_out


def run_forward(ops, mode, q, k, v, heads, dh, lens, Tk=0, want_lse=False, p=0.0, seed=0, layout="own strides"):
    """q [B, T, hd], k / v [B, Tk or T, hd] fp32 as seen -> (out fp32 [B, T, hd], lse fp32 [B, heads, T] or None), guards checked."""
    ops_, packing, _lib = ops
    B, T, hd = q.shape
    Tkv = k.shape[1]
    dt = STORE[mode]
    if layout == "own strides":  # three buffers, three row strides, NaN behind the last head
        qa, ldq = nan_padded(q.reshape(B * T, hd), dt, hd + 32), hd + 32
        ka, va = nan_padded(k.reshape(B * Tkv, hd), dt, hd + 40), nan_padded(v.reshape(B * Tkv, hd), dt, hd + 48)
        ldk, ldv = hd + 40, hd + 48
    else:  # the engine's cross-attention: dense q (ldq = hd), k and v the two column blocks of one [B * Tk, 2 hd] buffer
        qa, ldq = q.reshape(B * T, hd).to(dt).to(DEV), hd
        kv = torch.cat([k.reshape(B * Tkv, hd), v.reshape(B * Tkv, hd)], dim=1).to(dt).to(DEV)
        ka, va, ldk, ldv = kv, kv[:, hd:], 2 * hd, 2 * hd
    out = Guarded(B * T, hd, OUT_STORE[mode], split=mode == "x3")
    l32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    kw = dict(ldq=ldq, ldk=ldk, ldv=ldv, Tk=Tk, ldo=out.ld, dtype=code(_lib, mode))
    lse = None
    if want_lse or p > 0:
        lse = Guarded(1, B * heads * T, torch.float32)
        ops_.attention_fwd_lse(qa, ka, va, out.t, B, T, heads, dh, l32, dropout_p=p, seed=seed, lse=lse.t, **kw)
    else:
        ops_.attention(qa, ka, va, out.t, B, T, heads, dh, l32, **kw)
    got = out.values(packing).view(B, T, hd)
    return got, (lse.values().view(B, heads, T) if lse is not None else None)


def refused(_lib, call):
    """The dispatcher refuses: DN_EINVAL (-1) with a message."""
    with pytest.raises(_lib.DiffNormHipError) as e:
        call()
    assert "(-1)" in str(e.value), str(e.value)
    msg = _lib.load().dn_last_error()
    assert msg and len(msg.decode()) > 0


def assertless(e, tol):
    assert e < tol, (e, tol)


def fwd_accepts(mode, dh):
    if mode in ("f32", "x3"):
        return dh <= 96
    return dh % 8 == 0


# ------------------------------------------------------------------------------------------------------------ forward grid
# dim_head -> query counts.  Every head size meets every residue class of T in every mode: below 16 (1 or 15); 127 = 16k-1,
# 64k-1, 128k-1; 128 = 16k, 64k, 128k; 129 = 16k+1, 64k+1, 128k+1; the remaining lengths go round the head sizes.
FWD_T = {
    4: (1, 127, 128, 129, 16, 193),
    8: (15, 127, 128, 129, 17, 257),
    16: (1, 127, 128, 129, 63, 515),
    24: (15, 127, 128, 129, 64, 1024),
    32: (1, 127, 128, 129, 65, 192),
    48: (15, 127, 128, 129, 16, 515),
    64: (1, 127, 128, 129, 17, 193, 1024),
    80: (15, 127, 128, 129, 63, 257),
    96: (1, 127, 128, 129, 64, 192, 515),
    112: (15, 127, 128, 129, 65, 1024),
    128: (1, 127, 128, 129, 16, 193, 257),
}
FWD_CASES = [(mode, dh, T) for mode in MODES for dh, Ts in FWD_T.items() for T in Ts]


@pytest.mark.parametrize("mode,dh,T", FWD_CASES)
def test_forward_grid(ops, mode, dh, T):
    """Five sequences with key lengths T, T - 1, inside a key tile, 1, 0 in one call; then two of them without a mask."""
    _lib = ops[2]
    heads, B = 2, 5
    hd = heads * dh
    q, k, v = (seen(mode, seeded((B, T, hd), 100 + i)) for i in range(3))
    lens = lens_for(T)
    if not fwd_accepts(mode, dh):
        return refused(_lib, lambda: run_forward(ops, mode, q, k, v, heads, dh, lens))
    lse_mode = mode != "f16"
    opclass = mode if mode in ("bf16", "f16") else "fp32"
    for name, n, ll in (("lens", B, lens), ("nomask", 2, None)):
        key = (name, opclass, dh, T)
        want, want_lse = reference(key, q[:n], k[:n], v[:n], heads, ll)
        tol, tol_lse, emu = fwd_bound(mode, T >= 1024, key, q[:n], k[:n], v[:n], heads, ll)
        got, lse = run_forward(ops, mode, q[:n], k[:n], v[:n], heads, dh, ll, want_lse=lse_mode and name == "lens")
        e = relerr(got, want)
        print(f"GRID fwd {mode} dh={dh} T={T} {name}: emulated {emu} bound {tol:.3e} measured {e:.3e}")
        assert e < tol, (name, e, tol)
        if lse is not None:  # incl. the all-masked sequence: log2(T)
            el = (lse.double() - want_lse).abs().max().item()
            assert el < tol_lse, (name, el, tol_lse)


@pytest.mark.parametrize("mode", MODES)
def test_forward_long(ops, mode):
    """32 key tiles: T = 2048, one sequence without a mask and one ending inside the last tile but one."""
    heads, dh, T = 2, 64, 2048
    opclass = mode if mode in ("bf16", "f16") else "fp32"
    q, k, v = (seen(mode, seeded((1, T, heads * dh), 200 + i)) for i in range(3))
    for ll in (None, (1931,)):
        key = ("long", opclass, ll)
        want, want_lse = reference(key, q, k, v, heads, ll)
        tol, tol_lse, emu = fwd_bound(mode, True, key, q, k, v, heads, ll)
        got, lse = run_forward(ops, mode, q, k, v, heads, dh, ll, want_lse=mode != "f16")
        e = relerr(got, want)
        print(f"GRID long {mode} T={T} lens={ll}: emulated {emu:.3e} bound {tol:.3e} measured {e:.3e}")
        assert e < tol, (e, tol)
        if lse is not None:
            assert (lse.double() - want_lse).abs().max().item() < tol_lse


@pytest.mark.parametrize("mode", ("f16",))
def test_f16_refuses_training_arguments(ops, mode):
    ops_, packing, _lib = ops
    q, k, v = (seen(mode, seeded((2, 65, 64), 300 + i)) for i in range(3))
    refused(_lib, lambda: run_forward(ops, mode, q, k, v, 2, 32, None, want_lse=True))
    refused(_lib, lambda: run_forward(ops, mode, q, k, v, 2, 32, None, p=0.1, seed=5))
    x = q.view(130, 64).to(DEV, torch.float16)
    lse = torch.zeros(2, 2, 65, device=DEV)
    refused(_lib, lambda: ops_.attention_backward(x, x, x, x, x, lse, 2, 65, 2, 32, None))


# ------------------------------------------------------------------------------------------------------------ cross-attention
CROSS_SHAPES = ((130, 1), (130, 17), (64, 64), (40, 200), (200, 63), (200, 65), (257, 129), (515, 32))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dh", (32, 48, 64, 96))
@pytest.mark.parametrize("T,Tk", CROSS_SHAPES)
def test_cross_attention(ops, mode, dh, T, Tk):
    """Tk set explicitly (also where it equals T).  Without key lengths (two sequences, own strides) and, in the engine's layout
    (ldq = hd, k / v two column blocks of one buffer), with key lengths Tk, an inside value, 1, 0 and one above Tk (= Tk)."""
    heads, B = 2, 5
    hd = heads * dh
    opclass = mode if mode in ("bf16", "f16") else "fp32"
    q = seen(mode, seeded((B, T, hd), 400))
    k, v = (seen(mode, seeded((B, Tk, hd), 401 + i)) for i in range(2))
    lens = (Tk, max(1, Tk * 5 // 8), 1, 0, Tk + 9)
    for name, n, ll, layout in (("nomask", 2, None, "own strides"), ("lens", B, lens, "engine")):
        key = ("cross", name, opclass, dh, T, Tk)
        want, _ = reference(key, q[:n], k[:n], v[:n], heads, ll)
        tol, _, emu = fwd_bound(mode, False, key, q[:n], k[:n], v[:n], heads, ll)
        got, _ = run_forward(ops, mode, q[:n], k[:n], v[:n], heads, dh, ll, Tk=Tk, layout=layout)
        e = relerr(got, want)
        print(f"GRID cross {mode} dh={dh} T={T} Tk={Tk} {name}: emulated {emu} bound {tol:.3e} measured {e:.3e}")
        assert e < tol, (name, e, tol)
    # a key length above Tk is Tk: bit-equal to the same sequence run with length Tk
    assert torch.equal(got[4], run_forward(ops, mode, q[4:5], k[4:5], v[4:5], heads, dh, (Tk,), Tk=Tk, layout="engine")[0][0])


@pytest.mark.parametrize("mode", ("f32", "bf16", "x3"))
def test_lse_with_cross_attention_is_refused(ops, mode):
    q, k, v = seen(mode, seeded((2, 40, 64), 500)), seen(mode, seeded((2, 17, 64), 501)), seen(mode, seeded((2, 17, 64), 502))
    refused(ops[2], lambda: run_forward(ops, mode, q, k, v, 2, 32, None, Tk=17, want_lse=True))


# ------------------------------------------------------------------------------------------------------------ score dynamics
def dynamics_inputs(kind, B, T, heads, dh):
    """Natural-log scores spanning about +-20 through two planted coordinates of every head on top of small noise.
    'moving': a third of the queries see scores that rise from key tile to key tile (the running maximum and the rescale factor change
    at every key tile, maximum in the last tile), a third see them fall (maximum in the first tile), a third see a flat
    landscape with the maximum planted in the last key tile.  'equal': q = 0.  'dominant': one key outweighs all others."""
    hd = heads * dh
    q, k, v = seeded((B, T, hd), 600, 0.1).clone(), seeded((B, T, hd), 601).clone(), seeded((B, T, hd), 602).clone()
    amp = 20.0 * dh ** 0.5
    ramp = -1.0 + 2.0 * (torch.arange(T) // 64).float() / ((T - 1) // 64)  # one step per 64-key tile
    grp = torch.arange(T) % 3
    for h in range(heads):
        c0, c1 = h * dh, h * dh + 1
        if kind == "moving":
            k[:, :, c0] = ramp
            k[:, :, c1] = 0.0
            k[:, (T - 1) // 64 * 64:, c1] = 1.0
            q[:, :, c0] = torch.where(grp == 0, amp, torch.where(grp == 1, -amp, 0.0))
            q[:, :, c1] = torch.where(grp == 2, amp, 0.0)
        elif kind == "dominant":
            k[:, :, c0] = 0.0
            k[:, (T * 2) // 3, c0] = 1.0
            q[:, :, c0] = amp
    if kind == "equal":
        q.zero_()
    return q, k, v


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,T", [("moving", 515), ("moving", 2048), ("equal", 515), ("dominant", 515)])
def test_score_dynamics(ops, mode, kind, T):
    heads, dh = 2, 64
    B = 1 if T > 1024 else 2
    opclass = mode if mode in ("bf16", "f16") else "fp32"
    q, k, v = (seen(mode, t) for t in dynamics_inputs(kind, B, T, heads, dh))
    lens = None if B == 1 else (T, T - 37)
    key = ("dyn", kind, opclass, T)
    want, want_lse = reference(key, q, k, v, heads, lens)
    tol, tol_lse, emu = fwd_bound(mode, True, key, q, k, v, heads, lens)
    got, lse = run_forward(ops, mode, q, k, v, heads, dh, lens, want_lse=mode != "f16")
    e = relerr(got, want)
    el = (lse.double() - want_lse).abs().max().item() if lse is not None else float("nan")
    print(f"GRID dyn {mode} {kind} T={T}: emulated {emu:.3e} bound {tol:.3e} measured {e:.3e} | lse bound {tol_lse} measured {el:.3e}")
    assert e < tol, (e, tol)
    if lse is not None:
        assert el < tol_lse, (el, tol_lse)
    if kind == "moving":  # the cases are what they claim: the row maximum sits in the last key tile, the first, and moves
        s = torch.einsum("id,jd->ij", q[0, :, :dh].double(), k[0, :, :dh].double()) * dh ** -0.5
        first, last = s[:, :64].max(dim=1).values, s[:, (T - 1) // 64 * 64:].max(dim=1).values
        top = s.max(dim=1).values
        assert (last[0::3] == top[0::3]).all() and (first[1::3] == top[1::3]).all() and (last[2::3] == top[2::3]).all()
        assert 15 < top.max().item() < 25 and s.min().item() < -15


# ------------------------------------------------------------------------------------------------------------ backward
def bwd_accepts(mode, dh):
    return dh <= 96 if mode in ("f32", "x3") else dh % 8 == 0


def run_backward(ops, mode, q, k, v, do, heads, dh, lens, p=0.0, seed=0):
    """-> out, lse, dq, dk, dv, delta (fp32, host): forward with lse, then dn_attention_backward.  q / k / v / out / dO / dq / dk / dv are
    eight separate tensors; the six of the q / k / v / dq / dk / dv have six different row strides."""
    ops_, packing, _lib = ops
    B, T, hd = q.shape
    dt, split = STORE[mode], mode == "x3"
    flat = lambda t: t.reshape(B * T, hd)
    qa, ka, va = nan_padded(flat(q), dt, hd + 32), nan_padded(flat(k), dt, hd + 40), nan_padded(flat(v), dt, hd + 48)
    l32 = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    # the forward's O is the backward's operand: plain storage type here (x3: fp32, as the training engine keeps it)
    out = Guarded(B * T, hd, dt)
    lse = Guarded(1, B * heads * T, torch.float32)
    fmode = "f32" if split else mode
    ops_.attention_fwd_lse(qa, ka, va, out.t, B, T, heads, dh, l32, ldq=hd + 32, ldk=hd + 40, ldv=hd + 48, ldo=out.ld, dropout_p=p, seed=seed,
                           lse=lse.t, dtype=code(_lib, fmode))
    o_host, lse_host = out.values(), lse.values()
    oa = nan_padded(o_host, dt, hd + 56)
    doa = nan_padded(flat(do), dt, hd + 64)
    g = [Guarded(B * T, hd, OUT_STORE[mode], split=split, ld=wide(hd) + extra) for extra in (0, 32, 64)]
    delta = Guarded(1, B * heads * T, torch.float32)

    def call():
        for x in g:
            x.full.view(x.itype).fill_(x.pat)
        ops_.attention_backward(qa, ka, va, oa, doa, lse.t, B, T, heads, dh, l32, dropout_p=p, seed=seed, ldq=hd + 32,
                                ldk=hd + 40, ldv=hd + 48, ldo=hd + 56, lddo=hd + 64, dtype=code(_lib, mode), dq=g[0].t, dk=g[1].t,
                                dv=g[2].t, lddq=g[0].ld, lddk=g[1].ld, lddv=g[2].ld, delta=delta.t)
        return [x.t.view(x.itype).clone() for x in g]  # bits: the columns outside the range hold the NaN pattern

    return call, g, delta, o_host.view(B, T, hd), lse_host.view(B, heads, T)


def grads_of(g, packing, hd):
    return [x.values(packing) for x in g]


# dim_head -> sequence lengths (the same residue classes as the forward; 1024 once per padded template)
BWD_T = {
    4: (1, 63, 129),
    8: (17, 64, 257),
    16: (1, 65, 127, 1024),
    24: (17, 63, 129),
    48: (1, 64, 127, 257),
    64: (17, 65, 129, 1024),
    80: (1, 63, 127, 257),
    96: (17, 64, 129, 1024),
    128: (1, 65, 127, 257, 1024),
}
BWD_CASES = [(mode, dh, T) for mode in ("f32", "bf16", "x3") for dh, Ts in BWD_T.items() for T in Ts]


@pytest.mark.parametrize("mode,dh,T", BWD_CASES)
def test_backward_grid(ops, mode, dh, T):
    ops_, packing, _lib = ops
    heads, B = 2, 5
    hd = heads * dh
    sm = "f32" if mode == "x3" else mode
    q, k, v, do = (seen(sm, seeded((B, T, hd), 700 + i)) for i in range(4))
    lens = lens_for(T)
    if not bwd_accepts(mode, dh):
        if sm == "bf16":  # dim_head * 2 bytes is not a multiple of 16: forward and backward each refuse
            refused(_lib, lambda: run_backward(ops, mode, q, k, v, do, heads, dh, lens))
        x, lse = q.view(B * T, hd).to(DEV, STORE[sm]), torch.zeros(B, heads, T, device=DEV)  # f32 / x3 at 128 dims: no instantiation
        gq = [torch.zeros(B * T, wide(hd) * (2 if mode == "x3" else 1), device=DEV, dtype=OUT_STORE[mode]) for _ in range(3)]
        return refused(_lib, lambda: ops_.attention_backward(x, x, x, x, x, lse, B, T, heads, dh, None, dtype=code(_lib, mode), dq=gq[0],
                                                             dk=gq[1], dv=gq[2], lddq=wide(hd), lddk=wide(hd), lddv=wide(hd)))
    want_o, want_lse, wq, wk, wv = reference(("bwd", sm, dh, T), q, k, v, heads, lens, grad=do)
    call, g, delta, got_o, got_lse = run_backward(ops, mode, q, k, v, do, heads, dh, lens)
    first = call()
    dq, dk, dv = grads_of(g, packing, hd)
    assert relerr(got_o, want_o) < FWD_TOL[sm]
    assert (got_lse.double() - want_lse).abs().max().item() < LSE_TOL[sm]
    # delta = sum_d dO * O of the O the backward was given
    want_delta = (seen(sm, got_o).double() * do.double()).view(B, T, heads, dh).sum(-1).transpose(1, 2)
    assert relerr(delta.values().view(B, heads, T), want_delta) < BWD_TOL["f32"]  # fp32 arithmetic on stored values in every mode: the backward's fp32 bound
    live = torch.tensor([n > 0 for n in lens])
    for name, got, want in (("dq", dq, wq), ("dk", dk, wk), ("dv", dv, wv)):
        got = got.view(B, T, hd)
        assert torch.isfinite(got[~live]).all(), name  # the all-masked sequence: finite
        # T = 1: one key, softmax = 1, dq = dk = 0 exactly -- no scale of their own: measured against the scale of dv of the same call
        e = relerr(got[live], want[live]) if T > 1 else (got[live].double() - want[live]).abs().max().item() / wv[live].abs().max().item()
        print(f"GRID bwd {mode} dh={dh} T={T} {name}: bound {BWD_TOL[mode]:.1e} measured {e:.3e}")
        assert e < BWD_TOL[mode], (name, e)
    if mode == "x3":  # hi + lo of the split store = the fp32 result of the same kernels
        c32, g32, _, _, _ = run_backward(ops, "f32", q, k, v, do, heads, dh, lens)
        c32()
        for a, b in zip((dq, dk, dv), grads_of(g32, packing, hd)):
            assert relerr(a, b) < 2.0 ** -15
    if T == max(BWD_T[dh]):  # no atomics: bit-reproducible
        second = call()
        assert all(torch.equal(a, b) for a, b in zip(first, second))


# ------------------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("mode", ("f32", "bf16", "x3"))
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("dh,T", [(48, 65), (64, 129), (96, 515), (64, 515), (48, 129)])
def test_dropout(ops, mode, p, dh, T):
    """Forward in f32, bf16 and x3 (attn_x3_kernel<.., true> up to 64 dims), lse bit-equal with and without; backward in f32 / bf16."""
    ops_, packing, _lib = ops
    heads, B = 2, 3
    hd = heads * dh
    seed = 0x0BADC0DE12345678 + 977 * T + dh
    sm = "f32" if mode == "x3" else mode
    q, k, v, do = (seen(sm, seeded((B, T, hd), 800 + i)) for i in range(4))
    lens = (T, (T * 5) // 8, 1)
    keep = dropout_keep_mask(B, heads, T, T, p, seed)
    key = ("drop", sm, dh, T, p)
    want_o, want_lse, wq, wk, wv = reference(key, q, k, v, heads, lens, keep=keep, p=p, grad=do)
    tol, tol_lse, emu = fwd_bound(mode, False, key, q, k, v, heads, lens, keep=keep, p=p)
    got, lse = run_forward(ops, mode, q, k, v, heads, dh, lens, p=p, seed=seed)
    got0, lse0 = run_forward(ops, mode, q, k, v, heads, dh, lens, want_lse=True)
    e = relerr(got, want_o)
    print(f"GRID drop {mode} dh={dh} T={T} p={p}: emulated {emu} bound {tol:.3e} measured {e:.3e}")
    assert e < tol, (e, tol)
    assert torch.equal(lse, lse0) and not torch.equal(got, got0)
    assert (lse.double() - want_lse).abs().max().item() < tol_lse
    if mode == "x3":
        return
    call, g, delta, got_o, _ = run_backward(ops, mode, q, k, v, do, heads, dh, lens, p=p, seed=seed)
    call()
    # Every sequence with more than one key, and dv everywhere: float64 autograd at the project's bound.  dq / dk of the ONE-KEY
    # sequence are exactly zero in autograd (P = 1, dS cancels), but bf16 stores O = v / (1 - p) rounded and the backward takes
    # delta = sum dO * O from it, so the cancellation is off by 2^-9 per query and sums over the T queries into dk (exact only when
    # 1 / (1 - p) is a power of two).  There the operator is held, at the same project bound, to what its formulas give in float64
    # for the O it was handed (attention_grads_stored_out(out=...)); the distance to autograd is printed next to what the rounding
    # of O alone accounts for (emulated, no kernel involved), for DESIGN.md.
    one = torch.tensor([n == 1 for n in lens])
    tol_b = 1e-4 if mode == "f32" else 2.5e-2
    scale = lambda want: max(want.abs().max().item(), 1e-30)
    lt = torch.tensor(lens)
    given = attention_grads_stored_out(q, k, v, do, heads, lt, keep, p, out=got_o)
    emu_g = attention_grads_stored_out(q, k, v, do, heads, lt, keep, p, r_out=round_to(STORE[mode]))
    for name, gg, want, giv, emu in zip(("dq", "dk", "dv"), grads_of(g, packing, hd), (wq, wk, wv), given, emu_g):
        gg = gg.view(B, T, hd).double()
        many = (gg[~one] - want[~one]).abs().max().item() / scale(want)
        assert many < tol_b, (name, "more than one key", many, tol_b)
        auto = (gg[one] - want[one]).abs().max().item() / scale(want)
        held = (gg[one] - giv[one]).abs().max().item() / scale(want)
        cost = (emu[one] - want[one]).abs().max().item() / scale(want)
        print(f"GRID dropbwd {mode} dh={dh} T={T} p={p} {name}: bound {tol_b:.1e} others {many:.3e} one-key vs its stored O {held:.3e} | "
              f"one-key vs autograd: emulated {cost:.3e} measured {auto:.3e}")
        assert (auto if name == "dv" else held) < tol_b, (name, "one key", auto, held, tol_b)


# ------------------------------------------------------------------------------------------------------------ grid remap
# workgroups = B * heads * ceil(T / 128)
REMAP = {1: (1, 1, 100), 3: (1, 3, 128), 7: (7, 1, 77), 8: (2, 2, 256), 9: (3, 3, 127), 45: (3, 5, 300), 105: (3, 5, 800)}


@pytest.mark.parametrize("waves8", (0, 1))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nwg", sorted(REMAP))
def test_xcd_block_remap_covers_every_workgroup(ops, hip_option, waves8, mode, nwg):
    """dn_xcd_block_map must be a bijection for any grid size: forward, dK/dV and dQ kernels on NaN-filled outputs, every row
    written and equal to the reference; both wave layouts."""
    ops_, packing, _lib = ops
    B, heads, T = REMAP[nwg]
    assert B * heads * ((T + 127) // 128) == nwg
    dh = 16
    hd = heads * dh
    hip_option("attn_waves8", waves8)
    sm = "f32" if mode == "x3" else mode
    if mode == "f16":  # inference mode: forward only
        q, k, v = (seen(mode, seeded((B, T, hd), 900 + i)) for i in range(3))
        lens = tuple(max(1, T - 17 * b) for b in range(B))
        want_o, _ = reference(("remap", mode, nwg), q, k, v, heads, lens)
        return assertless(relerr(run_forward(ops, mode, q, k, v, heads, dh, lens)[0], want_o), FWD_TOL[mode])
    q, k, v, do = (seen(sm, seeded((B, T, hd), 900 + i)) for i in range(4))
    lens = tuple(max(1, T - 17 * b) for b in range(B))
    want_o, want_lse, wq, wk, wv = reference(("remap", sm, nwg), q, k, v, heads, lens, grad=do)
    tol, _, _ = fwd_bound(mode, False, ("remap", sm, nwg), q, k, v, heads, lens)
    got, _ = run_forward(ops, mode, q, k, v, heads, dh, lens)
    assert relerr(got, want_o) < tol
    call, g, delta, _, _ = run_backward(ops, mode, q, k, v, do, heads, dh, lens)
    call()
    for name, gg, want in zip(("dq", "dk", "dv"), grads_of(g, packing, hd), (wq, wk, wv)):
        assert relerr(gg.view(B, T, hd), want) < BWD_TOL[mode], name
    delta.values()


def test_x3_split_store_is_the_fp32_result(ops):
    """Heads of 80 / 96 dims in DN_BF16X3 run the exact-fp32 kernel with a split store: hi + lo equals the DN_F32 output to 2^-15."""
    for dh, T in ((80, 129), (96, 200)):
        q, k, v = (seeded((2, T, 2 * dh), 950 + i) for i in range(3))
        a, _ = run_forward(ops, "x3", q, k, v, 2, dh, (T, T // 3))
        b, _ = run_forward(ops, "f32", q, k, v, 2, dh, (T, T // 3))
        assert relerr(a, b) < 2.0 ** -15
