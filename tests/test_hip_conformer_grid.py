"""dn_rel_attention and dn_glu_dwconv at the places tests/test_hip_conformer.py leaves out: head width 32 (there, one more value of
its dk list, and here through the engine), 1 / 3 / 8 heads, key lengths on a tile edge with tiles behind them, finite garbage behind
a length, strided operands through the C ABI with a sentinel around a strided `out`, a position table poisoned outside the offsets a
batch has, a running maximum that rises (falls) on every key tile; the depthwise kernel at its frame-tile edges, with k = 1 and
k = 63, saturated gates and a sentinel around `out`.  Bars are test_hip_conformer's; "same bits" cases use torch.equal."""
import ctypes as C
import functools
import types

import pytest
import torch

import conformer_ref as R
from test_hip_conformer import (DEV, ENGINE_TOL, FWD_TOL, STORE, UNIT, _attn_case, _attn_ref, _glu_dwconv_bound, _glu_dwconv_ref, _randn,
                                _rt)

pytestmark = pytest.mark.gpu

MODES = ["f32", "x3", "f16", "bf16"]
TK = 64  # keys per tile of rel_attn_kernel
SENTINEL = -777.0


def _dev(t, mode):
    return t.to(STORE[mode]).to(DEV)


def _run(mode, q, k, v, pos, u, vb, lens, H, Tmax):
    from diffnorm_amd import ops

    return ops.rel_attention(*(_dev(t, mode) for t in (q, k, v, pos)), u.to(DEV), vb.to(DEV), lens.to(DEV), H, Tmax - 1, x3=mode == "x3")


@functools.lru_cache(maxsize=None)
def _want(mode, case, *args):
    """(float64 restatement on the operands the device holds, its max, the bar, the format's own cost) of case(*args), one of the
    cached case builders below -- once per mode and case."""
    q, k, v, pos, u, vb, lens, H, Tmax = case(*args)
    ins = [_rt(t, mode) for t in (q, k, v, pos)]
    want = _attn_ref(*ins, u.double(), vb.double(), lens, H, Tmax)
    scale = want.abs().max().item()
    bound, emu = FWD_TOL[mode], None
    if mode in UNIT:
        emu = (_attn_ref(*ins, u.double(), vb.double(), lens, H, Tmax, rnd=lambda t: _rt(t.float(), mode)) - want).abs().max().item() / scale
        bound = max(bound, 4 * emu)
    return want, scale, bound, emu


def _check_parity(mode, label, case, *args):
    """The rule of test_rel_attention_matches_float64 on every query row of case(*args)."""
    want, scale, bound, emu = _want(mode, case, *args)
    got = _run(mode, *case(*args))
    err = (got.double().cpu() - want).abs().max().item() / scale
    print(f"rel_attention {label} {mode}: emulated {emu if emu is None else f'{emu:.3e}'} bound {bound:.3e} measured {err:.3e}")
    assert torch.isfinite(got).all() and err < bound


# ---- 2. heads ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _heads_case(H):
    """dk = 16, T = 70, B = 2 (lengths 70 and 45); head h's bias_u row is offset by +h and its bias_v row by -h."""
    dk, T, B, Tmax = 16, 70, 2, 70 + 37
    s = 7000 + H
    q, k, v = (_randn(s + i, B, T, H * dk) for i in range(3))
    pos = _randn(s + 3, 2 * Tmax - 1, H * dk)
    off = torch.arange(H, dtype=torch.float32)[:, None]
    u, vb = 0.5 * _randn(s + 4, H, dk) + off, 0.5 * _randn(s + 5, H, dk) - off
    return q, k, v, pos, u, vb, torch.tensor([T, 45]), H, Tmax


def head_roll_sensitivity(H, mode):
    """No device needed.  How far the float64 restatement moves, relative to the output's max, when every head is given the next
    head's bias rows: what a kernel that indexed the biases with the wrong head would produce."""
    q, k, v, pos, u, vb, lens, _, Tmax = _heads_case(H)
    want, scale, _, _ = _want(mode, _heads_case, H)
    ins = [_rt(t, mode) for t in (q, k, v, pos)]
    rolled = _attn_ref(*ins, u.roll(1, 0).double(), vb.roll(1, 0).double(), lens, H, Tmax)
    return (rolled - want).abs().max().item() / scale


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H", [1, 3, 8])
def test_rel_attention_heads(mode, H):
    """One head, an odd head count and the recipe's 8: hc = h * dk indexes q, k, v, pos, both biases and out.  With more than one head
    the case is first shown (on the CPU) to tell the heads apart: the restatement with the bias rows rolled by one head differs from
    the true one by more than 100 x the bar -- capped at 1.0, the whole of the output's scale: two softmax averages of the same V
    cannot be told to differ by the 2 .. 4 x their own maximum that 100 x the bf16 bar asks."""
    bound = _want(mode, _heads_case, H)[2]
    if H > 1:
        sens = head_roll_sensitivity(H, mode)
        print(f"rel_attention heads H={H} {mode}: rolled biases move the restatement by {sens:.3e} (100 x bar {100 * bound:.3e})")
        assert sens > min(100 * bound, 1.0)
    _check_parity(mode, f"heads H={H}", _heads_case, H)


# ---- 3. / 4. lengths on tile edges, garbage behind a length ------------------------------------------------------------------------
EDGE_LENS = {"a": (63, 64, 65, 200), "b": (127, 128, 129, 1)}


@functools.lru_cache(maxsize=None)
def _edge_case(dk, which, fill="random"):
    """T = 200, H = 2, four sequences whose lengths sit on and beside the edges of the 64-key tiles.  fill: what the k and v rows
    behind a length hold -- "random" (as q), "zero", or "garbage" (+-1e4, the sign alternating along rows and columns)."""
    H, B, T, Tmax = 2, 4, 200, 237
    s = 9000 + dk + (0 if which == "a" else 50)
    q, k, v = (_randn(s + i, B, T, H * dk) for i in range(3))
    pos = _randn(s + 3, 2 * Tmax - 1, H * dk)
    u, vb = 0.5 * _randn(s + 4, H, dk), 0.5 * _randn(s + 5, H, dk)
    lens = torch.tensor(EDGE_LENS[which])
    if fill != "random":
        behind = (torch.arange(T)[None, :] >= lens[:, None])[:, :, None]
        sign = 1.0 - 2.0 * ((torch.arange(T)[:, None] + torch.arange(H * dk)[None, :]) % 2).float()
        kj, vj = ((1e4 * sign)[None], (-1e4 * sign)[None]) if fill == "garbage" else (torch.zeros(1, T, H * dk),) * 2
        k, v = torch.where(behind, kj, k), torch.where(behind, vj, v)
    return q, k, v, pos, u, vb, lens, H, Tmax


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("dk", [16, 64])
def test_rel_attention_lengths_on_tile_edges(mode, which, dk):
    """Lengths 63 / 64 / 65 / 200 and 127 / 128 / 129 / 1 inside T = 200: the key loop stops after 1, 2 or 3 of the 4 tiles, or masks
    all but one key of a tile.  Every query row is compared, the rows behind a sequence's length included."""
    _check_parity(mode, f"edge lengths {EDGE_LENS[which]} dk={dk}", _edge_case, dk, which)


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("dk", [16, 64])
def test_rel_attention_ignores_finite_garbage_behind_a_length(mode, which, dk):
    """+-1e4 in the k and v rows behind every length gives the same bits as zeros there (finite values only: 0 x NaN is NaN in the
    restatement as well)."""
    clean, dirty = _run(mode, *_edge_case(dk, which, "zero")), _run(mode, *_edge_case(dk, which, "garbage"))
    assert torch.isfinite(clean).all() and torch.equal(clean, dirty)


# ---- 5. strided operands through the C ABI -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dk", [16, 32, 64])
def test_rel_attention_strided_operands(mode, dk):
    """The engine's layout: q, k, v the three column slices of one [B, T, 3 hd] buffer, pos a column slice of a [rows, 2 hd] table with
    offset 0 in its middle, out (f32, f16, bf16) a column slice of a [B, T, hd + 64] buffer with one row in front and one behind, all
    pre-filled with a sentinel.  The slice is, bit for bit, what contiguous copies give, and no sentinel outside it changes.  x3:
    strided inputs; the split-row output keeps its own layout."""
    from diffnorm_amd import _lib, ops, packing

    q, k, v, pos, u, vb, lens, H, Tmax = _attn_case(dk, 65)
    B, T, hd = q.shape
    x3 = mode == "x3"
    want = ops.rel_attention(*(_dev(t, mode) for t in (q, k, v, pos)), u.to(DEV), vb.to(DEV), lens.to(DEV), H, Tmax - 1, x3=x3)
    qkv = _dev(torch.cat([q, k, v], -1), mode)  # [B, T, 3 hd]
    table = _dev(torch.cat([_randn(5, *pos.shape), pos], -1), mode)  # [2 Tmax - 1, 2 hd]: the offsets' rows in columns hd .. 2 hd
    ud, vd, ld = u.to(DEV), vb.to(DEV), lens.to(DEV, torch.int32)
    es = qkv.element_size()
    a = _lib.RelAttnParams()
    a.q, a.k, a.v = qkv.data_ptr(), qkv.data_ptr() + hd * es, qkv.data_ptr() + 2 * hd * es
    a.ldq = a.ldk = a.ldv = 3 * hd
    a.pos, a.ldp, a.pos_zero_row, a.pos_rows = table.data_ptr() + hd * es, 2 * hd, Tmax - 1, table.shape[0]
    a.bias_u, a.bias_v, a.lengths = ud.data_ptr(), vd.data_ptr(), ld.data_ptr()
    a.B, a.T, a.heads, a.dim_head, a.scale = B, T, H, dk, dk ** -0.5
    if x3:
        out = torch.empty(B, T, 2 * hd, dtype=torch.bfloat16, device=DEV)
        a.out, a.ldo, a.dtype = out.data_ptr(), hd, _lib.DN_BF16X3
    else:
        ldo, col = hd + 64, 32
        buf = torch.full((B * T + 2, ldo), SENTINEL, dtype=STORE[mode], device=DEV)
        before = buf.clone()
        a.out, a.ldo, a.dtype = buf.data_ptr() + (ldo + col) * es, ldo, {"f32": _lib.DN_F32, "f16": _lib.DN_F16, "bf16": _lib.DN_BF16}[mode]
    _lib.check(_lib.load().dn_rel_attention(C.byref(a), _lib.current_stream()), "dn_rel_attention")
    torch.cuda.synchronize()
    if x3:
        assert torch.equal(packing.unsplit_rows(out), want)
        return
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[1:-1, col:col + hd] = True
    assert torch.equal(buf[1:-1, col:col + hd].reshape(B, T, hd), want)
    assert torch.equal(buf[~inside], before[~inside])


def test_rel_attention_c_abi_refuses_strides_it_cannot_honour():
    """A row stride below heads * dim_head, or one that takes a 16-byte fragment (of split rows: a group of 32 elements) off its alignment, is
    DN_EINVAL and no launch."""
    from diffnorm_amd import _lib

    T, H, dk = 17, 2, 16
    q = torch.zeros(1, T, 3 * H * dk, device=DEV)
    pos = torch.zeros(2 * T - 1, H * dk, device=DEV)
    u = torch.zeros(H, dk, device=DEV)
    out = torch.full((T + 2, 3 * H * dk), SENTINEL, device=DEV)
    f32, x3 = _lib.DN_F32, _lib.DN_BF16X3
    for field, ld, dtype in (("ldq", H * dk - 4, f32), ("ldk", H * dk + 2, f32), ("ldv", H * dk - 16, f32), ("ldp", H * dk + 1, f32), ("ldo", H * dk - 4, f32),
                             ("ldo", H * dk + 2, f32), ("ldo", H * dk + 16, x3)):  # split rows: groups of 32 elements
        a = _lib.RelAttnParams()
        a.q = a.k = a.v = q.data_ptr()
        a.out, a.pos, a.bias_u, a.bias_v = out.data_ptr() + out.shape[1] * 4, pos.data_ptr(), u.data_ptr(), u.data_ptr()
        a.ldq = a.ldk = a.ldv = a.ldo = a.ldp = H * dk
        a.B, a.T, a.heads, a.dim_head, a.dtype, a.scale = 1, T, H, dk, dtype, dk ** -0.5
        a.pos_zero_row, a.pos_rows = T - 1, 2 * T - 1
        setattr(a, field, ld)
        with pytest.raises(_lib.DiffNormHipError):
            _lib.check(_lib.load().dn_rel_attention(C.byref(a), _lib.current_stream()), "dn_rel_attention")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---- 6. the band never leaves its offsets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("T", [1, 17, 65, 130])
@pytest.mark.parametrize("dk", [32])
def test_rel_attention_reads_no_table_row_outside_its_offsets(mode, T, dk):
    """The table is built for T + 37 frames; every row outside [zero - (T - 1), zero + (T - 1)] is NaN.  The clamp of the band keeps
    the 128 staged rows inside those offsets (at T = 1 and T = 17 most of the band lies outside them): finite, and the same bits as
    with the unpoisoned table."""
    q, k, v, pos, u, vb, lens, H, Tmax = _attn_case(dk, T)
    poisoned = pos.clone()
    poisoned[: Tmax - 1 - (T - 1)] = float("nan")
    poisoned[Tmax - 1 + T:] = float("nan")
    assert int(torch.isnan(poisoned[:, 0]).sum()) == 2 * 37 and not torch.isnan(poisoned[Tmax - T: Tmax - 1 + T]).any()
    clean = _run(mode, q, k, v, pos, u, vb, lens, H, Tmax)
    got = _run(mode, q, k, v, poisoned, u, vb, lens, H, Tmax)
    assert torch.isfinite(got).all() and torch.equal(got, clean)


# ---- 7. the running maximum --------------------------------------------------------------------------------------------------------
RAMP = 0.12  # k[b, j, 0] = RAMP * j (rising) or RAMP * (T - 1 - j) (falling), against q[.., 0] + u[0] = 8 +- 0.9: the content score moves
#              by (q0 + 8) * 0.12 * 64 / 4 = 14 .. 17 per whole key tile and by 42 .. 53 from the first key to the last -- exp(53) = 1e23
#              is finite in float32.  The fourth tile of T = 200 holds 8 keys, so the row maximum moves by only (q0 + 8) * 0.12 * 8 / 4
#              = 1.7 .. 2.1 between the last two tiles of the rising case: the random part of a score (the other 15 columns of k and
#              the position term, both scaled by 0.2) has a standard deviation of 0.3 to stay below that.


@functools.lru_cache(maxsize=None)
def _ramp_case(rising):
    dk, T, B, H, Tmax = 16, 200, 2, 1, 237
    s = 4000
    q, k, v = (_randn(s + i, B, T, dk) for i in range(3))
    pos = 0.2 * _randn(s + 3, 2 * Tmax - 1, dk)
    u, vb = 0.5 * _randn(s + 4, H, dk), 0.5 * _randn(s + 5, H, dk)
    u[0, 0] = 8.0
    q[:, :, 0] *= 0.25
    k = 0.2 * k
    j = torch.arange(T, dtype=torch.float32)
    k[:, :, 0] = RAMP * (j if rising else (T - 1) - j)
    return q, k, v, pos, u, vb, torch.tensor([T, T]), H, Tmax


def tile_maxima(rising, mode):
    """No device needed.  Per-tile maxima [B, T, 4] of the float64 scores of the ramp case, on the operands the device holds."""
    q, k, v, pos, u, vb, lens, H, Tmax = _ramp_case(rising)
    q, k, pos = (_rt(t, mode) for t in (q, k, pos))
    B, T, dk = q.shape
    p = pos[Tmax - 1 - (T - 1): Tmax - 1 + T]
    ac = (q + u.double()[0]) @ k.transpose(-1, -2)
    bd_all = (q + vb.double()[0]) @ p.transpose(-1, -2)
    idx = (T - 1) + torch.arange(T)[:, None] - torch.arange(T)[None, :]
    sc = (ac + torch.gather(bd_all, 2, idx[None].expand(B, T, T))) * dk ** -0.5
    assert sc.max() - sc.min() < 80  # exp of the whole range is finite in float32
    return torch.stack([sc[..., j0:j0 + TK].max(-1).values for j0 in range(0, T, TK)], -1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
def test_rel_attention_running_maximum(mode, rising):
    """T = 200 (4 key tiles), dk = 16, one head, full lengths, k[.., 0] = RAMP * key index (or its mirror): the running maximum of
    EVERY query row rises on each tile, so all of acc_o and l_run are rescaled by alpha < 1 three times -- or falls on each tile, so
    alpha == 1 throughout and the later tiles' P are tiny.  The monotone tile maxima are checked on the float64 scores first."""
    mx = tile_maxima(rising, mode)
    step = mx[..., 1:] - mx[..., :-1]
    print(f"rel_attention running maximum {'rising' if rising else 'falling'} {mode}: tile-to-tile steps of the row maxima {step.min().item():.2f} .. "
          f"{step.max().item():.2f}, first to last {(mx[..., -1] - mx[..., 0]).abs().min().item():.1f} .. {(mx[..., -1] - mx[..., 0]).abs().max().item():.1f}")
    assert bool((step > 0).all() if rising else (step < 0).all())
    _check_parity(mode, "running maximum " + ("rising" if rising else "falling"), _ramp_case, rising)


# ---- dn_glu_dwconv -----------------------------------------------------------------------------------------------------------------
def _dw_case(S, k, Cc, B=2):
    x = _randn(3 * S + k + Cc, B, S, 2 * Cc)
    return x, _randn(17 + k + Cc, Cc, k) * k ** -0.5, 0.3 * _randn(19 + k + Cc, Cc)


def _dw_check(mode, x, w, shift, label):
    from diffnorm_amd import _lib, ops

    want = _glu_dwconv_ref(_rt(x, mode), w, shift)
    assert torch.isfinite(want).all()
    scale = want.abs().max().item()
    got = ops.glu_dwconv(_dev(x, mode), w.to(DEV), shift.to(DEV), dtype=_lib.DN_BF16X3 if mode == "x3" else None)
    err = (got.double().cpu() - want).abs().max().item()
    bound = _glu_dwconv_bound(mode, scale)
    print(f"glu_dwconv {label} {mode}: bound {bound:.3e} measured {err:.3e}")
    assert got.shape == want.shape and torch.isfinite(got).all() and err < bound


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("k,Cc", [(1, 64), (15, 128), (63, 64)])
def test_glu_dwconv_frame_tile_edges(mode, S, k, Cc):
    """Frames on and beside the edges of the 32-frame tile; k = 1 (no halo), 15, and 63 (DW_KMAX: a halo of 31 + 31 rows, longer than
    the tile).  The bound of test_glu_dwconv_matches_float64."""
    _dw_check(mode, *_dw_case(S, k, Cc), f"k={k} C={Cc} S={S}")


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_glu_dwconv_saturated_gates(mode):
    """Gates of +-30 and +-80 in blocks of 8 channels: sigmoid is 1 - 1e-13, 1e-13, 1 and 2e-35 there; exp(80) is finite in fp32."""
    S, k, Cc = 33, 3, 64
    x, w, shift = _dw_case(S, k, Cc)
    gate = torch.tensor([30.0, -30.0, 80.0, -80.0]).repeat_interleave(8).repeat(Cc // 32)
    x[:, :, Cc:] = gate[None, None, :] * torch.where(torch.arange(S) % 2 == 0, 1.0, -1.0)[None, :, None]
    _dw_check(mode, x, w, shift, "saturated gates")


@pytest.mark.parametrize("mode", MODES)
def test_glu_dwconv_stores_nothing_outside_out(mode):
    """S = 33 (one frame in the last tile), k = 63: `out` sits between two sentinel rows, handed over through the C ABI; the rows
    between them are what ops.glu_dwconv gives, the sentinels stay."""
    from diffnorm_amd import _lib, ops

    S, k, Cc, B = 33, 63, 64, 2
    x, w, shift = _dw_case(S, k, Cc)
    code = {"f32": _lib.DN_F32, "x3": _lib.DN_BF16X3, "f16": _lib.DN_F16, "bf16": _lib.DN_BF16}[mode]
    xd, wd, sd = _dev(x, mode), w.to(DEV), shift.to(DEV)
    width = 2 * Cc if mode == "x3" else Cc  # split rows: a bf16 tensor of twice the width
    buf = torch.full((B * S + 2, width), SENTINEL, dtype=torch.bfloat16 if mode == "x3" else STORE[mode], device=DEV)
    before = buf.clone()
    out_ptr = buf.data_ptr() + width * buf.element_size()
    _lib.check(_lib.load().dn_glu_dwconv(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), out_ptr, B, S, Cc, k, code, _lib.current_stream()), "dn_glu_dwconv")
    torch.cuda.synchronize()
    from diffnorm_amd import packing

    inner = buf[1:-1].reshape(B, S, width)
    assert torch.equal(packing.unsplit_rows(inner) if mode == "x3" else inner, ops.glu_dwconv(xd, wd, sd, dtype=code))
    assert torch.equal(buf[0], before[0]) and torch.equal(buf[-1], before[-1])


# ---- the engine at head width 32 ---------------------------------------------------------------------------------------------------
TINY32 = types.SimpleNamespace(**{**vars(R.TINY), "heads": 2})  # embed 64 / 2 heads: d_k = 32; nothing else changes


@functools.lru_cache(maxsize=None)
def _tiny32():
    """Seeded weights, B = 2, L = 150 (lengths 150 / 97 -> S = 38, 38 / 25 frames), the float64 restatement on the CPU -- once."""
    sd = R.make_state_dict(TINY32, 32032)
    feats, lens = R.make_features(2, 150, (150, 97), TINY32.input_dim, 32033)
    with torch.no_grad():
        want, ol = R.encode(sd, TINY32, feats, lens, torch.float64)
    return sd, feats, lens, want, ol


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_conformer_encoder_at_head_width_32(dtype):
    """ConformerEncoderEngine with dim / heads == 32 against the float64 restatement, valid frames; output lengths exact."""
    from diffnorm_amd import nar_decoder

    c = TINY32
    assert c.embed_dim // c.heads == 32
    sd, feats, lens, want, wl = _tiny32()
    eng = nar_decoder.ConformerEncoderEngine(sd, c.input_dim, c.conv_channels, c.kernel_sizes[0], c.embed_dim, c.ffn_dim, c.layers, c.heads,
                                             c.depthwise_kernel, dtype=dtype, device=DEV)
    out, ol = eng.forward(feats.to(DEV), lens.to(DEV))
    assert ol.cpu().tolist() == wl.tolist()
    valid = torch.arange(want.shape[1])[None, :] < wl[:, None]
    bar = ENGINE_TOL[dtype] * max(1.0, want.abs().max().item() / 4)
    err = (out.double().cpu() - want)[valid].abs().max().item()
    print(f"conformer encoder, d_k = 32, {dtype}: bound {bar:.3e} measured {err:.3e} (output scale {want.abs().max().item():.2f})")
    assert out.shape == want.shape and err < bar
