"""GPU checks of the split-operand (bf16x3) VAE training engine: three bf16 MFMAs per product on split-row operands (include/
diffnorm_hip.h), every non-operand tensor fp32 as in the exact-fp32 mode.

Operators, bit for bit: every element-wise training kernel in bf16x3 on split inputs equals the split of the fp32 kernel's output on
the de-split inputs (both compute in fp32 and a split row de-splits exactly); the split operand transposes equal
split(transpose(de-split)); the work copy that refresh / sync_work make equals split(master).

Parity against the reference's fixtures at the bars the f32 tests hold: per-tensor 1e-3 (tests/golden/vae_train.npz,
vae_train_full.npz, vae_train_batch.npz), the five-update trajectory at 2e-3, train-mode dropout against the oracle with the restated
mask at 1e-3.  Structure: staged backward == whole backward, side-stream weight gradients change nothing, the Level-1 plugin path
updating through p.data equals FlatOptimizer, the diffusion engine refuses bf16x3."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffnorm_oracle as O
import train_oracle as TO
from gen_golden_configs import CHAIN_VAE, seeded
from test_hip_train import _FairseqAdamThroughData, _bench_batch, _grads_close, _sample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG = CHAIN_VAE
X3 = "bf16x3"


def _lib():
    from diffnorm_amd import _lib

    return _lib, _lib.load()


def _stream():
    from diffnorm_amd import _lib

    return _lib.current_stream()


def _engine(sd=None, dtype=X3):
    from diffnorm_amd import training

    sd = O.make_vae_state_dict(CFG, "train") if sd is None else sd
    return training.VaeTrainEngine(sd, dim=CFG.dim, latent_dim=CFG.latent_dim, dtype=dtype, device=DEV, depth=CFG.depth,
                                   heads=CFG.heads, dim_head=CFG.dim_head, stacks=CFG.stacks, layers=CFG.layers), sd


def _batch(g):
    feat = seeded((3, 48, CFG.dim), 31)
    return feat, torch.from_numpy(g["units"]), torch.from_numpy(g["lens"])


# ---------------------------------------------------------------------------------------------------------------- operators
def sp(t, weight=False):
    """fp32 [..., K] -> split rows on the device (bf16 [..., 2K])."""
    from diffnorm_amd import packing

    return packing.split_rows(t.float().cpu(), weight=weight).to(DEV)


def desp(t):
    """split rows -> the fp32 values they hold, on the device."""
    from diffnorm_amd import packing

    return packing.unsplit_rows(t.cpu()).to(DEV).contiguous()


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    ia = a.view(torch.int16 if a.element_size() == 2 else torch.int32)
    ib = b.view(torch.int16 if b.element_size() == 2 else torch.int32)
    n = int((ia != ib).sum())
    assert n == 0, f"{n} of {ia.numel()} elements differ"


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _inputs(M, ld, seed, scale=1.0, cols=None):
    """seeded fp32 [M, ld] (columns >= cols zero) and its split form: the x3 kernel reads xs, the f32 kernel desp(xs)."""
    t = _rand((M, ld), seed, scale)
    if cols is not None:
        t[:, cols:] = 0
    xs = sp(t)
    return xs, desp(xs)


def test_elementwise_kernels_split_equal_split_of_f32():
    L, lib = _lib()
    F32, S = L.DN_F32, L.DN_BF16X3
    chk = L.check
    B, T, ld = 3, 40, 128
    M = B * T
    z32 = lambda *s: torch.zeros(*s, device=DEV)
    zsp = lambda m, n: torch.zeros(m, 2 * n, dtype=torch.bfloat16, device=DEV)
    h_s, h_f = _inputs(M, ld, 1, 2.0)
    r_s, r_f = _inputs(M, ld, 2)
    d_s, d_f = _inputs(M, ld, 3)
    # gate forward / backward (:525-530)
    o_s, o_f = zsp(M, ld), z32(M, ld)
    chk(lib.dn_gate_forward(h_s.data_ptr(), r_s.data_ptr(), o_s.data_ptr(), S, M, ld, T, None, 0, 0, _stream()), "gate x3")
    chk(lib.dn_gate_forward(h_f.data_ptr(), r_f.data_ptr(), o_f.data_ptr(), F32, M, ld, T, None, 0, 0, _stream()), "gate f32")
    same_bits(o_s, sp(o_f))
    o_s, o_f = zsp(M, ld), z32(M, ld)
    chk(lib.dn_gate_backward(d_s.data_ptr(), h_s.data_ptr(), o_s.data_ptr(), S, M, ld, T, None, 0, 0, None, 0, _stream()), "gate bwd x3")
    chk(lib.dn_gate_backward(d_f.data_ptr(), h_f.data_ptr(), o_f.data_ptr(), F32, M, ld, T, None, 0, 0, None, 0, _stream()), "gate bwd f32")
    same_bits(o_s, sp(o_f))
    # GEGLU forward / backward on the packed [8 value ; 8 gate] columns (:881-884)
    ip = 128
    p_s, p_f = _inputs(M, 2 * ip, 4, 1.5)
    o_s, o_f = zsp(M, ip), z32(M, ip)
    chk(lib.dn_geglu_forward(p_s.data_ptr(), o_s.data_ptr(), S, M, ip, _stream()), "geglu x3")
    chk(lib.dn_geglu_forward(p_f.data_ptr(), o_f.data_ptr(), F32, M, ip, _stream()), "geglu f32")
    same_bits(o_s, sp(o_f))
    o_s, o_f = zsp(M, 2 * ip), z32(M, 2 * ip)
    chk(lib.dn_geglu_backward(d_s.data_ptr(), p_s.data_ptr(), o_s.data_ptr(), S, M, ip, _stream()), "geglu bwd x3")
    chk(lib.dn_geglu_backward(d_f.data_ptr(), p_f.data_ptr(), o_f.data_ptr(), F32, M, ip, _stream()), "geglu bwd f32")
    same_bits(o_s, sp(o_f))
    # RMSNorm backward: dy split, dx fp32 and its operand copy dx_act (:620-639)
    D, Dp = 96, 128
    x = _rand((M, Dp), 5).to(DEV)
    x[:, D:] = 0
    gamma = (1 + 0.1 * _rand((D,), 6)).to(DEV)
    dy_s, dy_f = _inputs(M, Dp, 7, cols=D)
    scratch = torch.zeros(int(lib.dn_rmsnorm_backward_scratch_bytes(B, T, D)) // 4 + 64, device=DEV)
    outs = {}
    for name, dy, dt in (("x3", dy_s, S), ("f32", dy_f, F32)):
        dx, dg = z32(M, Dp), z32(D)
        act = zsp(M, Dp) if dt == S else z32(M, Dp)
        chk(lib.dn_rmsnorm_backward(x.data_ptr(), Dp, dy.data_ptr(), Dp, dt, B, T, D, gamma.data_ptr(), None, 0, 0, None, dx.data_ptr(),
                                    act.data_ptr(), dt, Dp, dg.data_ptr(), None, 0, scratch.data_ptr(), _stream()), "rmsnorm bwd " + name)
        outs[name] = (dx, act, dg)
    same_bits(outs["x3"][0], outs["f32"][0])
    same_bits(outs["x3"][1], sp(outs["f32"][1]))
    same_bits(outs["x3"][2], outs["f32"][2])
    # posterior sample / backward (distributions.py:24-41, 62-74)
    Z, ldz, ldo = 8, 64, 64
    params = _rand((M, 2 * Z), 8, 2.0).to(DEV)
    noise, dz = _rand((M, Z), 9).to(DEV), z32(M, ldz)
    dz[:, :Z] = _rand((M, Z), 10).to(DEV)
    lens = torch.tensor([40, 17, 29], dtype=torch.int32, device=DEV)
    outs = {}
    for name, dt in (("x3", S), ("f32", F32)):
        z, kl = z32(M, ldz), z32(M)
        act = zsp(M, ldz) if dt == S else z32(M, ldz)
        chk(lib.dn_posterior_sample(params.data_ptr(), 2 * Z, noise.data_ptr(), Z, z.data_ptr(), act.data_ptr(), dt, ldz, M, Z, T, lens.data_ptr(),
                                    kl.data_ptr(), _stream()), "posterior " + name)
        dp = zsp(M, ldo) if dt == S else z32(M, ldo)
        chk(lib.dn_posterior_backward(params.data_ptr(), 2 * Z, noise.data_ptr(), Z, dz.data_ptr(), ldz, dp.data_ptr(), dt, ldo, M, Z, T,
                                      lens.data_ptr(), C.c_float(1e-3), _stream()), "posterior bwd " + name)
        outs[name] = (act, dp)
    same_bits(outs["x3"][0], sp(outs["f32"][0]))
    same_bits(outs["x3"][1], sp(outs["f32"][1]))
    # label-smoothed CE gradient (d logits) over the padded vocabulary
    V, ldd = 1004, 1024
    logits = _rand((M, V), 11, 2.0).to(DEV)
    tgt = torch.randint(4, V, (M,), generator=torch.Generator().manual_seed(12)).to(DEV, torch.int32)
    tgt[5] = 0
    outs = {}
    for name, dt in (("x3", S), ("f32", F32)):
        rows = z32(M, 4)
        dl = zsp(M, ldd) if dt == S else z32(M, ldd)
        chk(lib.dn_lsce_loss_grad(logits.data_ptr(), V, tgt.data_ptr(), M, V, C.c_float(0.1), C.c_float(0.01), rows.data_ptr(), dl.data_ptr(),
                                  dt, ldd, _stream()), "lsce " + name)
        outs[name] = dl
    same_bits(outs["x3"], sp(outs["f32"]))
    # masked MSE gradient's operand copy d_rec_act
    pred = _rand((M, Dp), 13).to(DEV)
    pred[:, D:] = 0
    tg = _rand((M, D), 14).to(DEV)
    outs = {}
    for name, dt in (("x3", S), ("f32", F32)):
        dpred = z32(M, Dp)
        act = zsp(M, Dp) if dt == S else z32(M, Dp)
        chk(lib.dn_masked_mse_grad(pred.data_ptr(), Dp, tg.data_ptr(), D, M, D, T, lens.data_ptr(), C.c_float(0.5), None, dpred.data_ptr(), Dp, 1,
                                   act.data_ptr(), dt, Dp, _stream()), "mse " + name)
        outs[name] = act
    same_bits(outs["x3"], sp(outs["f32"]))
    # column sums (bias gradients), sums over groups, row conversions
    scr = torch.zeros(1 << 20, device=DEV)
    cs = {}
    for name, src, dt in (("x3", h_s, S), ("f32", h_f, F32)):
        out = z32(B, ld)
        chk(lib.dn_colsum(src.data_ptr(), ld, dt, B, T, ld, out.data_ptr(), ld, C.c_float(1.0), 0, scr.data_ptr(), _stream()), "colsum " + name)
        cs[name] = out
    same_bits(cs["x3"], cs["f32"])
    g_s, g_f = _inputs(4 * M, ld, 15)
    n = M * ld
    o_s, o_f = zsp(M, ld), z32(M, ld)
    chk(lib.dn_sum_groups(g_s.data_ptr(), n, 4, o_s.data_ptr(), S, n, _stream()), "sum_groups x3")
    chk(lib.dn_sum_groups(g_f.data_ptr(), n, 4, o_f.data_ptr(), F32, n, _stream()), "sum_groups f32")
    same_bits(o_s, sp(o_f))
    src = _rand((M, 100), 16).to(DEV)
    o_s, o_f = zsp(M, ld), z32(M, ld)
    chk(lib.dn_convert_rows(src.data_ptr(), F32, 100, o_s.data_ptr(), S, ld, M, 100, _stream()), "convert f32 -> x3")
    chk(lib.dn_convert_rows(src.data_ptr(), F32, 100, o_f.data_ptr(), F32, ld, M, 100, _stream()), "convert f32 -> f32")
    same_bits(o_s, sp(o_f))
    back = z32(M, ld)
    chk(lib.dn_convert_rows(o_s.data_ptr(), S, ld, back.data_ptr(), F32, ld, M, ld, _stream()), "convert x3 -> f32")
    same_bits(back, desp(o_s))


def test_split_transposes_equal_split_of_transpose():
    from diffnorm_amd import packing

    L, lib = _lib()
    # packed weights -> the data-gradient operand: 3 matrices [128 rows (R = 100 valid)][192] -> [256][128], weight order both sides
    w = _rand((3, 128, 192), 21)
    w[:, 100:] = 0
    ws = sp(w, weight=True)
    dst = torch.zeros(3, 256, 2 * 128, dtype=torch.bfloat16, device=DEV)
    L.check(lib.dn_transpose_weights(ws.data_ptr(), L.DN_BF16X3, 3, 128 * 192, 100, 192, dst.data_ptr(), 256 * 128, 128, 256, _stream()),
            "transpose_weights x3")
    want = torch.zeros(3, 256, 128)
    want[:, :192, :100] = packing.unsplit_rows(ws.cpu())[:, :100].transpose(1, 2)
    same_bits(dst, sp(want, weight=True))
    # the weight gradient's K-sliced operand copies: dY^T as the A operand ([hi | lo]), X^T (front-shifted) as the W operand ([lo | hi])
    B, T, Cc, ld, front = 3, 50, 90, 128, 2
    Tp = 64
    chunk = 64
    cols_total = B * Tp
    rows, rows_total, row0 = 128, 256, 128
    x_s, x_f = _inputs(B * T, ld, 22, cols=Cc)
    xv = x_f.cpu()
    ref = torch.zeros(cols_total // chunk, rows_total, chunk)
    for b in range(B):
        for t in range(T):
            j = b * Tp + front + t
            ref[j // chunk, row0: row0 + Cc, j % chunk] = xv[b * T + t, :Cc]
    for order in (0, 1):
        dst = torch.zeros(cols_total // chunk, rows_total, 2 * chunk, dtype=torch.bfloat16, device=DEV)
        L.check(lib.dn_transpose_slices(x_s.data_ptr(), L.DN_BF16X3, ld, B, T, Cc, front, Tp, cols_total, chunk, dst.data_ptr(), rows, rows_total,
                                        row0, order, _stream()), "transpose_slices x3")
        same_bits(dst[:, row0:], sp(ref[:, row0:], weight=bool(order)))
        f32 = torch.zeros(cols_total // chunk, rows_total, chunk, device=DEV)
        L.check(lib.dn_transpose_slices(x_f.data_ptr(), L.DN_F32, ld, B, T, Cc, front, Tp, cols_total, chunk, f32.data_ptr(), rows, rows_total,
                                        row0, 0, _stream()), "transpose_slices f32")
        same_bits(f32[:, row0:], ref[:, row0:])


def _work_is_split_master(eng):
    torch.cuda.synchronize()
    same_bits(eng.work, sp(eng.master.cpu(), weight=True))


def test_work_copy_is_split_master_after_load_adam_and_external_updates(golden):
    from diffnorm_amd import optim, training

    g = golden("vae_train")
    eng, _ = _engine()
    assert eng.work.numel() == 2 * eng.n_params and eng.work.dtype == torch.bfloat16 and eng.adam_copy is None
    _work_is_split_master(eng)  # load_state_dict -> sync_work
    feat, units, lens = _batch(g)
    tr = training.VaeTrainer(eng, lr=1e-3, warmup_updates=1, attn_dropout=0.0)
    sample = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": lens, "ntokens": int(lens.sum()), "nsentences": 3}
    before = eng.master.clone()
    tr.train_step([sample], noises=[torch.from_numpy(g["post_noise"])])  # dn_adam_step + refresh
    assert not torch.equal(before, eng.master)
    _work_is_split_master(eng)
    opt = optim.FlatOptimizer(eng, lr=1e-3)
    eng.forward(feat, units, lens, noise=torch.from_numpy(g["post_noise"]))
    opt.zero_grad()
    eng.backward()
    opt.multiply_grads(1.0 / 3)
    opt.step()
    _work_is_split_master(eng)
    eng.master.add_(1e-3 * torch.randn(eng.n_params, generator=torch.Generator().manual_seed(3)).to(DEV))  # an external update of master
    eng.sync_work()
    _work_is_split_master(eng)


# ------------------------------------------------------------------------------------------------------------ parity
def test_vae_losses_and_gradients_match_reference_x3(golden):
    g = golden("vae_train")
    feat, units, lens = _batch(g)
    eng, _ = _engine()
    stats, logits, _ = eng.forward(feat, units, lens, noise=torch.from_numpy(g["post_noise"]), ntokens=int(lens.sum()), want_logits=True)
    eng.zero_grad()
    eng.backward()
    s = stats.cpu().double().numpy()
    for i, k in enumerate(("loss", "nll_loss", "mse_loss", "kl_loss", "acc")):
        print(f"x3 {k}: {s[i]!r} reference {float(g[k])!r}")
        assert abs(s[i] - float(g[k])) <= 1e-4 * max(1.0, abs(float(g[k]))), (k, s[i], float(g[k]))
    assert np.abs(logits.cpu().numpy()[:, :4] - g["logits_head"]).max() < 1e-3
    grads = eng.grad_dict()
    worst = TO.compare_grads(grads, g, "g/", rtol=1e-3)
    print("bf16x3 vae_train: worst relative gradient error vs the reference:", worst)
    total = float(torch.sqrt(sum(v.double().pow(2).sum() for v in grads.values())))
    assert abs(total - float(g["g/total_norm"])) <= 1e-3 * float(g["g/total_norm"])


def test_fullsize_vae_training_step_matches_reference_x3(golden):
    from diffnorm_amd import training
    from gen_golden_configs import FULL_VAE

    g = golden("vae_train_full")
    sd = O.make_vae_state_dict(FULL_VAE, "full")
    eng = training.VaeTrainEngine(sd, dtype=X3, device=DEV)
    del sd
    feat = seeded((2, 64, FULL_VAE.dim), 41)
    units, lens = torch.from_numpy(g["units"]), torch.from_numpy(g["lens"])
    stats, logits, _ = eng.forward(feat, units, lens, noise=torch.from_numpy(g["post_noise"]), ntokens=int(lens.sum()), want_logits=True)
    eng.zero_grad()
    eng.backward()
    s = stats.cpu().double().numpy()
    for i, k in enumerate(("loss", "nll_loss", "mse_loss", "kl_loss")):
        assert abs(s[i] - float(g[k])) <= 2e-4 * max(1.0, abs(float(g[k]))), (k, s[i], float(g[k]))
    assert np.abs(logits.cpu().numpy()[:, :4, :64] - g["logits_head"]).max() < 1e-3
    worst = TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3)
    print("bf16x3 vae_train_full: worst relative gradient error vs the reference:", worst)


def test_bench_shape_vae_training_step_matches_reference_x3(golden):
    from diffnorm_amd import training
    from gen_golden_configs import FULL_VAE

    g = golden("vae_train_batch")
    eng = training.VaeTrainEngine(O.make_vae_state_dict(FULL_VAE, "full"), dtype=X3, device=DEV)
    feat, lens = _bench_batch(24, 512, FULL_VAE.dim, int(g["batch_seed"]))
    assert torch.equal(lens, torch.from_numpy(g["lens"]))
    units = torch.from_numpy(g["units"])
    noise = seeded(tuple(int(v) for v in g["post_noise_shape"]), int(g["post_noise_seed"])).transpose(1, 2).contiguous()
    stats, logits, _ = eng.forward(feat, units, lens, noise=noise, ntokens=int(lens.sum()), want_logits=True)
    eng.zero_grad()
    eng.backward()
    s = stats.cpu().double().numpy()
    for i, k in enumerate(("loss", "nll_loss", "mse_loss", "kl_loss")):
        assert abs(s[i] - float(g[k])) <= 2e-4 * max(1.0, abs(float(g[k]))), (k, s[i], float(g[k]))
    assert np.abs(logits.cpu().numpy()[:, :4, :64] - g["logits_head"]).max() < 1e-3
    worst = TO.compare_grads(eng.grad_dict(), g, "g/", rtol=1e-3)
    print("bf16x3 vae_train_batch: worst relative gradient error vs the reference:", worst)


def test_five_update_trajectory_matches_reference_x3(golden):
    from diffnorm_amd import training

    g = golden("vae_train")
    feat, units, lens = _batch(g)
    lr, warm, warm_init, b1, b2, clip = (float(v) for v in g["hyper"])
    eng, _ = _engine()
    tr = training.VaeTrainer(eng, lr=lr, betas=(b1, b2), clip_norm=clip, warmup_updates=int(warm), warmup_init_lr=warm_init, attn_dropout=0.0)
    sample = {"reduce_target": feat, "reduce_target_unit": units, "reduce_target_lengths": lens, "ntokens": int(lens.sum()),
              "nsentences": feat.shape[0]}
    traj = g["traj"]
    for it in range(traj.shape[0]):
        logged, norm = tr.train_step([sample], noises=[torch.from_numpy(g[f"traj_noise{it}"])])
        got = logged.cpu().double().numpy()
        for col, name in enumerate(("loss", "nll", "mse", "kl")):
            assert abs(got[col] - traj[it, col]) <= 2e-3 * max(1.0, abs(traj[it, col])), (it, name, got[col], traj[it, col])
        assert abs(got[4] - traj[it, 4]) < 1e-2
        assert abs(float(norm) - traj[it, 5]) <= 2e-3 * traj[it, 5], (it, float(norm), traj[it, 5])
    worst = TO.compare_grads(eng.state_dict(), g, "p_end/", rtol=2e-3)
    print("bf16x3 trajectory: worst relative parameter error after five updates:", worst)


def test_train_mode_attention_dropout_vae_x3(golden):
    from dropout_mask import layer_keep

    g = golden("vae_train")
    feat, units, lens = _batch(g)
    noise = torch.from_numpy(g["post_noise"])
    eng, sd = _engine()
    eng.attn_dropout, eng.dropout_seed = 0.1, 77
    stats = eng.forward(feat, units, lens, noise=noise, ntokens=int(lens.sum()))
    eng.zero_grad()
    eng.backward()
    lo, hi = eng._batch.dropout_seed_lo, eng._batch.dropout_seed_hi
    with O.attention_dropout("vae", 0.1, layer_keep(0.1, lo, hi)):
        want_loss, want = TO.vae_loss_and_grads(sd, CFG, feat, units, lens, noise)
    s = stats.cpu().double().numpy()
    for i, k in enumerate(("loss", "nll_loss", "mse_loss", "kl_loss")):
        assert abs(s[i] - want_loss[k]) <= 1e-4 * max(1.0, abs(want_loss[k])), (k, s[i], want_loss[k])
    assert abs(s[0] - float(g["loss"])) > 1e-4
    print("bf16x3 train-mode dropout: worst relative gradient error vs the oracle with the same mask:", _grads_close(eng.grad_dict(), want, 1e-3))


# ---------------------------------------------------------------------------------------------------------- structure
def test_staged_backward_is_the_whole_backward_x3(golden):
    g = golden("vae_train")
    feat, units, lens = _batch(g)
    eng, _ = _engine()
    noise = torch.from_numpy(g["post_noise"])
    eng.forward(feat, units, lens, noise=noise)
    eng.zero_grad()
    eng.backward()
    whole = eng.grads.clone()
    eng.forward(feat, units, lens, noise=noise)
    eng.zero_grad()
    for st in range(eng.n_stages):
        eng.backward(st, st)
        off, cnt = eng.stage_ranges()[st]
        assert torch.equal(eng.grads[off: off + cnt], whole[off: off + cnt]), f"stage {st} did not complete its range"
    assert torch.equal(eng.grads, whole)


def test_weight_gradients_on_the_side_stream_change_nothing_x3(golden, hip_option):
    g = golden("vae_train")
    feat, units, lens = _batch(g)
    noise = torch.from_numpy(g["post_noise"])
    eng, _ = _engine()
    grads = {}
    for mode in ("0", "1", "1", "0", "1"):
        hip_option("wgrad_stream", int(mode))
        eng.forward(feat, units, lens, noise=noise)
        eng.zero_grad()
        if mode == "1" and "staged" not in grads:
            for st in range(eng.n_stages):
                eng.backward(st, st)
            grads["staged"] = eng.grads.clone()
        else:
            eng.backward()
        torch.cuda.synchronize()
        grads.setdefault(mode, eng.grads.clone())
        assert torch.equal(eng.grads, grads["0"]), mode
    assert torch.equal(grads["staged"], grads["0"])


def test_level1_with_an_optimizer_that_updates_through_p_data_x3(golden):
    """The plugin model built with --hip-dtype bf16x3: fairseq's Adam through p.data (master only; the bridge's sync_work makes the
    split work copy) gives the same three updates as the HIP-backed FlatOptimizer, at the f32 test's bars."""
    import types

    from diffnorm_amd import fairseq_plugin, optim  # noqa: F401
    from diffnorm_amd.fairseq_plugin import registry

    g = golden("vae_train")

    def build():
        args = types.SimpleNamespace(arch="speech_vae_decoder", criterion="speech_vae_decoder_loss", latent_dim=CFG.latent_dim,
                                     feature_dim=CFG.dim, hip_dtype=X3, target_code_size=1000, data="", optimizer="adam", lr=[1e-3])
        task = registry.TASK_REGISTRY["speech_decoder"].setup_task(args)
        model = task.build_model(args)
        model.load_state_dict({"encoder." + k: v for k, v in O.make_vae_state_dict(CFG, "train").items()}, strict=True)
        model.to(DEV)
        model.encoder.attn_dropout = 0.0
        return task, model, task.build_criterion(args)

    task, model, criterion = build()
    assert model.encoder._train_engine.dtype == __import__("diffnorm_amd")._lib.DN_BF16X3
    ext = _FairseqAdamThroughData(model, lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
    task2, model2, criterion2 = build()
    ref = optim.FlatOptimizer(model2.encoder._train_engine, lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
    losses = []
    for it in range(3):
        sample = _sample(g, torch.from_numpy(g[f"traj_noise{it % 3}"]))
        ext.zero_grad()
        loss, n, _ = task.train_step(sample, model, criterion, ext, it)
        ref.zero_grad()
        loss2, _, _ = task2.train_step(sample, model2, criterion2, ref, it)
        losses.append(float(loss.detach()))
        assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-5 * abs(float(loss2.detach())), (it, float(loss.detach()), float(loss2.detach()))
        ext.multiply_grads(1.0 / n)
        ref.multiply_grads(1.0 / n)
        ext.step()
        ref.step()
        pa, pb = model.encoder._train_engine.master, model2.encoder._train_engine.master
        assert float((pa - pb).norm() / pb.norm()) < 1e-6, (it, float((pa - pb).norm() / pb.norm()))
    assert len(set(losses)) == 3


def test_diffusion_engine_refuses_x3():
    from diffnorm_amd import training
    from gen_golden_configs import CHAIN_EPS

    with pytest.raises(ValueError, match="VAE training engine is the one bf16x3 training engine"):
        training.EpsTrainEngine(O.make_eps_state_dict(CHAIN_EPS, "train"), CHAIN_EPS, None, timesteps=200, dtype=X3, device=DEV)
