"""Classifier-free-guided mask-predict decoding on the GPU (the reference's `nar_cg` evaluation, research/TranSpeech/nat_gen.py:192-236):
the null-source table (dn_nar_null_cross), the decoder pass over 2 B rows (dn_nar_decoder_forward_guided) folded and literal, the fused
guided update (dn_cmlm_guided_step) and NARS2UTDecoderModel.guided_mask_predict eager and as a replayed hipGraph, against the REAL
classes' outputs (tests/golden/nar_cg.npz) and the CPU restatement (tests/nar_cg_ref.py)."""
import numpy as np
import pytest
import torch

import nar_cg_ref as G
import nar_oracle as N
from gen_golden_nar_configs import CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [("f32", 1e-3), ("bf16x3", 1e-3), ("f16", 1e-2), ("bf16", 6e-2)]  # the decoder bound of tests/test_hip_refine.py
TOL = dict(MODES)
_cache = {}


def sd():
    if "sd" not in _cache:
        _cache["sd"] = N.make_nar_state_dict(CFG, "nar")
    return _cache["sd"]


def model(dtype, use_graph=False):
    from diffnorm_amd import nar_decoder

    key = (dtype, use_graph)
    if key not in _cache:
        _cache[key] = nar_decoder.NARS2UTDecoderModel(sd(), CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype=dtype, device=DEV,
                                                      use_graph=use_graph)
    return _cache[key]


def engine(dtype):
    return model(dtype).engine


def enc_dict(enc_sbd, lens):
    pad = torch.arange(enc_sbd.size(0))[None, :] >= lens[:, None]
    return {"encoder_out": [enc_sbd.to(DEV)], "encoder_padding_mask": [pad.to(DEV)], "encoder_embedding": [], "encoder_states": [], "src_tokens": [],
            "src_lengths": []}


def fixture_enc(g):
    return enc_dict(torch.from_numpy(g["enc_out"]), torch.from_numpy(g["src_lens"]))


def decoder_bound(dtype, ref):
    return TOL[dtype] * max(1.0, float(ref.abs().max()) / 4)


@pytest.mark.parametrize("dtype,bound", [("f32", 1e-5), ("bf16x3", 1e-5), ("f16", 2e-3), ("bf16", 1.6e-2)])
def test_null_source_table(dtype, bound):
    """c_l of dn_nar_null_cross against the float64 evaluation of W_o (W_v e_null + b_v) + b_o from the state dict, relative to
    max |c_l|.  The 2-byte bounds stand for two operand roundings (half a unit of 2^-10 / 2^-7 each, activation and weight) through the
    two contractions of the formula, accumulated in fp32; f32 and the split operands keep 1e-5."""
    ref = G.null_rows(sd(), CFG)
    tab = engine(dtype).null_cross(CFG.bos).cpu().double()
    err = float((tab - ref).abs().max() / ref.abs().max())
    print(f"null-source table {dtype}: max err / max|c_l| = {err:.3e} (max|c_l| {float(ref.abs().max()):.3f})")
    assert tab.shape == ref.shape and err <= bound


@pytest.mark.parametrize("dtype,tol", MODES)
def test_guided_pass_matches_the_real_reference(golden, dtype, tol):
    g = golden("nar_cg")
    m = model(dtype)
    eng = m.engine
    eng.null_cross(int(g["null_token"]))
    ckv, slen = m._prepared(fixture_enc(g))
    tok = torch.from_numpy(g["s0_tok_in"]).to(DEV).int().contiguous()
    both = eng.forward_guided(tok, ckv, slen).cpu()
    cond, null = torch.from_numpy(g["cond0"]), torch.from_numpy(g["null0"])
    bound = tol * max(1.0, float(max(cond.abs().max(), null.abs().max())) / 4)
    for name, got, ref in (("cond", both[0], cond), ("null", both[1], null)):
        err = float((got - ref).abs().max())
        print(f"guided pass {dtype} {name}: max abs err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, name
    for s in (0.5, 3.0):  # |err| <= (1 + s) e_cond + s e_null
        got = eng.guided_logits(tok, ckv, slen, s).cpu()
        err = float((got - (cond + s * (cond - null))).abs().max())
        print(f"guided pass {dtype} scaled s={s}: max abs err {err:.3e} (bound {(1 + 2 * s) * bound:.3e})")
        assert err <= (1 + 2 * s) * bound, s


@pytest.mark.parametrize("S", [1, 23, 128])
@pytest.mark.parametrize("dtype,tol", MODES)
def test_fold_against_the_literal_null_half(golden, hip_option, dtype, tol, S):
    """Option nar_cg_fold 1 (+ c_l) against 0 (encoder attention over S copies of the null key / value, on the device): the null half
    agrees to 2e-6 of the logit scale in f32 -- the rounding of sum_S (1/S) v and of the online softmax's rescaling, a few ulp per
    layer -- and to the mode's decoder bound otherwise; the conditioned half runs the same launches and is bit-identical."""
    g = golden("nar_cg")
    m = model(dtype)
    eng = m.engine
    eng.null_cross(CFG.bos)
    B = 4
    gen = torch.Generator().manual_seed(900 + S)
    enc = torch.randn(S, B, CFG.embed_dim, generator=gen)
    lens = torch.tensor([S, max(1, S // 3), max(1, S - 1), max(1, S // 2)])
    ckv, slen = m._prepared(enc_dict(enc, lens))
    tok = torch.from_numpy(g["s0_i1_tok"]).to(DEV).int().contiguous()  # partly masked, ragged, one row of two tokens
    hip_option("nar_cg_fold", 1)
    on = eng.forward_guided(tok, ckv, slen).cpu()
    hip_option("nar_cg_fold", 0)
    off = eng.forward_guided(tok, ckv, slen).cpu()
    scale = float(off.abs().max())
    err = float((on[1] - off[1]).abs().max())
    bound = 2e-6 * scale if dtype == "f32" else tol * max(1.0, scale / 4)
    print(f"fold vs literal {dtype} S={S}: null half max abs diff {err:.3e} (bound {bound:.3e}, logit scale {scale:.2f})")
    assert torch.equal(on[0], off[0])
    assert err <= bound


def kernel_inputs(T, scale, step, max_step, V=1004, B=3, unk=3, pad=1, eos=2):
    """Random logits and a ragged, partly masked batch whose decisions keep the fixture's margins: the arg-max column of every row
    of the scaled logits is raised (through the conditioned logit), further at the positions to keep until a gap stands at the re-mask boundary;
    the conditions themselves are CHECKED by the caller (nar_cg_ref.margins), not assumed."""
    gen = torch.Generator().manual_seed(1000 * T + int(10 * scale) + step)
    cond, null = torch.randn(B, T, V, generator=gen), torch.randn(B, T, V, generator=gen)
    lens = [T, max(2, T // 2), 2]
    tok = torch.randint(4, V, (B, T), generator=gen)
    for b, n in enumerate(lens):  # as many masked positions as the loop itself leaves for this iteration
        masked = torch.randperm(n - 1, generator=gen)[: n - 1 if step == 0 else int((n - 2) * (1 - step / max_step))]
        tok[b, masked] = unk
        tok[b, n - 1] = eos
        tok[b, n:] = pad
    top = (cond + scale * (cond - null)).argmax(-1, keepdim=True)
    raise_top = lambda rows, by: cond.scatter_add_(2, top, (by * rows / (1 + scale)).unsqueeze(-1))
    raise_top(torch.ones(B, T), 0.25)  # every arg-max clear of its runner-up
    if step + 1 < max_step:  # the positions to keep are raised until a gap stands at the re-mask boundary
        masked = tok.eq(unk)
        score = lambda: torch.where(masked, torch.log_softmax((cond + scale * (cond - null)).double(), -1).max(-1)[0], torch.zeros(B, T, dtype=torch.float64))
        sc = score()
        keep = torch.zeros(B, T)
        for b in range(B):
            filled = torch.where(masked[b], top[b, :, 0], tok[b])  # (the count is taken after the arg-max went in: it may be `pad` itself)
            k = int(float(torch.tensor(float(filled.ne(pad).sum() - 2), dtype=torch.float32) * (1 - (step + 1) / max_step)))
            keep[b, sc[b].sort(stable=True)[1][k:]] = 1.0
        keep = keep * masked
        for _ in range(24):
            sc = score()
            low = torch.where(keep.bool() | ~masked, torch.full_like(sc, -1e9), sc).max(1, keepdim=True)[0]  # the highest score to be re-masked
            todo = keep * (sc < low + 0.05)
            if not bool(todo.any()):
                break
            raise_top(todo, 1.0)
    return cond, null, tok


@pytest.mark.parametrize("T", [2, 5, 33, 257, 2048])
def test_guided_update_kernel(T):
    """dn_cmlm_guided_step alone against the torch restatement on given logits: V = 1004, B = 3 ragged, first / middle / last
    iteration, both scales; tokens and predicted exactly, scores 1e-5 relative + 2e-6.  The logits lie between NaN guards (the two
    halves are contiguous by the ABI, so the guards stand in front of the conditioned half and behind the null half; V = 1004 is
    no multiple of the 64 lanes, so a lane that ran past a row's end would read the next row -- or the guard)."""
    from diffnorm_amd import _lib

    lib = _lib.load()
    B, V, unk, pad, max_step, guard = 3, 1004, 3, 1, 10, 4096
    for scale in (0.5, 3.0):
        for step in (0, 4, 9):
            cond, null, tok = kernel_inputs(T, scale, step, max_step)
            scaled = cond + scale * (cond - null)
            m_arg, gap, zeros = G.margins(scaled, tok, step, max_step, unk, pad)
            assert m_arg >= G.MARGIN and gap >= G.MARGIN and zeros == 0, (T, scale, step, m_arg, gap, zeros)
            ref_tok, ref_sc, ref_pred = G.guided_update(scaled, tok, step, max_step, unk, pad)
            n = B * T * V
            buf = torch.full((2 * n + 2 * guard,), float("nan"), dtype=torch.float32)
            buf[guard: guard + n] = cond.reshape(-1)
            buf[guard + n: guard + 2 * n] = null.reshape(-1)
            buf = buf.to(DEV)
            t_dev = tok.to(DEV).int().contiguous()
            sc_dev = torch.full((B, T), 7.0, device=DEV)  # stale scores: the kernel starts from zero (nat_gen.py:197)
            pred = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
            step_dev = torch.tensor([step], dtype=torch.int32, device=DEV)
            t2, sc2, pred2 = t_dev.clone(), sc_dev.clone(), pred.clone()
            with torch.cuda.device(DEV):
                _lib.check(lib.dn_cmlm_guided_step(buf.data_ptr() + 4 * guard, scale, t_dev.data_ptr(), sc_dev.data_ptr(), pred.data_ptr(), B, T, V, step,
                                                   max_step, unk, pad, _lib.current_stream()), "dn_cmlm_guided_step")
                _lib.check(lib.dn_cmlm_guided_step_dev(buf.data_ptr() + 4 * guard, scale, t2.data_ptr(), sc2.data_ptr(), pred2.data_ptr(), B, T, V,
                                                       step_dev.data_ptr(), max_step, unk, pad, _lib.current_stream()), "dn_cmlm_guided_step_dev")
            for tk, sc, pr in ((t_dev, sc_dev, pred), (t2, sc2, pred2)):
                assert tk.cpu().long().tolist() == ref_tok.tolist(), (T, scale, step)
                assert pr.cpu().long().tolist() == ref_pred.tolist(), (T, scale, step)
                np.testing.assert_allclose(sc.cpu().numpy(), ref_sc.numpy(), rtol=1e-5, atol=2e-6)


def run_loop(m, g, scale, enc=None):
    hist = []
    out = m.guided_mask_predict(enc if enc is not None else fixture_enc(g), torch.from_numpy(g["tgt_lens"]), int(g["n_iters"]), scale,
                                null_token=int(g["null_token"]), history=hist)
    assert torch.equal(out, hist[-1][0])
    return hist


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_guided_mask_predict_reproduces_the_reference(golden, dtype):
    """The loop of nat_gen.py:192-236 on the HIP engine against the REAL classes: tokens and predicted after every iteration exactly,
    at both scales (scores 2e-4, the bound of the unguided loop's), eager; and the replayed graph bit-identical to eager."""
    g = golden("nar_cg")
    for si, scale in enumerate(g["scales"].tolist()):
        eager = run_loop(model(dtype, False), g, scale)
        graph = run_loop(model(dtype, True), g, scale)
        for i, (tok, sc, pred) in enumerate(eager):
            assert tok.cpu().tolist() == g[f"s{si}_i{i}_tok"].tolist(), (scale, i)
            assert pred.cpu().tolist() == g[f"s{si}_i{i}_pred"].tolist(), (scale, i)
            assert np.abs(sc.cpu().numpy() - g[f"s{si}_i{i}_sc"]).max() < 2e-4
            for a, b in zip(eager[i], graph[i]):
                assert torch.equal(a, b), (scale, i)


def test_graph_copies_the_source_on_every_call(golden):
    """Two different encoder outputs of equal (B, T, S) decoded back to back through ONE model with use_graph: each equals its
    eager result (the graph's static keys / values and lengths are refreshed per call, not per address)."""
    g = golden("nar_cg")
    lens = torch.from_numpy(g["src_lens"])
    gen = torch.Generator().manual_seed(77)
    encs = [fixture_enc(g), enc_dict(torch.randn(g["enc_out"].shape, generator=gen), lens.flip(0))]
    for enc in encs + encs[:1]:
        fresh = lambda: {k: list(v) for k, v in enc.items() if not k.startswith("_")}
        graph = run_loop(model("f32", True), g, 3.0, fresh())
        eager = run_loop(model("f32", False), g, 3.0, fresh())
        for i in range(len(eager)):
            for a, b in zip(eager[i], graph[i]):
                assert torch.equal(a, b), i
    assert sum(1 for k in model("f32", True)._graphs if k[5] == 3.0) == 1  # one capture served the three sources


@pytest.mark.parametrize("use_graph", [False, True])
def test_without_a_scale_the_loop_runs_the_conditioned_half_alone(golden, use_graph):
    """cg_scale None / 0 (use_cg = cg_scale > 0): the same loop on engine.forward's logits and the restated update."""
    g = golden("nar_cg")
    m = model("f32", use_graph)
    tgt, n = torch.from_numpy(g["tgt_lens"]), int(g["n_iters"])
    for scale in (None, 0.0):
        hist = run_loop(m, g, scale)
        ckv, slen = m._prepared(fixture_enc(g))
        tok = G.initial_tokens(tgt, CFG)
        for step in range(n):
            logits = m.engine.forward(tok.to(DEV).int().contiguous(), ckv, slen).cpu()
            tok, sc, pred = G.guided_update(logits, tok, step, n, CFG.unk, CFG.pad)
            assert hist[step][0].cpu().tolist() == tok.tolist() and hist[step][2].cpu().tolist() == pred.tolist(), step
            np.testing.assert_allclose(hist[step][1].cpu().numpy(), sc.numpy(), rtol=1e-5, atol=2e-6)


def test_refusals(golden):
    from diffnorm_amd import _lib, nar_decoder

    lib = _lib.load()
    g = golden("nar_cg")
    B, T, V = 2, 4, 8
    lg = torch.zeros(2, B, T, V, device=DEV)
    tok = torch.full((B, T), 3, dtype=torch.int32, device=DEV)
    sc = torch.zeros(B, T, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for scale in (0.0, -0.5):
        assert lib.dn_cmlm_guided_step(lg.data_ptr(), scale, tok.data_ptr(), sc.data_ptr(), tok.data_ptr(), B, T, V, 0, 4, 3, 1, None) == -1
        assert b"scale" in lib.dn_last_error()
        assert lib.dn_cmlm_guided_step_dev(lg.data_ptr(), scale, tok.data_ptr(), sc.data_ptr(), tok.data_ptr(), B, T, V, step.data_ptr(), 4, 3, 1, None) == -1
        assert b"scale" in lib.dn_last_error()
    assert lib.dn_cmlm_guided_step(lg.data_ptr(), 1.0, tok.data_ptr(), sc.data_ptr(), tok.data_ptr(), 1, 2049, V, 0, 4, 3, 1, None) == -1
    assert b"2048" in lib.dn_last_error()
    # a fresh engine: the guided pass before dn_nar_null_cross
    eng = nar_decoder.NarDecoderEngine(sd(), CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV)
    enc = torch.from_numpy(g["enc_out"]).transpose(0, 1).contiguous().to(DEV)
    ckv = eng.cross_kv(enc)
    slen = torch.from_numpy(g["src_lens"]).to(DEV).int()
    t = torch.from_numpy(g["s0_tok_in"]).to(DEV).int().contiguous()
    with pytest.raises(_lib.DiffNormHipError, match="dn_nar_null_cross"):
        eng.forward_guided(t, ckv, slen)
    eng.null_cross(0)
    long = torch.full((1, 2049), 3, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.DiffNormHipError, match="2048"):
        eng.forward_guided(long, ckv[:, :1].contiguous(), slen[:1])
