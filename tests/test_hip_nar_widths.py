"""The NAR S2UT transformer engines (NarEncoderEngine, NarDecoderEngine) against the float64 restatement of oracle/nar_oracle.py and
tests/nar_cg_ref.py evaluated here: at the recipe's widths (D = 512, FFN 2048, 8 heads of 64, conv_channels 1024; 2 layers, so every
per-layer offset occurs with l = 1) -- where dn_conv_gemm and dn_attention run other kernels than at the fixtures' D = 64 -- and, at the
fixture width, at the edges of the launch geometry: one token, the 64 boundary, the last admitted length, the shortest and the longest
source.  Everything is computed from seeded tensors; engines and references are built once per module."""
import functools

import numpy as np
import pytest
import torch

import conformer_ref as R
import nar_cg_ref as G
import nar_oracle as N
from gen_golden_nar_configs import CFG, ENC_CFG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["f32", "bf16x3", "f16", "bf16"]
ENGINE_TOL = {"f32": 1e-3, "bf16x3": 1e-3, "f16": 1e-2, "bf16": 6e-2}  # test_hip_refine.py's and test_hip_conformer.py's
F32_FACTOR = 8  # f32: within 8 x the error of the same restatement run in float32 on the CPU (another summation order, the device's exp)
WIDE = N.NarConfig(layers=2)  # 512 / 2048 / 8 heads / 1004
WIDE_ENC = N.NarEncoderConfig(layers=2)  # 80 -> 1024 -> 512, kernels 5, 5
B, T, S = 3, 130, 76
TGT_LENS, SRC_LENS = (130, 2, 65), (76, 1, 65)


def _randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).float()


def _double(sd):
    return {k: v.double() for k, v in sd.items()}


def _tokens(lengths, T, seed, cfg=WIDE):
    """Unit ids in [4, vocab), the last one present; about 40 % `unk`; `pad` behind each row's length and nowhere else."""
    rs = np.random.RandomState(seed)
    tok = torch.from_numpy(rs.randint(4, cfg.vocab, (len(lengths), T)))
    tok[torch.from_numpy(rs.random_sample(tok.shape) < 0.4)] = cfg.unk
    tok[0, 0] = cfg.vocab - 1
    return tok.masked_fill(torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None], cfg.pad)


def _conditions(tok, src_lens, S, cfg=WIDE):
    """What the kernels assume of their input, on the reference side: pad only as a suffix, a valid key in every row of both attentions."""
    nonpad = tok.ne(cfg.pad)
    n = nonpad.sum(1)
    assert bool((nonpad == (torch.arange(tok.size(1))[None, :] < n[:, None])).all()), "pad inside a row"
    assert int(n.min()) >= 1 and int(min(src_lens)) >= 1 and int(max(src_lens)) <= S


def _pad_mask(lens, S):
    return torch.arange(S)[None, :] >= torch.as_tensor(lens)[:, None]


def _bar(dtype, ref):
    return ENGINE_TOL[dtype] * max(1.0, float(ref.abs().max()) / 4)


def _report(what, dtype, err, bar, e32=None):
    tail = "" if e32 is None else f"; float32 restatement {e32:.3e}, x{F32_FACTOR} = {F32_FACTOR * e32:.3e}, ratio {err / e32:.2f}"
    print(f"{what} {dtype}: max abs err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}{tail}")


# ------------------------------------------------------------------------------------------------------------- decoder at the recipe's widths
@functools.lru_cache(maxsize=None)
def _wide():
    """Weights, the batch of sections 1-3 and its float64 references (and the float32 restatement's distance from them) -- once."""
    sd = N.make_nar_state_dict(WIDE, "nar-widths")
    sd64 = _double(sd)
    tok = _tokens(TGT_LENS, T, 4101)
    assert int(tok.max()) == WIDE.vocab - 1 and 0.3 < float(tok.eq(WIDE.unk).sum()) / sum(TGT_LENS) < 0.5
    _conditions(tok, SRC_LENS, S)
    enc = _randn(4102, B, S, WIDE.embed_dim)
    pad = _pad_mask(SRC_LENS, S)
    valid = tok.ne(WIDE.pad)
    with torch.no_grad():
        cond = N.decoder_logits(sd64, WIDE, tok, enc.double().transpose(0, 1), pad, normalize=False)
        null = G.null_logits(sd64, WIDE, tok, S, WIDE.bos)
        e32_cond = float((N.decoder_logits(sd, WIDE, tok, enc.transpose(0, 1), pad, normalize=False).double() - cond)[valid].abs().max())
        e32_null = float((G.null_logits(sd, WIDE, tok, S, WIDE.bos).double() - null)[valid].abs().max())
    return dict(sd=sd, sd64=sd64, tok=tok, enc=enc, pad=pad, valid=valid, cond=cond, null=null, e32_cond=e32_cond, e32_null=e32_null)


@functools.lru_cache(maxsize=None)
def _wide_engine(dtype):
    from diffnorm_amd import nar_decoder

    return nar_decoder.NarDecoderEngine(_wide()["sd"], layers=WIDE.layers, dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _wide_pass(dtype):
    """The plain pass of section 1 on the device (shared by the guided test's bit comparison)."""
    w, eng = _wide(), _wide_engine(dtype)
    slen = torch.tensor(SRC_LENS, dtype=torch.int32, device=DEV)
    tok = w["tok"].to(DEV).int().contiguous()
    ckv = eng.cross_kv(w["enc"].to(DEV))
    return tok, ckv, slen, eng.forward(tok, ckv, slen).clone()


@pytest.mark.parametrize("dtype", MODES)
def test_decoder_pass_at_the_recipe_widths(dtype):
    """dn_nar_cross_kv (grouped over the layers) + dn_nar_decoder_forward at D = 512: B = 3, T = 130, S = 76, target lengths 130 / 2 / 65
    and source lengths 76 / 1 / 65 -- several query and key tiles in both attentions, the loop's shortest row, a length on each side of
    64, a source of one frame.  Logits on the non-pad positions against float64; f32 also within 8 x the float32 restatement's error."""
    w = _wide()
    got = _wide_pass(dtype)[3].cpu().double()
    err = float((got - w["cond"])[w["valid"]].abs().max())
    bar = _bar(dtype, w["cond"][w["valid"]])
    _report(f"NAR decoder, recipe widths (logit scale {float(w['cond'][w['valid']].abs().max()):.2f}),", dtype, err, bar, w["e32_cond"] if dtype == "f32" else None)
    assert bool(torch.isfinite(got[w["valid"]]).all()) and err <= bar
    if dtype == "f32":
        assert err <= F32_FACTOR * w["e32_cond"]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_guided_pass_at_the_recipe_widths(dtype):
    """dn_nar_null_cross + dn_nar_decoder_forward_guided on the same batch: the conditioned half is the plain pass bit for bit, the null
    half matches the float64 cg_forward restatement under the bars of the plain pass, and cond + 2 (cond - null) stays within
    (1 + 2 * 2) pass bars of the float64 halves' (three terms, each within the pass bar)."""
    w, eng = _wide(), _wide_engine(dtype)
    tok, ckv, slen, plain = _wide_pass(dtype)
    eng.null_cross(WIDE.bos)
    both = eng.forward_guided(tok, ckv, slen)
    assert torch.equal(both[0], plain)
    v = w["valid"]
    err = float((both[1].cpu().double() - w["null"])[v].abs().max())
    bar = _bar(dtype, w["null"][v])
    _report(f"NAR decoder, recipe widths, null half (logit scale {float(w['null'][v].abs().max()):.2f}),", dtype, err, bar, w["e32_null"] if dtype == "f32" else None)
    assert err <= bar
    if dtype == "f32":
        assert err <= F32_FACTOR * w["e32_null"]
    s = 2.0
    want = w["cond"] + s * (w["cond"] - w["null"])
    got = eng.guided_logits(tok, ckv, slen, s).cpu().double()
    err = float((got - want)[v].abs().max())
    bar = (1 + 2 * s) * ENGINE_TOL[dtype] * max(1.0, float(max(w["cond"][v].abs().max(), w["null"][v].abs().max())) / 4)
    _report("NAR decoder, recipe widths, cond + 2 (cond - null),", dtype, err, bar)
    assert err <= bar


def test_length_predictor_at_the_recipe_width():
    """dn_nar_predict_lengths (masked mean + 256-way arg-max, fp32 in every mode) against float64 on a batch with src_len = 1 and
    src_len = S: exact, and the same integers from the f32 and the bf16 engine.  The float64 logits keep a top-2 margin of at least
    1e-3 x their scale in every row (asserted here, on the reference)."""
    w = _wide()
    assert 1 in SRC_LENS and S in SRC_LENS
    enc64 = w["enc"].double().transpose(0, 1)
    keep = (~w["pad"]).double()
    pooled = (enc64.transpose(0, 1) * keep[:, :, None]).sum(1) / keep.sum(1, keepdim=True)
    logits = pooled @ w["sd64"]["embed_length.weight"].t()
    top = logits.topk(2, -1)[0]
    margin, scale = top[:, 0] - top[:, 1], float(logits.abs().max())
    print(f"length predictor: top-2 margins {[round(float(m), 4) for m in margin]} at logit scale {scale:.2f}")
    assert float(margin.min()) >= 1e-3 * scale
    want = N.predict_lengths(w["sd64"], enc64, w["pad"])
    assert want.tolist() == logits.argmax(-1).tolist()
    slen = torch.tensor(SRC_LENS, dtype=torch.int32, device=DEV)
    got = {dtype: _wide_engine(dtype).predict_lengths(w["enc"].to(DEV), slen).cpu().tolist() for dtype in ("f32", "bf16")}
    assert got["f32"] == want.tolist() and got["bf16"] == got["f32"]


# ------------------------------------------------------------------------------------------------------------- decoder launch-geometry edges
@functools.lru_cache(maxsize=None)
def _fixture_sd():
    sd = N.make_nar_state_dict(CFG, "nar")
    return sd, _double(sd)


@functools.lru_cache(maxsize=None)
def _fixture_engine():
    from diffnorm_amd import nar_decoder

    return nar_decoder.NarDecoderEngine(_fixture_sd()[0], CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV)


@functools.lru_cache(maxsize=None)
def _edge_case(T, S):
    """B = 2: a full row and a row of target length 2 (1 at T = 1) and source length 1; tokens, encoder output, float64 logits."""
    tlens, slens = (T, min(2, T)), (S, 1)
    tok = _tokens(tlens, T, 5000 + 7 * T + S, CFG)
    _conditions(tok, slens, S, CFG)
    enc = _randn(5001 + 7 * T + S, 2, S, CFG.embed_dim)
    with torch.no_grad():
        want = N.decoder_logits(_fixture_sd()[1], CFG, tok, enc.double().transpose(0, 1), _pad_mask(slens, S), normalize=False)
    return tok, enc, slens, want


def _run_edge(eng, T, S):
    tok, enc, slens, _ = _edge_case(T, S)
    return eng.forward(tok.to(DEV).int().contiguous(), eng.cross_kv(enc.to(DEV)), torch.tensor(slens, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("T,S", [(1, 1), (2, 1), (63, 64), (64, 65), (65, 63), (257, 130), (1024, 3)])
def test_decoder_edges_of_the_launch_geometry(T, S):
    """The fixture width (D = 64), f32: one token and one frame, both sides of the 64 boundary, several tiles of both, and T = 1024 --
    the last length max_pos = 1026 admits: the last row of the sinusoidal table, half of the embedding kernel's position array."""
    tok, _, _, want = _edge_case(T, S)
    got = _run_edge(_fixture_engine(), T, S).cpu().double()
    v = tok.ne(CFG.pad)
    err, bar = float((got - want)[v].abs().max()), _bar("f32", want[v])
    _report(f"NAR decoder edge T={T} S={S}", "f32", err, bar)
    assert bool(torch.isfinite(got[v]).all()) and err <= bar


def test_decoder_refuses_a_length_beyond_the_positional_table():
    """T = 1025 needs row 1026 of a 1026-row table: DiffNormHipError, and nothing is launched (the output keeps its contents)."""
    from diffnorm_amd import _lib

    eng = _fixture_engine()
    Tbad = 1025
    tok = torch.full((2, Tbad), CFG.unk, dtype=torch.int32, device=DEV)
    ckv = eng.cross_kv(_randn(5002, 2, 3, CFG.embed_dim).to(DEV))
    out = torch.full((2, Tbad, CFG.vocab), 7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.DiffNormHipError):
        eng.forward(tok, ckv, torch.tensor([3, 1], dtype=torch.int32, device=DEV), out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_decoder_workspace_regrowth_leaves_the_result_alone():
    """One engine of its own: the (257, 130) case grows the workspace, (2, 1) runs in a corner of it, (257, 130) again reuses it -- the
    first and the third result are the same bits, and both are the float64 reference's within the bar."""
    from diffnorm_amd import nar_decoder

    eng = nar_decoder.NarDecoderEngine(_fixture_sd()[0], CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV)
    first = _run_edge(eng, 257, 130).clone()
    n = eng._ws.numel()
    small = _run_edge(eng, 2, 1).cpu().double()
    third = _run_edge(eng, 257, 130)
    assert eng._ws.numel() == n and torch.equal(first, third)
    for (T_, S_), got in (((257, 130), third.cpu().double()), ((2, 1), small)):
        tok, _, _, want = _edge_case(T_, S_)
        v = tok.ne(CFG.pad)
        assert float((got - want)[v].abs().max()) <= _bar("f32", want[v])


# ------------------------------------------------------------------------------------------------------------- speech encoder
@functools.lru_cache(maxsize=None)
def _wide_enc():
    """Recipe widths, 2 layers: B = 2, L = 301, lengths 301 / 170 -> S = 76, output lengths 76 / 43; float64 and the float32 restatement."""
    sd = N.make_nar_encoder_state_dict(WIDE_ENC, "narenc-widths")
    feats, lens = R.make_features(2, 301, (301, 170), WIDE_ENC.input_dim, 4201)
    with torch.no_grad():
        want, pad, ol = N.encoder_forward(_double(sd), WIDE_ENC, feats.double(), lens)
        want = want.transpose(0, 1)  # [S, B, D] -> [B, S, D]
        e32 = float((N.encoder_forward(sd, WIDE_ENC, feats, lens)[0].transpose(0, 1).double() - want)[~pad].abs().max())
    assert want.shape[1] == 76 and ol.tolist() == [76, 43]
    return sd, feats, lens, want, pad, ol, e32


@functools.lru_cache(maxsize=None)
def _wide_enc_engine(dtype):
    from diffnorm_amd import nar_decoder

    return nar_decoder.NarEncoderEngine(_wide_enc()[0], layers=WIDE_ENC.layers, dtype=dtype, device=DEV)


@pytest.mark.parametrize("dtype", MODES)
def test_speech_encoder_at_the_recipe_widths(dtype):
    """dn_nar_encoder_forward at 80 -> 1024 -> 512 (first gather padded to K0 = padk(400), second contraction K = 2560), FFN 2048, 8 heads
    of 64: valid frames against float64, output lengths exact; f32 also within 8 x the float32 restatement's error."""
    _, feats, lens, want, pad, ol, e32 = _wide_enc()
    out, got_l = _wide_enc_engine(dtype).forward(feats.to(DEV), lens.to(DEV))
    assert got_l.cpu().tolist() == ol.tolist() and out.shape == want.shape
    err, bar = float((out.cpu().double() - want)[~pad].abs().max()), _bar(dtype, want[~pad])
    _report(f"NAR speech encoder, recipe widths (output scale {float(want[~pad].abs().max()):.2f}),", dtype, err, bar, e32 if dtype == "f32" else None)
    assert err <= bar
    if dtype == "f32":
        assert err <= F32_FACTOR * e32


@functools.lru_cache(maxsize=None)
def _fixture_enc_sd():
    sd = N.make_nar_encoder_state_dict(ENC_CFG, "narenc")
    return sd, _double(sd)


@functools.lru_cache(maxsize=None)
def _fixture_enc_engine(max_pos=6002):
    from diffnorm_amd import nar_decoder

    E = ENC_CFG
    return nar_decoder.NarEncoderEngine(_fixture_enc_sd()[0], E.input_dim, E.conv_channels, E.kernel_sizes[0], E.embed_dim, E.ffn_dim, E.layers, E.heads,
                                        max_pos=max_pos, dtype="f32", device=DEV)


def _check_fixture_encoder(what, feats, lens):
    with torch.no_grad():
        want, pad, ol = N.encoder_forward(_fixture_enc_sd()[1], ENC_CFG, feats.double(), lens)
    want = want.transpose(0, 1)
    assert int(ol.min()) >= 1  # no row without a valid key
    out, got_l = _fixture_enc_engine().forward(feats.to(DEV), lens.to(DEV))
    assert got_l.cpu().tolist() == ol.tolist() and out.shape == want.shape
    err, bar = float((out.cpu().double() - want)[~pad].abs().max()), _bar("f32", want[~pad])
    _report(what, "f32", err, bar)
    assert bool(torch.isfinite(out).all()) and err <= bar


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8, 9])
def test_speech_encoder_shortest_sources(L):
    """The fixture width, f32, B = 2 with lengths L and max(1, L - 2): both parities of both stride-2 layers, the one-frame output, and
    frames behind an utterance's end taking part in the subsampler as upstream.  Lengths exact, valid frames within the bar."""
    feats, lens = R.make_features(2, L, (L, max(1, L - 2)), ENC_CFG.input_dim, 4300 + L)
    _check_fixture_encoder(f"NAR speech encoder L={L}", feats, lens)


def test_speech_encoder_longest_source():
    """B = 1, L = 6000: S = 1500 frames, the longest source max_pos = 6002 is sized for, against float64 on every frame."""
    feats, lens = R.make_features(1, 6000, (6000,), ENC_CFG.input_dim, 4400)
    _check_fixture_encoder("NAR speech encoder L=6000", feats, lens)


def test_speech_encoder_refuses_a_source_beyond_the_positional_table():
    """L = 100 is 25 frames; a table of 20 rows does not hold their positions: refused before anything is launched."""
    from diffnorm_amd import _lib

    feats, lens = R.make_features(1, 100, (100,), ENC_CFG.input_dim, 4500)
    with pytest.raises(_lib.DiffNormHipError):
        _fixture_enc_engine(20).forward(feats.to(DEV), lens.to(DEV))


# ------------------------------------------------------------------------------------------------------------- encoder -> decoder at width
def test_encoder_output_feeds_the_decoder_at_the_recipe_widths():
    """f32, two layers each: the encoder's fp32 [B, S, 512] output and its out_lengths go straight into dn_nar_cross_kv and the decoder
    pass; float64 decoder_logits on the float64 encoder_forward output, masked by the reference's own lengths."""
    w = _wide()
    _, feats, lens, enc64, pad, ol, _ = _wide_enc()
    tok = _tokens((130, 65), T, 4601)
    _conditions(tok, ol.tolist(), enc64.shape[1])
    with torch.no_grad():
        want = N.decoder_logits(w["sd64"], WIDE, tok, enc64.transpose(0, 1), pad, normalize=False)
    enc, slen = _wide_enc_engine("f32").forward(feats.to(DEV), lens.to(DEV))
    eng = _wide_engine("f32")
    got = eng.forward(tok.to(DEV).int().contiguous(), eng.cross_kv(enc), slen).cpu().double()
    v = tok.ne(WIDE.pad)
    err, bar = float((got - want)[v].abs().max()), _bar("f32", want[v])
    _report(f"NAR encoder -> decoder, recipe widths (logit scale {float(want[v].abs().max()):.2f}),", "f32", err, bar)
    assert err <= bar
