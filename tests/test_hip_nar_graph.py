"""The captured iteration under both mask-predict loops (diffnorm_amd/nar_decoder.py, _IterationGraph) against the eager, host-stepped
paths of a second model on the same weights: back-to-back utterance batches whose encoder keys / values may land on one address, a
re-ordered batch, a later larger call that re-allocates the engine's workspace, and the one bounded cache.  f32, the fixture model;
both models run the same kernels on the same inputs, so every comparison is torch.equal on tokens, scores and predicted."""
import gc

import pytest
import torch

import nar_oracle as N
from gen_golden_nar_configs import CFG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def build(use_graph):
    from diffnorm_amd import nar_decoder

    if "sd" not in _cache:
        _cache["sd"] = N.make_nar_state_dict(CFG, "nar")
    return nar_decoder.NARS2UTDecoderModel(_cache["sd"], CFG.embed_dim, CFG.ffn_dim, CFG.layers, CFG.heads, CFG.vocab, dtype="f32", device=DEV,
                                           use_graph=use_graph)


def model(use_graph):
    if use_graph not in _cache:
        _cache[use_graph] = build(use_graph)
    return _cache[use_graph]


def enc_dict(enc_sbd, lens=None):
    pad = [(torch.arange(enc_sbd.size(0))[None, :] >= lens[:, None]).to(DEV)] if lens is not None else []
    return {"encoder_out": [enc_sbd.to(DEV)], "encoder_padding_mask": pad, "encoder_embedding": [], "encoder_states": [], "src_tokens": [],
            "src_lengths": []}


def sources(g):
    """The fixture's encoder output and a seeded random one of the same (B, S) with the source lengths the other way round; the
    target lengths of the fixture's tokens (ragged, T = 31)."""
    lens = torch.from_numpy(g["src_lens"])
    gen = torch.Generator().manual_seed(41)
    a = lambda: enc_dict(torch.from_numpy(g["enc_out"]), lens)
    rnd = torch.randn(g["enc_out"].shape, generator=gen)
    b = lambda: enc_dict(rnd, lens.flip(0))
    return a, b, torch.from_numpy(g["tokens"]).ne(CFG.pad).sum(1)


def iterate(m, enc, tgt, steps, max_step, state=None):
    """forward_decoder for every step of `steps` -> the last state and (tokens, scores, predicted) after each."""
    st = state if state is not None else m.initialize_output_tokens(enc, None, true_length=tgt)
    outs = []
    for step in steps:
        st = m.forward_decoder(st._replace(step=step, max_step=max_step, history=[]), enc)
        outs.append((st.output_tokens, st.output_scores, st.history[0]))
    return st, outs


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("tokens", "scores", "predicted"), a, b):
            assert torch.equal(x, y), (what, i, name)


def the_graph(m, B, T, S, max_step):
    return m._graphs[(False, B, T, S, max_step, None)]


def test_back_to_back_batches_through_forward_decoder_and_refine(golden):
    """Two different encoder outputs of equal (B, S) and target lengths, the first one's dict dropped before the second is prepared
    (the allocator may hand its keys / values the same address): every iteration on the second equals eager on the second."""
    a, b, tgt = sources(golden("nar_decoder"))
    mg, me = model(True), model(False)
    for name, run in (("forward_decoder", lambda m, enc: iterate(m, enc, tgt, range(3), 3)),
                      ("refine", lambda m, enc: (None, [m.refine(m.initialize_output_tokens(enc, None, true_length=tgt)._replace(step=0, max_step=3), enc, 3)]))):
        addr = []
        for src in (a, b):
            enc = src()
            got = run(mg, enc)[1]
            addr.append(enc["_ckv"].data_ptr())
            if name == "refine":  # tokens and scores of the state after three iterations, predicted from the graph's buffer
                B, T = got[0].output_tokens.shape
                got = [(got[0].output_tokens, got[0].output_scores, the_graph(mg, B, T, enc["_ckv"].shape[2], 3).predicted.long())]
            want = iterate(me, src(), tgt, range(3), 3)[1]
            same(got, want[-len(got):], (name, "first" if src is a else "second"))
            del enc
            gc.collect()
        print(f"{name}: the second batch's keys / values {'landed on' if addr[0] == addr[1] else 'did not land on'} the first one's address")


def test_reordered_batch(golden):
    """One iteration, then the generator's re-ordering (B unchanged: the same cached graph serves it): the next iteration equals
    eager on the re-ordered source, and the re-ordered dict is a new source."""
    a, _, tgt = sources(golden("nar_decoder"))
    mg, me = model(True), model(False)
    order = torch.tensor([2, 0, 3, 1], device=DEV)
    outs = []
    for m in (mg, me):
        enc = a()
        st, _ = iterate(m, enc, tgt, [0], 3)
        enc2 = m.encoder.reorder_encoder_out(enc, order)
        assert enc2["_src_id"] != enc["_src_id"] and not torch.equal(enc2["_ckv"], enc["_ckv"])
        st = st._replace(output_tokens=st.output_tokens.index_select(0, order), output_scores=st.output_scores.index_select(0, order))
        outs.append(iterate(m, enc2, tgt, [1], 3, state=st)[1])
    same(outs[0], outs[1], "reordered")
    assert sum(1 for k in mg._graphs if k[:5] == (False, 4, int(tgt.max()), 23, 3)) == 1


def test_a_larger_later_call_does_not_reach_the_captured_iteration(golden):
    """The captured small iteration keeps its own workspace: after a larger batch made the engine re-allocate its shared one, the
    same graph object decodes another small source and equals eager."""
    a, b, tgt = sources(golden("nar_decoder"))
    mg, me = build(True), model(False)
    eng = mg.engine
    B, T, S = 4, 40, 64
    small = int(eng.lib.dn_nar_workspace_bytes(eng.handle, 4, int(tgt.max()), 23))
    assert int(eng.lib.dn_nar_workspace_bytes(eng.handle, B, T, S)) > small
    same(iterate(mg, a(), tgt, range(2), 4)[1], iterate(me, a(), tgt, range(2), 4)[1], "before")
    g0 = the_graph(mg, 4, int(tgt.max()), 23, 4)
    captured, ws0 = g0.graph, eng._ws.data_ptr()
    assert captured is not None and len(mg._graphs) == 1
    gen = torch.Generator().manual_seed(43)
    big, big_tgt = torch.randn(S, B, CFG.embed_dim, generator=gen), torch.tensor([T, 17, 2, 33])
    same(iterate(mg, enc_dict(big), big_tgt, [0], 4)[1], iterate(me, enc_dict(big), big_tgt, [0], 4)[1], "larger")
    print(f"engine workspace {'moved' if eng._ws.data_ptr() != ws0 else 'stayed'}; {eng._ws.numel()} bytes now, the small pass needs {small}")
    same(iterate(mg, b(), tgt, range(2), 4)[1], iterate(me, b(), tgt, range(2), 4)[1], "after")
    assert the_graph(mg, 4, int(tgt.max()), 23, 4) is g0 and g0.graph is captured and len(mg._graphs) == 2


def test_one_bounded_cache(golden):
    """Both loops share one cache: one entry per distinct (kind, shape, n_iters, scale) used, never more than 16, oldest out."""
    a, b, tgt = sources(golden("nar_decoder"))
    c = golden("nar_cg")
    mg, me = build(True), model(False)
    T = int(tgt.max())
    for src in (a, b):
        enc = src()
        st, _ = iterate(mg, enc, tgt, range(3), 3)
        mg.refine(st._replace(step=0, max_step=3), enc, 3)
        iterate(mg, mg.encoder.reorder_encoder_out(enc, torch.tensor([1, 0, 3, 2], device=DEV)), tgt, [1], 3, state=st)
    iterate(mg, a(), tgt, range(2), 4)
    iterate(mg, enc_dict(torch.randn(64, 4, CFG.embed_dim, generator=torch.Generator().manual_seed(43))), torch.tensor([40, 17, 2, 33]), [0], 4)
    cg_enc = lambda: enc_dict(torch.from_numpy(c["enc_out"]), torch.from_numpy(c["src_lens"]))
    cg_tgt, n = torch.from_numpy(c["tgt_lens"]), int(c["n_iters"])
    for scale in (3.0, None, 3.0, None):
        mg.guided_mask_predict(cg_enc(), cg_tgt, n, scale, null_token=int(c["null_token"]))
    Tc = int(cg_tgt.max()) + 1
    want = {(False, 4, T, 23, 3, None), (False, 4, T, 23, 4, None), (False, 4, 40, 64, 4, None), (True, 4, Tc, 23, n, 3.0), (True, 4, Tc, 23, n, None)}
    assert len(mg._graphs) == len(want) and {k[:6] for k in mg._graphs} == want
    first = next(iter(mg._graphs))
    for max_step in range(5, 18):  # 13 more shapes of the loop: 18 keys asked for in all
        got = iterate(mg, a(), tgt, [0], max_step)[1]
        assert len(mg._graphs) <= 16
    assert len(mg._graphs) == 16 and first not in mg._graphs and (False, 4, T, 23, 17, None) in mg._graphs
    same(got, iterate(me, a(), tgt, [0], 17)[1], "after eviction")
