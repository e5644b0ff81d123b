"""Classifier-free-guided mask-predict decoding (research/TranSpeech/nat_gen.py:192-236, cg_forward nar_transformer.py:123-183) on the
CPU: the restatement tests/nar_cg_ref.py against what the REAL classes wrote (tests/golden/nar_cg.npz), the algebra that makes the
null half's encoder attention one constant row per layer, and the C-ABI names of the feature."""
import os
import re

import numpy as np
import pytest
import torch

import nar_cg_ref as G
import nar_oracle as N
from gen_golden_nar_configs import CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dn_nar_null_cross_bytes", "dn_nar_null_cross", "dn_nar_null_table", "dn_nar_guided_workspace_bytes", "dn_nar_decoder_forward_guided",
       "dn_cmlm_guided_step", "dn_cmlm_guided_step_dev"]


@pytest.fixture(scope="module")
def sd():
    return N.make_nar_state_dict(CFG, "nar")


def fixture_inputs(g):
    lens = torch.from_numpy(g["src_lens"])
    enc = torch.from_numpy(g["enc_out"])
    pad = torch.arange(enc.size(0))[None, :] >= lens[:, None]
    return enc, pad, torch.from_numpy(g["tgt_lens"])


def test_restatement_reproduces_the_real_classes(golden, sd):
    g = golden("nar_cg")
    enc, pad, tgt = fixture_inputs(g)
    assert int(tgt.min()) == 1 and int(g["null_token"]) == CFG.bos
    n = int(g["n_iters"])
    for si, scale in enumerate(g["scales"].tolist()):
        hist, (cond, null) = G.guided_mask_predict(sd, CFG, enc, pad, tgt, n, scale)
        if si == 0:
            for name, got in (("cond0", cond), ("null0", null)):
                err = float((got - torch.from_numpy(g[name])).abs().max())
                print(f"{name}: max abs err {err:.3e}")
                assert err <= 5e-5
        for i, (tok, sc, pred) in enumerate(hist):
            assert tok.tolist() == g[f"s{si}_i{i}_tok"].tolist(), (scale, i)
            assert pred.tolist() == g[f"s{si}_i{i}_pred"].tolist(), (scale, i)
            np.testing.assert_allclose(sc.numpy(), g[f"s{si}_i{i}_sc"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("S", [1, 7, 64])
def test_encoder_attention_over_a_null_source_is_one_constant_row(sd, S):
    """The algebra: S equal keys / values -> a uniform softmax -> every query's output is c_l, whatever the query, S and the batch."""
    c = G.null_rows(sd, CFG)
    g = torch.Generator().manual_seed(5 + S)
    q = torch.randn(3, 11, CFG.embed_dim, generator=g) * 2
    mem = sd["embed_tokens.weight"][CFG.bos][None, None, :].expand(3, S, -1).contiguous()
    for l in range(CFG.layers):
        out = N._attention(sd, f"layers.{l}.encoder_attn.", q, mem, None, CFG.heads)
        err = float((out.double() - c[l]).abs().max() / c[l].abs().max())
        assert err <= 1e-6, (l, S, err)


def test_new_entries_are_declared_and_bound():
    from diffnorm_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffnorm_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
    lib = _lib.load()
    with _lib.option("nar_cg_fold", 0):
        assert _lib.get_option("nar_cg_fold") == 0
    assert lib.dn_nar_guided_workspace_bytes(None, 1, 1, 1) == 0 and lib.dn_nar_null_cross_bytes(None) == 0
    z = torch.zeros(8, dtype=torch.int32)  # host memory: both calls must be refused before any launch
    f = torch.ones(2 * 8, dtype=torch.float32)
    for scale in (0.0, -1.0):
        assert lib.dn_cmlm_guided_step(f.data_ptr(), scale, z.data_ptr(), f.data_ptr(), z.data_ptr(), 1, 2, 4, 0, 4, 3, 1, None) == -1
        assert b"scale" in lib.dn_last_error()
    assert lib.dn_cmlm_guided_step(f.data_ptr(), 1.0, z.data_ptr(), f.data_ptr(), z.data_ptr(), 1, 2049, 4, 0, 4, 3, 1, None) == -1
    assert b"2048" in lib.dn_last_error()
