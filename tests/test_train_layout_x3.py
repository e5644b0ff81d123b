"""CPU check of the split-operand (bf16x3) VAE training engine's flat-buffer layout (no GPU: create / param_count / aux_bytes /
offsets / stage_range / workspace_bytes are host logic).  For every VAE row of tests/golden/train_layout.npz the bf16x3 engine has the
f32 row's parameter count, offsets and stage ranges (the packed layout does not depend on the arithmetic), the f32 row's aux bytes
(esize(DN_BF16X3) is 4: a split-row element takes the bytes of an fp32 one), every packed tensor on a 32-element boundary (split rows
are laid out per 32 elements) and positive workspace sizes no smaller than the f32 row's.  The diffusion engine refuses bf16x3."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gen():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    spec = importlib.util.spec_from_file_location("gen_train_layout", os.path.join(ROOT, "tools", "gen_train_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_x3_vae_layout_equals_the_f32_rows(gen):
    from diffnorm_amd import _lib

    assert not [v for v in gen.WGRAD_ENV if v in os.environ]
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_layout.npz"))
    names, CFG = g["names"], g["CFG"]
    lib = _lib.load()
    rows = [i for i in range(len(CFG)) if CFG[i][0] == gen.VAE and CFG[i][1] == _lib.DN_F32]
    assert len(rows) == 6
    for i in rows:
        row = CFG.copy()
        row[i, 1] = _lib.DN_BF16X3
        got = gen.measure(lib, row, i)
        name = str(names[i])
        for k in ("head", "offsets", "stages"):  # head = (param_count, aux_bytes, number of offsets)
            want = g[f"{k}_{i}"]
            assert got[k].shape == want.shape and np.array_equal(got[k], want), (name, k, want.tolist()[:8], got[k].tolist()[:8])
        assert (got["offsets"] % 32 == 0).all(), (name, got["offsets"][got["offsets"] % 32 != 0].tolist())
        assert int(got["head"][0]) % 32 == 0, name
        want_ws = g[f"ws_{i}"]
        assert got["ws"].shape == want_ws.shape and (got["ws"] > 0).all() and (got["ws"] >= want_ws).all(), (name, got["ws"].tolist(), want_ws.tolist())


def test_x3_diffusion_engine_is_refused(gen):
    from diffnorm_amd import _lib

    lib = _lib.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_layout.npz"))
    CFG = g["CFG"]
    i = next(i for i in range(len(CFG)) if CFG[i][0] == gen.EPS and CFG[i][1] == _lib.DN_F32)
    row = CFG.copy()
    row[i, 1] = _lib.DN_BF16X3
    with pytest.raises(_lib.DiffNormHipError, match="VAE"):
        gen.Handle(lib, row[i])


def test_host_dtype_gate():
    """training._training_dtype: the VAE engine takes bf16x3, the diffusion engine names the VAE as the one x3 training engine."""
    from diffnorm_amd import _lib, training

    assert training._training_dtype("bf16x3", split_ok=True) == _lib.DN_BF16X3
    assert training._training_dtype("f32") == _lib.DN_F32 and training._training_dtype("bf16") == _lib.DN_BF16
    with pytest.raises(ValueError, match="VAE training engine is the one bf16x3 training engine"):
        training._training_dtype("bf16x3")
    with pytest.raises(ValueError):
        training._training_dtype("f16", split_ok=True)
