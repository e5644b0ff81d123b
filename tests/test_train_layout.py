"""CPU check of the training engines' flat-buffer layout (no GPU: dn_{vae,eps}_train_create / _param_count / _aux_bytes / _offsets /
_stage_range / _workspace_bytes are host logic): the library reproduces tests/golden/train_layout.npz -- parameter count, aux
bytes, every packed tensor's offset, every backward stage's gradient range and the workspace size at five batch shapes (the eps
engine's with and without the frozen VAE), for the tiny, smoke, recipe and two odd configs in f32 and bf16.

The table was generated ONCE, by tools/gen_train_layout.py on the commit before the two engines were moved onto one flat-parameter
core, so it pins the byte layout that refactor had to keep.  Regenerate it only for a change that is meant to move the layout."""
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


def test_layout_reproduces_the_table(gen):
    from diffnorm_amd import _lib

    assert not [v for v in gen.WGRAD_ENV if v in os.environ]  # read once by plan_wgrad; they change workspace_bytes
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_layout.npz"))
    names, CFG = g["names"], g["CFG"]
    want_names, want_cfg = gen.build()
    assert list(names) == want_names and np.array_equal(CFG, want_cfg)  # the generator still describes the stored rows
    assert np.array_equal(g["shapes"], np.array(gen.SHAPES))
    assert len(CFG) == 20 and set(CFG[:, 0]) == {gen.VAE, gen.EPS} and set(CFG[:, 1]) == {_lib.DN_F32, _lib.DN_BF16}
    lib = _lib.load()
    for i, name in enumerate(names):
        got = gen.measure(lib, CFG, i)
        for k, v in got.items():
            want = g[f"{k}_{i}"]
            assert v.shape == want.shape and np.array_equal(v, want), (str(name), k, want.tolist()[:8], v.tolist()[:8])
        depth = int(CFG[i][gen.COLS.index("depth")])
        assert got["stages"].shape == (depth + 3, 2) and got["ws"].shape[0] == len(gen.SHAPES) and (got["ws"] > 0).all()
        # the Python table of packed tensors has one entry per offset the library reports
        assert len(gen.entries(CFG[i])) == int(got["head"][2]) == len(got["offsets"]), str(name)
        # the stages tile the whole buffer, back to front
        assert int(got["stages"][:, 1].sum()) == int(got["head"][0]) and int(got["stages"][-1, 0]) == 0
