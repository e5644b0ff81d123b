"""CPU check of dn_conv_gemm's routing (no GPU: the route is host logic): the library reproduces tests/golden/gemm_routes.npz --
tile, K order, shared staged rows and band (dn_conv_gemm_route) and dn_conv_gemm_kblocked_ok for a deterministic sweep of
contractions, forced tiles, twin launches, bands and run-time options, and for the contractions of the eps-predictor's sampling
step as the engines issue them (tools/gen_gemm_routes.py wrote it)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# start-up A/B knobs read once by the route (the suite never sets them); the table is their defaults
ROUTE_ENV = ("DN_GEMM_TILE", "DN_GEMM_HEUR", "DN_352_ROUTE", "DN_X3_192", "DN_BIG_HALO", "DN_FAT_HALO", "DN_GEMM_BAND")


@pytest.fixture(scope="module")
def gen():
    from diffnorm_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    spec = importlib.util.spec_from_file_location("gen_gemm_routes", os.path.join(ROOT, "tools", "gen_gemm_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_routes_reproduce_the_table(gen):
    from diffnorm_amd import _lib

    assert not [v for v in ROUTE_ENV if v in os.environ]
    g = np.load(os.path.join(ROOT, "tests", "golden", "gemm_routes.npz"))
    P, R, engine = g["P"], g["R"], g["engine"]
    assert len(P) > 10000 and engine.sum() > 0
    got = gen.answer_all(_lib.load(), P, engine)
    bad = np.nonzero((got != R).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), P[i][:len(gen.HEAD)].tolist(), R[i].tolist(), got[i].tolist()) for i in bad[:10]]
    # the table covers every tile, both K orders, shared rows and K-blocked shapes
    assert set(R[:, 0]) == {-1, 1, 2, 3, 4, 5, 6, 7, 8, 9} and R[:, 1].any() and R[:, 2].any() and R[:, 4].any()
