"""Host side of diffnorm_amd/metrics.py (no GPU): the restatement the device is held to (tests/edit_distance_ref.py), ErrorRate's
arithmetic, the tokenisation of wer / cer, the argument checks that refuse a call before anything is launched, and
normalize.reduce_token against the numpy restatement of dn_reduce_units' four outputs."""
import math

import numpy as np
import pytest
import torch

import edit_distance_ref as R


def test_vectorised_and_loop_forms_agree():
    rng = np.random.RandomState(0)
    for case in range(200):
        alphabet = (2, 4, 1004)[case % 3]
        a, b = (rng.randint(0, alphabet, size=rng.randint(0, 65)) for _ in range(2))
        assert R.edit_distance(a, b) == R.edit_distance_loop(a.tolist(), b.tolist()), (a.tolist(), b.tolist())


def test_textbook_cases():
    codes = lambda s: [ord(c) for c in s]
    for a, b, want in (("kitten", "sitting", 3), ("flaw", "lawn", 2), ("", "abc", 3), ("abc", "", 3), ("", "", 0), ("abc", "abc", 0)):
        assert R.edit_distance(codes(a), codes(b)) == want == R.edit_distance_loop(codes(a), codes(b)), (a, b)


def test_error_rate_arithmetic_and_empty_references():
    from diffnorm_amd.metrics import ErrorRate

    er = ErrorRate([1, 0, 3, 2], [4, 5, 0, 0], [4, 5, 3, 2])
    assert (er.total_errors, er.total_ref_len, er.total_hyp_len) == (6, 9, 14) and er.rate == 6 / 9
    assert er.item_rates[:2] == [0.25, 0.0] and all(math.isinf(r) for r in er.item_rates[2:])
    empty = ErrorRate([0, 2], [0, 0], [0, 2])
    assert empty.item_rates[0] == 0.0 and math.isinf(empty.item_rates[1])
    with pytest.raises(ValueError, match="references are empty"):
        empty.rate
    with pytest.raises(ValueError, match="references are empty"):
        ErrorRate([], [], []).rate
    with pytest.raises(ValueError):
        ErrorRate([1], [1, 2], [1])
    import diffnorm_amd

    assert diffnorm_amd.ErrorRate is ErrorRate and callable(diffnorm_amd.wer) and callable(diffnorm_amd.cer)
    assert callable(diffnorm_amd.edit_distance) and callable(diffnorm_amd.reduce_units) and callable(diffnorm_amd.unit_error_rate)


def test_word_and_character_ids():
    from diffnorm_amd import metrics as M

    h, r = M.word_ids(["the cat  the hat", ""], ["the hat\tcat", "a the"])
    assert h == [[0, 1, 0, 2], []] and r == [[0, 2, 1], [3, 0]]  # one dictionary over the batch, repeated words one id
    flag = "\U0001F1E9\U0001F1EA"  # two code points outside the BMP
    h, r = M.char_ids(["e\u0301 x", flag], ["\u00e9", ""])
    assert h == [[0x65, 0x301, 0x20, 0x78], [0x1F1E9, 0x1F1EA]] and r == [[0xE9], []]
    for fn in (M.wer, M.cer):
        with pytest.raises(ValueError, match="hypotheses against"):
            fn(["a"], ["a", "b"])
        with pytest.raises(ValueError, match="lists of strings"):
            fn("a b", ["a b"])
        assert fn([], []).errors == []
        assert "Case" in fn.__doc__ or "case" in fn.__doc__


def test_lengths_are_refused_by_name_before_any_launch(monkeypatch):
    from diffnorm_amd import _lib
    from diffnorm_amd import metrics as M

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_launch)
    pad = torch.zeros(2, 8, dtype=torch.int32)
    ok = [3, 8]
    with pytest.raises(ValueError, match=r"a_len\[1\] = 8193.*at most 8192"):
        M.edit_distance(torch.zeros(2, 8200, dtype=torch.int32), pad, [3, 8193], ok)
    with pytest.raises(ValueError, match=r"b_len\[0\] = 9000.*at most 8192"):
        M.edit_distance(pad, pad, ok, [9000, 1])
    with pytest.raises(ValueError, match=r"a_len\[0\] = -1.*negative"):
        M.edit_distance(pad, pad, torch.tensor([-1, 2]), ok)
    with pytest.raises(ValueError, match=r"b_len\[1\] = 9 exceeds the leading dimension 8"):
        M.edit_distance(pad, pad, ok, [1, 9])
    with pytest.raises(ValueError, match=r"a_len\[0\] = 4 exceeds the leading dimension 3"):
        M.edit_distance([[1, 2, 3], [4]], [[1], [2]], a_len=[4, 1])
    with pytest.raises(ValueError, match="at most 8192"):
        M.edit_distance([[0] * 8193], [[0]])
    with pytest.raises(ValueError, match="at most 8192"):
        M.edit_distance(torch.zeros(1, 8193, dtype=torch.int32), pad[:1], [5], [5])  # the leading dimension itself
    with pytest.raises(ValueError, match="needs its rows' lengths"):
        M.edit_distance(pad, pad)
    with pytest.raises(ValueError, match=r"units_len\[0\] = 9 exceeds"):
        M.reduce_units(pad, [9, 1])
    with pytest.raises(ValueError, match=r"hyp_units_len\[0\] = 8193"):
        M.unit_error_rate([[1] * 8193], [[1]])
    with pytest.raises(ValueError, match="at most 8192"):
        M.wer(["w " * 8193], ["w"])
    assert _lib.EDIT_DISTANCE_MAX_LEN == M.MAX_LEN == 8192


def test_the_c_entry_points_refuse_bad_arguments():
    """On the host, before any launch (the checks of dn_edit_distance / dn_reduce_units come first; pointers are never followed)."""
    import ctypes as C

    from diffnorm_amd import _lib

    lib = _lib.load()
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    assert lib.dn_edit_distance_workspace_bytes(1, 8193, 4) == 0 and lib.dn_edit_distance_workspace_bytes(0, 4, 4) == 0
    assert lib.dn_edit_distance_workspace_bytes(3, 8192, 100) == 3 * 2 * 8256 * 4

    def dist(lda=8, ldb=8, B=1, panel=0, ws=p, nbytes=1 << 20, a=p):
        return lib.dn_edit_distance(a, lda, p, p, ldb, p, B, p, panel, ws, nbytes, None)

    for bad, word in ((dict(lda=8193), b"lda=8193"), (dict(ldb=8193), b"ldb=8193"), (dict(lda=0), b"lda=0"), (dict(B=0), b"B=0"),
                      (dict(panel=32), b"panel_cols=32"), (dict(panel=96 + 1), b"panel_cols"), (dict(panel=4096), b"panel_cols"),
                      (dict(ws=None), b"workspace"), (dict(nbytes=16), b"workspace"), (dict(a=None), b"null")):
        assert dist(**bad) == -1 and word in lib.dn_last_error(), bad
    assert lib.dn_reduce_units(p, p, 0, 8, p + 64, p, None, None, None) == -1 and b"dn_reduce_units" in lib.dn_last_error()
    assert lib.dn_reduce_units(p, p, 1, 8, p, p, None, None, None) == -1 and b"aliases" in lib.dn_last_error()
    assert lib.dn_reduce_units(None, p, 1, 8, p, p, None, None, None) == -1


def test_reduce_token_against_the_numpy_restatement():
    from diffnorm_amd.normalize import reduce_token

    rng = np.random.RandomState(3)
    units = rng.randint(0, 3, size=(9, 70))
    units[6] = 5                      # one run
    units[7] = np.arange(70)          # every token its own run
    lengths = [70, 33, 1, 0, 64, 65, 70, 70, 2]
    red, rlen, dur, first = R.reduce_rows(units, lengths)
    for b, n in enumerate(lengths):
        dedup, durations, keep = reduce_token(units[b, :n].tolist())
        if n == 0:  # the host definition is not called on empty utterances; the restatement gives no run
            assert rlen[b] == 0 and not red[b].any() and not dur[b].any() and not first[b].any()
            continue
        k = len(dedup)
        assert rlen[b] == k and red[b, :k].tolist() == dedup and dur[b, :k].tolist() == durations and first[b, :k].tolist() == keep.tolist()
        assert not red[b, k:].any() and not dur[b, k:].any() and not first[b, k:].any() and sum(durations) == n
    assert rlen[6] == 1 and dur[6, 0] == 70 and rlen[7] == 70
