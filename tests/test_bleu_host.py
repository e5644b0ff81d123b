"""Host side of BLEU (no GPU): the Counter restatement (tests/bleu_ref.py) against the recorded results of the reference's libbleu
(tests/golden/bleu_stats.json, tools/gen_golden_bleu.py), the two score rules of diffnorm_amd/metrics.py against worked cases and
the reference's recorded Scorer.score(), BleuScore's arithmetic, and the refusals of the wrapper and of the C entry points before
anything is launched.

The worked scores are computed here in float64 from their closed forms; a score is a product of a handful of correctly rounded
float64 operations (four divisions, four logarithms, a sum, one exponential), so the two sides may differ by a few units of
2^-53 ~ 1.1e-16 relative: REL = 1e-13 leaves three decimal orders over that and is ten orders under any wrong rule."""
import math

import pytest
import torch

import bleu_ref as R

REL = 1e-13
approx = lambda v: pytest.approx(v, rel=REL, abs=0.0)


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def test_the_restatement_equals_every_recorded_row(golden):
    pairs = golden["pairs"]
    assert len(pairs) >= 300 and sum(len(p["hyp"]) >= 1000 for p in pairs) >= 3
    for p in pairs:
        assert R.stats(p["hyp"], p["ref"]) == p["stats"], (p["hyp"], p["ref"])
    short = [p["stats"] for p in pairs[: golden["n_short"]]]
    assert R.total(short) == golden["corpus"]
    assert {max(p["hyp"] + p["ref"]) >= 4 for p in pairs} == {True, False}  # narrow and wide alphabets are both there


def test_none_is_the_references_scorer(golden):
    """Scorer.score() (fairseq/scoring/bleu.py:132-151) recorded over the corpus sums: the same float64 operations in the same order."""
    from diffnorm_amd import metrics as M

    st = golden["corpus"]
    assert golden["scorer_score"] is not None
    assert R.score(st, "none") == golden["scorer_score"] == M.bleu_score(st[2::2], st[3::2], st[0], st[1], "none")
    assert all(v > 0 for v in st) and M.bleu_score(st[2::2], st[3::2], st[0], st[1], "exp") == golden["scorer_score"]


WORKED = [  # hyp, ref, stats, score under "none", score under "exp"
    ([1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [5, 5, 5, 5, 4, 4, 3, 3, 2, 2], 100.0, 100.0),
    ([1, 2, 3, 4, 9, 9], [1, 2, 3, 4, 5, 6], [6, 6, 4, 6, 3, 5, 2, 4, 1, 3], 100 * (1 / 15) ** 0.25, 100 * (1 / 15) ** 0.25),
    ([1, 2, 3, 9, 4, 5], [1, 2, 3, 4, 5], [6, 5, 5, 6, 3, 5, 1, 4, 0, 3], 0.0, 100 * (1 / 48) ** 0.25),
    ([1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [4, 6, 4, 4, 3, 3, 2, 2, 1, 1], 100 * math.exp(-0.5), 100 * math.exp(-0.5)),
    ([7, 7, 7], [7], [3, 1, 1, 3, 0, 2, 0, 1, 0, 0], 0.0, 0.0),
    ([], [1, 2, 3], [0, 3, 0, 0, 0, 0, 0, 0, 0, 0], 0.0, 0.0),
    ([1, 2, 3], [], [3, 0, 0, 3, 0, 2, 0, 1, 0, 0], 0.0, 0.0),
]


def test_worked_cases_under_both_rules():
    from diffnorm_amd import metrics as M

    for hyp, ref, st, none, exp in WORKED:
        assert R.stats(hyp, ref) == st, (hyp, ref)
        for smooth, want in (("none", none), ("exp", exp)):
            for got in (R.score(st, smooth), M.bleu_score(st[2::2], st[3::2], st[0], st[1], smooth)):
                assert got == approx(want) if want else got == 0.0, (hyp, ref, smooth, got, want)
            assert M.bleu_score(st[2::2], st[3::2], st[0], st[1], smooth) == R.score(st, smooth)
            assert M.bleu_precisions(st[2::2], st[3::2], smooth) == R.precisions(st, smooth)
    # the smoothed precision of the third case: 1 / (2 * 3)
    assert M.bleu_precisions([5, 3, 1, 0], [6, 5, 4, 3], "exp") == [5 / 6, 3 / 5, 1 / 4, 1 / 6]
    # two zero orders double k twice: 1 / (2 c_3), 1 / (4 c_4); none below the first zero count
    assert M.bleu_precisions([5, 3, 0, 0], [6, 5, 4, 3], "exp") == [5 / 6, 3 / 5, 1 / 8, 1 / 12]
    assert M.bleu_precisions([2, 1, 0, 0], [2, 1, 0, 0], "exp") == [1.0, 1.0, 0.0, 0.0]
    assert M.bleu_score([0, 0, 0, 0], [6, 5, 4, 3], 6, 6, "exp") == 0.0  # no unigram match: 0, not a smoothed number
    with pytest.raises(ValueError, match="smooth 'floor'"):
        M.bleu_score([1, 1, 1, 1], [1, 1, 1, 1], 4, 4, "floor")


def test_exp_equals_none_where_nothing_is_zero(golden):
    from diffnorm_amd import metrics as M

    seen = 0
    for p in golden["pairs"]:
        st = p["stats"]
        if all(v > 0 for v in st[2:]):
            seen += 1
            assert R.score(st, "exp") == R.score(st, "none") == M.bleu_score(st[2::2], st[3::2], st[0], st[1], "exp") > 0.0
        else:
            assert R.score(st, "none") == 0.0
    assert seen >= 50
    for h, r in ((5, 9), (9, 5), (7, 7)):  # both forms of the brevity penalty, on either side of 1
        assert M.bleu_brevity(h, r, "exp") == M.bleu_brevity(h, r, "none") == R.brevity([h, r], "exp") == min(1.0, math.exp(1 - r / h))
    assert M.bleu_brevity(0, 5, "none") == M.bleu_brevity(0, 5, "exp") == 0.0


def score_of(rows, smooth="exp"):
    from diffnorm_amd.metrics import BleuScore

    return BleuScore([r[2::2] for r in rows], [r[3::2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], smooth)


def test_bleu_score_is_the_corpus_score_of_the_summed_statistics(golden):
    rows = [p["stats"] for p in golden["pairs"][:40]]
    for smooth in ("exp", "none"):
        b = score_of(rows, smooth)
        tot = R.total(rows)
        assert b.total_matches == tot[2::2] and b.total_counts == tot[3::2] and (b.total_hyp_len, b.total_ref_len) == (tot[0], tot[1])
        assert b.score == R.score(tot, smooth) and b.precisions == R.precisions(tot, smooth) and b.brevity_penalty == R.brevity(tot, smooth)
        assert b.item_scores == [R.score(r, smooth) for r in rows]
        mean = sum(b.item_scores) / len(rows)
        assert abs(b.score - mean) > 1e-3 * b.score  # not the mean of the items
    two = [WORKED[0][2], WORKED[4][2]]  # [100, 0] item by item; the sums 6/8, 4/6, 3/4, 2/2 with hyp 8 >= ref 6
    b = score_of(two)
    assert b.item_scores == [100.0, 0.0] and b.score == approx(100 * (6 / 8 * 4 / 6 * 3 / 4) ** 0.25)
    line = b.format()
    assert line.startswith("BLEU4 = %.2f, 75.0/66.7/75.0/100.0 (BP=1.000, ratio=1.333, syslen=8, reflen=6)" % b.score), line
    assert score_of([]).score == 0.0 and score_of([]).item_scores == [] and "syslen=0" in score_of([]).format()


def test_bleu_score_add_merges_batches(golden):
    from diffnorm_amd.metrics import BleuScore

    rows = [p["stats"] for p in golden["pairs"][:30]]
    a, b, whole = score_of(rows[:11]), score_of(rows[11:]), score_of(rows)
    s = a + b
    assert isinstance(s, BleuScore) and s == whole and s.score == whole.score and s.item_scores == a.item_scores + b.item_scores
    assert (a + score_of([])).score == a.score and len(a.matches) == 11  # the operands are left alone
    with pytest.raises(ValueError, match="smooth 'exp' \\+ smooth 'none'"):
        a + score_of(rows[11:], "none")
    with pytest.raises(ValueError, match="4 orders"):
        BleuScore([[1, 2, 3]], [[1, 2, 3]], [1], [1])
    with pytest.raises(ValueError, match="2 rows of matches"):
        BleuScore([[1] * 4] * 2, [[1] * 4], [1], [1])
    with pytest.raises(ValueError, match="smooth"):
        BleuScore([], [], [], [], "add-k")


def test_the_wrapper_refuses_by_name_before_any_launch(monkeypatch):
    from diffnorm_amd import _lib
    from diffnorm_amd import metrics as M

    def no_launch(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "load", no_launch)
    pad = torch.zeros(2, 8, dtype=torch.int32)
    ok = [3, 8]
    with pytest.raises(ValueError, match=r"hyp_len\[1\] = 8193.*at most 8192"):
        M.bleu_stats(torch.zeros(2, 8200, dtype=torch.int32), pad, [3, 8193], ok)
    with pytest.raises(ValueError, match=r"ref_len\[0\] = -1.*negative"):
        M.bleu_stats(pad, pad, ok, torch.tensor([-1, 2]))
    with pytest.raises(ValueError, match=r"ref_len\[1\] = 9 exceeds the leading dimension 8"):
        M.bleu_stats(pad, pad, ok, [1, 9])
    with pytest.raises(ValueError, match="at most 8192"):
        M.bleu_stats([[0] * 8193], [[0]])
    with pytest.raises(ValueError, match="needs its rows' lengths"):
        M.bleu_stats(pad, pad)
    with pytest.raises(ValueError, match=r"hyp_units_len\[0\] = 8193"):
        M.unit_bleu([[1] * 8193], [[1]])
    with pytest.raises(ValueError, match="smooth 'floor'"):
        M.unit_bleu([[1]], [[1]], smooth="floor")
    with pytest.raises(ValueError, match="at most 8192"):
        M.bleu(["w " * 8193], ["w"])
    with pytest.raises(ValueError, match="bleu: 1 hypotheses against 2 references"):
        M.bleu(["a"], ["a", "b"])
    with pytest.raises(ValueError, match="lists of strings"):
        M.bleu("a b", ["a b"])
    with pytest.raises(ValueError, match="lists of strings"):
        M.bleu(["a b"], "a b")
    with pytest.raises(ValueError, match="smooth 'floor'"):
        M.bleu(["a"], ["a"], smooth="floor")
    empty = M.bleu([], [])
    assert empty.matches == [] and empty.score == 0.0
    assert "13a" in M.bleu.__doc__ and "sacrebleu" in M.__doc__ and "NOT" in M.__doc__


def test_the_c_entry_points_refuse_bad_arguments():
    """On the host, before any launch (the checks come first; pointers are never followed)."""
    import ctypes as C

    from diffnorm_amd import _lib

    lib = _lib.load()
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    size = lib.dn_bleu_stats_workspace_bytes
    assert size(1, 8193, 4) == 0 and size(1, 4, 8193) == 0 and size(0, 4, 4) == 0 and size(1, 0, 4) == 0 and size(-1, 4, 4) == 0
    need = size(3, 8192, 8192)
    assert 0 < need <= 64 and size(1, 1, 1) == need  # one path for every pair: a token size

    def stats(ld_hyp=8, ld_ref=8, B=1, ws=p, nbytes=1 << 10, hyp=p, out=p):
        return lib.dn_bleu_stats(hyp, ld_hyp, p, p, ld_ref, p, B, out, ws, nbytes, None)

    for bad, word in ((dict(ld_hyp=8193), b"ld_hyp=8193"), (dict(ld_ref=8193), b"ld_ref=8193"), (dict(ld_hyp=0), b"ld_hyp=0"), (dict(B=0), b"B=0"),
                      (dict(B=-3), b"B=-3"), (dict(ws=None), b"workspace"), (dict(nbytes=need - 1), b"workspace"), (dict(hyp=None), b"null"),
                      (dict(out=None), b"null")):
        assert stats(**bad) == -1, bad
        assert b"dn_bleu_stats" in lib.dn_last_error() and word in lib.dn_last_error(), (bad, lib.dn_last_error())
    assert _lib.BLEU_ORDER == 4 and _lib.BLEU_STATS == 10


def test_package_exports():
    import diffnorm_amd
    from diffnorm_amd import asr
    from diffnorm_amd import metrics as M

    assert diffnorm_amd.BleuScore is M.BleuScore and diffnorm_amd.bleu is M.bleu
    assert diffnorm_amd.bleu_stats is M.bleu_stats and diffnorm_amd.unit_bleu is M.unit_bleu
    assert callable(asr.AsrTranscriber.asr_bleu) and callable(asr.AsrTranscriber.score)
