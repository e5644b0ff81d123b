"""Host restatement of dn_bleu_stats and of the two score rules of diffnorm_amd/metrics.py: what tests/test_bleu_host.py pins (to the
recorded results of the reference's libbleu in tests/golden/bleu_stats.json and to worked cases) and tests/test_hip_bleu.py holds
the device to.

stats() is the collections.Counter form of fairseq/clib/libbleu/libbleu.cpp:73-109,138-156 for one pair:
    count_n = max(len(hyp) - n + 1, 0),    match_n = sum over n-grams g of min(count_hyp(g), count_ref(g)),    n = 1 .. 4
in the device's order [hyp_len, ref_len, match1, count1, ..., match4, count4].  score() is float64 arithmetic over ten such integers
(summed over a corpus, or of one item): "none" is Scorer.score (fairseq/scoring/bleu.py:132-151), "exp" the restated default
smoothing of sacreBLEU -- pinned to its statement in metrics.py and to the worked cases, not to the module."""
import json
import math
import os
from collections import Counter

ORDER = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleu_stats.json")


def ngrams(seq, n):
    seq = [int(t) for t in seq]
    return Counter(tuple(seq[i: i + n]) for i in range(len(seq) - n + 1))


def stats(hyp, ref):
    out = [len(hyp), len(ref)]
    for n in range(1, ORDER + 1):
        h, r = ngrams(hyp, n), ngrams(ref, n)
        out += [sum(min(c, r[g]) for g, c in h.items()), max(len(hyp) - n + 1, 0)]
    return out


def total(rows):
    """Column sums of a list of stats rows (the corpus statistics); ten zeros for no rows."""
    return [sum(col) for col in zip(*rows)] if rows else [0] * (2 + 2 * ORDER)


def precisions(st, smooth):
    m, c = st[2::2], st[3::2]
    if smooth == "none":
        return [mi / ci if ci > 0 else 0.0 for mi, ci in zip(m, c)]
    assert smooth == "exp", smooth
    out, k = [0.0] * ORDER, 1
    for n in range(ORDER):
        if c[n] == 0:
            break
        if m[n] == 0:
            k *= 2
            out[n] = 1 / (k * c[n])
        else:
            out[n] = m[n] / c[n]
    return out


def brevity(st, smooth):
    h, r = st[0], st[1]
    if h == 0:
        return 0.0
    if smooth == "none":
        return min(1, math.exp(1 - r / h))
    return 1.0 if h >= r else math.exp(1 - r / h)


def score(st, smooth="exp"):
    ps = precisions(st, smooth)
    if st[0] == 0 or st[2] == 0 or any(p <= 0 for p in ps):
        return 0.0
    psum = sum(math.log(p) for p in ps)
    return brevity(st, smooth) * math.exp(psum / ORDER) * 100


def load_golden():
    """tests/golden/bleu_stats.json (tools/gen_golden_bleu.py) -> its dictionary: "pairs" = [{"hyp", "ref", "stats"}], "corpus" =
    the column sums of the short pairs and, when the reference's Scorer could be loaded, its score() over them."""
    with open(GOLDEN) as f:
        return json.load(f)
