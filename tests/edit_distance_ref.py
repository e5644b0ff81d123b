"""Host restatement of the unit-cost Levenshtein distance (substitution, insertion, deletion cost 1 each) and of the four outputs of
dn_reduce_units: what tests/test_metrics_host.py pins and tests/test_hip_metrics.py holds the device to.

edit_distance is a row-wise numpy dynamic programme.  With row the previous row D[i - 1][0 .. n] and x = a[i - 1],
    new[0] = i,  new[j] = min(row[j] + 1, row[j - 1] + (b[j - 1] != x))          (deletion, substitution / match)
leaves the insertion chain D[i][j] = min over k <= j of new[k] + (j - k), which is minimum.accumulate(new - arange) + arange.
edit_distance_loop is the plain double loop (lengths up to 64), which pins the vectorised form."""
import numpy as np


def edit_distance(a, b) -> int:
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    n = len(b)
    ar = np.arange(n + 1, dtype=np.int64)
    row = ar.copy()
    new = np.empty(n + 1, dtype=np.int64)
    for i in range(1, len(a) + 1):
        new[0] = i
        np.minimum(row[1:] + 1, row[:-1] + (b != a[i - 1]), out=new[1:])
        row = np.minimum.accumulate(new - ar) + ar
    return int(row[n])


def edit_distance_loop(a, b) -> int:
    a, b = list(a), list(b)
    assert len(a) <= 64 and len(b) <= 64, "the double loop is the small-case pin"
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


def reduce_rows(units, lengths):
    """numpy restatement of dn_reduce_units: units [B, ld], lengths [B] -> (reduced, reduced_len, durations, first), zeros behind
    reduced_len[b] in the three [B, ld] outputs."""
    units = np.asarray(units, dtype=np.int64)
    B, ld = units.shape
    red, dur, first = (np.zeros((B, ld), dtype=np.int64) for _ in range(3))
    rlen = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = int(lengths[b])
        row = units[b, :n]
        starts = np.flatnonzero(np.concatenate([[True], row[1:] != row[:-1]])) if n else np.zeros(0, dtype=np.int64)
        k = len(starts)
        rlen[b] = k
        red[b, :k], first[b, :k] = row[starts], starts
        dur[b, :k] = np.diff(np.concatenate([starts, [n]]))
    return red, rlen, dur, first
