"""dn_bleu_stats on the device (csrc/bleu.hip) and the public layer over it (diffnorm_amd/metrics.py: bleu_stats, bleu, unit_bleu,
BleuScore; AsrTranscriber.asr_bleu) against the host restatement tests/bleu_ref.py and the recorded results of the reference's
libbleu (tests/golden/bleu_stats.json).  Everything on the device is integer arithmetic: every comparison is exact, and the scores
are compared through the same float64 function of the same ten integers.

The kernel's geometry the lengths are chosen around: one workgroup per pair sorts the N = hyp_len + ref_len n-gram start positions
in a bitonic network padded to the next power of two (so N = 2^k - 1, 2^k, 2^k + 1 are its edges); the workgroup has
pow2ceil(ld_hyp + ld_ref) / 16 threads, between 64 and 1024, and every thread then walks ceil(N / threads) sorted positions, runs
being joined across threads, waves (64 lanes) and the workgroup.  One path covers every pair up to 8192 + 8192: there is no
workspace path to hold equal."""
import numpy as np
import pytest
import torch

import bleu_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# (hyp_len, ref_len): the orders vanish one by one on either side; the network's power-of-two edges from 1 to 4096 positions; rows
# of 63 / 64 / 65 and 255 / 256 / 257; ragged pairs; the longest rows
SMALL = [(h, r) for h in range(6) for r in range(6)]
EDGES = [(63, 63), (64, 64), (65, 65), (63, 1), (1, 64), (31, 32), (32, 32), (32, 33), (255, 255), (256, 256), (257, 257), (255, 257), (127, 128),
         (128, 128), (128, 129), (511, 512), (512, 512), (513, 512), (1023, 1024), (1024, 1024), (1025, 1024), (2047, 2048), (2048, 2048), (2049, 2048),
         (1, 2500), (2500, 1), (700, 3000), (4097, 64)]
LONGEST = [(8191, 8192), (8192, 8192)]
ALPHABETS = [2, 4, 1004]


def draw(alphabet, lengths, seed=0):
    rng = np.random.RandomState(seed + alphabet)
    out = []
    for i, (nh, nr) in enumerate(lengths):
        hyp, ref = rng.randint(0, alphabet, size=nh).astype(np.int64), rng.randint(0, alphabet, size=nr).astype(np.int64)
        if i % 2 and min(nh, nr) > 1:  # a shared stretch in the middle: matches of every order also over a wide alphabet
            k = min(nh, nr) // 2
            hyp[nh - k:] = ref[:k]
        out.append((hyp.tolist(), ref.tolist()))
    return out


@pytest.fixture(scope="module")
def cases():
    """{alphabet: (pairs, restated statistics)} over SMALL + EDGES, computed once and left unchanged."""
    out = {}
    for alphabet in ALPHABETS:
        pairs = draw(alphabet, SMALL + EDGES)
        out[alphabet] = (pairs, [R.stats(h, r) for h, r in pairs])
    return out


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def padded(seqs, ld=None, fill=0):
    ld = max([len(s) for s in seqs] + [1]) if ld is None else ld
    out = np.full((len(seqs), ld), fill, dtype=np.int64)
    for i, s in enumerate(seqs):
        out[i, : len(s)] = s
    return torch.from_numpy(out).to(torch.int32), torch.tensor([len(s) for s in seqs], dtype=torch.int32)


def device_stats(pairs, ld_hyp=None, ld_ref=None, fill=0):
    from diffnorm_amd import metrics as M

    h, hl = padded([p[0] for p in pairs], ld_hyp, fill)
    r, rl = padded([p[1] for p in pairs], ld_ref, fill)
    got = M.bleu_stats(h.to(DEV), r.to(DEV), hl.to(DEV), rl.to(DEV))
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == (len(pairs), 10)
    return got.cpu().tolist()


def test_the_recorded_results_of_the_reference(golden):
    pairs = [(p["hyp"], p["ref"]) for p in golden["pairs"]]
    want = [p["stats"] for p in golden["pairs"]]
    n = golden["n_short"]
    assert device_stats(pairs[:n]) == want[:n]  # rows of 70
    assert device_stats(pairs[n:]) == want[n:]  # rows of 2000
    assert device_stats(pairs) == want


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_statistics_against_the_restatement(cases, alphabet):
    pairs, want = cases[alphabet]
    got = device_stats(pairs)  # one batch, rows of 4097 x 3000
    for n, g, w in zip(SMALL + EDGES, got, want):
        assert g == w, (n, g, w)
    for i, n in enumerate(SMALL + EDGES):  # and every pair alone, in rows of its own length: other leading dimensions and workgroup sizes
        assert device_stats(pairs[i: i + 1]) == [want[i]], n
    assert device_stats(pairs) == got  # bit-identical between calls


def test_the_longest_rows():
    pairs = draw(1004, LONGEST, seed=7) + draw(2, LONGEST, seed=7)
    want = [R.stats(h, r) for h, r in pairs]
    got = device_stats(pairs)
    assert got == want
    assert device_stats(pairs) == got
    assert device_stats(pairs[1:2]) == want[1:2]


def test_token_values_at_the_int32_edges():
    """Only equality of tokens matters: ids at +-2^31, 0 and -1 mixed, and keys that differ in the sign bit alone."""
    rng = np.random.RandomState(3)
    alphabet = np.array([INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX], dtype=np.int64)
    pairs = []
    for nh, nr in ((0, 3), (1, 1), (4, 4), (5, 9), (64, 65), (300, 257), (1000, 1100)):
        pairs.append((alphabet[rng.randint(0, 7, size=nh)].tolist(), alphabet[rng.randint(0, 7, size=nr)].tolist()))
    pairs.append(([INT32_MIN] * 9, [0] * 9))                      # the sign bit alone: no match
    pairs.append(([INT32_MIN, INT32_MAX] * 20, [INT32_MAX, INT32_MIN] * 20))
    pairs.append(([0, 0, 0, 0, 0], [0, 0, 0]))                      # token 0 is a token, not the mark of a row's end
    want = [R.stats(h, r) for h, r in pairs]
    assert want[-3][2] == 0 and want[-1] == [5, 3, 3, 5, 2, 4, 1, 3, 0, 2]
    assert device_stats(pairs) == want
    assert device_stats(pairs, 1200, 1100, INT32_MIN) == want


def test_clipping_extremes():
    rng = np.random.RandomState(5)
    x = rng.randint(0, 50, size=600).tolist()
    p3, p4 = [1, 2, 3] * 100, [1, 2, 3, 4] * 75
    pairs = [([7] * 100, [7] * 7), ([7] * 7, [7] * 100), (x, list(x)), (x, x[::-1]), (p3, p4), (p4, p3), ([7] * 4096, [7] * 4096), ([7] * 8192, [7] * 3)]
    want = [R.stats(h, r) for h, r in pairs]
    assert want[0] == [100, 7, 7, 100, 6, 99, 5, 98, 4, 97] and want[1] == [7, 100, 7, 7, 6, 6, 5, 5, 4, 4]
    assert want[2] == [600, 600, 600, 600, 599, 599, 598, 598, 597, 597]
    assert want[4][2:4] == [225, 300] and want[4][8] == 0  # 1 2 3 4 | 2 3 4 1 | ... : no 4-gram of the period-3 row
    assert device_stats(pairs) == want


def test_batch_independence(cases):
    pairs, want = cases[4]
    by_len = dict(zip(SMALL + EDGES, zip(pairs, want)))
    probe, st = by_len[(257, 257)]
    other, other_st = by_len[(32, 33)]
    for B in (1, 2, 33):
        for pos in sorted({0, B // 2, B - 1}):
            batch = [other] * B
            batch[pos] = probe
            got = device_stats(batch)
            assert got[pos] == st and all(g == other_st for i, g in enumerate(got) if i != pos), (B, pos)
    ragged = [p for p, n in zip(pairs, SMALL + EDGES) if max(n) <= 513]
    ragged_want = [w for w, n in zip(want, SMALL + EDGES) if max(n) <= 513]
    assert device_stats(ragged) == ragged_want  # minimal leading dimensions: 513 x 512
    for ld_hyp, ld_ref in ((513, 513), (600, 1500), (3000, 513), (8192, 8192)):  # the leading dimensions grow: more threads, more LDS
        assert device_stats(ragged, ld_hyp, ld_ref) == ragged_want, (ld_hyp, ld_ref)
    # what lies behind a sequence is never read into the result: INT32_MIN, or the other sequence's tokens
    assert device_stats(ragged, 600, 600, INT32_MIN) == ragged_want
    from diffnorm_amd import metrics as M

    h, hl = padded([p[0] for p in ragged], 600)
    r, rl = padded([p[1] for p in ragged], 600)
    for i, (x, y) in enumerate(ragged):
        h[i, len(x):] = torch.from_numpy(np.resize(np.asarray(y), 600 - len(x))) if len(y) else 7
        r[i, len(y):] = torch.from_numpy(np.resize(np.asarray(x), 600 - len(y))) if len(x) else 7
    assert M.bleu_stats(h.to(DEV), r.to(DEV), hl.to(DEV), rl.to(DEV)).cpu().tolist() == ragged_want
    # device lengths above the leading dimension and below 0 are clamped to [0, ld]
    full = [(p[0] + [7] * (600 - len(p[0])) if len(p[0]) else [7] * 600, p[1]) for p in ragged[:8]]
    h, _ = padded([p[0] for p in full], 600)
    r, rl = padded([p[1] for p in full], 600)
    over = torch.tensor([601, 1 << 20, INT32_MAX, 8193, 600, 9000, 700, 601], dtype=torch.int32)
    assert M.bleu_stats(h.to(DEV), r.to(DEV), over.to(DEV), rl.to(DEV)).cpu().tolist() == [R.stats(a, b) for a, b in full]
    under = torch.tensor([-1, INT32_MIN, -600, -1, -2, -3, -4, -5], dtype=torch.int32)
    assert M.bleu_stats(h.to(DEV), r.to(DEV), under.to(DEV), rl.to(DEV)).cpu().tolist() == [R.stats([], b) for _, b in full]


def test_host_inputs_and_lists_go_through_the_staging_buffer(cases):
    from diffnorm_amd import metrics as M

    pairs, want = cases[1004]
    some = [(p, w) for p, w, n in zip(pairs, want, SMALL + EDGES) if max(n) <= 257]
    lists_h, lists_r = [p[0] for p, _ in some], [p[1] for p, _ in some]
    assert M.bleu_stats(lists_h, lists_r).cpu().tolist() == [w for _, w in some]
    h, hl = padded(lists_h, 300, INT32_MIN)
    r, rl = padded(lists_r, 260, INT32_MIN)
    assert M.bleu_stats(h, r, hl, rl).cpu().tolist() == [w for _, w in some]
    with pytest.raises(ValueError, match="2 rows of hyp against 1 rows of ref"):
        M.bleu_stats([[1], [2]], [[1]])


# ------------------------------------------------------------------------------------------ the public layer
def host_score(rows, smooth):
    return R.score(R.total(rows), smooth), [R.score(r, smooth) for r in rows]


def test_unit_bleu_with_and_without_the_reduction(golden):
    from diffnorm_amd import metrics as M
    from diffnorm_amd.normalize import reduce_token

    hyp = [[5, 5, 7, 7, 7, 2, 9, 9, 4], [1, 1, 1], [], [4, 4, 9, 9, 3, 3, 3, 8, 1, 1, 6]]
    ref = [[5, 7, 3, 3, 2, 2, 9, 4, 4], [2], [8, 8], [4, 9, 3, 8, 8, 1, 6, 6]]
    hyp += [p["hyp"] for p in golden["pairs"][:40]]
    ref += [p["ref"] for p in golden["pairs"][:40]]
    for smooth in ("exp", "none"):
        raw = M.unit_bleu(hyp, ref, smooth=smooth)
        rows = [R.stats(h, r) for h, r in zip(hyp, ref)]
        assert [[h, r] + [v for mc in zip(m, c) for v in mc] for h, r, m, c in zip(raw.hyp_len, raw.ref_len, raw.matches, raw.totals)] == rows
        assert (raw.score, raw.item_scores) == host_score(rows, smooth)
        red = M.unit_bleu(hyp, ref, reduce=True, smooth=smooth)
        rh, rr = [reduce_token(h)[0] if h else [] for h in hyp], [reduce_token(r)[0] if r else [] for r in ref]
        rows = [R.stats(h, r) for h, r in zip(rh, rr)]
        assert red.hyp_len == [len(h) for h in rh] and red.ref_len == [len(r) for r in rr]
        assert red.matches == [r[2::2] for r in rows] and red.totals == [r[3::2] for r in rows]
        assert (red.score, red.item_scores) == host_score(rows, smooth)
    assert rows[3] == R.stats([4, 9, 3, 8, 1, 6], [4, 9, 3, 8, 1, 6]) and red.item_scores[3] == 100.0
    h, hl = padded(hyp, 80, INT32_MIN)
    r, rl = padded(ref, 75, INT32_MIN)
    dev = M.unit_bleu(h.to(DEV), r.to(DEV), reduce=True, hyp_len=hl.to(DEV), ref_len=rl.to(DEV), smooth="none")
    assert dev == red
    with pytest.raises(ValueError, match="unit_bleu: 2 hypotheses against 1 references"):
        M.unit_bleu([[1], [2]], [[1]])


def test_bleu_of_strings():
    from diffnorm_amd import metrics as M

    hyps = ["the cat sat on the mat", "hello  world again and again", "", "a b c", "The Quick brown fox jumps over the lazy dog"]
    refs = ["the cat sat on a mat today", "hello world again and again", "something here", "", "the quick brown fox jumped over the lazy dog"]
    for lowercase in (False, True):
        lo = (lambda s: s.lower()) if lowercase else (lambda s: s)
        hw, rw = M.word_ids([lo(s) for s in hyps], [lo(s) for s in refs])
        rows = [R.stats(h, r) for h, r in zip(hw, rw)]
        for smooth in ("exp", "none"):
            b = M.bleu(hyps, refs, smooth=smooth, lowercase=lowercase)
            assert b.matches == [r[2::2] for r in rows] and b.totals == [r[3::2] for r in rows]
            assert b.hyp_len == [len(h) for h in hw] and b.ref_len == [len(r) for r in rw]
            assert (b.score, b.item_scores) == host_score(rows, smooth) and b.score > 0.0
            assert b.item_scores[1] == 100.0 and b.item_scores[2] == b.item_scores[3] == 0.0
    assert M.bleu(hyps, refs, lowercase=True).total_matches[0] == M.bleu(hyps, refs).total_matches[0] + 2  # "The", "Quick"
    merged = M.bleu(hyps[:2], refs[:2]) + M.bleu(hyps[2:], refs[2:])  # ids are per call; the statistics do not depend on them
    assert merged == M.bleu(hyps, refs)


def test_asr_bleu_is_transcribe_then_bleu():
    import wav2vec_ref as W
    from diffnorm_amd import asr
    from diffnorm_amd import metrics as M
    from test_hip_wav2vec_ctc import engine

    tr = asr.AsrTranscriber(engine("f32"), W.SIL_TOKENS, "none")
    waves = [W.golden_wave(i) for i in range(len(W.GOLDEN_WAVES))]
    texts = tr.transcribe(waves)
    refs = [" ".join(t.split()[:-1] + ["zz"]).upper() if i % 2 else t for i, t in enumerate(texts)]
    for lowercase in (True, False):
        for smooth in ("exp", "none"):
            hyps, b = tr.asr_bleu(waves, refs, lowercase=lowercase, smooth=smooth)
            assert hyps == texts
            lo = (lambda s: s.lower()) if lowercase else (lambda s: s)
            hw, rw = M.word_ids([lo(s) for s in texts], [lo(s) for s in refs])
            rows = [R.stats(h, r) for h, r in zip(hw, rw)]
            assert b.matches == [r[2::2] for r in rows] and b.totals == [r[3::2] for r in rows] and b.smooth == smooth
            assert b.hyp_len == [len(h) for h in hw] and b.ref_len == [len(r) for r in rw]
            assert (b.score, b.item_scores) == host_score(rows, smooth)
    with pytest.raises(ValueError, match="references for"):
        tr.asr_bleu(waves, refs[:-1])
    with pytest.raises(ValueError, match="smooth"):
        tr.asr_bleu(waves, refs, smooth="floor")
    with pytest.raises(ValueError, match="not one string"):
        tr.asr_bleu(waves[:1], "a b")
