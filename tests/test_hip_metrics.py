"""dn_edit_distance and dn_reduce_units on the device (csrc/metrics.hip) and the public layer over them (diffnorm_amd/metrics.py,
AsrTranscriber.score, normalize(..., unit_changes=)) against the host restatement tests/edit_distance_ref.py and
normalize.reduce_token.  Everything is integer arithmetic: every comparison is exact.

The kernel's geometry the lengths are chosen around: 64 lanes, a per-lane strip of ceil(columns / 64) <= 32 columns (template steps
at 4 and 16 columns: 256 and 1024 tokens), panels of 2048 columns with the boundary column in the workspace (pairs whose SHORTER
side exceeds 2048), the shorter side taken as the columns; dn_reduce_units walks a row in chunks of 64."""
import numpy as np
import pytest
import torch

import edit_distance_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN = -(1 << 31)
LENGTHS = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 63), (64, 64), (65, 65), (127, 127), (128, 128), (129, 129), (1023, 1023), (1024, 1024),
           (1025, 1025), (1, 8192), (8192, 1), (4097, 64), (2049, 2049), (2500, 4100), (8192, 8192)]
ALPHABETS = [4, 1004]


def draw(alphabet, seed=0):
    rng = np.random.RandomState(seed + alphabet)
    return [(rng.randint(0, alphabet, size=na).astype(np.int32), rng.randint(0, alphabet, size=nb).astype(np.int32)) for na, nb in LENGTHS]


@pytest.fixture(scope="module")
def cases():
    """{alphabet: (pairs, restated distances)}, computed once and left unchanged."""
    out = {}
    for alphabet in ALPHABETS:
        pairs = draw(alphabet)
        out[alphabet] = (pairs, [R.edit_distance(a, b) for a, b in pairs])
    return out


def padded(seqs, ld=None, fill=0):
    ld = max([len(s) for s in seqs] + [1]) if ld is None else ld
    out = np.full((len(seqs), ld), fill, dtype=np.int64)
    for i, s in enumerate(seqs):
        out[i, : len(s)] = s
    return torch.from_numpy(out).to(torch.int32), torch.tensor([len(s) for s in seqs], dtype=torch.int32)


def device_distance(pairs, lda=None, ldb=None, fill_a=0, fill_b=0, panel_cols=0):
    from diffnorm_amd import metrics as M

    a, a_len = padded([p[0] for p in pairs], lda, fill_a)
    b, b_len = padded([p[1] for p in pairs], ldb, fill_b)
    return M.edit_distance(a.to(DEV), b.to(DEV), a_len.to(DEV), b_len.to(DEV), panel_cols=panel_cols).cpu().tolist()


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_distance_against_the_restatement(cases, alphabet):
    pairs, want = cases[alphabet]
    got = device_distance(pairs)  # one batch, rows of 8192
    print(f"alphabet {alphabet}: lengths {LENGTHS} -> {got}")
    assert got == want
    for i, n in enumerate(LENGTHS):  # and every pair alone, in rows of its own length: other leading dimensions and workgroup shapes
        assert device_distance(pairs[i: i + 1]) == [want[i]], n
    assert device_distance(pairs) == got  # bit-identical between calls


def test_named_cases():
    rng = np.random.RandomState(5)
    x = rng.randint(0, 7, size=700).astype(np.int32)
    y = rng.randint(100, 107, size=300).astype(np.int32)
    ins = lambda at: np.concatenate([x[:at], [99], x[at:]]).astype(np.int32)
    pairs = [(x, x.copy()), (x, y), (y, x), (ins(0), x), (ins(350), x), (ins(700), x), (x, ins(0)), (x, x[::-1].copy()),
             (x[:200], x[:200][::-1].copy())]
    got = device_distance(pairs)
    assert got[:7] == [0, 700, 700, 1, 1, 1, 1]
    assert got[7:] == [R.edit_distance(x, x[::-1]), R.edit_distance(x[:200], x[:200][::-1])]


def test_batch_independence(cases):
    pairs, want = cases[4]
    by_len = dict(zip(LENGTHS, zip(pairs, want)))
    probe, d = by_len[(1025, 1025)]
    other = by_len[(129, 129)][0]
    for B in (1, 5, 67):
        for pos in range(B):
            batch = [other] * B
            batch[pos] = probe
            got = device_distance(batch)
            assert got[pos] == d and all(g == by_len[(129, 129)][1] for i, g in enumerate(got) if i != pos), (B, pos)
    ragged = [p for p, n in zip(pairs, LENGTHS) if max(n) <= 1025]
    ragged_want = [w for w, n in zip(want, LENGTHS) if max(n) <= 1025]
    assert device_distance(ragged) == ragged_want == [device_distance([p])[0] for p in ragged]
    for lda, ldb in ((1025, 1025), (1030, 2048), (4099, 1025), (8192, 8192)):  # the leading dimensions grow
        assert device_distance(ragged, lda, ldb) == ragged_want, (lda, ldb)
    # what lies behind a sequence is never read into the result: INT32_MIN, or the other sequence's tokens
    assert device_distance(ragged, 1100, 1100, INT32_MIN, INT32_MIN) == ragged_want
    from diffnorm_amd import metrics as M

    a, a_len = padded([p[0] for p in ragged], 1100)
    b, b_len = padded([p[1] for p in ragged], 1100)
    for i, (x, y) in enumerate(ragged):
        a[i, len(x):] = torch.from_numpy(np.resize(y, 1100 - len(x))) if len(y) else 7
        b[i, len(y):] = torch.from_numpy(np.resize(x, 1100 - len(y))) if len(x) else 7
    assert M.edit_distance(a.to(DEV), b.to(DEV), a_len.to(DEV), b_len.to(DEV)).cpu().tolist() == ragged_want


@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_the_workspace_panels_agree_with_the_register_strips(cases, alphabet):
    """Pairs whose shorter side fits one panel never touch the workspace; swept in panels of 64, 256 and 1024 columns they go through
    the boundary column every 64 / 256 / 1024 columns, the path the long pairs take at 2048.  The same numbers."""
    pairs, want = cases[alphabet]
    short = [(p, w) for p, w, n in zip(pairs, want, LENGTHS) if max(n) <= 1025 or n == (4097, 64)]
    for panel in (64, 256, 1024, 2048):
        assert device_distance([p for p, _ in short], panel_cols=panel) == [w for _, w in short], panel
    long_ = [(p, w) for p, w, n in zip(pairs, want, LENGTHS) if n in ((2049, 2049), (2500, 4100))]
    assert device_distance([p for p, _ in long_], panel_cols=1024) == [w for _, w in long_]


def test_host_inputs_and_lists_go_through_the_staging_buffer(cases):
    from diffnorm_amd import metrics as M

    pairs, want = cases[1004]
    some = [(p, w) for p, w, n in zip(pairs, want, LENGTHS) if max(n) <= 129]
    lists_a, lists_b = [p[0].tolist() for p, _ in some], [p[1].tolist() for p, _ in some]
    assert M.edit_distance(lists_a, lists_b).cpu().tolist() == [w for _, w in some]
    a, a_len = padded(lists_a, 200, INT32_MIN)
    b, b_len = padded(lists_b, 140, INT32_MIN)
    d = M.edit_distance(a, b, a_len, b_len)
    assert d.is_cuda and d.dtype == torch.int32 and d.cpu().tolist() == [w for _, w in some]


# ------------------------------------------------------------------------------------------ dn_reduce_units
def check_reduce(units, lengths):
    from diffnorm_amd import metrics as M
    from diffnorm_amd.normalize import reduce_token

    units = np.asarray(units)
    got = [t.cpu().numpy() for t in M.reduce_units(torch.from_numpy(units).to(torch.int32).to(DEV), torch.tensor(lengths, dtype=torch.int32).to(DEV))]
    want = R.reduce_rows(units, lengths)
    for g, w, name in zip(got, want, ("reduced", "reduced_len", "durations", "first")):
        assert g.dtype == np.int32 and np.array_equal(g, w), name
    for b, n in enumerate(lengths):  # and the host definition itself
        dedup, durations, keep = reduce_token(units[b, :n].tolist())
        k = int(got[1][b])
        assert k == len(dedup) and got[0][b, :k].tolist() == dedup and (n == 0 or got[2][b, :k].tolist() == durations)
        assert got[3][b, :k].tolist() == keep.tolist()


def test_reduce_units_against_reduce_token():
    rng = np.random.RandomState(11)
    units = rng.randint(0, 3, size=(7, 300))
    check_reduce(units, [300, 299, 64, 65, 128, 1, 0])
    edge = rng.randint(0, 3, size=(8, 300))
    edge[0] = 9                       # all tokens equal: one run over every chunk boundary
    edge[1] = np.arange(300)          # all tokens distinct
    edge[4] = np.repeat(np.arange(30), 10)  # runs of 10 from frame 0: 60..69, 120..129, 190..199, 250..259 each cross a boundary
    edge[5, 3:] = np.repeat(np.arange(5), 64)[: 297]  # runs of 64 that start at 3, 67, ...: every run crosses one boundary
    edge[6, :64] = 1                  # a run that ends exactly at a chunk's last frame
    edge[6, 64:] = 2
    edge[7] = np.repeat(np.arange(150), 2)  # runs of 2, none across a boundary
    check_reduce(edge, [300, 300, 0, 1, 300, 300, 300, 300])
    tail = rng.randint(0, 3, size=(5, 300))  # the padding holds the row's last token: the run must end at the length
    lengths = [10, 64, 65, 200, 299]
    for b, n in enumerate(lengths):
        tail[b, n:] = tail[b, n - 1]
    check_reduce(tail, lengths)
    check_reduce(rng.randint(0, 2, size=(67, 130)), rng.randint(0, 131, size=67).tolist())  # more rows than a workgroup holds


# ------------------------------------------------------------------------------------------ the public layer
def test_unit_error_rate_wer_and_cer_on_a_hand_written_batch():
    from diffnorm_amd import metrics as M
    from diffnorm_amd.normalize import reduce_token

    hyp = [[5, 5, 7, 7, 7, 2], [1, 1, 1], [], [4, 4, 9]]
    ref = [[5, 7, 3, 3, 2, 2], [2], [8, 8], [4, 9, 9, 9]]
    er = M.unit_error_rate(hyp, ref)
    rh, rr = [reduce_token(h)[0] for h in hyp], [reduce_token(r)[0] for r in ref]
    assert er.errors == [R.edit_distance(h, r) for h, r in zip(rh, rr)] == [1, 1, 1, 0]
    assert er.hyp_len == [3, 1, 0, 2] and er.ref_len == [4, 1, 1, 2] and er.rate == 3 / 8
    raw = M.unit_error_rate(hyp, ref, reduce=False)
    assert raw.errors == [R.edit_distance(h, r) for h, r in zip(hyp, ref)] and raw.ref_len == [6, 1, 2, 4] and raw.hyp_len == [6, 3, 0, 3]
    hyps = ["the cat sat on the mat", "hello  world", "", "a b c", "na\u00efve caf\u00e9"]
    refs = ["the cat sat on a mat today", "hello world", "something here", "", "naive caf\u00e9"]
    w, c = M.wer(hyps, refs), M.cer(hyps, refs)
    hw, rw = M.word_ids(hyps, refs)
    assert w.errors == [R.edit_distance(h, r) for h, r in zip(hw, rw)] == [2, 0, 2, 3, 1]
    assert w.ref_len == [7, 2, 2, 0, 2] and w.hyp_len == [6, 2, 0, 3, 2] and w.rate == 8 / 13
    assert w.item_rates[1] == 0.0 and w.item_rates[3] == float("inf")
    assert c.errors == [R.edit_distance([ord(x) for x in h], [ord(x) for x in r]) for h, r in zip(hyps, refs)]
    assert c.ref_len == [len(r) for r in refs] and c.hyp_len == [len(h) for h in hyps]


def test_asr_score_is_transcribe_then_wer():
    import wav2vec_ref as W
    from diffnorm_amd import asr
    from test_hip_wav2vec_ctc import engine

    tr = asr.AsrTranscriber(engine("f32"), W.SIL_TOKENS, "none")
    waves = [W.golden_wave(i) for i in range(len(W.GOLDEN_WAVES))]
    texts = tr.transcribe(waves)
    refs = [" ".join(t.split()[:-1] + ["zz"]) if i % 2 else t for i, t in enumerate(texts)]
    for unit, ids in (("word", lambda s: s.split()), ("char", lambda s: [ord(ch) for ch in s])):
        hyps, er = tr.score(waves, refs, unit=unit)
        assert hyps == texts
        table = {}
        enc = lambda s: [table.setdefault(tok, len(table)) for tok in ids(s)]
        assert er.errors == [R.edit_distance(enc(h), enc(r)) for h, r in zip(texts, refs)]
        assert er.ref_len == [len(ids(r)) for r in refs] and er.hyp_len == [len(ids(h)) for h in texts]
    with pytest.raises(ValueError, match="unit"):
        tr.score(waves, refs, unit="phone")
    with pytest.raises(ValueError, match="references for"):
        tr.score(waves, refs[:-1])


def test_normalize_reports_unit_changes_and_leaves_the_lines_alone():
    from diffnorm_amd import normalize as N
    from diffnorm_amd.normalize import reduce_token
    from test_hip_chain_start import corpus, ldm_for

    m = ldm_for("f32")
    utts = corpus()
    for i, u in enumerate(utts):  # frame-level units with repeats, so that the reference side is a real reduction
        if i % 2:
            frames = np.repeat(np.asarray(u.reduce_tgt_unit), 2).tolist()
            utts[i] = N.Utterance(u.audio_id, u.src_audio, u.src_n_frames, u.feat.repeat_interleave(2, 0), frames, u.reduce_tgt_unit)

    def sample(feat, **kw):  # both paths draw the same noise: the chain's inputs are the common input
        kw.pop("noise_keys", None)
        torch.manual_seed(1234)
        return m.ddim_sample(feat, **kw)

    def check(lines, changes):
        assert len(changes) == len(lines) == len(utts)
        for u, line, c in zip(utts, lines, changes):
            units = [int(x) for x in line.split("\t")[3].split()]
            assert reduce_token(units)[0] == units
            assert c == (u.audio_id, R.edit_distance(units, u.reduce_tgt_unit), len(u.reduce_tgt_unit), len(units)), (u.audio_id, c)

    plain = N.normalize(sample, utts, start_step=4, batch_size=4, device=DEV)
    got = []
    assert N.normalize(sample, utts, start_step=4, batch_size=4, device=DEV, unit_changes=got) == plain
    check(plain, got)
    keyed_plain = N.normalize(sample, utts, start_step=4, batch_size=4, device=DEV, noise_seed=5)
    keyed = []
    assert N.normalize(sample, utts, start_step=4, batch_size=4, device=DEV, noise_seed=5, unit_changes=keyed) == keyed_plain
    check(keyed_plain, keyed)
    assert keyed_plain == plain and keyed == got  # the two paths on their common input
    budget = []
    lines = N.normalize(m.ddim_sample, utts, start_step=4, device=DEV, noise_seed=5, max_tokens=192, pad_multiple=8, unit_changes=budget)
    assert lines == N.normalize(m.ddim_sample, utts, start_step=4, device=DEV, noise_seed=5, max_tokens=192, pad_multiple=8)
    check(lines, budget)  # re-formed, length-sorted batches come back in utterance order
