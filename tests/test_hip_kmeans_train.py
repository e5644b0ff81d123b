"""Quantizer learning on the device (diffnorm_amd/kmeans.py over csrc/kmeans.hip) against the float64 restatement of
tests/kmeans_ref.py and the scikit-learn fixture tests/golden/kmeans_train.npz (tools/gen_golden_kmeans.py).

Bounds.  A centre is (c w + sum) / (w + count) with every sum in double and ONE rounding to fp32: against the restatement, which
does the same from the same fp32 centres, it may differ by the double arithmetic's order (1e-16) on either side of a rounding
boundary -- one fp32 ulp; the bound is 2 ulp at the centre's largest coordinate.  Column sums of k <= 1037 fp32 rows in double, rows
in ascending index: at most (k - 1) 2^-53 sum|x|.  Distances of dn_kmeans_min_dist: double accumulation, one rounding to fp32."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def km():
    from diffnorm_amd import kmeans

    return kmeans


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


_SETS = {}


def dataset(name):
    if name not in _SETS:
        X, which = R.blobs(name)
        idx, rows = R.batches_and_c0(name, X)
        _SETS[name] = (X, which, idx, R.initial_centers(name, X, rows))
    return _SETS[name]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32)))


@pytest.mark.parametrize("name", ["a", "b"])
def test_partial_fit_trajectory_against_the_restatement(km, golden, name):
    X, _, idx, c0 = dataset(name)
    n, D = c0.shape
    t = km.KMeansTrainer(n, D, device=DEV).init_centers(c0)
    Xd = torch.from_numpy(X).to(DEV)
    ref, w_ref, free = c0.copy(), np.zeros(n), True  # the free-running restatement, followed while every label has agreed
    excluded = total = 0
    worst = 0.0
    for s, b in enumerate(idx):
        before, w_before = t.centers_array(), t.weight_sums.cpu().numpy().copy()
        inertia, counts = t.partial_fit(Xd[torch.from_numpy(b.astype(np.int64)).to(DEV)])
        labels = t._labels[: len(b)].cpu().numpy()
        # the restatement of this step from the centres the device had
        want, l64, margin, inertia64, counts64 = R.step(before, w_before, X[b])
        sure = margin >= R.MARGIN
        excluded += int((~sure).sum())
        total += len(b)
        assert np.array_equal(labels[sure], l64[sure]), f"{name} step {s}: a label with margin >= {R.MARGIN} differs"
        if np.array_equal(labels, l64):
            got = t.centers_array()
            bound = 2 * ulp32(np.abs(want).max(1))[:, None]
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            assert np.all(err <= bound), f"{name} step {s}: centre error {err.max():.3e} over 2 ulp ({(err / bound).max() * 2:.2f} ulp)"
            assert np.array_equal(counts.cpu().numpy(), counts64) and np.array_equal(t.weight_sums.cpu().numpy(), w_before)
            assert abs(float(inertia.item()) - inertia64) <= 1e-12 * inertia64
            assert np.array_equal(t.half[:n].cpu().numpy(), R.half_norm(got))
        else:
            free = False
        if free:  # against the recorded scikit-learn error: the project's bar of 4 x the reference's own fp32 error
            ref, _, _, _, _ = R.step(ref, w_ref, X[b])
            dev_err = np.abs(t.centers_array().astype(np.float64) - ref).max()
            sk_err = max(float(golden[f"{name}_sk_err"][s]), float(ulp32(np.abs(ref).max())))
            worst = max(worst, dev_err / sk_err)
            assert dev_err <= 4 * sk_err, f"{name} step {s}: {dev_err:.3e} against scikit-learn's own {sk_err:.3e}"
    print(f"{name}: excluded {excluded}/{total} assignments; device error / scikit-learn's fp32 error, worst step: {worst:.3f}")
    assert excluded < 0.01 * total
    if name == "a":
        assert np.all(t.centers_array()[-1] == R.FAR) and float(t.weight_sums[-1]) == 0.0
    if free:
        assert np.abs(t.centers_array().astype(np.float64) - golden[f"{name}_ref_centers"][-1]).max() <= 2 * ulp32(np.abs(ref).max())


def _accumulate_case(km, M, D, n, labels, X=None, seed=0):
    from diffnorm_amd.hubert import kmeans_scores_tables

    rng = np.random.RandomState(seed)
    X = rng.standard_normal((M, D)).astype(np.float32) if X is None else X
    C = rng.standard_normal((n, D)).astype(np.float32)
    Cp, _ = kmeans_scores_tables(C)
    need = km.workspace_bytes(M, n)
    ws = torch.full((need + 256 + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    off = ((ws.data_ptr() + 255) & ~255) - ws.data_ptr()
    args = (torch.from_numpy(X).to(DEV), torch.from_numpy(labels.astype(np.int32)).to(DEV), Cp.to(DEV), n)
    sums, counts, inertia = km.accumulate(*args, workspace=ws)
    sums2, counts2, inertia2 = km.accumulate(*args, workspace=ws)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(counts, counts2) and torch.equal(inertia.view(torch.int64), inertia2.view(torch.int64))
    assert bool((ws[off + need:] == 0xA5).all()), "the workspace was written past dn_kmeans_workspace_bytes_train"
    X64 = X.astype(np.float64)
    want = np.zeros((n, D))
    np.add.at(want, labels, X64)
    mag = np.zeros((n, D))
    np.add.at(mag, labels, np.abs(X64))
    cnt = np.bincount(labels, minlength=n)
    assert np.array_equal(counts.cpu().numpy(), cnt)
    got = sums.cpu().numpy()
    assert np.all(np.abs(got - want) <= np.maximum(cnt - 1, 0)[:, None] * 2.0 ** -53 * mag)
    assert np.all(got[cnt == 0] == 0)
    q = float(((X64 - C[labels].astype(np.float64)) ** 2).sum())
    assert abs(float(inertia.item()) - q) <= 1e-12 * q
    return got


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1037])
@pytest.mark.parametrize("n,D", [(1, 32), (50, 768), (1000, 32)])
def test_accumulate_against_float64_index_add(km, M, n, D):
    labels = np.random.RandomState(M + n).randint(0, n, M)
    if n == 50:
        labels[labels % 7 == 3] = 0  # some clusters empty, one crowded
    _accumulate_case(km, M, D, n, labels)


def test_accumulate_one_cluster_owns_every_row_and_duplicated_rows(km):
    M, D, n = 1037, 768, 50  # 1037 rows in one cluster: five workgroups of the sort feed one list
    _accumulate_case(km, M, D, n, np.full(M, 17))
    rng = np.random.RandomState(4)
    X = np.repeat(rng.standard_normal((17, D)).astype(np.float32), 61, axis=0)
    _accumulate_case(km, M, D, n, rng.randint(0, n, M), X=X)


def test_accumulate_does_not_depend_on_where_the_rows_end(km):
    """The sums of the first rows' clusters are the same bits whether 64, 65 or 1037 rows follow in other clusters."""
    rng = np.random.RandomState(8)
    D, n = 768, 50
    X = rng.standard_normal((1037, D)).astype(np.float32)
    labels = rng.randint(0, n - 1, 1037)
    labels[300:] = n - 1
    base = _accumulate_case(km, 300, D, n, labels[:300], X=X[:300])
    for M in (364, 365, 1037):
        got = _accumulate_case(km, M, D, n, labels[:M], X=X[:M])
        assert np.array_equal(got[: n - 1].view(np.int64), base[: n - 1].view(np.int64))


def test_update_keeps_empty_clusters_and_rebuilds_the_half_norm_table(km):
    from diffnorm_amd.hubert import kmeans_scores_tables

    rng = np.random.RandomState(2)
    n, D = 50, 768
    C = rng.standard_normal((n, D)).astype(np.float32)
    Cp, half = kmeans_scores_tables(C)
    Cp, half = Cp.to(DEV), half.to(DEV)
    half[:n] = 123.0  # stale on purpose: only clusters with rows are rewritten
    w = rng.randint(0, 2000, n).astype(np.float64)
    counts = rng.randint(0, 40, n).astype(np.int32)
    counts[[3, 49]] = 0
    sums = rng.standard_normal((n, D)) * counts[:, None]
    wd = torch.from_numpy(w).to(DEV)
    km.update(Cp, half, wd, torch.from_numpy(sums).to(DEV), torch.from_numpy(counts).to(DEV), n)
    got, on = Cp[:n].cpu().numpy(), counts > 0
    assert np.array_equal(got[~on].view(np.int32), C[~on].view(np.int32)) and np.all(half[:n].cpu().numpy()[~on] == 123.0)
    assert np.array_equal(wd.cpu().numpy(), w + counts)
    want = (C[on].astype(np.float64) * w[on, None] + sums[on]) / (w[on] + counts[on])[:, None]
    assert np.all(np.abs(got[on] - want) <= ulp32(want))  # one rounding; 1 ulp covers a contracted multiply-add in the kernel
    _, table = kmeans_scores_tables(got)
    assert np.array_equal(half[:n].cpu().numpy()[on].view(np.int32), table[:n].numpy()[on].view(np.int32))
    assert torch.all(Cp[n:] == 0)


def test_min_dist_is_within_fp32_rounding_of_float64(km):
    rng = np.random.RandomState(6)
    for M, D, k in ((1037, 768, 8), (65, 32, 16), (1, 32, 1)):
        X = rng.standard_normal((M, D)).astype(np.float32)
        cand = X[rng.randint(0, M, k)] + (rng.standard_normal((k, D)) * 0.5).astype(np.float32)
        d = R.sq_dists(X, cand)
        cur = (rng.uniform(0.5, 1.5, M) * d.min(1).mean()).astype(np.float32)
        Xd, cd, md = torch.from_numpy(X).to(DEV), torch.from_numpy(cand).to(DEV), torch.from_numpy(cur).to(DEV)
        pot = km.min_dist(Xd, cd, md, commit=-1)
        assert torch.equal(md.cpu(), torch.from_numpy(cur))  # evaluation only reads
        want = np.minimum(cur.astype(np.float64)[:, None], d).sum(0)
        assert np.all(np.abs(pot.cpu().numpy() - want) <= 2.0 ** -23 * want)
        assert torch.equal(pot.view(torch.int64), km.min_dist(Xd, cd, md, commit=-1).view(torch.int64))
        j = k - 1
        km.min_dist(Xd, cd, md, commit=j)
        want_m = np.minimum(cur.astype(np.float64), d[:, j])
        assert np.all(np.abs(md.cpu().numpy() - want_m) <= ulp32(want_m))


def test_plus_plus_picks_what_the_restatement_picks(km):
    X, which, _, _ = dataset("a")
    t = km.KMeansTrainer(8, 32, device=DEV).init_plus_plus(X, seed=R.PP_SEED)
    picks = t.init_indices_.cpu().numpy()
    want, slack = R.plus_plus(X, 8, R.PP_SEED)
    assert sorted(which[picks]) == list(range(8))
    sure = np.concatenate([[True], np.cumprod(slack > 1e-6).astype(bool)])  # up to the first draw too close to a boundary
    assert sure.all() and np.array_equal(picks[sure], want[sure])
    assert np.array_equal(t.centers_array(), X[picks]) and np.array_equal(t.half[:8].cpu().numpy(), R.half_norm(X[picks]))
    Xb, _, _, _ = dataset("b")
    t = km.KMeansTrainer(50, 768, device=DEV).init_plus_plus(Xb, seed=3)
    want, slack = R.plus_plus(Xb, 50, 3)
    sure = np.concatenate([[True], np.cumprod(slack > 1e-6).astype(bool)])
    assert sure.sum() > 1 and np.array_equal(t.init_indices_.cpu().numpy()[sure], want[sure])


@pytest.mark.parametrize("init", ["k-means++", "c0"])
def test_fit_reaches_the_restatements_inertia(km, init):
    from diffnorm_amd.hubert import KMeansQuantizer

    X, _, _, c0 = dataset("a")
    start = init if init == "k-means++" else c0[:8]
    args = dict(batch_size=256, max_iter=3, seed=21, max_no_improvement=10)
    t = km.KMeansTrainer(8, 32, device=DEV).fit(torch.from_numpy(X).to(DEV), init=start, **args)
    C64, steps, _ = R.fit(X, 8, start, **args)
    got, want = R.mean_inertia(X, t.centers_array()), R.mean_inertia(X, C64)
    print(f"fit from {init}: {t.n_steps_} steps (restatement {steps}); mean inertia {got:.6f} against {want:.6f}; score() {t.score(X):.6f}")
    assert got <= 1.02 * want
    assert abs(t.score(X) - got) <= 1e-9 * got
    units = t.quantizer().predict(torch.from_numpy(X).to(DEV))
    assert torch.equal(units, KMeansQuantizer(t.centers_array(), device=DEV).predict(torch.from_numpy(X).to(DEV)))


def test_host_resident_features_give_the_same_centres(km, tmp_path):
    X, _, _, _ = dataset("b")
    args = dict(batch_size=256, max_iter=2, seed=5, max_no_improvement=None)
    on_device = km.KMeansTrainer(50, 768, device=DEV).fit(torch.from_numpy(X).to(DEV), **args).centers_array()
    assert np.array_equal(km.KMeansTrainer(50, 768, device=DEV).fit(X, **args).centers_array().view(np.int32), on_device.view(np.int32))
    paths = []
    for i, s in enumerate(range(0, len(X), 100)):
        paths.append(str(tmp_path / f"u{i}.feat.npy"))
        np.save(paths[-1], X[s: s + 100])
    from_files = km.KMeansTrainer(50, 768, device=DEV).fit(paths, **args)
    assert np.array_equal(from_files.centers_array().view(np.int32), on_device.view(np.int32))
    out = str(tmp_path / "km.npy")
    from_files.save_centers(out)
    assert np.array_equal(np.load(out), on_device)


def test_reassignment_moves_a_starved_centre_onto_the_data(km):
    X, _, _, c0 = dataset("a")  # c0's ninth centre never wins a row: with a ratio it is reassigned to a row of the batch
    t = km.KMeansTrainer(9, 32, device=DEV, reassignment_ratio=0.01)
    t.fit(torch.from_numpy(X).to(DEV), init=c0, batch_size=256, max_iter=2, seed=1, max_no_improvement=None)
    C = t.centers_array()
    assert np.abs(C).max() < 10 and float(t.weight_sums.min()) > 0
    assert np.array_equal(t.half[:9].cpu().numpy(), R.half_norm(C))


def test_refusals(km):
    from diffnorm_amd import _lib

    with pytest.raises(ValueError):
        km.KMeansTrainer(8, 48, device=DEV)
    X = torch.zeros(64, 48, device=DEV)
    with pytest.raises(ValueError):
        km.accumulate(X, torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(128, 48, device=DEV), 8)
    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    wp = (ws.data_ptr() + 255) & ~255
    buf = torch.zeros(128 * 64, dtype=torch.float64, device=DEV)
    assert lib.dn_kmeans_accumulate(X.data_ptr(), buf.data_ptr(), buf.data_ptr(), 64, 48, 8, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), wp, 1 << 19, None) == -1
    assert b"multiple of 32" in lib.dn_last_error()
    assert lib.dn_kmeans_min_dist(X.data_ptr(), 64, 32, buf.data_ptr(), 17, -1, buf.data_ptr(), buf.data_ptr(), wp, 1 << 19, None) == -1
    assert lib.dn_kmeans_update(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 8, 48, None) == -1
    assert lib.dn_kmeans_accumulate(X.data_ptr(), buf.data_ptr(), buf.data_ptr(), 64, 32, 8, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), wp, 16, None) < 0
    X = torch.zeros(64, 32, device=DEV)
    for bad in (-1, 8):
        labels = torch.zeros(64, dtype=torch.int32, device=DEV)
        labels[40] = bad
        with pytest.raises(ValueError, match="label"):
            km.accumulate(X, labels, torch.zeros(128, 32, device=DEV), 8)
    with pytest.raises(ValueError, match="n_clusters"):
        km.KMeansTrainer(100, 32, device=DEV).init_plus_plus(X, seed=0)
    with pytest.raises(ValueError):
        km.KMeansTrainer(100, 32, device=DEV).fit(X)
