"""Host checks of quantizer learning (no device): the float64 restatement of the mini-batch rule against the scikit-learn fixture,
the bookkeeping of KMeansTrainer.fit (MiniBatchSchedule, reassign_decision) with the device step replaced by the restatement,
to_sklearn()'s model, and the manifest sampling."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as R  # noqa: E402

from diffnorm_amd import data, kmeans  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_recorded_scikit_learn_trajectory(golden, name):
    X, _ = R.blobs(name)
    idx, rows = R.batches_and_c0(name, X)
    assert np.array_equal(idx, golden[f"{name}_idx"]) and np.array_equal(rows, golden[f"{name}_rows"])  # the seeds still give the data
    ref, margins, _ = R.trajectory(X, idx, R.initial_centers(name, X, rows))
    keep = slice(None) if name == "a" else slice(-1, None)
    assert np.array_equal(ref[keep], golden[f"{name}_ref_centers"])
    sk, err = golden[f"{name}_sk_centers"].astype(np.float64), golden[f"{name}_sk_err"]
    got = np.abs(ref[keep].astype(np.float64) - sk).reshape(len(sk), -1).max(1)
    assert np.allclose(got, err[keep], rtol=0, atol=1e-12)
    # scikit-learn's fp32 accumulation of <= 256 rows a step: far under 1e-4 of the data's scale; a wrong rule misses by O(1)
    assert err.max() < 1e-4 * np.abs(ref).max()
    assert (margins < R.MARGIN).mean() < 0.01
    if name == "a":  # the far centre never wins a row: count 0 keeps its bits
        assert np.all(ref[:, -1] == R.FAR)


def test_update_rule_leaves_empty_clusters_and_rounds_once():
    rng = np.random.RandomState(0)
    X = rng.standard_normal((40, 32)).astype(np.float32)
    C0 = np.concatenate([X[:3], np.full((1, 32), 50.0, np.float32)])
    w = np.array([5.0, 0.0, 2.0, 7.0])
    C1, labels, _, inertia, counts = R.step(C0, w, X)
    assert counts[3] == 0 and np.array_equal(C1[3], C0[3]) and w[3] == 7.0
    for j in range(3):
        rows = X[labels == j].astype(np.float64)
        w0 = [5.0, 0.0, 2.0][j]
        want = (C0[j].astype(np.float64) * w0 + rows.sum(0)) / (w0 + len(rows))
        assert np.allclose(C1[j], want, rtol=0, atol=np.spacing(np.abs(want).max().astype(np.float32)))
        assert w[j] == w0 + len(rows)
    assert np.isclose(inertia, sum(((X[m].astype(np.float64) - C0[labels[m]]) ** 2).sum() for m in range(40)), rtol=1e-12)


def test_schedule_step_count_batches_and_early_stop():
    s = kmeans.MiniBatchSchedule(2000, 8, batch_size=256, max_iter=3, seed=11, max_no_improvement=5)
    assert s.n_steps == 3 * 2000 // 256 and s.batch_size == 256 and s.monitors
    want = np.random.RandomState(11)
    for _ in range(3):
        assert np.array_equal(s.next_batch(), want.randint(0, 2000, 256))
    assert kmeans.MiniBatchSchedule(100, 8, batch_size=256, max_iter=2).batch_size == 100  # capped at the data
    with pytest.raises(ValueError):
        kmeans.MiniBatchSchedule(4, 8)
    # early stop as _mini_batch_convergence: the first step is ignored, the second seeds the average, then max_no_improvement
    # steps in a row without a new minimum of the average end the loop
    s = kmeans.MiniBatchSchedule(1000, 4, batch_size=100, max_no_improvement=3)
    inertias = [900.0, 500.0, 400.0, 450.0, 460.0, 470.0, 480.0]
    alpha, ewa, ewa_min, bad, stops = 100 * 2.0 / 1001, None, None, 0, []
    for i, v in enumerate(inertias):
        got = s.converged(i, v)
        if i == 0:
            assert not got
            continue
        ewa = v / 100 if ewa is None else ewa * (1 - alpha) + v / 100 * alpha
        if ewa_min is None or ewa < ewa_min:
            ewa_min, bad = ewa, 0
        else:
            bad += 1
        stops.append(got)
        assert got == (bad >= 3) and s.ewa_inertia == pytest.approx(ewa, rel=1e-15)
    assert stops[-1] or not any(stops)
    s = kmeans.MiniBatchSchedule(1000, 4, batch_size=100, max_no_improvement=None)
    assert not s.monitors and not any(s.converged(i, 1.0 + i) for i in range(50))
    s = kmeans.MiniBatchSchedule(1000, 4, batch_size=100, tol=0.5, max_no_improvement=None)
    assert not s.converged(0, 1.0, 0.0) and not s.converged(1, 1.0, 0.6) and s.converged(2, 1.0, 0.4)


def test_fit_loop_over_the_restatement_stops_where_scikit_learn_would():
    X, _ = R.blobs("a")
    idx, rows = R.batches_and_c0("a", X)
    C0 = X[rows]
    C, steps, drawn = R.fit(X, 8, C0, batch_size=256, max_iter=4, seed=5, max_no_improvement=None)
    assert steps == 4 * 2000 // 256 == len(drawn)
    rng = np.random.RandomState(5)
    assert all(np.array_equal(b, rng.randint(0, 2000, 256)) for b in drawn)
    C2, steps2, _ = R.fit(X, 8, C0, batch_size=256, max_iter=100, seed=5, max_no_improvement=3)
    assert 4 < steps2 < 100 * 2000 // 256  # the blobs are learned at once: the averaged inertia stops improving early
    assert R.mean_inertia(X, C2) < R.mean_inertia(X, C0)  # (random rows may start two centres in one blob: no more is promised)
    Cpp, _, _ = R.fit(X, 8, "k-means++", batch_size=256, max_iter=4, seed=5, max_no_improvement=None)
    assert R.mean_inertia(X, Cpp) < 1.2 * 32 * 0.2 ** 2  # D sigma^2: seeded one centre per blob, every blob is found


def test_plus_plus_restatement_picks_one_row_from_every_blob(golden):
    X, which = R.blobs("a")
    picks, slack = R.plus_plus(X, 8, R.PP_SEED)
    assert np.array_equal(picks, golden["a_pp_picks"])
    assert sorted(which[picks]) == list(range(8)) and slack.min() > 1e-6


def test_reassignment_decision_follows_scikit_learn():
    w = np.array([100.0, 0.5, 80.0, 0.0, 60.0, 0.2])
    rng = np.random.RandomState(3)
    clusters, rows, weight = kmeans.reassign_decision(w, 0.01, 50, rng)
    assert clusters.tolist() == [1, 3, 5] and weight == 60.0
    assert np.array_equal(rows, np.random.RandomState(3).choice(50, replace=False, size=3))
    assert kmeans.reassign_decision(w, 0.0, 50, rng) is None  # ratio 0: nothing is ever below 0
    # more candidates than half the batch: only the int(0.5 * rows) lowest weights are reassigned
    w = np.concatenate([np.arange(1.0, 11.0), [1000.0]])
    clusters, rows, weight = kmeans.reassign_decision(w, 0.5, 8, np.random.RandomState(0))
    assert clusters.tolist() == [0, 1, 2, 3] and len(rows) == 4 and weight == 5.0
    # the clock of MiniBatchKMeans._random_reassign
    s = kmeans.MiniBatchSchedule(10000, 100, batch_size=300)
    assert [s.random_reassign(False) for _ in range(8)] == [False, False, False, True, False, False, False, True]
    assert s.random_reassign(True) and s.n_since_last_reassign == 0
    s = kmeans.MiniBatchSchedule(10000, 100, batch_size=300)
    for _ in range(8):
        due = s.reassign_due()
        assert due == s.random_reassign(False)


def test_to_sklearn_model_predicts_the_restatements_arg_min():
    pytest.importorskip("sklearn")
    X, _ = R.blobs("a")
    idx, rows = R.batches_and_c0("a", X)
    ref, _, _ = R.trajectory(X, idx, R.initial_centers("a", X, rows))
    centers = ref[-1]
    km = kmeans.sklearn_model(centers, np.arange(len(centers), dtype=np.float64))
    assert np.array_equal(km.cluster_centers_, centers) and km.cluster_centers_.dtype == np.float32
    labels, margin, _ = R.assign(X, centers)
    got = km.predict(X)
    sure = margin >= R.MARGIN
    assert sure.mean() > 0.99 and np.array_equal(got[sure], labels[sure])


def test_to_sklearn_says_so_when_scikit_learn_is_missing(monkeypatch):
    monkeypatch.setitem(sys.modules, "sklearn.cluster", None)
    t = kmeans.KMeansTrainer.__new__(kmeans.KMeansTrainer)
    with pytest.raises(ImportError, match="scikit-learn"):
        t.to_sklearn()


def test_manifest_sampling_and_host_row_gather(tmp_path):
    rng = np.random.RandomState(0)
    feats = [(f"utt{i}.wav", rng.standard_normal((5 + i, 32)).astype(np.float32)) for i in range(20)]
    manifest = data.write_feature_manifest(str(tmp_path / "train"), feats)
    every = kmeans.sample_manifest(manifest, 1.0)
    assert [os.path.basename(p) for p in every] == [f"utt{i}.feat.npy" for i in range(20)]
    some = kmeans.sample_manifest(manifest, 0.25, seed=9)
    assert some == random.Random(9).sample(every, 5)
    rows = kmeans._HostRows(every)
    whole = np.concatenate([f for _, f in feats])
    assert rows.shape == whole.shape
    idx = rng.randint(0, len(whole), 64)
    out = np.empty((64, 32), np.float32)
    rows.gather(idx, out)
    assert np.array_equal(out, whole[idx])
    one = kmeans._HostRows(whole)
    one.gather(idx, out)
    assert np.array_equal(out, whole[idx])
    with pytest.raises(ValueError):
        kmeans._HostRows([whole, whole[:, :16]])
