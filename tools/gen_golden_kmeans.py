"""Writes tests/golden/kmeans_train.npz: scikit-learn's MiniBatchKMeans.partial_fit trajectories on the two seeded data sets of
tests/kmeans_ref.py, beside the float64 restatement of its update rule (arithmetic in float64, one rounding to fp32 per step).

The data, the batch index arrays and the initial centres are functions of the seeds in tests/kmeans_ref.py and are rebuilt by the
tests; stored are the batch indices and rows of C0 (so a change of a generator shows), and per data set
  sk_centers      scikit-learn's cluster_centers_ after every step -- data set (a); for (b) only after the last step, the twenty
                  [50, 768] tables would not fit a committed file
  ref_centers     the restatement's centres, the same steps
  sk_err          max |scikit-learn - restatement| after every step (scikit-learn's own fp32 error)
  margins         the float64 top-2 margins of every (step, row)
Asserted here: the restatement reproduces scikit-learn's trajectory to fp32 accumulation error with the same labels at every step;
under 1 % of the (step, row) margins are below 1e-4; k-means++ on (a) with n = 8 and the seed the GPU test uses picks one row from
every blob.  Needs scikit-learn (the tests do not)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_ref as R  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import MiniBatchKMeans

    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in R.SETS:
        X, which = R.blobs(name)
        idx, rows = R.batches_and_c0(name, X)
        c0 = R.initial_centers(name, X, rows)
        ref, margins, labels = R.trajectory(X, idx, c0)
        km = MiniBatchKMeans(n_clusters=len(c0), init=c0, n_init=1, reassignment_ratio=0)
        sk, err = [], []
        for t, b in enumerate(idx):
            km.partial_fit(X[b])
            sk.append(km.cluster_centers_.copy())
            # what scikit-learn assigned at this step: its centres before the step -> compare through the result
            err.append(float(np.abs(sk[-1].astype(np.float64) - ref[t].astype(np.float64)).max()))
        sk = np.stack(sk)
        scale = float(np.abs(ref[:, : R.SETS[name][3]]).max())
        # fp32 accumulation of <= 256 rows per step over 20 steps: a few hundred ulp at the most; a wrong rule misses by O(sigma)
        assert max(err) < 1e-4 * scale, (name, max(err), scale)
        if name == "a":
            assert np.array_equal(sk[:, -1], np.broadcast_to(c0[-1], sk[:, -1].shape)), "the far centre won a row"
        share = float((margins < R.MARGIN).mean())
        assert share < 0.01, (name, share)
        print(f"{name}: sklearn fp32 error per step max {max(err):.3e} (scale {scale:.2f}); margins under {R.MARGIN}: {share:.4%}")
        keep = slice(None) if name == "a" else slice(-1, None)
        out.update({f"{name}_idx": idx, f"{name}_rows": rows.astype(np.int32), f"{name}_sk_centers": sk[keep], f"{name}_ref_centers": ref[keep],
                    f"{name}_sk_err": np.array(err), f"{name}_margins": margins.astype(np.float32)})
    X, which = R.blobs("a")
    picks, slack = R.plus_plus(X, 8, R.PP_SEED)
    assert sorted(which[picks]) == list(range(8)), which[picks]
    assert slack.min() > 1e-6, slack.min()
    out["a_pp_picks"] = picks.astype(np.int32)
    print(f"k-means++ on (a), seed {R.PP_SEED}: picks {picks.tolist()} cover every blob; smallest boundary slack {slack.min():.2e}")
    np.savez_compressed(R.GOLDEN, **out)
    print(R.GOLDEN, os.path.getsize(R.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
