"""Writes tests/golden/ovo_n300_seed41.npz (k = 3, d = 16, uint8 rows), ovo_n301_seed42.npz (k = 4, d = 16,
real-valued rows, class sizes 120 / 90 / 84 / 7) and ovo_n330_seed43.npz (k = 10, d = 24, uint8 rows, 45 pairs):
scikit-learn's (LIBSVM's) one-vs-one models the OneVsOneSVC tests compare against.

Rows: per class a centre uniform in [60, 195] per feature, Gaussian noise of sigma 55, clipped to [0, 255] (and
rounded to uint8 unless the fixture is real-valued); the rows are shuffled and the labels are 3 i + 1 for class
index i, so that an index cannot pass for a label.  200 query rows of the same mixture.

Stored: X, labels, Xt, gamma, C and, of sklearn.svm.SVC(C=10, gamma=0.5, tol=1e-6, decision_function_shape="ovo")
fitted on the rows min-max scaled by the project's rule (a column range below 1e-12 scales by 1): support_,
n_support_, dual_coef_, intercept_, decision_function(Xt) (200 x P) and predict(Xt).  The tests read the files
and do not import scikit-learn.

The seeds are chosen so that at most 2 % of the query rows have a pair decision within FIXTURE_DEC_TOL
(tests/ovo_checks.py) of zero: the script prints the count per fixture and fails when a fixture breaks the cap.

    python scripts/make_ovo_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent

# n, k, d, seed, class sizes (None: even), uint8 rows
CASES = ((300, 3, 16, 41, None, True), (301, 4, 16, 42, (120, 90, 84, 7), False), (330, 10, 24, 43, None, True))
GAMMA, C, TOL, QUERIES = 0.5, 10.0, 1e-6, 200
NEAR_ZERO = 1e-4  # printed and capped here with a margin over tests/ovo_checks.FIXTURE_DEC_TOL
CAP = 0.02


def make(n, k, d, seed, sizes, u8):
    r = np.random.default_rng(seed)
    cent = r.uniform(60, 195, size=(k, d))
    if sizes is None:
        sizes = [n // k + (1 if i < n % k else 0) for i in range(k)]
    cls = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)])

    def rows(c):
        x = np.clip(cent[c] + r.normal(0, 55, size=(len(c), d)), 0, 255)
        return np.rint(x).astype(np.uint8) if u8 else x

    X = rows(cls)
    p = r.permutation(len(cls))
    X, cls = X[p], cls[p]
    ct = r.integers(0, k, size=QUERIES)
    return X, 3 * cls + 1, rows(ct), 3 * ct + 1


def scale(X, mn, mx):
    rg = np.where(mx - mn < 1e-12, 1.0, mx - mn)
    return (X.astype(np.float64) - mn) / rg


def main() -> None:
    import sklearn
    from sklearn.svm import SVC

    for n, k, d, seed, sizes, u8 in CASES:
        X, labels, Xt, labels_t = make(n, k, d, seed, sizes, u8)
        mn, mx = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
        m = SVC(C=C, gamma=GAMMA, tol=TOL, decision_function_shape="ovo", cache_size=500).fit(scale(X, mn, mx), labels)
        dec = m.decision_function(scale(Xt, mn, mx)).reshape(QUERIES, -1)
        pred = m.predict(scale(Xt, mn, mx))
        near = int((np.abs(dec).min(axis=1) <= NEAR_ZERO).sum())
        dst = ROOT / "tests" / "golden" / f"ovo_n{n}_seed{seed}.npz"
        os.makedirs(dst.parent, exist_ok=True)
        np.savez_compressed(dst, X=X, labels=labels.astype(np.int64), Xt=Xt, labels_t=labels_t.astype(np.int64),
                            gamma=np.array(GAMMA), C=np.array(C), support=m.support_.astype(np.int64),
                            n_support=m.n_support_.astype(np.int64), dual_coef=m.dual_coef_, intercept=m.intercept_,
                            decision=dec, predict=pred.astype(np.int64), sklearn_version=np.array(sklearn.__version__))
        print(dst, dst.stat().st_size, "bytes", "k", k, "n_support", m.n_support_.tolist(), "query accuracy",
              float(np.mean(pred == labels_t)), f"rows with min |decision| <= {NEAR_ZERO}:", near)
        if near > CAP * QUERIES:
            sys.exit(f"seed {seed}: {near} query rows near a zero decision, above the {CAP:.0%} cap: choose another seed")


if __name__ == "__main__":
    main()
