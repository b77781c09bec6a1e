"""Writes tests/golden/proba_n300_seed31.npz and proba_n301_seed32.npz: scikit-learn's (LIBSVM's) per-fold held-out
decision values and the sigmoid fitted to them, which the probability tests compare against.

Rows: tests/probability_checks.proba_rows(n, seed) -- n x 6 uniform real values with every column's smallest entry
exactly 0 and its largest exactly 1 (the solvers' min-max scaling is the identity; the GPU path needs scale=True),
noisy labels (seed 32: about 30 % positives), and 50 extra rows inside the same bounds.
Stored: X, y, folds (svm355.utils.data.stratified_folds(y, 5, seed)); cv_decision: row i's decision value under
sklearn.svm.SVC(kernel="rbf", C=10, gamma=0.5, tol=1e-6) fitted on the rows outside i's fold; (A, B) from
sklearn.calibration._sigmoid_calibration(cv_decision, y), which minimises Platt's objective with the targets of
Lin, Lin and Weng (P(y = +1 | f) = 1 / (1 + exp(A f + B))); Xq and proba: the 50 extra rows and [P(-1), P(+1)] of
the all-rows model's decision values through that sigmoid.  The tests read the files and do not import
scikit-learn.

    python scripts/make_probability_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

CASES = ((300, 31, 0.5), (301, 32, 0.3))  # n, seed, share of positives
C, GAMMA, K = 10.0, 0.5, 5


def main() -> None:
    import sklearn
    from sklearn.calibration import _sigmoid_calibration
    from sklearn.svm import SVC as SkSVC

    from probability_checks import proba_rows
    from svm355.utils.data import stratified_folds

    for n, seed, pos in CASES:
        X, y, Xq = proba_rows(n, seed, pos)
        folds = stratified_folds(y, K, seed)
        dec = np.zeros(n)
        for j in range(K):
            te = folds == j
            m = SkSVC(kernel="rbf", C=C, gamma=GAMMA, tol=1e-6, cache_size=500).fit(X[~te], y[~te])
            dec[te] = m.decision_function(X[te])
        A, B = _sigmoid_calibration(dec, y)
        full = SkSVC(kernel="rbf", C=C, gamma=GAMMA, tol=1e-6, cache_size=500).fit(X, y)
        z = A * full.decision_function(Xq) + B
        e = np.exp(-np.abs(z))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        proba = np.stack([np.where(z >= 0, big, small), np.where(z >= 0, small, big)], 1)
        dst = ROOT / "tests" / "golden" / f"proba_n{n}_seed{seed}.npz"
        os.makedirs(dst.parent, exist_ok=True)
        np.savez_compressed(dst, X=X, y=y, folds=folds, cv_decision=dec, A=np.array(float(A)), B=np.array(float(B)),
                            Xq=Xq, proba=proba, C=np.array(C), gamma=np.array(GAMMA),
                            sklearn_version=np.array(sklearn.__version__))
        print(dst, dst.stat().st_size, "bytes", "positives", int((y == 1).sum()), "A", float(A), "B", float(B),
              "held-out accuracy", float(np.mean(np.where(dec > 0, 1, -1) == y)))


if __name__ == "__main__":
    main()
