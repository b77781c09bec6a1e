"""Writes tests/golden/ovo_proba_n300_seed41.npz (k = 3), ovo_proba_n301_seed42.npz (k = 4) and
ovo_proba_n330_seed43.npz (k = 10): scikit-learn's (LIBSVM's) per-pair cross-validated decisions, the sigmoids
fitted to them and LIBSVM's pairwise coupling, which the OneVsOneSVC(cv=) tests compare against.

Rows, labels, query rows, C and gamma are those of the one-vs-one fixtures (tests/golden/ovo_n*_seed*.npz,
scripts/make_ovo_golden.py), read from those files and not touched; the rows are min-max scaled by the project's
rule before scikit-learn sees them, as there.

Stored:
  folds        svm355.utils.data.stratified_folds(class index, 5, seed)
  cv_decision  (n, k - 1) in the layout of dual_coef_: for a row of class c, column j is its held-out decision in
               the pair (c, o), o = j for j < c, else j + 1, the pair's first class being the positive side.  Each
               pair and fold is a binary sklearn.svm.SVC(C, gamma, tol=1e-6) on the pair's rows outside the fold;
               a fold with none of the pair's rows is skipped
  probA, probB (P,) in LIBSVM's pair order: sklearn.calibration._sigmoid_calibration on the pair's held-out
               decisions and labels (Platt's objective with Lin, Lin and Weng's targets)
  proba        (200, k) for Xt: scikit-learn's multi-class SVC(probability=True, decision_function_shape="ovo")
               fitted on all rows, its _probA / _probB overwritten with the values above, predict_proba -- which
               is LIBSVM's own coupling on known sigmoids
The tests read the files and do not import scikit-learn.

The project's Newton fit of every pair's sigmoid must end "converged" on these decisions (a nearly separable
pair drives A towards -infinity and the fit to its iteration cap, where (A, B) are not comparable): the script
checks it with the host fit and fails if a pair does not, in which case that fixture needs rows of its own with
more overlap.  The three fixtures pass as they are (sigma 55 against centres in [60, 195]).

    python scripts/make_ovo_proba_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = ((300, 41), (301, 42), (330, 43))
TOL, FOLDS = 1e-6, 5


def scale(X, mn, mx):
    rg = np.where(mx - mn < 1e-12, 1.0, mx - mn)
    return (X.astype(np.float64) - mn) / rg


def main() -> None:
    import sklearn
    from sklearn.calibration import _sigmoid_calibration
    from sklearn.svm import SVC

    from svm355.ops.cpu import platt_fit
    from svm355.utils.data import stratified_folds

    for n, seed in CASES:
        g = np.load(ROOT / "tests" / "golden" / f"ovo_n{n}_seed{seed}.npz")
        X, labels, Xt, C, gamma = g["X"], g["labels"], g["Xt"], float(g["C"]), float(g["gamma"])
        mn, mx = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
        Xs, Xts = scale(X, mn, mx), scale(Xt, mn, mx)
        classes = np.unique(labels)
        k = len(classes)
        cls = np.searchsorted(classes, labels)
        folds = stratified_folds(cls, FOLDS, seed)
        cv_decision = np.zeros((n, k - 1))
        probA, probB, status = [], [], []
        for a in range(k):
            for b in range(a + 1, k):
                rows = np.flatnonzero((cls == a) | (cls == b))
                y = np.where(cls[rows] == a, 1, -1)
                dec = np.zeros(len(rows))
                for j in np.unique(folds[rows]):
                    te = folds[rows] == j
                    m = SVC(kernel="rbf", C=C, gamma=gamma, tol=TOL, cache_size=500).fit(Xs[rows[~te]], y[~te])
                    dec[te] = m.decision_function(Xs[rows[te]])  # classes_ = [-1, 1]: positive is a
                A, B = _sigmoid_calibration(dec, y)
                probA.append(float(A))
                probB.append(float(B))
                status.append(platt_fit(dec, y.astype(np.int32)).status)
                cv_decision[rows, np.where(cls[rows] == a, b - 1, a)] = dec
        if set(status) != {"converged"}:
            sys.exit(f"seed {seed}: sigmoid fits ended {status}: this fixture needs rows of its own with more overlap")
        full = SVC(C=C, gamma=gamma, tol=TOL, decision_function_shape="ovo", probability=True, random_state=0,
                   cache_size=500).fit(Xs, labels)
        full._probA = np.array(probA)
        full._probB = np.array(probB)
        proba = full.predict_proba(Xts)
        dst = ROOT / "tests" / "golden" / f"ovo_proba_n{n}_seed{seed}.npz"
        os.makedirs(dst.parent, exist_ok=True)
        np.savez_compressed(dst, folds=folds, cv_decision=cv_decision, probA=np.array(probA), probB=np.array(probB),
                            proba=proba, sklearn_version=np.array(sklearn.__version__))
        print(dst, dst.stat().st_size, "bytes", "k", k, "A in", [min(probA), max(probA)], "B in",
              [min(probB), max(probB)], "argmax = vote on", float(np.mean(classes[proba.argmax(1)] == g["predict"])))


if __name__ == "__main__":
    main()
