"""Writes tests/golden/oneclass_n300_seed21.npz (nu = 0.2), oneclass_n300_seed22.npz (nu = 0.05) and
oneclass_n301_seed23.npz (nu = 0.5: nu n = 150.5, a fractional start point): scikit-learn's (LIBSVM's) one-class
SVM solutions the one-class tests compare against.

Rows: tests/svr_checks.real_rows(n, seed) -- n x 8 uniform real values with every column's smallest entry exactly
0 and its largest exactly 1, so the solvers' min-max scaling is the identity (the GPU solver needs scale=True).
Stored: X, nu, gamma, and of sklearn.svm.OneClassSVM(kernel="rbf", gamma=0.5, nu=nu, tol=1e-6): the dual
coefficients (LIBSVM's scaling: 0 <= alpha <= 1, sum = nu n), the support indices, rho (= offset_ = -intercept_)
and the decision values on X.  The tests read the files and do not import scikit-learn.

    python scripts/make_oneclass_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

CASES = ((300, 21, 0.2), (300, 22, 0.05), (301, 23, 0.5))  # n, seed, nu
GAMMA = 0.5


def main() -> None:
    import sklearn
    from sklearn.svm import OneClassSVM as SkOneClassSVM

    from svr_checks import real_rows

    for n, seed, nu in CASES:
        X, _ = real_rows(n, seed)
        m = SkOneClassSVM(kernel="rbf", gamma=GAMMA, nu=nu, tol=1e-6, cache_size=500).fit(X)
        dst = ROOT / "tests" / "golden" / f"oneclass_n{n}_seed{seed}.npz"
        os.makedirs(dst.parent, exist_ok=True)
        np.savez_compressed(dst, X=X, nu=np.array(nu), gamma=np.array(GAMMA), dual_coef=m.dual_coef_[0],
                            support=m.support_.astype(np.int64), rho=np.array(float(m.offset_[0])),
                            decision=m.decision_function(X), sklearn_version=np.array(sklearn.__version__))
        dec = m.decision_function(X)
        free = int(np.sum((m.dual_coef_[0] > 1e-12) & (m.dual_coef_[0] < 1 - 1e-12)))
        print(dst, dst.stat().st_size, "bytes", "n_sv", len(m.support_), "sum", m.dual_coef_.sum(), "free", free,
              "negative", int((dec < 0).sum()), "rho", float(m.offset_[0]))


if __name__ == "__main__":
    main()
