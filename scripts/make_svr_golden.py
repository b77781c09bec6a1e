"""Writes tests/golden/svr_n300_seed{11,12}.npz: scikit-learn's (LIBSVM's) epsilon-SVR solutions the SVR tests
compare against.

Rows: 300 x 8 uniform real values, with every column's smallest entry set to exactly 0 and its largest to
exactly 1, so the solvers' min-max scaling is the identity (the GPU solver needs scale=True).  Targets: a sine
of a random projection plus noise.  Stored: X, z, C, gamma, epsilon, the predictions on X and the intercept of
sklearn.svm.SVR(kernel="rbf", tol=1e-6), its dual coefficients as a 300-vector (0 off the support) and its
support-vector count.  The tests read the files and do not import scikit-learn.

    python scripts/make_svr_golden.py
"""
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SEEDS = (11, 12)
N, D = 300, 8
C, GAMMA, EPSILON = 10.0, 0.5, 0.1


def rows_and_targets(seed: int):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, D))
    for j in range(D):  # exact column bounds: min-max scaling leaves the rows as they are
        X[np.argmin(X[:, j]), j] = 0.0
        X[np.argmax(X[:, j]), j] = 1.0
    z = np.sin(X @ rng.normal(size=D)) + 0.05 * rng.normal(size=N)
    return X, z


def main() -> None:
    import sklearn
    from sklearn.svm import SVR as SkSVR

    for seed in SEEDS:
        X, z = rows_and_targets(seed)
        m = SkSVR(kernel="rbf", C=C, gamma=GAMMA, epsilon=EPSILON, tol=1e-6, cache_size=500).fit(X, z)
        beta = np.zeros(N)
        beta[m.support_] = m.dual_coef_[0]
        dst = ROOT / "tests" / "golden" / f"svr_n300_seed{seed}.npz"
        os.makedirs(dst.parent, exist_ok=True)
        np.savez_compressed(dst, X=X, z=z, C=np.array(C), gamma=np.array(GAMMA), epsilon=np.array(EPSILON),
                            pred=m.predict(X), beta=beta, intercept=np.array(float(m.intercept_[0])),
                            n_sv=np.array(len(m.support_)), sklearn_version=np.array(sklearn.__version__))
        print(dst, dst.stat().st_size, "bytes", "n_sv", len(m.support_))


if __name__ == "__main__":
    main()
