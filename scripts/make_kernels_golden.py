"""Writes tests/golden/kfun_n300_seed21.npz: scikit-learn's (LIBSVM's) SVC and epsilon-SVR solutions with the
linear, polynomial and sigmoid kernels that the kernel tests compare against.

Rows: 300 x 20 uniform real values, with every column's smallest entry set to exactly 0 and its largest to
exactly 1, so the solvers' min-max scaling is the identity.  Labels: the sign of a noisy linear score; targets: a
sine of a projection plus noise.  Per kernel (tests/kfun_checks.py has the parameters) the file holds the decision
values / predictions on X of sklearn.svm.SVC / SVR(tol=1e-6).  The tests read the file and do not import
scikit-learn.

    python scripts/make_kernels_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from kfun_checks import C, EPSILON, KERNELS, N, SEED, rows_labels_targets  # noqa: E402


def main() -> None:
    import sklearn
    from sklearn.svm import SVC as SkSVC, SVR as SkSVR

    X, y, z = rows_labels_targets(N, SEED)
    out = {"X": X, "y": y, "z": z, "sklearn_version": np.array(sklearn.__version__)}
    for name, kw in KERNELS.items():
        sk = dict(kernel=kw["kernel"], degree=kw.get("degree", 3), gamma=kw.get("gamma", 1.0), coef0=kw.get("coef0", 0.0),
                  C=C, tol=1e-6, cache_size=500)
        out[f"svc_{name}"] = SkSVC(**sk).fit(X, y).decision_function(X)
        out[f"svr_{name}"] = SkSVR(epsilon=EPSILON, **sk).fit(X, z).predict(X)
    dst = ROOT / "tests" / "golden" / f"kfun_n{N}_seed{SEED}.npz"
    os.makedirs(dst.parent, exist_ok=True)
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
