"""Writes tests/golden/dist_n300.npz: scikit-learn's (LIBSVM's) SVC and epsilon-SVR solutions with the laplacian and
chi2 kernels that the distance-kernel tests compare against.

Rows: kfun_checks.rows_labels_targets(300, 21) -- 300 x 20 uniform values whose min-max scaling is the identity -- and
50 held-out rows of the same kind (seed 99).  scikit-learn has neither kernel in its SVMs, so the fits are
sklearn.svm.SVC / SVR(kernel="precomputed", tol=1e-6) on sklearn.metrics.pairwise.laplacian_kernel / chi2_kernel with
the parameters of tests/dist_checks.py; the file holds their decision values / predictions on the held-out rows.  The
tests read the file and do not import scikit-learn.

    python scripts/make_dist_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from dist_checks import KERNELS  # noqa: E402
from kfun_checks import C, EPSILON, N, SEED, rows_labels_targets  # noqa: E402


def main() -> None:
    import sklearn
    from sklearn.metrics.pairwise import chi2_kernel, laplacian_kernel
    from sklearn.svm import SVC as SkSVC, SVR as SkSVR

    X, y, z = rows_labels_targets(N, SEED)
    Xq = rows_labels_targets(50, 99)[0]
    out = {"X": X, "y": y, "z": z, "Xq": Xq, "sklearn_version": np.array(sklearn.__version__)}
    for name, kw in KERNELS.items():
        gram = {"laplacian": laplacian_kernel, "chi2": chi2_kernel}[name]
        K, Kq = gram(X, X, gamma=kw["gamma"]), gram(Xq, X, gamma=kw["gamma"])
        sk = dict(kernel="precomputed", C=C, tol=1e-6, cache_size=500)
        out[f"svc_{name}"] = SkSVC(**sk).fit(K, y).decision_function(Kq)
        out[f"svr_{name}"] = SkSVR(epsilon=EPSILON, **sk).fit(K, z).predict(Kq)
    dst = ROOT / "tests" / "golden" / "dist_n300.npz"
    os.makedirs(dst.parent, exist_ok=True)
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
