"""Writes tests/golden/degenerate_svr_n240.npz and degenerate_svc_n330.npz: scikit-learn's (LIBSVM's) solutions
on training sets with identical rows that carry conflicting labels or different targets (the degenerate-pair
tests compare against them; LIBSVM floors a non-positive curvature and lets the box clip the step).

* svr_n240: tests/degenerate_checks.real_svr() -- 200 x 8 real rows in [0, 1] (exact column bounds: min-max
  scaling is the identity) and 40 replicates of the first rows with targets + 0.5 N(0, 1); SVR(C=10, gamma=0.5,
  epsilon=0.1, tol=1e-6).  Stored: X, z, the parameters, the predictions on X.
* svc_n330: tests/degenerate_checks.svc_fixture_rows() -- 300 random uint8 rows (d = 10) and 30 copies with
  flipped labels; SVC(C=10, gamma=0.05, tol=1e-6) on the rows / 255 (their min-max scaling).  Stored: X, y, the
  conflicting pairs, the parameters, the decision values on X.

The tests read the files and do not import scikit-learn.

    python scripts/make_degenerate_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    import sklearn
    from sklearn.svm import SVC as SkSVC
    from sklearn.svm import SVR as SkSVR

    import degenerate_checks as G

    dst = ROOT / "tests" / "golden"
    os.makedirs(dst, exist_ok=True)
    ver = np.array(sklearn.__version__)

    X, z = G.real_svr()
    C, gamma, epsilon = 10.0, G.REAL_GAMMA, 0.1
    m = SkSVR(kernel="rbf", C=C, gamma=gamma, epsilon=epsilon, tol=1e-6, cache_size=500).fit(X, z)
    out = dst / "degenerate_svr_n240.npz"
    np.savez_compressed(out, X=X, z=z, C=np.array(C), gamma=np.array(gamma), epsilon=np.array(epsilon),
                        pred=m.predict(X), n_sv=np.array(len(m.support_)), sklearn_version=ver)
    print(out, out.stat().st_size, "bytes", "n_sv", len(m.support_))

    X, y, pairs = G.svc_fixture_rows()
    C, gamma = 10.0, 0.05
    Xs = X.astype(np.float64) / 255.0
    m = SkSVC(kernel="rbf", C=C, gamma=gamma, tol=1e-6, cache_size=500).fit(Xs, y)
    out = dst / "degenerate_svc_n330.npz"
    np.savez_compressed(out, X=X, y=y, pairs=pairs, C=np.array(C), gamma=np.array(gamma),
                        dec=m.decision_function(Xs), n_sv=np.array(len(m.support_)), sklearn_version=ver)
    print(out, out.stat().st_size, "bytes", "n_sv", len(m.support_))


if __name__ == "__main__":
    main()
