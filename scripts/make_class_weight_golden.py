"""Writes tests/golden/class_weight_n600_seed77.npz: scikit-learn's (LIBSVM's) solution of the weighted
problems the class-weight tests compare against.

Rows: synthetic_mnist(600, seed=77), min-max scaled as the solvers scale them.  Per weight pair
(A: pos 2.0 / neg 0.5, B: pos 0.5 / neg 2.0): alpha (600 doubles, 0 off the support) and the intercept of
sklearn.svm.SVC(C=10, gamma=0.00125, tol=2e-7, class_weight={1: w_pos, -1: w_neg}).  The tests read the
file and do not import scikit-learn.

    python scripts/make_class_weight_golden.py
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PAIRS = {"A": (2.0, 0.5), "B": (0.5, 2.0)}


def main() -> None:
    import sklearn
    from sklearn.svm import SVC as SkSVC

    from svm355.utils.data import MinMaxScaler, synthetic_mnist

    ds = synthetic_mnist(600, seed=77)
    Xs = MinMaxScaler().fit(ds.X).transform(ds.X)
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (wp, wn) in PAIRS.items():
        m = SkSVC(C=10.0, kernel="rbf", gamma=0.00125, tol=2e-7, class_weight={1: wp, -1: wn}, cache_size=500)
        m.fit(Xs, ds.y)
        alpha = np.zeros(len(ds.y))
        alpha[m.support_] = np.abs(m.dual_coef_[0])
        # scikit-learn's decision is sum(alpha y K) + intercept with classes_ = [-1, 1]: positive = class +1
        assert list(m.classes_) == [-1, 1]
        assert np.array_equal(np.sign(m.dual_coef_[0]), ds.y[m.support_])
        out[f"alpha_{name}"] = alpha
        out[f"intercept_{name}"] = np.array(float(m.intercept_[0]))
        out[f"weights_{name}"] = np.array([wp, wn])
        box = np.where(ds.y == 1, 10.0 * wp, 10.0 * wn)
        bounded = alpha >= box * (1 - 1e-9)
        free = (alpha > 1e-8) & ~bounded
        print(name, {"bounded+": int((bounded & (ds.y == 1)).sum()), "bounded-": int((bounded & (ds.y == -1)).sum()),
                     "free+": int((free & (ds.y == 1)).sum()), "free-": int((free & (ds.y == -1)).sum())})
    dst = ROOT / "tests" / "golden" / "class_weight_n600_seed77.npz"
    os.makedirs(dst.parent, exist_ok=True)
    np.savez_compressed(dst, **out)
    print(dst, dst.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
