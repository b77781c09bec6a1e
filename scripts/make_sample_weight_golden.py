"""Writes tests/golden/sample_weight_n300.npz: the scikit-learn reference of the sample-weight tests.

Rows in [0, 1] whose every column holds a 0 and a 1 (min-max scaling is the identity), labels, targets, weights drawn
from {0, 1e-3, 0.5, 1, 3, 100}, 100 held-out rows, and the decision values of sklearn.svm.SVC / SVR fitted with
sample_weight twice: at tol = 1e-10 (the reference) and at the tests' tolerance (LIBSVM's tol is 2 x ours).  The
largest difference between the two runs, delta, is the reference's own sensitivity to the stop tolerance; the tests
allow 10 delta.  Needs numpy and scikit-learn only:  python scripts/make_sample_weight_golden.py
"""
from pathlib import Path

import numpy as np
from sklearn.svm import SVC, SVR

N, M, D, SEED = 300, 100, 8, 20260
C, GAMMA, EPSILON, TOL = 2.0, 0.5, 0.05, 1e-3  # TOL: the tests' stop tolerance (scikit-learn's default)


def main():
    rng = np.random.default_rng(SEED)
    X = rng.random((N, D))
    X[0], X[1] = 0.0, 1.0
    Xte = rng.random((M, D))
    s = np.sin(3.0 * X[:, 0]) + X[:, 1] * X[:, 2] - X[:, 3]
    y = np.where(s + 0.3 * rng.standard_normal(N) > np.median(s), 1, -1).astype(np.int32)
    z = s + 0.1 * rng.standard_normal(N)
    w = rng.choice([0.0, 1e-3, 0.5, 1.0, 3.0, 100.0], N)
    out = {"X": X, "Xte": Xte, "y": y, "z": z, "w": w, "C": C, "gamma": GAMMA, "epsilon": EPSILON, "tol": TOL}
    for name, make, t in (("svc", lambda tol: SVC(C=C, gamma=GAMMA, tol=tol, cache_size=200), y),
                          ("svr", lambda tol: SVR(C=C, gamma=GAMMA, epsilon=EPSILON, tol=tol), z)):
        ref = make(1e-10).fit(X, t, sample_weight=w)
        at = make(2 * TOL).fit(X, t, sample_weight=w)
        dec = (lambda m: m.decision_function(Xte)) if name == "svc" else (lambda m: m.predict(Xte))
        out[f"{name}_ref"], out[f"{name}_tol"] = dec(ref), dec(at)
        out[f"{name}_delta"] = float(np.max(np.abs(out[f"{name}_ref"] - out[f"{name}_tol"])))
        print(f"{name}: delta = {out[f'{name}_delta']:.3e}, {len(ref.support_)} support vectors")
    path = Path(__file__).resolve().parent.parent / "tests" / "golden" / "sample_weight_n300.npz"
    np.savez(path, **out)
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
