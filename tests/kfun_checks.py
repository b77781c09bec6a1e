"""Cases and bounds shared by the linear / polynomial / sigmoid kernel tests (test_kfun_cpu.py, test_gpu_kfun_*.py)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -53
N, D, SEED = 300, 20, 21
C, EPSILON = 1.0, 0.1
# estimator keywords per case; the sigmoid's gamma = 1 / d and coef0 = -1 keep its Gram close to positive
# semidefinite on rows in [0, 1], where scikit-learn and the CPU estimator agree as closely as for poly
KERNELS = {
    "linear": dict(kernel="linear"),
    "poly": dict(kernel="poly", degree=3, gamma=0.5, coef0=1.0),
    "sigmoid": dict(kernel="sigmoid", gamma=1.0 / D, coef0=-1.0),
}
# scikit-learn fixture (scripts/make_kernels_golden.py, tol = 1e-6 on both sides): the solvers stop at different
# points of the same tau-band, so the margin is measured, not derived (the rule of svr_checks.py).  The CPU
# estimators' largest |decision value - fixture| was, for (SVC, SVR): linear 2.06e-5 / 6.49e-6, poly 9.35e-6 /
# 2.28e-6, sigmoid 1.38e-6 / 1.37e-6; the bound is 10 x the larger of each pair.  The GPU fit is held to the same.
FIXTURE_TOL = {"linear": 2.06e-4, "poly": 9.35e-5, "sigmoid": 1.38e-5}


# the device's tanh against the longdouble reference's, measured through the store epilogue over the store test's
# range of arguments, t in [-1, 0], with t exact (d = 1, gamma = 1, coef0 = -1, x on a 2^-20 grid, z = 1) so that
# no dot-product error is mixed in (profiles/kernels.md); asserted at 4 x, since libm error varies with the argument
TANH_DEV = 5.82e-17


def rows_labels_targets(n: int, seed: int, d: int = D):
    """n x d real-valued rows in [0, 1] whose min-max scaling is the identity, +-1 labels and smooth targets."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    for j in range(d):
        X[np.argmin(X[:, j]), j] = 0.0
        X[np.argmax(X[:, j]), j] = 1.0
    w = np.linspace(-1.0, 1.0, d)
    y = np.where(X @ w + 0.3 * rng.normal(size=n) > 0, 1, -1).astype(np.int32)
    z = np.sin(X @ w) + 0.05 * rng.normal(size=n)
    return np.ascontiguousarray(X), y, np.ascontiguousarray(z)


def load_fixture() -> dict:
    g = np.load(GOLDEN / f"kfun_n{N}_seed{SEED}.npz")
    return {k: g[k] for k in g.files}


def kernel_ref(A, B, kernel="linear", degree=3, gamma=1.0, coef0=0.0):
    """(K, bound): the kernel block in longdouble rounded to float64, and the issue's elementwise bound of the
    device's float64 evaluation without the sigmoid's tanh term (the caller adds that)."""
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    d = A.shape[1]
    dot, adot = Al @ Bl.T, np.abs(Al) @ np.abs(Bl).T
    if kernel == "linear":
        return dot.astype(np.float64), ((d + 2) * U * adot).astype(np.float64)
    t = gamma * dot + coef0
    dt = (d + 3) * U * (gamma * adot + abs(coef0))
    if kernel == "sigmoid":
        return np.tanh(t).astype(np.float64), dt.astype(np.float64)
    K = t ** degree
    return K.astype(np.float64), (degree * np.abs(t) ** (degree - 1) * dt + (degree + 1) * U * np.abs(K)).astype(np.float64)
