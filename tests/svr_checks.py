"""Cases and checks shared by the epsilon-SVR tests (test_svr_cpu.py, test_gpu_svr.py)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

# scikit-learn fixture (scripts/make_svr_golden.py, tol = 1e-6 on both sides): the two solvers stop at different
# points of the same tau-band, so the margin is measured, not derived -- the CPU oracles' largest |prediction -
# fixture| over both seeds was 5.29e-6 (pairwise, seed 11; decomposition 5.03e-6; seed 12: 2.73e-6 / 2.26e-6),
# and the bound is 10 x that.  The GPU fit is held to the same number.
FIXTURE_PRED_TOL = 5.3e-5


def load_fixture(seed: int) -> dict:
    g = np.load(GOLDEN / f"svr_n300_seed{seed}.npz")
    out = {k: g[k] for k in ("X", "z", "pred", "beta")}
    out.update({k: float(g[k]) for k in ("C", "gamma", "epsilon", "intercept")})
    out["n_sv"] = int(g["n_sv"])
    return out


def real_rows(n: int, seed: int, d: int = 8, noise: float = 0.05, bounds_of=None):
    """n x d real-valued rows in [0, 1] and a smooth target with noise.  Every column's smallest entry is exactly
    0 and its largest exactly 1, so min-max scaling is the identity (bounds_of given: rows for prediction,
    left as drawn)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    if bounds_of is None:
        for j in range(d):
            X[np.argmin(X[:, j]), j] = 0.0
            X[np.argmax(X[:, j]), j] = 1.0
    z = np.sin(X @ np.linspace(-2.0, 2.0, d)) + noise * rng.normal(size=n)
    return np.ascontiguousarray(X), np.ascontiguousarray(z)


def rbf_numpy(A, B, gamma):
    d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
    return np.exp(-gamma * d2)


def check_kkt(K, z, a, a_star, b, C, epsilon, tau, eps=1e-12):
    """The optimality conditions the stop rule b_low <= b_high + 2 tau implies, with b its midpoint and r = z -
    (K beta - b): a variable strictly inside its box has its f within tau of b (|r - epsilon| <= tau for a_k,
    |r + epsilon| <= tau for a*_k); at 0 it is on the feasible side (r <= epsilon + tau for a_k, r >= -epsilon -
    tau for a*_k: together |r| <= epsilon + tau where beta_k = 0); at C on the other (r >= epsilon - tau, r <=
    -epsilon + tau).  The equality constraint and the box hold as well."""
    n = z.shape[0]
    beta = a - a_star
    r = z - (K @ beta - b)
    slack = tau + 1e-9
    assert np.all(a >= 0) and np.all(a <= C) and np.all(a_star >= 0) and np.all(a_star <= C)
    assert abs(beta.sum()) <= 1e-9 * C * n
    free, zero, full = (a > eps) & (a < C - eps), a <= eps, a >= C - eps
    assert np.all(np.abs(r[free] - epsilon) <= slack), np.abs(r[free] - epsilon).max()
    assert np.all(r[zero] <= epsilon + slack)
    assert np.all(r[full] >= epsilon - slack)
    free, zero, full = (a_star > eps) & (a_star < C - eps), a_star <= eps, a_star >= C - eps
    assert np.all(np.abs(r[free] + epsilon) <= slack), np.abs(r[free] + epsilon).max()
    assert np.all(r[zero] >= -epsilon - slack)
    assert np.all(r[full] <= -epsilon + slack)
    none = (a <= eps) & (a_star <= eps)
    assert np.all(np.abs(r[none]) <= epsilon + slack)
