"""Cases and checks shared by the one-class SVM tests (test_oneclass_cpu.py, test_gpu_oneclass.py)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

FIXTURES = ((300, 21), (300, 22), (301, 23))  # (n, seed); nu = 0.2, 0.05, 0.5 (scripts/make_oneclass_golden.py)

# scikit-learn fixture (scripts/make_oneclass_golden.py, tol = 1e-6 on both sides): decision values scale with
# nu n (rho = 25.5, 5.8 and 75.5 in the three fixtures) and LIBSVM stops elsewhere in the same tau band, so the
# margin is measured, not derived -- the CPU oracles' largest |decision - fixture decision| was
#   seed 21 (nu 0.2):  pairwise 1.48e-6, decomposition 1.36e-6   (|rho - fixture| 1.2e-7 / 3.5e-7)
#   seed 22 (nu 0.05): pairwise 2.05e-6, decomposition 9.93e-7   (3.7e-8 / 1.5e-7)
#   seed 23 (nu 0.5):  pairwise 9.24e-7, decomposition 9.54e-7   (6.9e-8 / 2.8e-7)
# and the bound is 10 x the largest (2.052e-6), the margin and the reasoning of svr_checks.FIXTURE_PRED_TOL.  The
# GPU fit is held to the same number.
FIXTURE_DEC_TOL = 2.052e-5


def load_fixture(n: int, seed: int) -> dict:
    g = np.load(GOLDEN / f"oneclass_n{n}_seed{seed}.npz")
    out = {k: g[k] for k in ("X", "dual_coef", "support", "decision")}
    out.update({k: float(g[k]) for k in ("nu", "gamma", "rho")})
    return out


def check_kkt(K, alpha, rho, nu, tau, eps=1e-12):
    """The optimality conditions the stop rule b_low <= b_high + 2 tau implies, with rho its midpoint and f = K
    alpha: the box and the equality sum alpha = nu n; a variable strictly inside the box has |f_i - rho| <= tau; at
    0 it has f_i >= rho - tau, at 1 f_i <= rho + tau.  The nu-property follows from these (a point with f_i < rho -
    tau is at 1, and every point at 1 is a support vector): #{f_i < rho - tau} <= nu n <= #{alpha_i > eps}."""
    n = alpha.shape[0]
    f = K @ alpha
    slack = tau + 1e-9
    assert np.all(alpha >= 0) and np.all(alpha <= 1)
    assert abs(alpha.sum() - nu * n) <= 1e-9 * n, alpha.sum() - nu * n
    free, zero, full = (alpha > eps) & (alpha < 1 - eps), alpha <= eps, alpha >= 1 - eps
    assert np.all(np.abs(f[free] - rho) <= slack), np.abs(f[free] - rho).max()
    assert np.all(f[zero] >= rho - slack)
    assert np.all(f[full] <= rho + slack)
    assert int((f < rho - slack).sum()) <= nu * n <= int((alpha > eps).sum())
