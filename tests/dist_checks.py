"""Cases, the longdouble reference and the bounds shared by the laplacian / chi2 kernel tests (test_*dist_*.py)."""
import numpy as np

from kfun_checks import GOLDEN, U

# estimator keywords per case: on rows uniform in [0, 1] with d = 20 both give kernel values around 0.4
KERNELS = {"laplacian": dict(kernel="laplacian", gamma=0.1), "chi2": dict(kernel="chi2", gamma=0.25)}
# the device's exp against the longdouble reference's, measured through the store epilogue over the block test's range
# of arguments -gamma D in [-2, 0] with the argument exact (laplacian, d = 1, gamma = 2, z = 0 and x on a 2^-20 grid,
# so D = x and gamma D = 2 x carry no rounding; profiles/dist_kernels.md); asserted at 4 x
EXP_DEV = 9.14e-17
# |decision value| differences of two CPU fits of the same estimator at tol = 1e-5 and 1e-6 on the fit test's rows,
# largest over the 50 held-out rows, for (SVC, SVR): laplacian 4.81e-6 / 5.90e-6, chi2 6.60e-6 / 6.61e-6.  Both backends
# stop inside the same tau-band, so the GPU fit is held to 10 x the larger of each pair (the rule of svr_checks.py;
# profiles/dist_kernels.md).  The scikit-learn fixture (scripts/make_dist_golden.py, tol = 1e-6 on both sides) is held
# to the same margin.
DEC_TOL = {"laplacian": 5.90e-5, "chi2": 6.61e-5}
FIXTURE = GOLDEN / "dist_n300.npz"


def rows_with_zeros(n, d, seed):
    """n x d rows uniform in [0, 1] with about one value in six exactly 0, so that chi2 meets its 0 / 0 term."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, d))
    X[rng.random((n, d)) < 1.0 / 6.0] = 0.0
    return X


def kernel_ref(A, B, kernel, gamma, **_):
    """(K, bound): the kernel block in longdouble rounded to float64, and the elementwise bound of a float64 evaluation
    by one chain over k: K gamma c_d u D + 4 EXP_DEV, c_d = d + 1 (laplacian) or d + 4 (chi2) from one rounding per
    accumulate and the term's own operations.  Every term is >= 0, so D is also the sum of absolute terms."""
    a, b = A.astype(np.longdouble)[:, None, :], B.astype(np.longdouble)[None, :, :]
    s = a + b
    D = np.abs(a - b).sum(-1) if kernel == "laplacian" else np.where(s > 0, (a - b) ** 2 / np.where(s > 0, s, 1), 0).sum(-1)
    K, c = np.exp(-gamma * D), A.shape[1] + (1 if kernel == "laplacian" else 4)
    return K.astype(np.float64), (K * gamma * c * U * D).astype(np.float64) + 4 * EXP_DEV
