"""Cases and checks shared by the nu-SVC / nu-SVR tests (test_nusvm_cpu.py, test_gpu_nusvm.py)."""
import numpy as np

from svr_checks import real_rows

# NuSVC against SVC(C = 1 / r_) on the same rows: one problem, two tau-optimal points of it, so the margin is
# measured, not derived.  The CPU nu oracle against the CPU SVC (test_nusvm_cpu.py prints it): the largest
# |decision difference| on held-out rows was 2.970e-5 (n = 300, nu = 0.4, gamma = 0.5, tol = 1e-5; decisions are
# scaled by 1 / r).  The bound is 10 x that, the margin and the reasoning of svr_checks.FIXTURE_PRED_TOL; the GPU
# fit is held to the same number.
SVC_EQUIV_TOL = 2.97e-4

# (n, q): one selection block row of 8 blocks with 32 picks per list, and 32 blocks with 2
SHAPES = ((300, 1024), (1537, 256))


def labels(X, z, kind="mixed"):
    """+1 / -1 labels from the smooth target of ``real_rows``: "mixed" (by the median), "sorted" (the same, rows
    reordered so the first blocks hold one class only: returns the order too) or "skew" (1 : 3)."""
    cut = np.median(z) if kind != "skew" else np.quantile(z, 0.75)
    y = np.where(z > cut, 1, -1).astype(np.int32)
    if kind == "sorted":
        order = np.argsort(-y, kind="stable")
        return np.ascontiguousarray(X[order]), y[order]
    return X, y


def nusvc_case(n, seed, kind="mixed"):
    X, z = real_rows(n, seed=seed)
    return labels(X, z, kind)


def nu_feasible(y, nu):
    return nu * len(y) / 2.0 <= min(int((y == 1).sum()), int((y == -1).sum()))


def check_kkt(K, s, p, a, box, total, r, rho, tau, eps=1e-12):
    """The optimality conditions the stop rule max_c (b_low_c - b_high_c) <= 2 tau implies, from an FP64 kernel
    matrix K: signs s, linear term p, alpha a (nu-SVC: before the division by r), f = K (a s) + p, and per class
    b_+ = rho + r, b_- = rho - r.  The box and both equalities hold; a free point has |f - b_c| <= tau; a + point
    at 0 / a - point at the box is in I_high only (f >= b_c - tau), a + point at the box / a - point at 0 in I_low
    only (f <= b_c + tau)."""
    n = len(a)
    f = K @ (a * s) + p
    slack = tau + 1e-9
    assert np.all(a >= -1e-12) and np.all(a <= box + 1e-12)
    assert abs((a * s).sum()) <= 1e-9 * n, (a * s).sum()
    assert abs(a.sum() - total) <= 1e-9 * n, a.sum() - total
    for sign, b in ((1, rho + r), (-1, rho - r)):
        c = s == sign
        free, zero, full = c & (a > eps) & (a < box - eps), c & (a <= eps), c & (a >= box - eps)
        assert np.all(np.abs(f[free] - b) <= slack), np.abs(f[free] - b).max()
        high_only, low_only = (zero, full) if sign == 1 else (full, zero)
        assert np.all(f[high_only] >= b - slack)
        assert np.all(f[low_only] <= b + slack)


def kkt_nusvc(K, y, alpha_scaled, r, rho, nu, tau):
    check_kkt(K, y.astype(np.float64), 0.0, alpha_scaled * r, 1.0, nu * len(y), r, rho, tau)


def kkt_nusvr(K, z, alpha2, C, r, rho, nu, tau):
    n = len(z)
    s = np.concatenate([np.ones(n), -np.ones(n)])
    K2 = np.block([[K, K], [K, K]])
    check_kkt(K2, s, np.concatenate([-z, -z]), alpha2, C, C * nu * n, r, rho, tau)


def compare_traces(dt, ot):
    """Two solvers' traces, record by record, bit for bit; the number of outer iterations."""
    dr, orr = dt.records(), ot.records()
    assert len(dr) == len(orr) and len(dr) > 0
    for o, (a, b) in enumerate(zip(dr, orr)):
        assert a["m"] == b["m"], o
        np.testing.assert_array_equal(a["W"], b["W"], err_msg=f"outer {o}: working set")
        assert a["inner"] == b["inner"], o
        np.testing.assert_array_equal(a["bounds"], b["bounds"], err_msg=f"outer {o}: bounds")
        np.testing.assert_array_equal(a["cols"], b["cols"], err_msg=f"outer {o}: moved points")
        np.testing.assert_array_equal(a["coef"], b["coef"], err_msg=f"outer {o}: coefficients")
        np.testing.assert_array_equal(a["alpha"], b["alpha"], err_msg=f"outer {o}: alpha")
        np.testing.assert_array_equal(a["f"], b["f"], err_msg=f"outer {o}: f")
    return len(dr)
