"""Checks and cases shared by the decomposition solver's tests (test_gpu_decomp.py, test_gpu_decomp_oracle.py,
test_gpu_newton_step.py, test_decomp_oracle_cpu.py) and by scripts/newton_probe.py."""
import functools

import numpy as np


def kkt_gap_fp64(X, y, a, p):
    """b_low - b_high over ALL points from an independent FP64 RBF (torch, min-max scaled rows)."""
    import torch

    dev = torch.device("cuda:0")
    Xs = torch.from_numpy(X.astype(np.float64)).to(dev)
    mn, mx = Xs.min(0).values, Xs.max(0).values
    rng = torch.where(mx - mn < 1e-12, torch.ones_like(mx), mx - mn)
    Xs = (Xs - mn) / rng
    sq = (Xs * Xs).sum(1)
    ay = torch.from_numpy(a * y).to(dev)
    f = torch.empty(len(y), dtype=torch.float64, device=dev)
    for i0 in range(0, len(y), 4096):
        B = Xs[i0:i0 + 4096] @ Xs.T
        Kb = torch.exp(-p.gamma * torch.clamp(sq[i0:i0 + 4096, None] + sq[None, :] - 2.0 * B, min=0.0))
        f[i0:i0 + 4096] = Kb @ ay
    f = f.cpu().numpy() - y
    hi = ((y == 1) & (a < p.C - p.eps)) | ((y == -1) & (a > p.eps))
    lo = ((y == 1) & (a > p.eps)) | ((y == -1) & (a < p.C - p.eps))
    return f[lo].max() - f[hi].min()


# ---- one Newton polish step (decomp_newton.h): working sets with an exact free count ---------------------------
NEWTON_C = 10.0
NEWTON_CAP = 512  # kNewtonMaxFree: the largest free set a step may have, on the device and in the reference
# (m, |F|): the 2-point minimum; one below / at / one above the factorisation's 16-column panel and the back
# substitution's 64-column block (and their multiples); the cap of 512 and one below it
NEWTON_SIZES = [(2, 2), (3, 2), (40, 3), (64, 15), (64, 16), (64, 17), (100, 63), (100, 64), (100, 65), (300, 128),
                (300, 129), (600, 255), (600, 257), (512, 512), (1024, 511), (1024, 512)]
# the sizes every workgroup shape runs: a panel boundary, a block boundary, both with more rows than threads, the cap
NEWTON_SIZES_EVERY_NT = [(64, 17), (100, 65), (600, 257), (1024, 512)]
NEWTON_SIZES_ABOVE_CAP = [(1024, 513), (1024, 640), (1024, 1024)]


@functools.lru_cache(maxsize=None)
def newton_gram(m):
    """The working set's kernel matrix and labels: m synthetic-MNIST points (seed 7), min-max scaled, the
    solver's RBF (gamma 0.00125) with a unit diagonal.  Shared between cases: read-only."""
    from svm355.utils.data import MinMaxScaler, synthetic_mnist

    tr = synthetic_mnist(m, seed=7)
    X = MinMaxScaler().fit_transform(tr.X)
    sq = np.einsum("ij,ij->i", X, X)
    K = np.exp(-0.00125 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * X @ X.T, 0.0))
    np.fill_diagonal(K, 1.0)
    y = tr.y.astype(np.int32)
    K.flags.writeable = False
    y.flags.writeable = False
    return K, y


def bordered_solve(KFF, fF):
    """The step's linear system by plain mathematics: K_FF u - b 1 = -f_F, 1^T u = 0, solved by LU
    (numpy.linalg.solve) with two rounds of iterative refinement on extended-precision residuals, so its own
    error is far below the FP64 Cholesky's.  Returns (u, b)."""
    nf = len(fF)
    M = np.zeros((nf + 1, nf + 1))
    M[:nf, :nf] = KFF
    M[:nf, nf] = -1.0
    M[nf, :nf] = 1.0
    rhs = np.concatenate([-np.asarray(fF, dtype=np.float64), [0.0]])
    x = np.linalg.solve(M, rhs).astype(np.longdouble)
    Ml, rl = M.astype(np.longdouble), rhs.astype(np.longdouble)
    for _ in range(2):
        r = (rl - Ml @ x).astype(np.float64)
        x = x + np.linalg.solve(M, r)
    x = x.astype(np.float64)
    return x[:nf], float(x[nf])


class NewtonCase:
    """K (m x m, read-only), y, alpha and f by position (fresh arrays), free: the ascending free positions;
    u: the constructed solution of kind "full" (else None)."""

    def __init__(self, K, y, a, f, free, u=None):
        self.K, self.y, self.a, self.f, self.free, self.u = K, y, a, f, free, u

    @property
    def KFF(self):
        return self.K[np.ix_(self.free, self.free)]

    def direction(self):
        """dalpha of the full step on F (y u) and b, from bordered_solve."""
        u, b = bordered_solve(self.KFF, self.f[self.free])
        return np.where(self.y[self.free] == 1, u, -u), b


def newton_case(m, nf, kind, cut_at=None, dup=None):
    """A working set of m points with exactly nf free ones (C = 10, eps = 1e-12): the free positions an
    ascending random subset with alpha = uniform(2, 8), every other alpha exactly 0 or exactly C at random.
      kind "cut":  f = K (alpha y) - y; the free optimum lies far outside the box, so for nf >= 3 the step is
                   cut at a bound (code 2).
      kind "full": u = uniform(-1, 1) minus its mean, f_F = 0.37 - K_FF u, f elsewhere normal(): the step's
                   exact solution is u with b = 0.37, inside the box (code 1).
      cut_at:      (kind "cut") the F position whose alpha is then moved to within 1e-9 of the bound it is
                   heading for (the direction from bordered_solve; f is left as it was, so the direction, a
                   function of K_FF and f_F only, is unchanged): the step is cut there.
      dup:         (i, j): point j becomes a copy of point i (row and column of K, the label), so a K_FF
                   holding both is singular."""
    K, y = newton_gram(m)
    if dup is not None:
        i, j = dup
        K, y = K.copy(), y.copy()
        K[j, :] = K[i, :]
        K[:, j] = K[:, i]
        y[j] = y[i]
        assert K[j, j] == 1.0 and K[i, j] == 1.0
    rng = np.random.default_rng(100003 * m + 17 * nf + (0 if kind == "cut" else 1))
    a = np.where(rng.random(m) < 0.5, 0.0, NEWTON_C)
    free = np.sort(rng.choice(m, size=nf, replace=False))
    a[free] = rng.uniform(2.0, 8.0, size=nf)
    u = None
    if kind == "cut":
        f = K @ (a * y) - y
    else:
        assert kind == "full"
        u = rng.uniform(-1.0, 1.0, size=nf)
        u -= u.mean()
        f = rng.normal(size=m)
        f[free] = 0.37 - K[np.ix_(free, free)] @ u
    case = NewtonCase(K, y, a, f, free, u)
    if cut_at is not None:
        assert kind == "cut"
        d, _ = case.direction()
        k = cut_at % nf
        a[free[k]] = NEWTON_C - 1e-9 if d[k] > 0.0 else 1e-9
        room = np.where(d > 0.0, NEWTON_C - a[free], a[free])
        tk = room / np.abs(d)
        assert d[k] != 0.0 and tk[k] < 0.5 * np.delete(tk, k).min(), "the forced cut is not the step's first bound"
    assert np.count_nonzero((a > 1e-12) & (a < NEWTON_C - 1e-12)) == nf
    return case
