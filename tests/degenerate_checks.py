"""Cases and checks shared by the degenerate-pair tests (test_decomp_degenerate_cpu.py, test_gpu_degenerate.py)
and by scripts/make_degenerate_golden.py: training sets that hold identical rows with conflicting labels (or,
for regression, different targets).  Two such rows have K = 1, so their pair has eta = 2 - 2 K = 0 (or a few
1e-16 from the FP64 Gram) and is violating until one of them sits at a bound: the decomposition solver floors
eta at eps there and lets the box clip the step (LIBSVM's rule); the pairwise solvers keep the reference's stop.

Every case builder is cached and returns read-only arrays: compute once, share, leave unchanged."""
import functools
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

PIXEL_GAMMA = 0.00125
REAL_GAMMA = 0.5
INNER_WSS = (1, 2, 3, 4)
WORKING_SETS = (64, 1024)  # the copies spread over many working sets / inside one

# scikit-learn fixtures (scripts/make_degenerate_golden.py, tol = 1e-6 on both sides).  The solvers stop at
# different points of the same tau-band, so the margins are measured, not derived: the largest |oracle - fixture|
# over the CPU oracles (the decomposition oracle's arms inner_wss 1 / 2 / 3 / 4 x q = 64 / 1024, and the pairwise
# oracle, which converges on both: its first-order choice never picks a copy while the pair is violating) was
#   degenerate_svr_n240:  5.222e-6 (predictions; decomposition, q = 1024, inner_wss 3; pairwise 3.73e-6)
#   degenerate_svc_n330:  1.102e-5 (decision values; decomposition, q = 64, inner_wss 1; pairwise 1.06e-5)
# and the bounds are 10 x that, as svr_checks.FIXTURE_PRED_TOL is.  The GPU fits are held to the same numbers.
FIXTURE_SVR_TOL = 5.3e-5
FIXTURE_SVC_TOL = 1.11e-4


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def scaled(X):
    """Min-max scaled FP64 rows with the reference's degenerate-range rule, in plain numpy."""
    X = np.asarray(X, dtype=np.float64)
    mn, mx = X.min(0), X.max(0)
    return (X - mn) / np.where(mx - mn < 1e-12, 1.0, mx - mn)


def rbf_direct(Xs, gamma):
    """The independent FP64 RBF of already scaled rows: direct squared differences, in row chunks; the upper
    triangle's blocks are computed and mirrored ((a - b)^2 = (b - a)^2 term by term, so nothing is lost)."""
    n = Xs.shape[0]
    Xs = np.ascontiguousarray(Xs[:, Xs.max(0) != Xs.min(0)])  # a constant column's differences are exactly 0
    K = np.empty((n, n))
    step = max(1, int(2**24 // max(1, n * Xs.shape[1])))
    for i0 in range(0, n, step):
        diff = Xs[i0:i0 + step, None, :] - Xs[None, i0:, :]
        blk = np.exp(-gamma * np.einsum("ijk,ijk->ij", diff, diff))
        K[i0:i0 + step, i0:] = blk
        K[i0:, i0:i0 + step] = blk.T
    return K


def gap(K, y, a, C, eps=1e-12):
    """b_low - b_high over all points from the kernel matrix K (the reference's stop test is gap <= 2 tau)."""
    y = y.astype(np.float64)
    f = K @ (a * y) - y
    hi = ((y == 1) & (a < C - eps)) | ((y == -1) & (a > eps))
    lo = ((y == 1) & (a > eps)) | ((y == -1) & (a < C - eps))
    return f[lo].max() - f[hi].min()


def pairs_rest_at_a_bound(a, pairs, C, eps=1e-12):
    """Every conflicting pair (i, j) ends with at least one member at its bound C: f_j - f_i = 2 at every alpha,
    so the pair stays violating while both have room."""
    i, j = pairs[:, 0], pairs[:, 1]
    return bool(np.all((a[i] >= C - eps) | (a[j] >= C - eps)))


# ---- (a) pixel classifier: uint8 rows, the first k rows appended again with flipped labels ----------------------
@functools.lru_cache(maxsize=None)
def pixel_classifier(n, k):
    """synthetic_mnist(n, seed=91) plus its first k rows with flipped labels.  Returns (X uint8, y, pairs)."""
    from svm355.utils.data import synthetic_mnist

    tr = synthetic_mnist(n, seed=91).compact()
    assert tr.X.dtype == np.uint8
    X = np.ascontiguousarray(np.concatenate([tr.X, tr.X[:k]]))
    y = np.concatenate([tr.y, -tr.y[:k]]).astype(np.int32)
    pairs = np.stack([np.arange(k), n + np.arange(k)], axis=1)
    return _frozen(X, y, pairs)


PIXEL_SIZES = [(600, 40), (1500, 100)]


# ---- (b) real-valued classifier: FP64-MFMA kernel values between two copies are 1 or 1 - ulp --------------------
@functools.lru_cache(maxsize=None)
def real_classifier(n=1200, k=80, seed=5):
    """n real-valued rows (svr_checks.real_rows, d = 8: min-max scaling is the identity), labels by the median of
    the smooth target; each of the first k rows is followed by a copy with the flipped label (n + k rows).  The
    copies sit next to their originals, inside one selection block, so that a working set of 64 holds both members
    of a pair whatever the kernel values' last bits are: appended at the end, the q = 64 solve floored 3 times on
    the host's kernel values and not at all on 4 of 8 ulp-level perturbations of them; next to the originals,
    2 - 3 times on every one (45 - 71 times at q = 1024).  Returns (X, y, pairs)."""
    from svr_checks import real_rows

    X, z = real_rows(n, seed=seed)
    y0 = np.where(z > np.median(z), 1, -1).astype(np.int32)
    idx = np.concatenate([np.repeat(np.arange(k), 2), np.arange(k, n)])
    X = np.ascontiguousarray(X[idx])
    y = y0[idx].copy()
    y[1:2 * k:2] *= -1
    pairs = np.stack([np.arange(0, 2 * k, 2), np.arange(1, 2 * k, 2)], axis=1)
    return _frozen(X, y.astype(np.int32), pairs)


# ---- (c) regression: replicated rows with different targets -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_svr(n=200, k=40, seed=3):
    """real_rows(n, seed) plus k replicates of its first rows with targets + 0.5 N(0, 1) (the fixture's rows).
    Returns (X, z)."""
    from svr_checks import real_rows

    X, z = real_rows(n, seed=seed)
    rng = np.random.default_rng(0)
    X = np.ascontiguousarray(np.concatenate([X, X[:k]]))
    z = np.concatenate([z, z[:k] + rng.normal(size=k) * 0.5])
    return _frozen(X, z)


@functools.lru_cache(maxsize=None)
def pixel_svr(n=600, k=40):
    """The pixel classifier's rows with a float target (the row's mean intensity / 16); the appended copies'
    targets are shifted by +0.75 / -0.75 alternating.  Returns (X uint8, z)."""
    X, _, _ = pixel_classifier(n, k)
    m = X.astype(np.float64).mean(axis=1) / 16.0
    z = m.copy()
    z[n:] += np.where(np.arange(k) % 2 == 0, 0.75, -0.75)
    return _frozen(X, np.ascontiguousarray(z))


# ---- (d) heavily duplicated low-range integer data --------------------------------------------------------------
def low_range_problem(seed, n, d, vmax):
    """n rows of d integer columns in 0..vmax: at most (vmax + 1)^d distinct rows, 4 for d = 2 and vmax = 1, 256
    for d = 4 and vmax = 3.  Random labels and targets; rows 0 and 1 span every column's range and carry both
    classes.  Returns (X uint8, y, z)."""
    rng = np.random.default_rng(seed)
    X = np.floor(rng.random((n, d)) * (vmax + 1)).astype(np.uint8)
    X[0], X[1] = 0, vmax
    y = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int32)
    y[0], y[1] = 1, -1
    z = rng.normal(size=n)
    return X, y, z


def low_range_strategy():
    from hypothesis import strategies as st

    return st.tuples(st.integers(0, 2**31 - 1), st.integers(200, 1500), st.integers(2, 4), st.integers(1, 3),
                     st.sampled_from([1.0, 10.0, 100.0]), st.sampled_from([0.00125, 0.01, 0.05]))


# ---- scikit-learn fixtures --------------------------------------------------------------------------------------
SVC_FIXTURE_N, SVC_FIXTURE_K, SVC_FIXTURE_D = 300, 30, 10


def svc_fixture_rows():
    """300 random uint8 rows (d = 10; rows 0 and 1 span 0..255 in every column, so min-max scaling divides by
    255) and 30 copies of rows 2..31 with flipped labels.  Returns (X uint8, y, pairs)."""
    rng = np.random.default_rng(0)
    n, k, d = SVC_FIXTURE_N, SVC_FIXTURE_K, SVC_FIXTURE_D
    X = rng.integers(0, 256, size=(n, d)).astype(np.uint8)
    X[0], X[1] = 0, 255
    y = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int32)
    y[0], y[1] = 1, -1
    X = np.ascontiguousarray(np.concatenate([X, X[2:2 + k]]))
    y = np.concatenate([y, -y[2:2 + k]]).astype(np.int32)
    pairs = np.stack([2 + np.arange(k), n + np.arange(k)], axis=1)
    return X, y, pairs


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """name "svr_n240": X, z, pred, C, gamma, epsilon;  "svc_n330": X (uint8), y, pairs, dec, C, gamma."""
    g = np.load(GOLDEN / f"degenerate_{name}.npz")
    out = {}
    for key in g.files:
        v = g[key]
        if v.ndim == 0:
            out[key] = v.item()
        else:
            v.flags.writeable = False
            out[key] = v
    return out
