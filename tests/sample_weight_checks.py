"""What the sample-weight tests share: the seeded inputs, the scikit-learn fixture and the KKT check in numpy."""
from pathlib import Path

import numpy as np

WEIGHT_SET = np.array([0.0, 1e-3, 0.5, 1.0, 3.0, 100.0])  # boxes over five decades, some points frozen
GAMMA, BOX, EPSILON = 0.5, 2.0, 0.05


def problem(n, seed, d=8, u8=False):
    """Rows in [0, 1] whose every column holds a 0 and a 1 (min-max scaling is the identity; u8: bytes whose every
    column holds 0 and 255, scaled rows = bytes / 255), labels with both classes weighted, targets, weights.
    Returns (X as stored, the scaled rows, y, z, w)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 256, (n, d)).astype(np.uint8) if u8 else rng.random((n, d))
    X[0], X[1] = 0, (255 if u8 else 1.0)
    Xs = X / 255.0 if u8 else X
    s = np.sin(3.0 * Xs[:, 0]) + Xs[:, 1] * Xs[:, 2] - Xs[:, 3]
    y = np.where(s > np.median(s), 1, -1).astype(np.int32)
    y[0], y[1] = 1, -1
    w = rng.choice(WEIGHT_SET, n)
    w[0], w[1] = 0.5, 3.0  # a positive weight in each class
    return X, Xs, y, s + 0.1 * rng.standard_normal(n), w


def load_fixture():
    return dict(np.load(Path(__file__).parent / "golden" / "sample_weight_n300.npz"))


def rbf(A, B, gamma):
    d2 = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
    return np.exp(-gamma * np.maximum(d2, 0.0))


def check_kkt(m, Xs, target, w, tol):
    """The fitted estimator's alpha against the weighted dual's conditions, in numpy float64: the box of every point
    exactly, frozen points, the equality, and the gap over the sets defined with C_i."""
    p, n = m.params, len(w)
    K = rbf(Xs, Xs, p.gamma)
    if hasattr(m, "alpha_star_"):  # SVR: a then a*, both on row k's box
        a, s = np.r_[m.alpha_, m.alpha_star_], np.r_[np.ones(n), -np.ones(n)]
        box = np.tile(p.C * w, 2)
        f = np.tile(K @ (m.alpha_ - m.alpha_star_), 2) + np.r_[m.epsilon - target, -m.epsilon - target]
    else:
        a, s, box = m.alpha_, target.astype(np.float64), p.box(target) * w
        f = K @ (a * s) - s
    assert np.all(a >= 0.0) and np.all(a <= box)
    assert np.all(a[np.tile(w, len(a) // n) == 0] == 0.0) and not np.isin(np.flatnonzero(w == 0), m.support_).any()
    assert abs(np.sum(s * a)) <= len(a) * box.max() * 2.0 ** -50
    hi = ((s == 1) & (a < box - p.eps)) | ((s == -1) & (a > p.eps))
    lo = ((s == 1) & (a > p.eps)) | ((s == -1) & (a < box - p.eps))
    gap = f[lo].max() - f[hi].min()
    print(f"{type(m).__name__}: gap {gap:.3e}, {len(m.support_)} support vectors, {np.count_nonzero(a == box)} at their box")
    assert gap <= 2 * tol + 1e-9
