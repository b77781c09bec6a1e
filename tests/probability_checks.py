"""Cases and checks shared by the probability / cross-validation tests (test_probability_cpu.py,
test_gpu_probability.py)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

FIXTURES = ((300, 31), (301, 32))  # (n, seed); 50 % and about 30 % positives (scripts/make_probability_golden.py)

# scikit-learn fixtures (scripts/make_probability_golden.py; C = 10, gamma = 0.5, tol = 1e-6 on both sides).  Both
# sides stop anywhere inside the same tau band, so the margins are measured, not derived: the CPU estimator
# (SVC(device="cpu", probability=True, tol=1e-6), the pairwise oracle per fold) deviated from the fixtures by at most
#   seed 31: held-out decisions 7.139e-6, (A, B) 6.419e-7, probabilities of the 50 extra rows 1.234e-6
#   seed 32: held-out decisions 5.799e-6, (A, B) 6.227e-8, probabilities of the 50 extra rows 1.342e-6
# and each bound is 10 x the larger of its two figures (the rule of oneclass_checks.FIXTURE_DEC_TOL).  The (A, B)
# figure also holds scikit-learn's own optimiser (L-BFGS on the same objective and targets) against Newton's stop
# rule.  The GPU estimator is held to the same numbers.
FIXTURE_DEC_TOL = 7.139e-5
FIXTURE_AB_TOL = 6.419e-6
FIXTURE_PROBA_TOL = 1.342e-5

GRAD_TOL = 1e-5  # LIBSVM's stop rule for the sigmoid fit: both gradient components below it


def proba_rows(n: int, seed: int, positives: float = 0.5):
    """(X, y, Xq): n x 6 uniform rows whose every column has smallest entry exactly 0 and largest exactly 1, labels
    +1 for about ``positives`` of the rows (the upper quantile of a smooth score plus noise, so the classes
    overlap), and 50 more rows inside the same bounds."""
    rng = np.random.default_rng(seed)
    X = rng.random((n, 6))
    for c in range(6):
        X[np.argmin(X[:, c]), c] = 0.0
        X[np.argmax(X[:, c]), c] = 1.0
    score = X[:, 0] + X[:, 1] * X[:, 2] - 0.5 * (X[:, 3] - 0.5) ** 2 + 0.15 * rng.standard_normal(n)
    y = np.where(score > np.quantile(score, 1.0 - positives), 1, -1).astype(np.int32)
    Xq = 0.02 + 0.96 * rng.random((50, 6))
    return X, y, Xq


def load_fixture(n: int, seed: int) -> dict:
    g = np.load(GOLDEN / f"proba_n{n}_seed{seed}.npz")
    out = {k: g[k] for k in ("X", "y", "folds", "cv_decision", "Xq", "proba")}
    out.update({k: float(g[k]) for k in ("A", "B", "C", "gamma")})
    return out


def fixture_deviation(m, g) -> tuple:
    """(held-out decisions, (A, B), probabilities): the largest absolute deviations of a fitted estimator from a
    fixture."""
    return (float(np.abs(m.cv_decision_ - g["cv_decision"]).max()),
            max(abs(m.probA_ - g["A"]), abs(m.probB_ - g["B"])),
            float(np.abs(m.predict_proba(g["Xq"]) - g["proba"]).max()))


def check_fixture(m, g, seed) -> None:
    d, ab, p = fixture_deviation(m, g)
    print(f"seed {seed}: max |cv decision - fixture| = {d:.3e} (bound {FIXTURE_DEC_TOL:.3e}), |(A, B) - fixture| = "
          f"{ab:.3e} (bound {FIXTURE_AB_TOL:.3e}), |proba - fixture| = {p:.3e} (bound {FIXTURE_PROBA_TOL:.3e})")
    np.testing.assert_array_equal(m.cv_folds_, g["folds"])
    assert d <= FIXTURE_DEC_TOL
    assert ab <= FIXTURE_AB_TOL
    assert p <= FIXTURE_PROBA_TOL


def platt_gradient(dec, y, A, B, use=None) -> tuple:
    """Both components of the gradient of Platt's objective at (A, B), recomputed in FP64 with LIBSVM's targets."""
    dec, y = np.asarray(dec, dtype=np.float64), np.asarray(y)
    if use is not None:
        dec, y = dec[np.asarray(use, dtype=bool)], y[np.asarray(use, dtype=bool)]
    npos, nneg = int((y > 0).sum()), int((y <= 0).sum())
    t = np.where(y > 0, (npos + 1.0) / (npos + 2.0), 1.0 / (nneg + 2.0))
    z = A * dec + B
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    d1 = t - p
    return float(np.sum(dec * d1)), float(np.sum(d1))


def platt_cases():
    """The four synthetic (decision, label) sets of the sigmoid tests, by name."""
    out = {}
    rng = np.random.default_rng(7)
    y = np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int32)
    f = y * rng.uniform(0.5, 12.0, 64)  # nearly separable, |f| up to 12: the overflow-safe branches
    f[:4] *= -0.2
    f[5], f[6] = 12.0, -12.0
    out["n64_separable"] = (f, y)
    for name, n, pos in (("n300", 300, 0.5), ("n301_30pct", 301, 0.3), ("n5000", 5000, 0.5)):
        y = np.where(rng.random(n) < pos, 1, -1).astype(np.int32)
        out[name] = (1.2 * y + 1.5 * rng.standard_normal(n), y)
    return out


def synthetic_pairs(n: int, seed: int):
    """n overlapping (decision, label) pairs with both classes present (n >= 2)."""
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(n) < 0.4, 1, -1).astype(np.int32)
    if n >= 2:
        y[0], y[-1] = 1, -1
    return 1.0 * y + 1.5 * rng.standard_normal(n), y


def block0_mask(n: int, per: int = 63) -> np.ndarray:
    """Rows 0 .. per - 1 (all of selection block 0 at n = 2,000, q = 64) plus every 5th row."""
    m = np.zeros(n, dtype=bool)
    m[:per] = True
    m[::5] = True
    return m


def check_kkt_training_part(K, y, alpha, b, mask, Cp, Cn, tau, eps=1e-12):
    """The optimality conditions of the training part (rows outside the mask) that the stop rule implies, with
    f = K (alpha y) - y recomputed: a free variable has |f_i - b| <= tau, and a bound one lies on its side."""
    tr = ~mask
    Kt, yt, a = K[np.ix_(tr, tr)], y[tr].astype(np.float64), alpha[tr]
    f = Kt @ (a * yt) - yt
    box = np.where(yt > 0, Cp, Cn)
    slack = tau + 1e-9
    # a few ulps outside the box are the solvers' own (a_i moves by a_j's rounded step): check_warm_start's slack
    assert np.all(a >= -1e-9 * box) and np.all(a <= box * (1 + 1e-9))
    assert abs(np.dot(a, yt)) <= 1e-9 * max(1.0, a.sum())
    high = ((yt > 0) & (a < box - eps)) | ((yt < 0) & (a > eps))
    low = ((yt > 0) & (a > eps)) | ((yt < 0) & (a < box - eps))
    assert np.all(f[high] >= b - slack), (b - f[high]).max()
    assert np.all(f[low] <= b + slack), (f[low] - b).max()
