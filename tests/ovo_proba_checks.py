"""Cases, references and bounds shared by the pairwise-coupling tests (test_ovo_proba_cpu.py,
test_gpu_ovo_proba_kernel.py, test_gpu_ovo_proba.py)."""
from pathlib import Path

import numpy as np

from ovo_checks import load_fixture as load_ovo_fixture, pairs

GOLDEN = Path(__file__).resolve().parent / "golden"

# scikit-learn fixtures (scripts/make_ovo_proba_golden.py: the one-vs-one fixtures' rows, C = 10, gamma = 0.5,
# tol = 1e-6 on both sides, 5 folds).  Both sides stop anywhere inside the same tau band, and scikit-learn fits
# the sigmoid with another optimiser, so the margins are measured, not derived: the CPU estimator
# (OneVsOneSVC(device="cpu", cv=5, tol=1e-6) with the fixture's folds) deviated from the fixtures by at most
#   seed 41 (k = 3):  held-out decisions 2.078e-6, (A, B) 4.308e-7, probabilities of the 200 query rows 9.321e-7
#   seed 42 (k = 4):  held-out decisions 1.862e-6, (A, B) 1.254e-6, probabilities 5.948e-7
#   seed 43 (k = 10): held-out decisions 1.231e-6, (A, B) 4.506e-6, probabilities 4.807e-7
# and every bound is 10 x its fixture's figure (the rule of probability_checks.FIXTURE_DEC_TOL).  The GPU
# estimator is held to the same numbers.
FIXTURE_TOL = {  # seed: (held-out decisions, (A, B), probabilities)
    41: (2.078e-5, 4.308e-6, 9.321e-6),
    42: (1.862e-5, 1.254e-5, 5.948e-6),
    43: (1.231e-5, 4.506e-5, 4.807e-6),
}

# The coupling kernel with the sigmoid (A, B given) against the host twin on the same inputs: the device's exp is
# not the host's, so this is measured, not derived.  Over sigmoid_cases() on an MI355X the largest
# |device proba - ops.cpu.ovo_couple proba| was 3.331e-16 (a last-bit difference of exp, carried through the
# sweeps) and no row's sweep count differed; the bound is 10 x that.  (A 10,000-row block of a fitted model's
# decisions, outside these cases, measured 6.66e-16: profiles/ovo_proba.md.)
SIGMOID_DEVICE_DIFF = 3.331e-16
SIGMOID_TOL = 10 * SIGMOID_DEVICE_DIFF

MIN_PROB = 1e-7


def load_fixture(n: int, seed: int) -> dict:
    """The one-vs-one fixture (rows, labels, query rows, C, gamma) with its calibration arrays."""
    fx = load_ovo_fixture(n, seed)
    g = np.load(GOLDEN / f"ovo_proba_n{n}_seed{seed}.npz")
    fx.update({k: g[k] for k in ("folds", "cv_decision", "probA", "probB", "proba")})
    return fx


def fixture_deviation(m, fx) -> tuple:
    return (float(np.abs(m.cv_decision_ - fx["cv_decision"]).max()),
            float(max(np.abs(m.probA_ - fx["probA"]).max(), np.abs(m.probB_ - fx["probB"]).max())),
            float(np.abs(m.predict_proba(fx["Xt"]) - fx["proba"]).max()))


def check_fixture(m, fx, seed) -> None:
    d, ab, p = fixture_deviation(m, fx)
    td, tab, tp = FIXTURE_TOL[seed]
    print(f"seed {seed}: max |cv decision - fixture| = {d:.3e} (bound {td:.3e}), |(A, B) - fixture| = {ab:.3e} "
          f"(bound {tab:.3e}), |proba - fixture| = {p:.3e} (bound {tp:.3e}); sigmoid fits {sorted(set(m.platt_status_))}")
    np.testing.assert_array_equal(m.cv_folds_, fx["folds"])
    assert m.cv_decision_.shape == fx["cv_decision"].shape and m.probA_.shape == fx["probA"].shape
    assert d <= td
    assert ab <= tab
    assert p <= tp


def loop_couple(dec, A=None, B=None):
    """ops.cpu.ovo_couple by plain Python loops over rows, classes and pairs, in the order the issue fixes (the
    reference of the host twin).  Returns (proba, label, iters)."""
    import math

    dec = np.asarray(dec, dtype=np.float64)
    m, P = dec.shape
    k = int(round((1 + math.sqrt(1 + 8 * P)) / 2))
    pr = pairs(k)
    proba = np.empty((m, k))
    label = np.empty(m, dtype=np.int32)
    iters = np.empty(m, dtype=np.int32)
    for i in range(m):
        r = [[0.0] * k for _ in range(k)]
        for pi, (a, b) in enumerate(pr):
            v = float(dec[i, pi])
            if A is not None:
                z = v * float(A[pi]) + float(B[pi])
                if z >= 0.0:
                    e = math.exp(-z)
                    v = e / (1.0 + e)
                else:
                    v = 1.0 / (1.0 + math.exp(z))
            if v < MIN_PROB:
                v = MIN_PROB
            elif v > 1.0 - MIN_PROB:
                v = 1.0 - MIN_PROB
            r[a][b] = v
            r[b][a] = 1.0 - v
        if k == 2:
            p, it = [r[0][1], r[1][0]], 0
        else:
            Q = [[0.0] * k for _ in range(k)]
            for t in range(k):
                s = 0.0
                for j in range(k):
                    if j != t:
                        s += r[j][t] * r[j][t]
                        Q[t][j] = -r[j][t] * r[t][j]
                Q[t][t] = s
            p = [1.0 / k] * k
            Qp = [0.0] * k
            cap, eps = max(100, k), 0.005 / k
            it = 0
            while it < cap:
                for t in range(k):
                    s = 0.0
                    for j in range(k):
                        s += Q[t][j] * p[j]
                    Qp[t] = s
                pQp = 0.0
                for t in range(k):
                    pQp += p[t] * Qp[t]
                if all(abs(Qp[t] - pQp) < eps for t in range(k)):  # a NaN never passes
                    break
                for t in range(k):
                    diff = (-Qp[t] + pQp) / Q[t][t]
                    p[t] += diff
                    pQp = (pQp + diff * (diff * Q[t][t] + 2.0 * Qp[t])) / (1.0 + diff) / (1.0 + diff)
                    for j in range(k):
                        Qp[j] = (Qp[j] + diff * Q[t][j]) / (1.0 + diff)
                        p[j] /= (1.0 + diff)
                it += 1
        proba[i] = p
        best = 0
        for c in range(1, k):
            if p[c] > p[best]:
                best = c
        label[i], iters[i] = best, it
    return proba, label, iters


def pair_probabilities(m: int, k: int, seed: int, spread: float = 1.0) -> np.ndarray:
    """(m, P) pair probabilities of m rows with a latent class score each: r_ab = s_a / (s_a + s_b) with a little
    noise, inside (0.02, 0.98).  ``spread`` scales the scores' range: a wider one takes more sweeps."""
    rng = np.random.default_rng(seed)
    s = np.exp(spread * rng.normal(size=(m, k)))
    pr = pairs(k)
    r = np.stack([s[:, a] / (s[:, a] + s[:, b]) for a, b in pr], 1) + 0.05 * rng.normal(size=(m, len(pr)))
    return np.clip(r, 0.02, 0.98)


def mixed_sweeps_block(k: int, m: int, seed: int) -> np.ndarray:
    """m consecutive rows (k >= 3) whose sweep counts differ: rows 0, 3, ... hold 0.5 on every pair (the start
    1 / k passes the stop test: no sweep), rows 1, 4, ... have class i mod k at 0.999 against every other (the
    most sweeps), rows 2, 5, ... are noisy."""
    r = pair_probabilities(m, k, seed, 1.0)
    r[0::3] = 0.5
    for i in range(1, m, 3):
        r[i] = 0.5
        c = i % k
        for pi, (a, b) in enumerate(pairs(k)):
            if a == c:
                r[i, pi] = 0.999
            elif b == c:
                r[i, pi] = 0.001
    return r


def sigmoid_cases():
    """(name, dec (m, P), A, B) for the coupling with the sigmoid: decisions of a few units, A in LIBSVM's usual
    range (negative: a positive decision favours the pair's first class), small B."""
    out = []
    for k, m, seed in ((2, 5, 1), (3, 257, 2), (5, 64, 3), (10, 200, 4), (33, 9, 5), (64, 5, 6)):
        rng = np.random.default_rng(100 + seed)
        P = k * (k - 1) // 2
        out.append((f"k{k}_m{m}", 1.5 * rng.normal(size=(m, P)), -rng.uniform(1.0, 4.0, P), 0.3 * rng.normal(size=P)))
    return out


def extreme_case(k: int = 4):
    """z = +-800 on every pair of some rows: both clamps engage, nothing may come out non-finite."""
    P = k * (k - 1) // 2
    dec = np.zeros((4, P))
    dec[0], dec[1] = 800.0, -800.0
    dec[2, ::2], dec[2, 1::2] = 800.0, -800.0
    dec[3] = np.linspace(-800.0, 800.0, P)
    return dec, -np.ones(P), np.zeros(P)


def check_invariants(proba, r, k, iters=None):
    """Rows on the simplex within 1e-12 with positive entries, and the returned p meets the stop rule recomputed
    in numpy: max |Qp - pQp| < 0.005 / k + 1e-12 (the slack: last-bit differences of a recomputed Q, whose
    entries are at most 1).  r: (m, P) clamped pair probabilities.  Rows that ran into the cap are skipped for the
    stop rule (iters given)."""
    proba = np.asarray(proba)
    assert np.all(np.isfinite(proba))
    assert np.all(np.abs(proba.sum(1) - 1.0) <= 1e-12), np.abs(proba.sum(1) - 1.0).max()
    assert np.all(proba > 0.0)
    if k == 2:
        return
    pr = pairs(k)
    for i in range(proba.shape[0]):
        if iters is not None and iters[i] >= max(100, k):
            continue
        R = np.zeros((k, k))
        for pi, (a, b) in enumerate(pr):
            R[a, b], R[b, a] = r[i, pi], 1.0 - r[i, pi]
        Q = -R.T * R
        Q[np.diag_indices(k)] = (R * R).sum(0)
        Qp = Q @ proba[i]
        pQp = proba[i] @ Qp
        assert np.abs(Qp - pQp).max() < 0.005 / k + 1e-12, (i, np.abs(Qp - pQp).max())


def sigmoid_r(dec, A, B):
    """The clamped pair probabilities of (dec, A, B) in numpy (for check_invariants)."""
    z = dec * A + B
    e = np.exp(-np.abs(z))
    return np.clip(np.where(z >= 0, e / (1.0 + e), 1.0 / (1.0 + e)), MIN_PROB, 1.0 - MIN_PROB)
