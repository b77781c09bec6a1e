"""Cases and checks shared by the one-vs-one tests (test_ovo_cpu.py, test_gpu_ovo.py, test_gpu_ovo_kernel.py)."""
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

# (n, seed): k = 3 uint8 rows; k = 4 real-valued rows (class sizes 120 / 90 / 84 / 7); k = 10 uint8 rows, 45 pairs
# (scripts/make_ovo_golden.py)
FIXTURES = ((300, 41), (301, 42), (330, 43))
GRAM_PATHS = {41: "int8-exact", 42: "fp64", 43: "int8-exact"}
FIT = dict(C=10.0, gamma=0.5, tol=1e-6)

# scikit-learn fixture (tol = 1e-6 on both sides): LIBSVM stops elsewhere in the same tau band, so the margin is
# measured, not derived -- the largest |decision - fixture decision| of the CPU pair solves
# (OneVsOneSVC(device="cpu", tol=1e-6)) over the 200 query rows and all pairs was
#   n 300 seed 41 (k = 3):   2.571e-6
#   n 301 seed 42 (k = 4):   2.563e-6
#   n 330 seed 43 (k = 10):  1.117e-6
# and the bound is 10 x the largest (2.5712e-6), the margin and the reasoning of svr_checks.FIXTURE_PRED_TOL and
# oneclass_checks.FIXTURE_DEC_TOL.  The GPU fit is held to the same number.
FIXTURE_DEC_TOL = 2.5712e-5
# A query row with a pair decision this close to zero may take the other vote: such rows are left out of the
# prediction comparison, at most 2 % of the 200.  In the fixtures themselves 0, 0 and 1 rows are that close (the
# closest decisions are 1.2e-2, 1.4e-4 and 4.0e-6; in seed 43 the next is 3.3e-5).
EXCLUDED_CAP = 0.02

# Device against host prediction on one model: beyond the two summation orders (vote_bound) the device's
# cross-kernel differs from the host's rbf_matrix (another exp, the norm expansion against the direct sum of
# squared differences).  Measured on an MI355X over the three fixtures' query rows against their GPU models'
# support vectors: the largest |rbf_gram - rbf_matrix| was 1.554e-15 (seed 41), 1.554e-15 (seed 42) and 2.554e-15
# (seed 43); a decision moves by at most that times sum |coef|, and the tests allow 10 x the largest.  (The
# tests print the difference they see next to this number.)
CROSS_KERNEL_DIFF = 2.554e-15


def load_fixture(n: int, seed: int) -> dict:
    g = np.load(GOLDEN / f"ovo_n{n}_seed{seed}.npz")
    out = {k: g[k] for k in ("X", "labels", "Xt", "labels_t", "support", "n_support", "dual_coef", "intercept",
                             "decision", "predict")}
    out.update({k: float(g[k]) for k in ("gamma", "C")})
    return out


def pairs(k: int):
    return [(a, b) for a in range(k) for b in range(a + 1, k)]


def brute_votes(K, start, coef, rho):
    """ovo_votes by loops over rows, pairs and support vectors (the reference of the host twin)."""
    k = len(start) - 1
    m = K.shape[0]
    dec = np.zeros((m, k * (k - 1) // 2))
    lab = np.zeros(m, dtype=np.int32)
    for i in range(m):
        votes = [0] * k
        for p, (a, b) in enumerate(pairs(k)):
            sa = sum(coef[b - 1, s] * K[i, s] for s in range(start[a], start[a + 1]))
            sb = sum(coef[a, s] * K[i, s] for s in range(start[b], start[b + 1]))
            dec[i, p] = sa + sb - rho[p]
            votes[a if dec[i, p] > 0 else b] += 1
        lab[i] = max(range(k), key=lambda c: (votes[c], -c))
    return dec, lab


def exact_case(k, wins):
    """One query row, one support vector per class with K = 1: the decision of the pair (a, b) is +1 when (a, b)
    is in `wins` (a takes the vote), else -1.  Integer arithmetic throughout.  Returns (K, start, coef, rho)."""
    coef = np.zeros((k - 1, k))
    for a, b in pairs(k):
        coef[b - 1, a] = 1.0 if (a, b) in wins else -1.0   # a's coefficient in the pair (a, b); b's stays 0
    return np.ones((1, k)), np.arange(k + 1), coef, np.zeros(k * (k - 1) // 2)


def tie_wins(k=10):
    """k = 10: classes 3 and 7 win every pair they are in, except that 7 loses to 3 and 3 loses to 5: both end with
    8 votes, everybody else with fewer."""
    return {(a, b) for a, b in pairs(k) if a in (3, 7) or b not in (3, 7)} - {(3, 5)}


def vote_bound(K, start, coef, rho):
    """(m, P): 2 (n_a + n_b + 2) 2^-53 (sum_s |coef_s K_s| + |rho|), the distance two FP64 summations of a pair's
    n_a + n_b terms in different orders can be apart."""
    k = len(start) - 1
    out = np.empty((K.shape[0], k * (k - 1) // 2))
    aK = np.abs(K)
    for p, (a, b) in enumerate(pairs(k)):
        sa, sb = slice(start[a], start[a + 1]), slice(start[b], start[b + 1])
        mag = aK[:, sa] @ np.abs(coef[b - 1, sa]) + aK[:, sb] @ np.abs(coef[a, sb]) + abs(rho[p])
        out[:, p] = 2.0 * ((sa.stop - sa.start) + (sb.stop - sb.start) + 2) * 2.0 ** -53 * mag
    return out


def coef_abs_sum(start, coef):
    """(P,): sum |coef| over a pair's two segments."""
    k = len(start) - 1
    return np.array([np.abs(coef[b - 1, start[a]:start[a + 1]]).sum() + np.abs(coef[a, start[b]:start[b + 1]]).sum()
                     for a, b in pairs(k)])


def check_structure(m, fx):
    """A fitted model against its training data: support_ grouped by class and ascending within each,
    n_support_, the box, every pair's equality constraint, and LIBSVM's slots."""
    labels, C = fx["labels"], fx["C"]
    k, S = len(m.classes_), len(m.support_)
    assert int(m.n_support_.sum()) == S and m.n_support_.shape == (k,)
    assert m.dual_coef_.shape == (k - 1, S) and m.rho_.shape == (k * (k - 1) // 2,)
    assert np.array_equal(m.intercept_, -m.rho_)
    start = np.concatenate([[0], np.cumsum(m.n_support_)])
    for c in range(k):
        ids = m.support_[start[c]:start[c + 1]]
        assert np.all(labels[ids] == m.classes_[c])       # the ids map back to rows of class c
        assert np.all(np.diff(ids) > 0)                   # ascending within the class
    assert np.all(np.abs(m.dual_coef_) <= C * (1 + 1e-12))
    n = len(labels)
    for a, b in pairs(k):
        ca, cb = m.dual_coef_[b - 1, start[a]:start[a + 1]], m.dual_coef_[a, start[b]:start[b + 1]]
        # a is the +1 side: the only signs its slots allow (the box's own slack: the pairwise oracle's clip can
        # leave an alpha an ulp of C below 0)
        assert np.all(ca >= -1e-12 * C) and np.all(cb <= 1e-12 * C)
        assert abs(ca.sum() + cb.sum()) <= 1e-9 * C * n, (a, b, ca.sum() + cb.sum())
    assert np.all((np.abs(m.dual_coef_) > m.params.sv_tol).any(0))  # every column is somebody's support vector


def check_against_fixture(m, fx):
    """Decisions within FIXTURE_DEC_TOL of scikit-learn's; the same prediction on every query row whose fixture
    decisions all lie farther than that from zero (at least 98 % of them)."""
    dec = m.decision_function(fx["Xt"])
    diff = float(np.abs(dec - fx["decision"]).max())
    print(f"max |decision - fixture| = {diff:.3e} (bound {FIXTURE_DEC_TOL:.3e})")
    assert dec.shape == fx["decision"].shape
    assert diff <= FIXTURE_DEC_TOL, diff
    sure = np.abs(fx["decision"]).min(axis=1) > FIXTURE_DEC_TOL
    assert (~sure).sum() <= EXCLUDED_CAP * len(sure), int((~sure).sum())
    pred = m.predict(fx["Xt"])
    assert np.array_equal(pred[sure], fx["predict"][sure])
    return dec
