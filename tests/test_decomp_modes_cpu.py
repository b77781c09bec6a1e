"""What each mode of the decomposition solver refuses, on the CPU oracle: mode kind x solver feature.

The expected matrix below is written out from the behaviour before the refusals moved into one table
(csrc/include/decomp_mode.h); it is not derived from that table.  Every refused cell raises with the mode's
phrase and the feature's phrase, every allowed cell converges.  Cells the oracle's C entries cannot express
(only the classifier's entries take a warm start or more than one rank) are left out."""
import numpy as np
import pytest

from svm355 import SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C

from svr_checks import rbf_numpy, real_rows

GAMMA = 0.5
R, A = "refused", "allowed"

# the sentence's subject per kind, and the phrase per feature
MODE_PHRASE = {
    "twin": "the regression (twin) solve does not support",
    "oneclass": "the one-class solve does not support",
    "heldout": "the held-out solve does not support",
    "weighted": "class weights are not supported with",  # the classifier with class weights
}
FEATURE_PHRASE = {
    "distributed": "the distributed solve (world > 1)",
    "warm": "a warm start",
    "shrinking": "shrinking",
    "newton": "the Newton polish (SVM355_DECOMP_NEWTON)",
    "weights": "class weights",
}

# kind -> feature -> refused / allowed.  "weighted" is the classifier with class weights, every feature on top
# of them; its "weights" cell is the weights alone on one rank.
EXPECT = {
    "classify": {"distributed": A, "warm": A, "shrinking": A, "newton": A, "weights": A},
    "weighted": {"distributed": A, "warm": A, "shrinking": R, "newton": R, "weights": A},  # the oracle: world > 1 runs
    "twin": {"shrinking": R, "newton": R, "weights": R},
    "oneclass": {"shrinking": R, "newton": R, "weights": A},  # the entry clears the weights: the box is 1
    "heldout": {"shrinking": R, "newton": R, "weights": A},
}
CELLS = [(k, f) for k, row in EXPECT.items() for f in row]


@pytest.fixture(scope="module")
def problem():
    X, z = real_rows(64, seed=11)
    rng = np.random.default_rng(12)
    y = np.where(np.arange(64) % 2 == 0, 1, -1).astype(np.int32)
    rng.shuffle(y)
    held = (np.arange(64) % 4 == 3)  # both classes stay in the fit
    assert {1, -1} <= set(y[~held].tolist())
    K = rbf_numpy(X, X, GAMMA)
    assert K.shape == (64, 64)
    return K, y, z, held


def _solve(kind, feature, problem):
    K, y, z, held = problem
    weighted = kind == "weighted" or feature == "weights"
    p = SVMParams(gamma=GAMMA, shrinking=feature == "shrinking", weight_pos=2.0 if weighted else 1.0,
                  weight_neg=0.5 if weighted else 1.0)
    if kind == "twin":
        return C.decomp_train_gram_svr(K, z, p)[1]
    if kind == "oneclass":
        return C.decomp_train_gram_oneclass(K, p, nu=0.3)[1]
    if kind == "heldout":
        return C.decomp_train_gram_heldout(K, y, held, p)[1]
    if feature == "distributed":
        return C.decomp_train_gram_dist(K, y, p, world=2)[1]
    return C.decomp_train_gram(K, y, p, alpha=np.zeros(64) if feature == "warm" else None)[1]


@pytest.mark.parametrize("kind,feature", CELLS, ids=[f"{k}-{f}" for k, f in CELLS])
def test_mode_feature_cell(kind, feature, problem, monkeypatch):
    if feature == "newton":
        monkeypatch.setenv("SVM355_DECOMP_NEWTON", "1")
    else:
        monkeypatch.delenv("SVM355_DECOMP_NEWTON", raising=False)
    if EXPECT[kind][feature] == A:
        assert _solve(kind, feature, problem).stop_reason == "converged"
        return
    with pytest.raises(N.NativeError) as ei:
        _solve(kind, feature, problem)
    msg = str(ei.value)
    assert MODE_PHRASE[kind] in msg and FEATURE_PHRASE[feature] in msg, msg
