"""One-vs-one multi-class SVC on the GPU (models/ovo.py): the scikit-learn fixtures, the plumbing around the
unchanged decomposition solver (gathered pair rows, LIBSVM's layout), side-by-side against one-after-another
solves, device against host prediction, persistence, and the ten-digit small_mnist problem."""
import numpy as np
import pytest
import torch

from svm355 import OneVsOneSVC
from svm355.ops import cpu as C
from svm355.ops import device as D

from ovo_checks import (CROSS_KERNEL_DIFF, EXCLUDED_CAP, FIT, FIXTURE_DEC_TOL, FIXTURES, GRAM_PATHS,
                        check_against_fixture, check_structure, coef_abs_sum, load_fixture, pairs, vote_bound)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fitted():
    """The three fixtures and their GPU models, fitted once."""
    out = {}
    for n, seed in FIXTURES:
        fx = load_fixture(n, seed)
        out[seed] = (fx, OneVsOneSVC(device="cuda:0", **FIT).fit(fx["X"], fx["labels"]))
    return out


@pytest.mark.parametrize("seed", [s for _, s in FIXTURES])
def test_fixture(fitted, seed):
    fx, m = fitted[seed]
    check_against_fixture(m, fx)
    check_structure(m, fx)
    assert all(s == "converged" for s in m.stop_reasons_)
    assert m.timings_["gram_path"] == GRAM_PATHS[seed] and m.timings_["solver"] == "decomp"
    assert len(m.pair_timings_) == len(m.rho_)
    assert all(t["gram_path"] == GRAM_PATHS[seed] for t in m.pair_timings_.values())
    assert m.score(fx["Xt"], fx["labels_t"]) > 0.78


def _host_bound(m, fx):
    """Host decisions of the model's own support vectors and coefficients, and the bound a device decision may be
    off by: the two summation orders plus 10 x the measured cross-kernel difference times sum |coef|."""
    start = np.concatenate([[0], np.cumsum(m.n_support_)])
    sv = m._host_sv_rows()
    Xq = m.scaler_.transform(fx["Xt"])
    Kh = C.rbf_matrix(Xq, sv, m.params.gamma, 1)
    ref, rlab = C.ovo_votes(Kh, start, m.dual_coef_, m.rho_)
    bound = vote_bound(Kh, start, m.dual_coef_, m.rho_) + 10 * CROSS_KERNEL_DIFF * coef_abs_sum(start, m.dual_coef_)
    # the measurement behind CROSS_KERNEL_DIFF, printed
    dm = m._dev_model
    Xd = D.upload_rows(fx["Xt"], DEV)
    _, _, nq = D.minmax_scale_(Xd, dm["d"], dm["mn"], dm["mx"])
    Kd = D.rbf_gram(Xd, nq, dm["Xs"], dm["ns"], m.params.gamma)[:, : len(sv)].cpu().numpy()
    print(f"max |rbf_gram - rbf_matrix| = {np.abs(Kd - Kh).max():.3e} (recorded {CROSS_KERNEL_DIFF:.1e})")
    return ref, rlab, bound


@pytest.mark.parametrize("seed", [s for _, s in FIXTURES])
def test_device_prediction_against_host(fitted, seed):
    fx, m = fitted[seed]
    ref, rlab, bound = _host_bound(m, fx)
    dec = m.decision_function(fx["Xt"])
    err = np.abs(dec - ref)
    print(f"max |device - host| = {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound), float((err - bound).max())
    sure = np.all(np.abs(ref) > bound, axis=1)
    np.testing.assert_array_equal(m.predict(fx["Xt"])[sure], m.classes_[rlab[sure]])


def test_plumbing_is_exact(fitted):
    """Fixture 3 (45 pairs): every pair's coefficients are, bit for bit, alpha y of a direct train_decomp on that
    pair's rows gathered here with torch and given the model's bounds; a row left out of the union has
    alpha <= sv_tol in every pair; support_ maps back to the training rows."""
    fx, m = fitted[43]
    X, labels = fx["X"], fx["labels"]
    k = len(m.classes_)
    start = np.concatenate([[0], np.cumsum(m.n_support_)])
    Xu = torch.from_numpy(X).to(DEV)
    mn, mx = m.scaler_.min_, m.scaler_.max_
    for p, (a, b) in enumerate(pairs(k)):
        ia, ib = np.flatnonzero(labels == m.classes_[a]), np.flatnonzero(labels == m.classes_[b])
        rows = Xu[torch.from_numpy(np.concatenate([ia, ib])).to(DEV)].contiguous()
        y = torch.from_numpy(np.concatenate([np.ones(len(ia)), -np.ones(len(ib))]).astype(np.int32)).to(DEV)
        alpha = torch.zeros(len(ia) + len(ib), dtype=torch.float64, device=DEV)
        res, _ = D.train_decomp(rows, y, alpha, m.params, mn, mx)
        al = alpha.cpu().numpy()
        assert res.b == m.rho_[p] and res.iterations == m.n_iter_[p]
        for ids, seg, got, sign in ((ia, al[: len(ia)], m.dual_coef_[b - 1, start[a]:start[a + 1]], 1.0),
                                    (ib, al[len(ia):], m.dual_coef_[a, start[b]:start[b + 1]], -1.0)):
            cls = a if sign > 0 else b
            sup = m.support_[start[cls]:start[cls + 1]]
            pos = np.searchsorted(ids, sup)
            np.testing.assert_array_equal(ids[pos], sup)               # support ids are rows of this class
            np.testing.assert_array_equal(got, sign * seg[pos])        # bit for bit
            left_out = np.ones(len(ids), dtype=bool)
            left_out[pos] = False
            assert np.all(seg[left_out] <= m.params.sv_tol)
    # the device model's rows are the scaled training rows of support_
    np.testing.assert_array_equal(m._host_sv_rows(), m.scaler_.transform(X[m.support_]))


def test_side_by_side_equals_one_after_another(fitted):
    fx, m = fitted[43]
    one = OneVsOneSVC(device="cuda:0", concurrent_solves=1, **FIT).fit(fx["X"], fx["labels"])
    assert one.timings_["concurrent_solves"] == 1 and m.timings_["concurrent_solves"] == 10
    for name in ("dual_coef_", "rho_", "support_", "n_support_", "n_iter_"):
        np.testing.assert_array_equal(getattr(one, name), getattr(m, name), err_msg=name)


@pytest.mark.parametrize("seed", [41, 42])
def test_save_load(fitted, seed, tmp_path):
    """uint8 rows and real-valued rows: a model loaded on the GPU reproduces the bits, one loaded on the CPU is
    within the device-against-host bound."""
    fx, m = fitted[seed]
    m.save(tmp_path / "model")
    dec = m.decision_function(fx["Xt"])
    g = OneVsOneSVC.load(tmp_path / "model", device="cuda:0")
    np.testing.assert_array_equal(g.decision_function(fx["Xt"]), dec)
    np.testing.assert_array_equal(g.predict(fx["Xt"]), m.predict(fx["Xt"]))
    for name in ("dual_coef_", "rho_", "support_", "n_support_", "classes_"):
        np.testing.assert_array_equal(getattr(g, name), getattr(m, name), err_msg=name)
    h = OneVsOneSVC.load(tmp_path / "model", device="cpu")
    ref, rlab, bound = _host_bound(m, fx)
    assert h._dev_model is None
    assert np.all(np.abs(dec - h.decision_function(fx["Xt"])) <= bound)
    assert np.all(np.abs(dec - ref) <= bound)  # and of the host twin on the saved model


def test_refusals_before_device_work():
    X = np.random.default_rng(0).integers(0, 255, size=(130, 8)).astype(np.uint8)
    with pytest.raises(ValueError, match="at most 64"):
        OneVsOneSVC(device="cuda:0").fit(X, np.arange(130) % 65)
    with pytest.raises(ValueError, match="no rows"):
        OneVsOneSVC(device="cuda:0").fit(X, np.arange(130) % 3, classes=[0, 1, 2, 9])
    with pytest.raises(ValueError, match="transport"):
        OneVsOneSVC(device="cuda:0").fit(X, np.arange(130) % 3, transport=object())


def test_small_mnist_ten_digits(small_mnist):
    """1,200 / 400 rows, 10 digits: all 45 pairs converge; the accuracy is the CPU model's up to query rows with a
    CPU pair decision within FIXTURE_DEC_TOL of zero (at most 2 % of the 400, asserted on the CPU model alone)."""
    tr, te = small_mnist
    g = OneVsOneSVC(device="cuda:0").fit(tr.X, tr.labels)
    c = OneVsOneSVC(device="cpu").fit(tr.X, tr.labels)
    assert len(g.rho_) == 45 and len(g.classes_) == 10
    assert all(s == "converged" for s in g.stop_reasons_), g.stop_reasons_
    assert all(s != "max_iter" for s in c.stop_reasons_)
    cd = c.decision_function(te.X)
    unsure = int((np.abs(cd).min(axis=1) <= FIXTURE_DEC_TOL).sum())
    assert unsure <= EXCLUDED_CAP * len(te.labels), unsure
    pg, pc = g.predict(te.X), c.predict(te.X)
    hits_g, hits_c = int((pg == te.labels).sum()), int((pc == te.labels).sum())
    print(f"accuracy gpu {hits_g / len(te.labels):.4f} cpu {hits_c / len(te.labels):.4f} unsure rows {unsure} "
          f"union SVs gpu {len(g.support_)} cpu {len(c.support_)}")
    assert abs(hits_g - hits_c) <= unsure
    assert hits_g / len(te.labels) > 0.9
