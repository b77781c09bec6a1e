"""SVC / SVR with the linear, polynomial and sigmoid kernels on the CPU backend: scikit-learn fixtures, save / load."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest

from svm355 import SVC, SVR, SVMParams
from svm355 import _native as N
from svm355.ops import cpu as C

from kfun_checks import C as BOX, EPSILON, FIXTURE_TOL, GOLDEN, KERNELS, load_fixture


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.mark.parametrize("name", list(KERNELS))
def test_cpu_estimators_match_scikit_learn(fx, name):
    svc = SVC(C=BOX, tol=1e-6, device="cpu", **KERNELS[name]).fit(fx["X"], fx["y"])
    svr = SVR(C=BOX, tol=1e-6, epsilon=EPSILON, device="cpu", **KERNELS[name]).fit(fx["X"], fx["z"])
    assert svc.stop_reason_ == svr.stop_reason_ == "converged"
    dev_c = np.abs(svc.decision_function(fx["X"]) - fx[f"svc_{name}"]).max()
    dev_r = np.abs(svr.predict(fx["X"]) - fx[f"svr_{name}"]).max()
    print(f"{name}: SVC {dev_c:.3e} SVR {dev_r:.3e} (bound {FIXTURE_TOL[name]:.3e})")
    assert dev_c <= FIXTURE_TOL[name] and dev_r <= FIXTURE_TOL[name]
    assert svc.score(fx["X"], fx["y"]) == np.mean(np.where(fx[f"svc_{name}"] > 0, 1, -1) == fx["y"])


@pytest.mark.parametrize("cls,target", [(SVC, "y"), (SVR, "z")])
def test_save_load_round_trips_a_poly_model_and_old_files_load_as_rbf(fx, cls, target, tmp_path):
    m = cls(C=BOX, device="cpu", **KERNELS["poly"]).fit(fx["X"], fx[target])
    m.save(tmp_path)
    back = cls.load(tmp_path)
    assert (back.params.kernel, back.params.degree, back.params.coef0) == ("poly", 3, 1.0)
    np.testing.assert_array_equal(back.predict(fx["X"][:50]), m.predict(fx["X"][:50]))
    info = json.loads((tmp_path / "model.json").read_text())
    for k in ("kernel", "degree", "coef0"):  # a model file from before the kernel fields
        del info["params"][k]
    (tmp_path / "model.json").write_text(json.dumps(info))
    assert cls.load(tmp_path).params.kernel == "rbf"


def test_bad_kernel_arguments_raise():
    for kw in (dict(kernel="cosine"), dict(kernel="poly", degree=0), dict(kernel="poly", degree=17),
               dict(kernel="sigmoid", coef0=float("nan"))):
        with pytest.raises(ValueError):
            SVC(**kw)
    with pytest.raises(ValueError, match="probability"):
        SVC(kernel="linear", probability=True, device="cpu").fit(np.eye(4), np.array([1, -1, 1, -1]))
    with pytest.raises(ValueError, match="wss='second'"):
        SVC(kernel="linear", wss="second", device="cpu").fit(np.eye(4), np.array([1, -1, 1, -1]))
    with pytest.raises(ValueError, match="cross validation"):
        SVC(kernel="linear", device="cpu").cross_val_decision(np.eye(4), np.array([1, -1, 1, -1]), cv=2)


def test_rbf_oracle_outputs_are_the_parents_bit_for_bit():
    """kernel == 0: the decomposition oracle's alpha, b and iteration counts on one small case (classifier, two
    rules and both summation orders; twin mode) equal the fixture recorded before svm_params had kernel fields."""
    spec = importlib.util.spec_from_file_location(
        "make_oracle_rbf_golden", Path(__file__).resolve().parent.parent / "scripts" / "make_oracle_rbf_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    g = np.load(GOLDEN / "oracle_rbf_n128.npz")
    for name, (a, b, it) in mod.solves(np.ascontiguousarray(g["K"]), g["y"], g["z"]).items():
        np.testing.assert_array_equal(a, g[f"{name}_alpha"], err_msg=name)
        assert (b, it) == (float(g[f"{name}_b"]), int(g[f"{name}_iterations"])), name


@pytest.mark.parametrize("what,msg", [("world", r"linear kernel does not support the distributed solve \(world > 1\)"),
                                      ("warm", "linear kernel does not support a warm start"),
                                      ("shrinking", "linear kernel does not support shrinking"),
                                      ("wss3", "second-order single pair"),
                                      ("oneclass", "linear kernel does not support this mode"),
                                      ("pairwise_wss2", "kernel = 1 needs wss = 1")])
def test_the_oracles_refuse_what_a_dot_kernel_does_not_cover(fx, what, msg):
    """The refusal table the device driver shares (decomp_mode.h), on the CPU oracle."""
    X, y = fx["X"][:64], fx["y"][:64]
    p = SVMParams(kernel="linear", shrinking=what == "shrinking", wss=2 if what == "pairwise_wss2" else 1)
    K = C.kernel_gram(X, X, p)
    with pytest.raises(N.NativeError, match=msg):
        if what == "world":
            C.decomp_train_gram_dist(K, y, p, world=2, inner_wss=2)
        elif what == "warm":
            C.decomp_train_gram(K, y, p, alpha=np.zeros(64), inner_wss=2)
        elif what == "oneclass":
            C.decomp_train_gram_oneclass(K, p)
        elif what == "pairwise_wss2":
            C.smo_train_gram(K, y, p)
        else:
            C.decomp_train_gram(K, y, p, inner_wss=3 if what == "wss3" else 2)
