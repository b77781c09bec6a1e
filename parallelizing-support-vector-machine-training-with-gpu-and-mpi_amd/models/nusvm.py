"""nu-SVC and nu-SVR (RBF; LIBSVM's ``-s 1`` and ``-s 4``, scikit-learn's ``NuSVC`` and ``NuSVR``) on the
decomposition solver's nu modes.

Both duals carry two equality constraints (``y'a = 0`` and ``e'a = const``; csrc/include/svm355.h has the problems),
so a feasible step moves a pair of points of one sign, the stop test is the larger of two per-class gaps, and two
multipliers, ``rho`` and ``r``, come out at the end.  The classifier's selection, build and inner-solve kernels pick
one pair over all points; these modes run kernels of their own (csrc/hip/decomp_nu.hip).

* ``NuSVC``: labels +1 / -1, ``0 < nu <= 1`` (a lower bound on the fraction of support vectors, an upper bound on
  the fraction of margin errors).  Infeasible when ``nu n / 2`` exceeds the smaller class.  ``dual_coef_`` is
  ``y alpha / r`` and the decision value ``sum_i dual_coef_i K(x_i, x) + intercept_`` with ``intercept_ = -rho / r``:
  a free point of either class has decision +-1.  ``SVC(C = 1 / r_)`` on the same rows solves the same problem.
* ``NuSVR``: targets z, box ``C``; ``nu`` replaces epsilon-SVR's tube width, which comes out as ``epsilon_ = -r``.

Backends
  device="cpu"   the decomposition oracle's nu modes (``svm_decomp_train_gram_nusvc`` / ``_nusvr``) on a host FP64
                 kernel matrix (n x n doubles: small n)
  device="cuda"  ``svmd_train_decomp_nusvc`` / ``_nusvr``: exact-integer kernel values for pixel rows, FP64 MFMA for
                 real-valued rows; decisions on the device decision kernel
"""
from __future__ import annotations

import os
import time

import numpy as np

from ..utils.config import SVMParams, default_threads
from ..utils.sparse import refuse_sparse
from ._device import KernelEstimator, _is_u8, _resolve_device, solve_on_rows

MAX_POINTS = 1048576  # the nu modes' selection: four candidate lists of every 4,096-point block in one working set


def _check_nu(nu) -> float:
    if not (np.isfinite(nu) and 0.0 < nu <= 1.0):
        raise ValueError(f"nu must be in (0, 1], got {nu!r}")
    return float(nu)


class _NuEstimator(KernelEstimator):
    """What the two estimators share: the fit's dispatch, the linear decision value, persistence."""

    KIND = ""   # model files' kind marker (model_io)
    NAME = ""

    def _init(self, nu, C, gamma, tol, eps, sv_tol, max_iter, device, n_threads, scale, working_set):
        self.nu = _check_nu(nu)
        self.params = SVMParams(C=C, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads())
        self.device = device
        self.scale = scale
        self.working_set = int(working_set)

    def _fit(self, X, target, points: int):
        dev = _resolve_device(self.device)
        X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        if X.ndim != 2 or target.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) with one label or target per row")
        if X.shape[0] < 2:
            raise ValueError(f"{self.NAME} needs at least 2 rows")
        if points > MAX_POINTS:
            raise ValueError(f"{self.NAME} takes at most {MAX_POINTS} points, got {points}")
        t0 = time.perf_counter()
        if dev == "cpu":
            from ..ops import cpu as C

            Xs = self._scaled_cpu(X)
            K = C.rbf_matrix(Xs, Xs, self.params.gamma, self.params.n_threads)
            alpha, res, _, (r, rho), _ = self._oracle(C)(K, target, self.params, nu=self.nu, q=self.working_set)
            self._finish(alpha, target, res, r, rho)
            self._dev = None
            self.support_vectors_ = Xs[self.support_].copy()
            self.timings_ = {"smo_ms": res.seconds * 1e3}
        else:
            if not self.scale:
                raise ValueError(f"{self.NAME} on a GPU needs scale=True (min-max scaled rows: the decomposition "
                                 "solver's exact-integer plan, or the FP64 rows it solves on)")
            import torch

            device = torch.device(dev)
            td = torch.from_numpy(target).to(device)
            alpha = torch.empty(points, dtype=torch.float64, device=device)  # the start is written on the device
            rows, out = solve_on_rows(X, device, lambda rw: self._device_solve(rw, td, alpha, target))
            if out is None:
                raise ValueError(f"{self.NAME}: the decomposition solver does not cover these rows (its FP64-row "
                                 "workspace, n x 1024 doubles, does not fit the device)")
            res, tm, (r, rho) = out
            self._finish(alpha.cpu().numpy(), target, res, r, rho)
            self._adopt_rows(rows)
            self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _set_result(self, res, r, rho) -> None:
        self.r_, self.rho_ = r, rho
        self.b_ = res.b
        self.intercept_ = -res.b
        self.n_iter_ = res.iterations  # the solvers' count: pair updates + 1, as SVC's
        self.stop_reason_ = res.stop_reason
        self.result_ = res

    def _decision(self, X: np.ndarray) -> np.ndarray:
        """sum_k dual_coef_k K(x_k, x) - b over the support vectors."""
        self._check_X(X)
        if self._dev is not None:
            from ..ops import device as D

            dv = self._dev
            Xq, nq = self._device_queries(X)
            return D.decision(dv["Xs"], dv["ns"], dv["coef"], Xq, nq, self.params.gamma, self.b_).cpu().numpy()
        from ..ops import cpu as C

        X = np.ascontiguousarray(X, dtype=np.float64)
        Xq = self.scaler_.transform(X) if self.scaler_ is not None else X
        return C.decision(self.support_vectors_, np.where(self.dual_coef_ > 0, 1, -1).astype(np.int32),
                          np.abs(self.dual_coef_), Xq, self.params.gamma, self.b_, self.params.n_threads)

    # ------------------------------------------------------------------ persistence
    def save(self, directory: str | os.PathLike) -> None:
        """The classifier's model files with labels = sign(dual_coef_) and alphas = |dual_coef_|, and the kind marker."""
        from ..models.model_io import save_model

        save_model(directory, ids=self.support_, labels=np.where(self.dual_coef_ > 0, 1, -1),
                   alphas=np.abs(self.dual_coef_), b=self.b_, sv_rows=self.support_vectors_, scaler=self.scaler_,
                   params=self.params, kind=self.KIND,
                   meta={"n_iter": self.n_iter_, "stop_reason": self.stop_reason_, "nu": self.nu, "r": self.r_,
                         "rho": self.rho_})

    @classmethod
    def load(cls, directory: str | os.PathLike, device: str = "cpu"):
        from ..models.model_io import load_model

        m = load_model(directory)
        if m["kind"] != cls.KIND:
            raise ValueError(f"{directory} holds a {m['kind']!r} model, not a {cls.NAME} (load it with its own class)")
        p, meta = m["params"], m["meta"]
        est = cls(nu=meta.get("nu", 0.5), gamma=p.gamma, tol=p.tau, eps=p.eps, sv_tol=p.sv_tol, max_iter=p.max_iter,
                  device=device, scale=m["scaler"] is not None, **cls._load_kw(p))
        est.scaler_ = m["scaler"]
        est.support_ = m["ids"]
        est.dual_coef_ = m["alphas"] * m["labels"]
        est.b_ = m["b"]
        est.intercept_ = -m["b"]
        est.r_, est.rho_ = meta.get("r"), meta.get("rho")
        if cls.KIND == "nusvr" and est.r_ is not None:
            est.epsilon_ = -est.r_
        est.n_iter_ = meta.get("n_iter")
        est.stop_reason_ = meta.get("stop_reason")
        est.support_vectors_ = m["sv_rows"]
        if _resolve_device(device) != "cpu":
            if est.scaler_ is None:
                raise ValueError(f"{cls.NAME} on a GPU needs a scaled model (scale=True)")
            est._upload_model(_resolve_device(device))
        return est

    @staticmethod
    def _load_kw(p) -> dict:
        return {}


class NuSVC(_NuEstimator):
    KIND, NAME = "nusvc", "NuSVC"

    def __init__(self, nu: float = 0.5, gamma: float = 0.00125, tol: float = 1e-5, eps: float = 1e-12,
                 sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto", n_threads: int = 0,
                 scale: bool = True, working_set: int = 1024):
        # the box is 1: C is not a parameter of the problem (the native solvers do not read it)
        self._init(nu, 1.0, gamma, tol, eps, sv_tol, max_iter, device, n_threads, scale, working_set)

    def fit(self, X: np.ndarray, y: np.ndarray) -> "NuSVC":
        refuse_sparse(X)
        y = np.ascontiguousarray(y)
        if not np.all((y == 1) | (y == -1)):
            raise ValueError("NuSVC takes labels +1 / -1")
        y = y.astype(np.int32)
        n_pos = int(np.sum(y == 1))
        if self.nu * len(y) / 2.0 > min(n_pos, len(y) - n_pos):  # before any upload
            raise ValueError(f"specified nu is infeasible: nu n / 2 = {self.nu * len(y) / 2.0:g} exceeds the smaller "
                             f"class ({min(n_pos, len(y) - n_pos)} points)")
        return self._fit(X, y, len(y))

    def _oracle(self, C):
        return C.decomp_train_gram_nusvc

    def _device_solve(self, rows, yd, alpha, y):
        from ..ops import device as D

        return D.train_decomp_nusvc(rows.rows, yd, alpha, self.params, rows.mn_h, rows.mx_h, nu=self.nu,
                                    n_pos=int(np.sum(y == 1)), working_set=self.working_set)

    def _finish(self, alpha: np.ndarray, y: np.ndarray, res, r: float, rho: float) -> None:
        self.alpha_ = np.maximum(alpha, 0.0)  # a / r; a pair update can leave a variable a few ulp below 0
        self.support_ = np.flatnonzero(self.alpha_ > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = (self.alpha_ * y)[self.support_]
        self._set_result(res, r, rho)

    def decision_function(self, X: np.ndarray) -> np.ndarray:
        return self._decision(X)

    def predict(self, X: np.ndarray) -> np.ndarray:
        """+1 where the decision value is > 0, else -1 (SVC's rule)."""
        return np.where(self._decision(X) > 0, 1, -1).astype(np.int64)

    def score(self, X: np.ndarray, y: np.ndarray) -> float:
        return float(np.mean(self.predict(X) == np.asarray(y)))


class NuSVR(_NuEstimator):
    KIND, NAME = "nusvr", "NuSVR"

    def __init__(self, nu: float = 0.5, C: float = 10.0, gamma: float = 0.00125, tol: float = 1e-5,
                 eps: float = 1e-12, sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto",
                 n_threads: int = 0, scale: bool = True, working_set: int = 1024):
        self._init(nu, C, gamma, tol, eps, sv_tol, max_iter, device, n_threads, scale, working_set)

    def fit(self, X: np.ndarray, z: np.ndarray) -> "NuSVR":
        refuse_sparse(X)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if not np.all(np.isfinite(z)):
            raise ValueError("the targets z hold NaN or infinite values")
        return self._fit(X, z, 2 * len(z))

    def _oracle(self, C):
        return C.decomp_train_gram_nusvr

    def _device_solve(self, rows, zd, alpha, z):
        from ..ops import device as D

        return D.train_decomp_nusvr(rows.rows, zd, alpha, self.params, rows.mn_h, rows.mx_h, nu=self.nu,
                                    working_set=self.working_set)

    def _finish(self, alpha2: np.ndarray, z: np.ndarray, res, r: float, rho: float) -> None:
        from .svr import split_twins

        self.alpha_, self.alpha_star_ = split_twins(alpha2, self.params.C)
        beta = self.alpha_ - self.alpha_star_
        self.support_ = np.flatnonzero(np.abs(beta) > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = beta[self.support_]
        self._set_result(res, r, rho)
        self.epsilon_ = -r

    def predict(self, X: np.ndarray) -> np.ndarray:
        """sum_k (a_k - a*_k) K(x_k, x) - rho over the support vectors (a model without any predicts -rho)."""
        return self._decision(X)

    def score(self, X: np.ndarray, z: np.ndarray) -> float:
        """The coefficient of determination R^2 = 1 - sum (z - pred)^2 / sum (z - mean z)^2."""
        z = np.asarray(z, dtype=np.float64)
        res = z - self.predict(X)
        return float(1.0 - np.sum(res * res) / np.sum((z - z.mean()) ** 2))

    @staticmethod
    def _load_kw(p) -> dict:
        return {"C": p.C}
