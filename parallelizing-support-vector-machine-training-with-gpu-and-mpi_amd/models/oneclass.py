"""One-class SVM (RBF; LIBSVM's ``-s 2``, scikit-learn's ``OneClassSVM``) on the solvers of :class:`svm355.SVC`.

The dual, in LIBSVM's scaling: minimise ``1/2 a' K a`` over ``0 <= a_i <= 1`` with ``sum a_i = nu n``, 0 < nu < 1.
It is the classifier's dual with every sign +1, box 1 and no linear term: ``f_i = sum_j a_j K_ij``, ``I_high = {a_i <
1 - eps}``, ``I_low = {a_i > eps}``, the stop test ``b_low <= b_high + 2 tol`` and ``rho = (b_high + b_low) / 2``
are the classifier's.  The equality is carried by LIBSVM's feasible start (``floor(nu n)`` ones, then the fraction).
The decision value of x is ``sum_k a_k K(x_k, x) - rho``; the label is +1 where it is > 0, else -1.

Backends
  device="cpu"   the pairwise oracle from that start (``svm_smo_train_oneclass``)
  device="cuda"  the working-set decomposition solver's one-class mode (decomp.hip): the start is written on the
                 device and its f summed by the chunked start, one f update per 1,024 start columns; exact-integer
                 kernel values for pixel rows, FP64 MFMA for real-valued rows; decisions on the device kernel
"""
from __future__ import annotations

import os
import time

import numpy as np

from ..utils.config import SVMParams, default_threads
from ._device import KernelEstimator, _is_u8, _resolve_device, solve_on_rows

KIND = "oneclass"  # model files' kind marker (model_io)


class OneClassSVM(KernelEstimator):
    def __init__(self, nu: float = 0.5, gamma: float = 0.00125, tol: float = 1e-5, eps: float = 1e-12,
                 sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto", n_threads: int = 0,
                 scale: bool = True, working_set: int = 1024):
        if not (np.isfinite(nu) and 0.0 < nu < 1.0):
            raise ValueError(f"nu must be in (0, 1), got {nu!r}")
        # the box is 1: C is not a parameter of the problem (the native solvers do not read it)
        self.params = SVMParams(C=1.0, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads())
        self.nu = float(nu)
        self.device = device
        self.scale = scale
        self.working_set = int(working_set)

    # ------------------------------------------------------------------ fit
    def fit(self, X: np.ndarray, y=None) -> "OneClassSVM":
        """Fits on the unlabelled rows X (y is ignored, as scikit-learn's)."""
        dev = _resolve_device(self.device)
        X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        if X.ndim != 2:
            raise ValueError("X must be (n, d)")
        if X.shape[0] < 2:
            raise ValueError("OneClassSVM needs at least 2 rows")
        t0 = time.perf_counter()
        if dev == "cpu":
            self._fit_cpu(X)
        else:
            if not self.scale:
                raise ValueError("OneClassSVM on a GPU needs scale=True (min-max scaled rows: the decomposition "
                                 "solver's exact-integer plan, or the FP64 rows it solves on)")
            self._fit_cuda(X, dev)
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _finish(self, alpha: np.ndarray, res) -> None:
        # the pair update can leave a variable a few ulp outside its bound (SVR's split_twins has the reason)
        self.alpha_ = np.clip(alpha, 0.0, 1.0)
        self.support_ = np.flatnonzero(self.alpha_ > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = self.alpha_[self.support_]
        self.rho_ = res.b
        self.b_ = res.b
        self.intercept_ = -res.b
        self.offset_ = res.b
        self.n_iter_ = res.iterations  # the solvers' count: pair updates + 1, as SVC's
        self.stop_reason_ = res.stop_reason
        self.result_ = res

    def _fit_cpu(self, X):
        from ..ops import cpu as C

        Xs = self._scaled_cpu(X)
        alpha, res = C.smo_train_oneclass(Xs, self.params, self.nu)
        self._finish(alpha, res)
        self._dev = None
        self.support_vectors_ = Xs[self.support_].copy()
        self.timings_ = {"smo_ms": res.seconds * 1e3}

    def _fit_cuda(self, X, dev):
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        alpha = torch.empty(X.shape[0], dtype=torch.float64, device=device)  # the start is written on the device
        # pixel rows stay bytes on the device (the exact-integer plan reads them); FP64 rows are scaled there and
        # quantised when they admit the plan, else solved with FP64-MFMA kernel values
        rows, out = solve_on_rows(X, device, lambda r: D.train_decomp_oneclass(
            r.rows, alpha, self.params, r.mn_h, r.mx_h, nu=self.nu, working_set=self.working_set))
        if out is None:
            raise ValueError("OneClassSVM: the decomposition solver does not cover these rows (its FP64-row "
                             "workspace, n x 1024 doubles, does not fit the device)")
        res, tm = out
        self._finish(alpha.cpu().numpy(), res)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    # ------------------------------------------------------------------ inference
    def decision_function(self, X: np.ndarray) -> np.ndarray:
        """sum_k alpha_k K(x_k, x) - rho over the support vectors."""
        self._check_X(X)
        if self._dev is not None:
            from ..ops import device as D

            dv = self._dev
            Xq, nq = self._device_queries(X)
            return D.decision(dv["Xs"], dv["ns"], dv["coef"], Xq, nq, self.params.gamma, self.rho_).cpu().numpy()
        from ..ops import cpu as C

        X = np.ascontiguousarray(X, dtype=np.float64)
        Xq = self.scaler_.transform(X) if self.scaler_ is not None else X
        return C.decision(self.support_vectors_, np.ones(len(self.dual_coef_), dtype=np.int32), self.dual_coef_, Xq,
                          self.params.gamma, self.rho_, self.params.n_threads)

    def score_samples(self, X: np.ndarray) -> np.ndarray:
        """The unshifted score sum_k alpha_k K(x_k, x) = decision_function(X) + rho_."""
        return self.decision_function(X) + self.rho_

    def predict(self, X: np.ndarray) -> np.ndarray:
        """+1 (inlier) where the decision value is > 0, else -1 (the serial and GPU paths' rule, and LIBSVM's)."""
        return np.where(self.decision_function(X) > 0, 1, -1).astype(np.int64)

    # ------------------------------------------------------------------ persistence
    def save(self, directory: str | os.PathLike) -> None:
        """The classifier's model files with labels all +1, alphas = alpha, b = rho, and the kind marker."""
        from ..models.model_io import save_model

        save_model(directory, ids=self.support_, labels=np.ones(len(self.support_), dtype=np.int32),
                   alphas=self.dual_coef_, b=self.rho_, sv_rows=self.support_vectors_, scaler=self.scaler_,
                   params=self.params, kind=KIND,
                   meta={"n_iter": self.n_iter_, "stop_reason": self.stop_reason_, "nu": self.nu})

    @classmethod
    def load(cls, directory: str | os.PathLike, device: str = "cpu") -> "OneClassSVM":
        from ..models.model_io import load_model

        m = load_model(directory)
        if m["kind"] != KIND:
            raise ValueError(f"{directory} holds a {m['kind']!r} model, not a one-class SVM (load it with its own "
                             "class)")
        p = m["params"]
        oc = cls(nu=m["meta"].get("nu", 0.5), gamma=p.gamma, tol=p.tau, eps=p.eps, sv_tol=p.sv_tol,
                 max_iter=p.max_iter, device=device, scale=m["scaler"] is not None)
        oc.scaler_ = m["scaler"]
        oc.support_ = m["ids"]
        oc.dual_coef_ = m["alphas"]
        oc.rho_ = oc.b_ = oc.offset_ = m["b"]
        oc.intercept_ = -m["b"]
        oc.n_iter_ = m["meta"].get("n_iter")
        oc.stop_reason_ = m["meta"].get("stop_reason")
        oc.support_vectors_ = m["sv_rows"]
        if _resolve_device(device) != "cpu":
            oc._upload_model(_resolve_device(device))
        return oc

    def _upload_model(self, dev: str) -> None:
        if self.scaler_ is None:
            raise ValueError("OneClassSVM on a GPU needs a scaled model (scale=True)")
        super()._upload_model(dev)
