"""epsilon-SVR (RBF) on the solvers of :class:`svm355.SVC`.

epsilon-SVR is the classifier's box-constrained problem over 2n variables that come in pairs ("twins") sharing a
kernel row: for row k, variable k is ``a_k`` with sign +1 and variable k + n is ``a*_k`` with sign -1; the start is
``f_k = epsilon - z_k``, ``f_{k+n} = -epsilon - z_k``; selection, the stop test ``b_low <= b_high + 2 tol``, the
clip and ``b = (b_high + b_low) / 2`` are the classifier's.  The model is ``beta = a - a*`` and a prediction is
``sum_k beta_k K(x_k, x) - b``.

Backends
  device="cpu"   the pairwise oracle on duplicated rows (``svm_smo_train_svr``; small n)
  device="cuda"  the working-set decomposition solver in twin mode (decomp.hip): the kernel work of the f update
                 (the int8 / FP64-MFMA GEMV, the column store and the column cache) runs over the n rows, as a
                 classification of them would, and each row's sum is added to both twins; exact-integer kernel
                 values for pixel rows, FP64 MFMA for real-valued rows; prediction on the device decision kernel
"""
from __future__ import annotations

import os
import time

import numpy as np

from ..utils.config import SVMParams, default_threads
from ._device import KernelEstimator, _is_u8, _resolve_device, solve_on_rows

KIND = "svr"  # model files' kind marker (model_io)


def split_twins(alpha2: np.ndarray, C: float):
    """The solvers' 2n values as (a, a*), each clamped into the box [0, C].  The pair update clips one of its two
    variables and moves the other by the same amount (the reference's arithmetic, which the classifier shares),
    so a variable that lands on a bound can miss it by a few ulp, on either side; the model keeps no such
    residue outside the box."""
    n = alpha2.shape[0] // 2
    return np.clip(alpha2[:n], 0.0, C), np.clip(alpha2[n:], 0.0, C)


class SVR(KernelEstimator):
    def __init__(self, C: float = 10.0, gamma: float = 0.00125, epsilon: float = 0.1, tol: float = 1e-5,
                 eps: float = 1e-12, sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto",
                 n_threads: int = 0, scale: bool = True, working_set: int = 1024):
        if not (np.isfinite(epsilon) and epsilon >= 0):
            raise ValueError(f"epsilon must be finite and >= 0, got {epsilon!r}")
        self.params = SVMParams(C=C, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads())
        self.epsilon = float(epsilon)
        self.device = device
        self.scale = scale
        self.working_set = int(working_set)

    # ------------------------------------------------------------------ fit
    def fit(self, X: np.ndarray, z: np.ndarray) -> "SVR":
        dev = _resolve_device(self.device)
        X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if X.ndim != 2 or z.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) and z (n,)")
        if not np.all(np.isfinite(z)):
            raise ValueError("the targets z hold NaN or infinite values")
        if 2 * X.shape[0] > 2**31 - 1:
            raise ValueError(f"n = {X.shape[0]} rows are 2 n > 2^31 - 1 variables")
        t0 = time.perf_counter()
        if dev == "cpu":
            self._fit_cpu(X, z)
        else:
            if not self.scale:
                raise ValueError("SVR on a GPU needs scale=True (min-max scaled rows: the decomposition solver's "
                                 "exact-integer plan, or the FP64 rows it solves on)")
            if X.shape[0] < 2:
                raise ValueError("SVR on a GPU needs at least 2 rows")
            self._fit_cuda(X, z, dev)
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _finish(self, alpha2: np.ndarray, res) -> None:
        self.alpha_, self.alpha_star_ = split_twins(alpha2, self.params.C)
        beta = self.alpha_ - self.alpha_star_
        self.support_ = np.flatnonzero(np.abs(beta) > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = beta[self.support_]
        self.b_ = res.b
        self.intercept_ = -res.b
        self.n_iter_ = res.iterations  # the solvers' count: pair updates + 1, as SVC's
        self.stop_reason_ = res.stop_reason
        self.result_ = res

    def _fit_cpu(self, X, z):
        from ..ops import cpu as C

        Xs = self._scaled_cpu(X)
        alpha2, res = C.smo_train_svr(Xs, z, self.params, self.epsilon)
        self._finish(alpha2, res)
        self._dev = None
        self.support_vectors_ = Xs[self.support_].copy()
        self.timings_ = {"smo_ms": res.seconds * 1e3}

    def _fit_cuda(self, X, z, dev):
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        zd = torch.from_numpy(z).to(device)
        alpha = torch.empty(2 * X.shape[0], dtype=torch.float64, device=device)  # the cold start zeroes it
        # pixel rows stay bytes on the device (the exact-integer plan reads them); FP64 rows are scaled there and
        # quantised when they admit the plan, else solved with FP64-MFMA kernel values
        rows, out = solve_on_rows(X, device, lambda r: D.train_decomp_svr(
            r.rows, zd, alpha, self.params, r.mn_h, r.mx_h, epsilon=self.epsilon, working_set=self.working_set))
        if out is None:
            raise ValueError("SVR: the decomposition solver does not cover these rows (its FP64-row workspace, "
                             "n x 1024 doubles, does not fit the device)")
        res, tm = out
        self._finish(alpha.cpu().numpy(), res)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    # ------------------------------------------------------------------ inference
    def predict(self, X: np.ndarray) -> np.ndarray:
        """sum_k beta_k K(x_k, x) - b over the support vectors (a model without any predicts -b)."""
        self._check_X(X)
        if self._dev is not None:
            from ..ops import device as D

            dv = self._dev
            Xq, nq = self._device_queries(X)
            return D.decision(dv["Xs"], dv["ns"], dv["coef"], Xq, nq, self.params.gamma, self.b_).cpu().numpy()
        from ..ops import cpu as C

        X = np.ascontiguousarray(X, dtype=np.float64)
        Xq = self.scaler_.transform(X) if self.scaler_ is not None else X
        return C.decision(self.support_vectors_, np.where(self.dual_coef_ > 0, 1, -1), np.abs(self.dual_coef_), Xq,
                          self.params.gamma, self.b_, self.params.n_threads)

    def score(self, X: np.ndarray, z: np.ndarray) -> float:
        """The coefficient of determination R^2 = 1 - sum (z - pred)^2 / sum (z - mean z)^2."""
        z = np.asarray(z, dtype=np.float64)
        r = z - self.predict(X)
        return float(1.0 - np.sum(r * r) / np.sum((z - z.mean()) ** 2))

    # ------------------------------------------------------------------ persistence
    def save(self, directory: str | os.PathLike) -> None:
        """The classifier's model files with labels = sign(beta) and alphas = |beta|, and the kind marker."""
        from ..models.model_io import save_model

        save_model(directory, ids=self.support_, labels=np.where(self.dual_coef_ > 0, 1, -1),
                   alphas=np.abs(self.dual_coef_), b=self.b_, sv_rows=self.support_vectors_, scaler=self.scaler_,
                   params=self.params, kind=KIND,
                   meta={"n_iter": self.n_iter_, "stop_reason": self.stop_reason_, "epsilon": self.epsilon})

    @classmethod
    def load(cls, directory: str | os.PathLike, device: str = "cpu") -> "SVR":
        from ..models.model_io import load_model

        m = load_model(directory)
        if m["kind"] != KIND:
            raise ValueError(f"{directory} holds a {m['kind']!r} model, not an SVR (load it with its own class)")
        p = m["params"]
        svr = cls(C=p.C, gamma=p.gamma, epsilon=m["meta"].get("epsilon", 0.1), tol=p.tau, eps=p.eps, sv_tol=p.sv_tol,
                  max_iter=p.max_iter, device=device, scale=m["scaler"] is not None)
        svr.scaler_ = m["scaler"]
        svr.support_ = m["ids"]
        svr.dual_coef_ = m["alphas"] * m["labels"]
        svr.b_ = m["b"]
        svr.intercept_ = -m["b"]
        svr.n_iter_ = m["meta"].get("n_iter")
        svr.stop_reason_ = m["meta"].get("stop_reason")
        svr.support_vectors_ = m["sv_rows"]
        if _resolve_device(device) != "cpu":
            svr._upload_model(_resolve_device(device))
        return svr

    def _upload_model(self, dev: str) -> None:
        if self.scaler_ is None:
            raise ValueError("SVR on a GPU needs a scaled model (scale=True)")
        super()._upload_model(dev)
