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
from typing import Optional

import numpy as np

from ..utils.config import SVMParams, default_threads
from ..utils.sparse import is_sparse, toarray
from ._device import (KernelEstimator, SparseTrainRows, TrainRows, _is_u8, _resolve_device, check_chi2_rows, check_dot_kernel,
                      check_f32_rows, check_row_dtype, newton_polish_on, check_sample_weight, host_kernel_decision, solve_on_rows)

KIND = "svr"  # model files' kind marker (model_io)


def split_twins(alpha2: np.ndarray, C):
    """The solvers' 2n values as (a, a*), each clamped into the box [0, C] (C: one box, or a box per row).  The pair update clips one of its two
    variables and moves the other by the same amount (the reference's arithmetic, which the classifier shares),
    so a variable that lands on a bound can miss it by a few ulp, on either side; the model keeps no such
    residue outside the box."""
    n = alpha2.shape[0] // 2
    return np.clip(alpha2[:n], 0.0, C), np.clip(alpha2[n:], 0.0, C)


class SVR(KernelEstimator):
    def __init__(self, C: float = 10.0, gamma: float = 0.00125, epsilon: float = 0.1, tol: float = 1e-5,
                 eps: float = 1e-12, sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto",
                 n_threads: int = 0, scale: bool = True, working_set: int = 1024, kernel: str = "rbf", degree: int = 3,
                 coef0: float = 0.0, row_dtype: str = "float64"):
        self.row_dtype = check_row_dtype(row_dtype)  # "float32" / "float16": as SVC's (rows_f32.hip, rows_f16.hip)
        if not (np.isfinite(epsilon) and epsilon >= 0):
            raise ValueError(f"epsilon must be finite and >= 0, got {epsilon!r}")
        self.params = SVMParams(C=C, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads(), kernel=kernel,
                                degree=degree, coef0=coef0)  # kernel: as SVC's
        self.epsilon = float(epsilon)
        self.device = device
        self.scale = scale
        self.working_set = int(working_set)

    # ------------------------------------------------------------------ fit
    def fit(self, X: np.ndarray, z: np.ndarray, sample_weight: Optional[np.ndarray] = None) -> "SVR":
        """sample_weight (scikit-learn's): n weights >= 0; both variables of row k have the box [0, C * w_k], and a
        weight of 0 leaves the row out.  The decomposition oracle's twin mode on the CPU, the decomposition solver
        with a box per point on a GPU (decomp_box.hip: RBF only); not stored in the model.  None: the unweighted fit."""
        dev = _resolve_device(self.device)
        if self.params.precomputed:
            return self._fit_precomputed(X, z, dev, sample_weight)
        sparse = is_sparse(X)  # CSR rows: solved as they are on a GPU, densified for the CPU oracle
        if sample_weight is not None and sparse:
            check_sample_weight(sample_weight, 0, None, 0.0, **{"sparse input": True})
        if sparse and dev == "cpu":
            X, sparse = toarray(X), False
        check_dot_kernel(self.params, sparse_rows=sparse and self.params.kernel != "linear")  # csr_linear.hip
        f32, f16 = self.row_dtype == "float32", self.row_dtype == "float16"
        if f32 or f16:  # what float32 / float16 rows do not cover, before any device work
            check_f32_rows(self.row_dtype, **{"sparse (CSR) rows": sparse, f"kernel={self.params.kernel!r}": self.params.gram_kernel,
                              "scale=False": not self.scale,
                              "the Newton polish (SVM355_DECOMP_NEWTON)": dev != "cpu" and newton_polish_on()})
        if f16 and getattr(X, "dtype", None) == np.float16:  # as it is, on either device (2 bytes a value over PCIe)
            X = np.ascontiguousarray(X)
        elif (f32 or f16) and dev != "cpu":  # as it is when it is float32; any other dtype (uint8 exactly) cast once
            X = np.ascontiguousarray(X, dtype=np.float32)
        elif not sparse:
            X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if len(X.shape) != 2 or z.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) and z (n,)")
        if not np.all(np.isfinite(z)):
            raise ValueError("the targets z hold NaN or infinite values")
        if 2 * X.shape[0] > 2**31 - 1:
            raise ValueError(f"n = {X.shape[0]} rows are 2 n > 2^31 - 1 variables")
        sw = None
        if sample_weight is not None:
            sw = check_sample_weight(sample_weight, z.shape[0], np.full(z.shape[0], self.params.C), self.params.eps,
                                     **{"row_dtype='float32'": f32, "row_dtype='float16'": f16, f"kernel={self.params.kernel!r}": self.params.gram_kernel,
                                        "scale=False on a GPU": dev != "cpu" and not self.scale})
        t0 = time.perf_counter()
        if dev == "cpu":
            self._fit_cpu(X, z, sw)
        else:
            if not self.scale:
                raise ValueError("SVR on a GPU needs scale=True (min-max scaled rows: the decomposition solver's "
                                 "exact-integer plan, or the FP64 rows it solves on)")
            if X.shape[0] < 2:
                raise ValueError("SVR on a GPU needs at least 2 rows")
            if sw is not None:
                self._fit_cuda(X, z, dev, sw)
            elif f32:
                self._fit_cuda_f32(X, z, dev)
            elif f16:
                self._fit_cuda_f16(X, z, dev)
            elif sparse:
                self._fit_cuda_sparse(X, z, dev)
            else:
                self._fit_cuda(X, z, dev)
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _fit_precomputed(self, K, z, dev, sample_weight) -> "SVR":
        """kernel="precomputed": K is the (n, n) Gram (models/_precomputed.py).  The decomposition oracle's twin mode
        on it on the CPU; on a GPU the decomposition solver with the Gram as its row source (decomp_gram.hip)."""
        from . import _precomputed as G
        from ..ops import cpu as C

        G.check_options(self, K, sample_weight)
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.ndim != 1 or not np.all(np.isfinite(z)):
            raise ValueError("the targets z must be (n,) and finite")
        K = G.as_gram(K, z.shape[0], dev)
        if z.shape[0] < 2 or 2 * z.shape[0] > 2**31 - 1:
            raise ValueError(f"n = {z.shape[0]} rows: SVR needs 2 <= n with 2 n <= 2^31 - 1 variables")
        t0 = time.perf_counter()
        if dev != "cpu":
            alpha2, res, self.timings_ = G.fit_device(self, K, dev, 2 * z.shape[0], z=z, epsilon=self.epsilon)
        else:
            G.check_host(K)
            alpha2, res, _, _ = C.decomp_train_gram_svr(K, z, self.params, self.epsilon, q=self.working_set, inner_wss=2)
            self.timings_ = {"smo_ms": res.seconds * 1e3}
        self._finish(alpha2, res)
        G.adopt(self, z.shape[0], dev)
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _finish(self, alpha2: np.ndarray, res, sw=None) -> None:
        # sample weights: row k's own box C w_k (split_twins clips elementwise)
        self.alpha_, self.alpha_star_ = split_twins(alpha2, self.params.C if sw is None else self.params.C * sw)
        beta = self.alpha_ - self.alpha_star_
        self.support_ = np.flatnonzero(np.abs(beta) > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = beta[self.support_]
        self.b_ = res.b
        self.intercept_ = -res.b
        self.n_iter_ = res.iterations  # the solvers' count: pair updates + 1, as SVC's
        self.stop_reason_ = res.stop_reason
        self.result_ = res

    def _fit_cpu(self, X, z, sw=None):
        from ..ops import cpu as C

        Xs = self._scaled_cpu(X)
        check_chi2_rows(self.params, Xs)  # scale=False: the rows as they came
        if sw is not None:  # the decomposition oracle's twin mode with a box per row, on the host RBF Gram
            K = C.rbf_matrix(Xs, Xs, self.params.gamma, self.params.n_threads)
            alpha2, res, _, _ = C.decomp_train_gram_sw(K, z, sw, self.params, epsilon=self.epsilon, q=self.working_set,
                                                       fp64_rows=True)
        elif self.params.gram_kernel:  # the decomposition oracle's twin mode on the host Gram (its second-order pair)
            alpha2, res, _, _ = C.decomp_train_gram_svr(C.kernel_gram(Xs, Xs, self.params), z, self.params,
                                                        self.epsilon, q=self.working_set, inner_wss=2)
        else:
            alpha2, res = C.smo_train_svr(Xs, z, self.params, self.epsilon)
        self._finish(alpha2, res, sw)
        self._dev = None
        self.support_vectors_ = Xs[self.support_].copy()
        self.timings_ = {"smo_ms": res.seconds * 1e3}

    def _fit_cuda(self, X, z, dev, sw=None):
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        zd = torch.from_numpy(z).to(device)
        alpha = torch.empty(2 * X.shape[0], dtype=torch.float64, device=device)  # the cold start zeroes it
        # pixel rows stay bytes on the device (the exact-integer plan reads them); FP64 rows are scaled there and
        # quantised when they admit the plan, else solved with FP64-MFMA kernel values
        wd = torch.from_numpy(sw).to(device) if sw is not None else None
        rows, out = solve_on_rows(X, device, lambda r: D.train_decomp_svr(
            r.rows, zd, alpha, self.params, r.mn_h, r.mx_h, epsilon=self.epsilon, working_set=self.working_set)
            if wd is None else D.train_decomp_sw(r.rows, zd, wd, alpha, self.params, r.mn_h, r.mx_h, epsilon=self.epsilon,
                                                 working_set=self.working_set),
            bytes_ok=not self.params.gram_kernel)  # a dot-product kernel: the FP64 rows, scaled on the device
        if out is None:
            raise ValueError("SVR: the decomposition solver does not cover these rows (its FP64-row workspace, "
                             "n x 1024 doubles, does not fit the device)")
        res, tm = out
        self._finish(alpha.cpu().numpy(), res, sw)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    def _fit_cuda_sparse(self, X, z, dev):
        """CSR rows: scaled by their column maxima on the device, kernel values from the CSR x panel kernel."""
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        rows = SparseTrainRows.upload(X, device)
        alpha = torch.empty(2 * rows.csr.n, dtype=torch.float64, device=device)
        res, tm = D.train_decomp_csr(rows.csr, alpha, self.params, z=torch.from_numpy(z).to(device),
                                     epsilon=self.epsilon, working_set=self.working_set)
        self._finish(alpha.cpu().numpy(), res)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    def _fit_cuda_f32(self, X, z, dev, row_dtype="float32"):
        """float32 rows: scaled and rounded once on the device, kernel values from the FP32-MFMA block."""
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        rows = TrainRows.upload(X, device, row_dtype=row_dtype)
        alpha = torch.empty(2 * X.shape[0], dtype=torch.float64, device=device)
        train = D.train_decomp_f16 if row_dtype == "float16" else D.train_decomp_f32
        res, tm = train(rows.rows, rows.sqn, rows.d, alpha, self.params, z=torch.from_numpy(z).to(device),
                        epsilon=self.epsilon, working_set=self.working_set)
        self._finish(alpha.cpu().numpy(), res)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    def _fit_cuda_f16(self, X, z, dev):
        """float16 rows (rows_f16.hip): the float32 routing with the other row source."""
        self._fit_cuda_f32(X, z, dev, row_dtype="float16")

    # ------------------------------------------------------------------ inference
    def predict(self, X: np.ndarray) -> np.ndarray:
        """sum_k beta_k K(x_k, x) - b over the support vectors (a model without any predicts -b)."""
        self._check_X(X)
        if self._dev is not None:
            return self._device_decide(X).cpu().numpy()
        from ..ops import cpu as C

        if not self.params.precomputed:  # a query Gram keeps its dtype: anything but float64 raises
            X = np.ascontiguousarray(toarray(X) if is_sparse(X) else X, dtype=np.float64)
        Xq = self.scaler_.transform(X) if self.scaler_ is not None else X
        if self.params.gram_kernel:
            return host_kernel_decision(self, Xq, self.dual_coef_)
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
                   meta={"n_iter": self.n_iter_, "stop_reason": self.stop_reason_, "epsilon": self.epsilon,
                         **({"n_fit": self.n_fit_} if self.params.precomputed else {})})

    @classmethod
    def load(cls, directory: str | os.PathLike, device: str = "cpu") -> "SVR":
        from ..models.model_io import load_model

        m = load_model(directory)
        if m["kind"] != KIND:
            raise ValueError(f"{directory} holds a {m['kind']!r} model, not an SVR (load it with its own class)")
        p = m["params"]
        svr = cls(C=p.C, gamma=p.gamma, epsilon=m["meta"].get("epsilon", 0.1), tol=p.tau, eps=p.eps, sv_tol=p.sv_tol,
                  max_iter=p.max_iter, device=device, scale=m["scaler"] is not None, kernel=p.kernel, degree=p.degree,
                  coef0=p.coef0)
        svr.scaler_ = m["scaler"]
        svr.support_ = m["ids"]
        svr.dual_coef_ = m["alphas"] * m["labels"]
        svr.b_ = m["b"]
        svr.intercept_ = -m["b"]
        svr.n_iter_ = m["meta"].get("n_iter")
        svr.stop_reason_ = m["meta"].get("stop_reason")
        svr.support_vectors_ = m["sv_rows"]
        if "n_fit" in m["meta"]:  # a precomputed kernel: the queries' width
            svr.n_fit_ = int(m["meta"]["n_fit"])
        if _resolve_device(device) != "cpu":
            svr._upload_model(_resolve_device(device))
        return svr

    def _upload_model(self, dev: str) -> None:
        if self.scaler_ is None and not self.params.precomputed:
            raise ValueError("SVR on a GPU needs a scaled model (scale=True)")
        super()._upload_model(dev)
