"""Kernel SVM estimator (RBF, one-vs-rest binary) with a CPU oracle backend and an MI355X backend.

``SVC.fit`` runs the reference pipeline — min-max scaling fitted on the training rows
(main3.cpp:57-89), first-order SMO with the reference stop rules (main3.cpp:162-294) — and keeps
the support vectors (alpha > sv_tol, main3.cpp:297-304).  ``predict`` is sign(sum alpha y K - b)
over the SVs (main3.cpp:391-402; the serial/GPU programs map 0 to -1, the cascades to +1 — see
``zero_is_positive``).

Backends
  device="cpu"   native C++ oracle (bit-exact reference arithmetic), ``n_threads`` workers
  device="cuda"  gfx950 kernels: H2D, fused min/max + scale + row norms, the exact-integer int8-MFMA
                 RBF Gram (f64-MFMA for real-valued data) kept resident in HBM, the persistent
                 device SMO (one launch, register-resident slices), MFMA decision function over the
                 SVs; ``kcache="rows"`` (automatic when the Gram does not fit) solves on the HBM row
                 cache instead
"""
from __future__ import annotations

import json
import os
import time
from pathlib import Path
from typing import Optional

import numpy as np

from ..utils.config import SVMParams, default_threads
from ..utils.data import check_folds, check_warm_start, resolve_class_weight, stratified_folds
from ._device import KernelEstimator, _is_u8, _resolve_device, platt_probability, scaled_cpu, solve_on_rows


class SVC(KernelEstimator):
    def __init__(self, C: float = 10.0, gamma: float = 0.00125, tol: float = 1e-5, eps: float = 1e-12,
                 sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto", n_threads: int = 0,
                 scale: bool = True, zero_is_positive: bool = False, gram: str = "auto", kcache: str = "auto",
                 wss: str = "first", solver: str = "auto", working_set: int = 1024, shrinking=False,
                 class_weight=None, probability: bool = False, cv: int = 5, cv_seed: int = 0):
        if wss not in ("first", "second"):
            raise ValueError("wss must be 'first' (the reference's selection) or 'second'")
        if solver not in ("auto", "smo", "decomp"):
            raise ValueError("solver must be 'auto' (decomp on GPUs, smo on the CPU), 'decomp' (working-set "
                             "decomposition) or 'smo' (the reference's pairwise SMO over all n points)")
        self.params = SVMParams(C=C, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads(),
                                wss=2 if wss == "second" else 1, shrinking=shrinking)
        # class weights (scikit-learn's class_weight, LIBSVM's -wi): None, "balanced" (n / (2 n_c), resolved
        # per fit from the labels) or {1: w_pos, -1: w_neg}; row i's box is [0, C * w(y_i)].  The CPU oracle
        # and the GPU decomposition solver take them; the pairwise GPU solver, shrinking and the knobs that
        # route to the pairwise solver (gram=, kcache=, wss="second") raise with them.
        resolve_class_weight(class_weight)  # the option's form; the weights themselves per fit
        self.class_weight = class_weight
        self.device = device
        self.scale = scale
        self.zero_is_positive = zero_is_positive
        self._sv_host = None
        self.gram = gram  # "auto" | "fp64" | "int" (device backend Gram path, see ops.device.train)
        self.kcache = kcache  # "auto" | "full" (resident Gram) | "rows" (on-demand HBM row cache)
        self._dev = None  # device-side model state (torch tensors)
        # "decomp" (the GPU default): working sets of up to `working_set` points solved in one workgroup
        # with the reference's stop test on all n points (decomp.hip; exact-integer kernel values for
        # pixel rows, FP64 MFMA for real-valued rows; cold or warm start) -- the same support vectors,
        # b within the stop tolerance, a different pair sequence.  "smo": the reference's solver (one
        # pair per iteration over all n points, resident Gram or row cache; the CPU oracle's, the CPU
        # default).  "auto" resolves per fit by device.  shrinking (the decomposition solver, as LIBSVM's /
        # scikit-learn's option): selection and the f update on the active points only, the stop test
        # still on all n (decomp_shrink.h); True, False (the default: measured slower on the headline shapes,
        # profiles/shrinking.md), or a pass every k outer iterations.
        self.solver = solver
        self.working_set = int(working_set)
        # probability (LIBSVM's -b 1, scikit-learn's probability=True): fit also runs cv-fold cross-validation
        # and fits Platt's sigmoid P(y = +1 | f) = 1 / (1 + exp(A f + B)) to the held-out decision values
        # (probA_, probB_, cv_decision_, cv_folds_; predict_proba).  On a GPU the folds are the decomposition
        # solver's held-out mode -- the ordinary solve on the shared device rows with the fold's labels masked
        # to 0 -- run side by side with the final model; predict stays the sign of the decision value.
        self.probability = bool(probability)
        self.cv = int(cv)
        self.cv_seed = int(cv_seed)
        if self.probability and self.cv < 2:
            raise ValueError(f"probability=True needs cv >= 2 folds, got cv={cv}")
        self.probA_ = self.probB_ = None

    # ------------------------------------------------------------------ fit
    def fit(self, X: np.ndarray, y: np.ndarray, alpha0: Optional[np.ndarray] = None,
            folds: Optional[np.ndarray] = None) -> "SVC":
        """folds (probability=True only): an explicit fold id per row instead of stratified_folds(y, cv, cv_seed)."""
        dev = _resolve_device(self.device)
        # uint8 pixel rows stay compact up to the device (8x less H2D; widened to FP64 there)
        X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) and y (n,)")
        if not np.all(np.abs(y) == 1):
            raise ValueError("labels must be +1/-1 (use svm355.utils.data.one_vs_rest)")
        wp, wn = resolve_class_weight(self.class_weight, y)
        self.params = self.params.replace(weight_pos=wp, weight_neg=wn)
        self.class_weight_ = {1: wp, -1: wn}
        if self.params.weighted:
            self._check_weighted(dev)
        if alpha0 is not None:
            alpha0 = check_warm_start(alpha0, y, self.params.box(y) if self.params.weighted else self.params.C)
        if folds is not None and not self.probability:
            raise ValueError("folds= is the cross-validation of probability=True (or use cross_val_decision)")
        self.probA_ = self.probB_ = self.cv_decision_ = self.cv_folds_ = self.platt_ = None
        self.classes_ = np.array([-1, 1], dtype=np.int32)
        t0 = time.perf_counter()
        if self.probability:
            self._check_cv(dev, alpha0)
            folds = self._folds(y, self.cv, self.cv_seed, folds)
            if dev == "cpu":
                self._fit_cpu(X, y, None)
                self._fit_probability_cpu(X, y, folds)
            else:
                self._fit_cuda_probability(X, y, folds, dev)
        elif dev == "cpu":
            self._fit_cpu(X, y, alpha0)
        else:
            self._fit_cuda(X, y, alpha0, dev)
        self.fit_time_ = time.perf_counter() - t0
        return self

    # ------------------------------------------------------------------ cross-validation and probabilities
    def _check_cv(self, dev: str, alpha0=None) -> None:
        """What cross-validation (and so probability=True) does not cover raises here, before any device work."""
        what = "probability=True / cross-validation"
        if alpha0 is not None:
            raise ValueError(f"{what} does not take a warm start (alpha0): every fold is a cold solve")
        if self.params._shrink_code() > 0:
            raise ValueError(f"{what} is not supported with shrinking (the held-out solve has none)")
        if dev == "cpu":
            return
        if self.solver == "smo":
            raise ValueError(f"{what} on a GPU runs on the decomposition solver's held-out mode, not solver='smo'")
        if not self.scale:
            raise ValueError(f"{what} on a GPU needs scale=True (the decomposition solver's min-max scaled rows)")
        for name, on in (("wss='second'", self.params.wss == 2), (f"gram={self.gram!r}", self.gram != "auto"),
                         (f"kcache={self.kcache!r}", self.kcache != "auto")):
            if on:
                raise ValueError(f"{what} on a GPU runs on the decomposition solver, which {name} (the pairwise "
                                 "solver) rules out")

    @staticmethod
    def _folds(y: np.ndarray, cv: int, seed: int, folds) -> np.ndarray:
        if folds is None:
            if int(cv) < 2:
                raise ValueError(f"cross-validation needs cv >= 2 folds, got cv={cv}")
            folds = stratified_folds(y, int(cv), int(seed))
        return check_folds(folds, y)

    def _cv_cpu(self, Xs: np.ndarray, y: np.ndarray, folds: np.ndarray):
        """Held-out decision values on the CPU: the pairwise oracle fits each fold's training rows (already
        scaled with all rows' bounds) and svm_decision scores the fold.  Returns (n values, per-fold ms)."""
        from ..ops import cpu as C

        dec = np.zeros(y.shape[0])
        fold_ms = []
        for j in range(int(folds.max()) + 1):
            t0 = time.perf_counter()
            te = folds == j
            Xtr, ytr = np.ascontiguousarray(Xs[~te]), np.ascontiguousarray(y[~te])
            a, res, _ = C.smo_train(Xtr, ytr, self.params)
            sv = a > self.params.sv_tol
            dec[te] = C.decision(Xtr[sv], ytr[sv], a[sv], np.ascontiguousarray(Xs[te]), self.params.gamma, res.b,
                                 self.params.n_threads)
            fold_ms.append((time.perf_counter() - t0) * 1e3)
        return dec, fold_ms

    def _fit_probability_cpu(self, X, y, folds) -> None:
        from ..ops import cpu as C

        t0 = time.perf_counter()
        dec, fold_ms = self._cv_cpu(scaled_cpu(X, self.scale)[0], y, folds)
        t1 = time.perf_counter()
        self._set_platt(C.platt_fit(dec, y), dec, folds)
        self.timings_.update({"cv_ms": (t1 - t0) * 1e3, "platt_ms": (time.perf_counter() - t1) * 1e3,
                              "fold_ms": fold_ms})

    def _set_platt(self, pl, dec: np.ndarray, folds: np.ndarray) -> None:
        self.platt_ = pl
        self.probA_, self.probB_ = pl.A, pl.B
        self.cv_decision_ = dec
        self.cv_folds_ = folds

    def _cv_device(self, X, y, folds, device, final: bool, concurrent_solves: Optional[int] = None):
        """The fold solves on the GPU, and with ``final`` the model's own solve beside them: the rows go to the
        device once, and every solve is the decomposition solver on them -- a fold's with its rows' labels masked
        to 0 (held-out mode: their f - b is their held-out decision value, no prediction pass) -- one per host
        thread and stream through the one-vs-rest pool (its width rule and column-cache share).  Returns the
        TrainRows and a dict: "yd", "dec" (device, n: the folds' disjoint held-out vectors summed), "final" ((alpha,
        result, timing) or None), "fold_timings", "cv_ms", "width"."""
        import torch

        from ..ops import device as D
        from .multiclass import _pool, pool_shape, pool_stream

        n = X.shape[0]
        k = int(folds.max()) + 1
        masks_h = np.stack([(folds == j).astype(np.uint8) for j in range(k)], 0)
        tasks = ([-1] if final else []) + list(range(k))
        width, frac = pool_shape(len(tasks), concurrent_solves, *X.shape)

        def solve_all(rows):
            yd = torch.from_numpy(y).to(device)
            masks = torch.from_numpy(masks_h).to(device)
            alphas = torch.zeros((k + 1, n), dtype=torch.float64, device=device)
            decs = torch.zeros((k, n), dtype=torch.float64, device=device)
            torch.cuda.synchronize(device)
            t1 = time.perf_counter()

            def solve(j):
                with pool_stream(device, frac):
                    if j < 0:
                        return D.train_decomp(rows.rows, yd, alphas[k], self.params, rows.mn_h, rows.mx_h,
                                              working_set=self.working_set)
                    return D.train_decomp_heldout(rows.rows, yd, masks[j], alphas[j], decs[j], self.params, rows.mn_h,
                                                  rows.mx_h, working_set=self.working_set)

            outs = dict(zip(tasks, _pool(width).map(solve, tasks)))
            torch.cuda.synchronize(device)
            if any(o is None for o in outs.values()):
                return None
            dec = decs.sum(0)  # disjoint and zero elsewhere: exact in any order
            torch.cuda.synchronize(device)
            return {"yd": yd, "dec": dec, "final": (alphas[k],) + outs[-1] if final else None,
                    "fold_timings": [outs[j][1] for j in range(k)], "cv_ms": (time.perf_counter() - t1) * 1e3,
                    "width": width}

        rows, out = solve_on_rows(X, device, solve_all)
        if out is None:
            raise ValueError("the decomposition solver does not cover these rows (n beyond its shapes, or the "
                             "FP64-row solve's workspace does not fit the device); cross-validation on a GPU "
                             "needs it")
        return rows, out

    def _fit_cuda_probability(self, X, y, folds, dev) -> None:
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        rows, cv = self._cv_device(X, y, folds, device, final=True)
        alpha, res, tm = cv["final"]
        t0 = time.perf_counter()
        pl = D.platt_fit(cv["dec"], cv["yd"])
        platt_ms = (time.perf_counter() - t0) * 1e3
        self._finish(alpha.cpu().numpy(), y, res)
        self._adopt_rows(rows)
        self._set_platt(pl, cv["dec"].cpu().numpy(), folds)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm, "cv_ms": cv["cv_ms"],
                         "platt_ms": platt_ms, "fold_ms": [t["total_ms"] for t in cv["fold_timings"]],
                         "concurrent_solves": cv["width"]}

    def cross_val_decision(self, X: np.ndarray, y: np.ndarray, cv: int = 5, seed: int = 0,
                           folds: Optional[np.ndarray] = None, concurrent_solves: Optional[int] = None) -> np.ndarray:
        """The n held-out decision values of k-fold cross-validation with this estimator's options: row i's value
        comes from the model fitted without row i's fold.  folds: an explicit fold id per row instead of
        ``stratified_folds(y, cv, seed)``.  Min-max scaling is that of all rows, and class_weight="balanced"
        resolves on all labels.  Fits no sigmoid and leaves the estimator's own model alone.  On a GPU the folds
        run ``concurrent_solves`` at a time (default: all of them while the rows fit the last-level cache)."""
        dev = _resolve_device(self.device)
        X = np.ascontiguousarray(X, dtype=np.uint8 if (dev != "cpu" and _is_u8(X)) else np.float64)
        y = np.ascontiguousarray(y, dtype=np.int32)
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) and y (n,)")
        if not np.all(np.abs(y) == 1):
            raise ValueError("labels must be +1/-1 (use svm355.utils.data.one_vs_rest)")
        wp, wn = resolve_class_weight(self.class_weight, y)
        self.params = self.params.replace(weight_pos=wp, weight_neg=wn)
        if self.params.weighted:
            self._check_weighted(dev)
        self._check_cv(dev)
        folds = self._folds(y, cv, seed, folds)
        if dev == "cpu":
            return self._cv_cpu(scaled_cpu(X, self.scale)[0], y, folds)[0]
        import torch

        _, out = self._cv_device(X, y, folds, torch.device(dev), final=False, concurrent_solves=concurrent_solves)
        self.cv_timings_ = {"cv_ms": out["cv_ms"], "fold_ms": [t["total_ms"] for t in out["fold_timings"]],
                            "concurrent_solves": out["width"]}
        return out["dec"].cpu().numpy()

    def cross_val_score(self, X: np.ndarray, y: np.ndarray, cv: int = 5, seed: int = 0,
                        folds: Optional[np.ndarray] = None) -> float:
        """The held-out accuracy of k-fold cross-validation (LIBSVM's -v k): the share of rows whose held-out
        decision value has their label's sign (``zero_is_positive`` as in predict)."""
        dec = self.cross_val_decision(X, y, cv, seed, folds)
        pos = dec >= 0 if self.zero_is_positive else dec > 0
        return float(np.mean(np.where(pos, 1, -1) == np.asarray(y)))

    def predict_proba(self, X: np.ndarray) -> np.ndarray:
        """(m, 2) probabilities in the order of classes_ = [-1, 1]: Platt's sigmoid of decision_function(X), in
        its overflow-safe form, on the host."""
        if self.probA_ is None:
            raise ValueError("predict_proba needs a model fitted with probability=True")
        return platt_probability(self.probA_ * self.decision_function(X) + self.probB_)

    def _check_weighted(self, dev: str) -> None:
        """Class weights run on the CPU oracle and on the GPU decomposition solver (no shrinking); everything
        else raises here, before any device work."""
        p = self.params
        if p._shrink_code() > 0:
            p.refuse_weights("shrinking")
        if dev == "cpu":
            return
        if self.solver == "smo":
            p.refuse_weights("the GPU pairwise solver (solver='smo')")
        for name, on in (("wss='second'", p.wss == 2), (f"gram={self.gram!r}", self.gram != "auto"),
                         (f"kcache={self.kcache!r}", self.kcache != "auto"), ("scale=False", not self.scale)):
            if on:
                p.refuse_weights(f"{name} (the GPU pairwise solver)")

    def _finish(self, alpha: np.ndarray, y: np.ndarray, res) -> None:
        self.alpha_ = alpha
        self.support_ = np.flatnonzero(alpha > self.params.sv_tol).astype(np.int64)
        self.dual_coef_ = alpha[self.support_] * y[self.support_]
        self.support_labels_ = y[self.support_].astype(np.int32)
        self.b_ = res.b
        self.intercept_ = -res.b
        self.n_iter_ = res.iterations
        self.stop_reason_ = res.stop_reason
        self.result_ = res

    def _fit_cpu(self, X, y, alpha0):
        from ..ops import cpu as C

        if self.solver == "decomp":
            raise ValueError("solver='decomp' runs on the GPU (device='cuda'); the CPU oracle is the pairwise SMO")
        Xs = self._scaled_cpu(X)
        alpha, res, _ = C.smo_train(Xs, y, self.params, alpha=alpha0, warm=alpha0 is not None)
        self._finish(alpha, y, res)
        self.support_vectors_ = Xs[self.support_].copy()
        self.timings_ = {"smo_ms": res.seconds * 1e3}

    def _fit_cuda(self, X, y, alpha0, dev):
        import torch

        from ..ops import device as D

        device = torch.device(dev)
        # auto: the decomposition unless a pairwise-only knob was asked for (second-order pair
        # selection, a forced Gram path or the row cache)
        decomp = self.solver == "decomp" or (self.solver == "auto" and self.params.wss != 2 and self.gram == "auto"
                                             and self.kcache == "auto")
        if decomp and not self.scale:
            if self.solver == "decomp":
                raise ValueError("solver='decomp' needs scale=True (min-max scaled rows: its exact-integer "
                                 "plan, or the FP64 rows it solves on)")
            decomp = False  # auto without scaling: the pairwise solver
        # uint8 pixel rows stay bytes on the device -- min/max, the exact-integer quantisation and the solver (the
        # decomposition, or the pairwise one on a resident exact-integer Gram) read them directly, and only the
        # support vectors are ever widened to scaled FP64 (for prediction): the same trajectory and model as from
        # the FP64 rows, minus their widen / scale / FP64-quantise passes.  FP64 host rows (the reference's
        # format), and bytes the solver declined, are scaled on the device, then quantised into the same integers
        # or -- real-valued data -- solved with FP64-MFMA kernel values.
        bytes_ok = X.dtype == np.uint8 and self.scale and (decomp or (
            self.gram in ("auto", "int") and self.kcache in ("auto", "full")
            and os.environ.get("SVM355_U8_TRAIN", "1") != "0"
            and (self.kcache != "auto" or D.gram_fits(X.shape[0], device))))
        warm = alpha0 is not None
        yd = torch.from_numpy(y).to(device)
        if warm:
            alpha = torch.from_numpy(np.ascontiguousarray(alpha0, dtype=np.float64)).to(device)
        else:
            alpha = torch.empty(X.shape[0], dtype=torch.float64, device=device)  # the cold start zeroes it

        def solve(r):
            u8 = r.sqn is None
            out = None
            if decomp:
                out = D.train_decomp(r.rows, yd, alpha, self.params, r.mn_h, r.mx_h, working_set=self.working_set,
                                     warm=warm)
                if out is None and not u8 and self.solver == "decomp":
                    raise ValueError("solver='decomp': the device rows' stride is not a multiple of 16, n is beyond the "
                                     "solver's 2^31 - 1 rows, or the FP64-row solve's workspace (n x 1024 doubles) does "
                                     "not fit the device")
            elif u8:
                out = D.train_u8(r.rows, yd, alpha, self.params, r.mn_h, r.mx_h, warm=warm)
            if out is not None or u8:  # bytes that nothing ran on (not an integer plan): the FP64 rows take over
                return out
            if self.params.weighted:  # then the decomposition or an error: never the pairwise solver
                self.params.refuse_weights("the GPU pairwise solver, which this fit falls back to (the decomposition "
                                           "solver does not cover these rows)")
            # the pairwise solver (also solver="auto" when the decomposition's workspace does not fit)
            return D.train(r.rows, r.sqn, yd, alpha, self.params, warm=warm, mn=r.mn, mx=r.mx, gram=self.gram,
                           kcache=self.kcache)

        rows, (res, tm) = solve_on_rows(X, device, solve, scale=self.scale, bytes_ok=bytes_ok)
        self._finish(alpha.cpu().numpy(), y, res)
        self._adopt_rows(rows)
        self.timings_ = {"upload_preprocess_ms": rows.upload_ms, **tm}

    # ------------------------------------------------------------------ inference
    def decision_function(self, X: np.ndarray) -> np.ndarray:
        self._check_X(X)
        if self._dev is not None:
            return self._device_decision(X).cpu().numpy()
        return self._host_decision(X)

    def _device_decision(self, X: np.ndarray):
        """Decision values as a device tensor (device models only)."""
        from ..ops import device as D

        dv = self._dev
        Xq, nq = self._device_queries(X)
        return D.decision(dv["Xs"], dv["ns"], dv["coef"], Xq, nq, self.params.gamma, self.b_)

    def _host_decision(self, X: np.ndarray) -> np.ndarray:
        from ..ops import cpu as C

        X = np.ascontiguousarray(X, dtype=np.float64)
        Xq = self.scaler_.transform(X) if self.scaler_ is not None else X
        return C.decision(self.support_vectors_, self.support_labels_, self.alpha_[self.support_], Xq,
                          self.params.gamma, self.b_, self.params.n_threads)

    def predict(self, X: np.ndarray) -> np.ndarray:
        dec = self.decision_function(X)
        pos = dec >= 0 if self.zero_is_positive else dec > 0
        return np.where(pos, 1, -1).astype(np.int32)

    def score(self, X: np.ndarray, y: np.ndarray) -> float:
        """Accuracy.  Device models count the correct signs on the device (count_correct)."""
        y = np.asarray(y)
        if self._dev is not None and len(y):
            from ..ops import device as D

            self._check_X(X)
            return D.count_correct(self._device_decision(X), y, self.zero_is_positive) / len(y)
        return float(np.mean(self.predict(X) == y))

    # ------------------------------------------------------------------ persistence
    def save(self, directory: str | os.PathLike, ids: Optional[np.ndarray] = None) -> None:
        """Reference model files (final_sv_{ids,labels,alphas}.txt, final_b.txt) + loadable extras."""
        from ..models.model_io import save_model

        save_model(directory, ids=self.support_ if ids is None else ids, labels=self.support_labels_,
                   alphas=self.alpha_[self.support_], b=self.b_, sv_rows=self.support_vectors_,
                   scaler=self.scaler_, params=self.params,
                   meta={"n_iter": self.n_iter_, "stop_reason": self.stop_reason_,
                         **({"probA": self.probA_, "probB": self.probB_} if self.probA_ is not None else {})})

    @classmethod
    def load(cls, directory: str | os.PathLike, device: str = "cpu") -> "SVC":
        from ..models.model_io import load_model

        m = load_model(directory)
        if m["kind"] != "svc":
            raise ValueError(f"{directory} holds a {m['kind']!r} model, not a classifier (load it with its own class)")
        p = m["params"]
        svc = cls(C=p.C, gamma=p.gamma, tol=p.tau, eps=p.eps, sv_tol=p.sv_tol, max_iter=p.max_iter, device=device,
                  scale=m["scaler"] is not None,
                  class_weight={1: p.weight_pos, -1: p.weight_neg} if p.weighted else None)
        svc.params = svc.params.replace(weight_pos=p.weight_pos, weight_neg=p.weight_neg)
        svc.class_weight_ = {1: p.weight_pos, -1: p.weight_neg}
        svc.scaler_ = m["scaler"]
        svc.support_ = m["ids"]
        svc.support_labels_ = m["labels"]
        svc.b_ = m["b"]
        svc.intercept_ = -m["b"]
        svc.support_vectors_ = m["sv_rows"]
        alphas = m["alphas"]
        # alpha_ is indexed by training row; a loaded model only knows its SVs.
        svc.alpha_ = np.zeros(int(svc.support_.max()) + 1 if len(svc.support_) else 0)
        svc.alpha_[svc.support_] = alphas
        svc.dual_coef_ = alphas * svc.support_labels_
        svc.classes_ = np.array([-1, 1], dtype=np.int32)
        if "probA" in m["meta"] and "probB" in m["meta"]:
            svc.probability = True
            svc.probA_, svc.probB_ = float(m["meta"]["probA"]), float(m["meta"]["probB"])
        if _resolve_device(device) != "cpu":
            svc._upload_model(_resolve_device(device))
        return svc
