"""Multi-class RBF SVM, one-vs-one: what LIBSVM and ``sklearn.svm.SVC`` train for more than two labels.

For k classes there are P = k (k - 1) / 2 pairs (a, b), a < b, in LIBSVM's order (0,1), (0,2), ..., (k-2,k-1);
class a is the pair's +1 side.  A pair is an ordinary two-class fit on the rows of its two classes, 2n/k rows
in place of n: all pairs together do (k - 1) n rows of kernel work against k n for one-vs-rest.  A decision
value > 0 votes for a, anything else (exactly 0 included) for b; the label is the class with the most votes,
the lowest class index on a tie.

One min/max over ALL training rows scales every pair (each solve is passed that ``mn`` / ``mx``), so the union
of support vectors has one scaling and a query row is scaled once.

On the GPU the rows are uploaded once and gathered once into a class-grouped copy (a stable sort by class
index: ids ascend within a class); a pair's rows are two contiguous slices of it packed into one small buffer,
and every pair is ``ops.device.train_decomp`` -- the decomposition solver, unchanged -- on its packed rows, the
pairs side by side on the persistent pool of ``OneVsRestSVC(solver="decomp")``.  (The rows are gathered, not
masked: a label of 0 on the shared rows would make every pair's f update run over all n rows, k/2 times the
kernel work, and produce decision values nobody wants.)  Prediction is one cross-kernel block against the
union of support vectors and the segmented vote kernel (csrc/hip/ovo.hip).

On the CPU (``device="cpu"``) a pair is the pairwise oracle ``ops.cpu.smo_train_gram`` on its block of one
``rbf_matrix`` over the scaled rows.  A pair's decision is the oracle's own (``svm_decision``: from -rho over the
pair's support vectors in ascending training-row order), so for k = 2 model and decisions are
``SVC(device="cpu")``'s bit for bit; the vote is ``ops.cpu.ovo_labels``, the rule of ``ops.cpu.ovo_votes`` (numpy,
the vote kernel's host twin, which sums class segment by class segment as the kernel does).

The fitted attributes are in scikit-learn's / LIBSVM's layout, so a model can be compared with
``sklearn.svm.SVC(decision_function_shape="ovo")``: ``support_`` (grouped by class, ascending within a class),
``n_support_``, ``dual_coef_`` ((k - 1, S): for a support vector of class c, row j holds its alpha * y in the
pair (c, o), o = j for j < c, else j + 1), ``rho_`` and ``intercept_ = -rho_``.

Probabilities (``cv=K``; LIBSVM's -b 1, scikit-learn's ``probability=True``): every pair gets Platt's sigmoid,
fitted to its rows' held-out decisions from K-fold cross-validation, and ``predict_proba`` couples the pair
probabilities of a query row into class probabilities by Wu, Lin and Weng's second method, as LIBSVM does
(``ops.device.ovo_couple``, csrc/hip/ovo_proba.hip; ``ops.cpu.ovo_couple`` on the CPU).  One fold vector over
all training rows serves every pair: a pair's folds are its restriction to the pair's rows, and a fold with none
of them is skipped for that pair.  On the GPU a pair's fold solves are the decomposition solver's held-out mode
on the pair's packed rows (``ops.device.train_decomp_heldout``), tasks on the pool beside the pair's own solve --
which is the ``cv=None`` solve unchanged, so the model is the same to the bit -- and one
``ops.device.platt_fit_batch`` launch fits all P sigmoids.  On the CPU every fold is the pairwise oracle on its
block of the one ``rbf_matrix``; for k = 2 with the same folds the result is ``SVC(device="cpu",
probability=True)``'s bit for bit.  ``probA_`` / ``probB_`` (P,) are in the pair order with LIBSVM's sign (the
pair's first class is the positive side), ``cv_decision_`` (n, k - 1) in the layout of ``dual_coef_``: for a row
of class c, column j is its held-out decision in the pair (c, o), o = j for j < c, else j + 1.
"""
from __future__ import annotations

import threading
import time
from typing import List, Optional

import numpy as np

from ..utils.config import SVMParams, default_threads
from ..utils.data import MinMaxScaler, check_folds_multiclass, stratified_folds
from ..utils.trace import trace_range
from ._device import (TrainRows, _resolve_device, check_query_shape, device_model_from_host, platt_probability,
                      scale_queries, scaled_cpu)

MAX_CLASSES = 64  # the vote kernel keeps the k (k - 1) segment sums of a query row in LDS (32 KB at 64)
FORMAT = "svm355-ovo-v1"

_UNSUPPORTED = {
    "class_weight": "class weights", "probability": "the probability= keyword (pass cv=K for pairwise-coupling probabilities)", "alpha0": "warm starts",
    "warm_start": "warm starts", "shrinking": "shrinking", "newton": "the Newton polish", "polish": "the Newton polish",
    "transport": "multi-GPU transports", "solver": "a solver other than the decomposition ('decomp')",
}


def _refuse(name: str, value) -> None:
    if value is None or value is False:
        return
    if name == "solver" and value in ("auto", "decomp"):
        return
    what = _UNSUPPORTED.get(name)
    if what is None:
        raise TypeError(f"OneVsOneSVC got an unexpected argument {name!r}")
    raise ValueError(f"OneVsOneSVC does not support {what} ({name}={value!r}): every pair is the plain cold-start "
                     "decomposition solve on one GPU (or the pairwise oracle on the CPU)")


class OneVsOneSVC:
    def __init__(self, C: float = 10.0, gamma: float = 0.00125, tol: float = 1e-5, eps: float = 1e-12,
                 sv_tol: float = 1e-8, max_iter: int = 100000, device: str = "auto", n_threads: int = 0,
                 concurrent_solves: Optional[int] = None, working_set: int = 1024, cv: Optional[int] = None,
                 cv_seed: int = 0, **unsupported):
        """``concurrent_solves`` (GPU): how many pair solves run side by side (default: all, at most 10).
        ``working_set``: the decomposition solver's working-set size.  ``cv=K`` (K >= 2; default None: no
        calibration, and nothing changes): fit also cross-validates every pair in K folds
        (``stratified_folds(class index, K, cv_seed)``, or ``fit(folds=)``) and fits its sigmoid, which gives
        ``predict_proba``.  Class weights, the ``probability=`` keyword (``cv=`` is its spelling here), warm
        starts, shrinking, the Newton polish, ``solver="smo"`` and transports are refused with a ``ValueError``."""
        for name, value in unsupported.items():
            _refuse(name, value)
        if cv is not None and (isinstance(cv, bool) or int(cv) != cv or int(cv) < 2):
            raise ValueError(f"cv must be None or a number of folds >= 2, got cv={cv!r}")
        self.cv = None if cv is None else int(cv)
        self.cv_seed = int(cv_seed)
        if concurrent_solves is not None and int(concurrent_solves) < 1:
            raise ValueError("concurrent_solves must be at least 1")
        self.params = SVMParams(C=C, gamma=gamma, tau=tol, eps=eps, sv_tol=sv_tol, max_iter=max_iter,
                                n_threads=n_threads if n_threads > 0 else default_threads())
        self.device = device
        self.concurrent_solves = concurrent_solves
        self.working_set = int(working_set)
        self._dev_model = None

    def _dev(self) -> str:
        return _resolve_device(self.device)

    # ------------------------------------------------------------------ fit
    def fit(self, X: np.ndarray, labels: np.ndarray, classes: Optional[List[int]] = None,
            transport=None, folds: Optional[np.ndarray] = None) -> "OneVsOneSVC":
        """folds (with ``cv`` only): an explicit fold id per training row in place of
        ``stratified_folds(class index, cv, cv_seed)``."""
        _refuse("transport", transport)
        if folds is not None and self.cv is None:
            raise ValueError("folds= is the cross-validation of a calibrated fit: pass cv= to the constructor")
        cuda = self._dev() != "cpu"
        X = np.ascontiguousarray(X, dtype=np.uint8 if (cuda and X.dtype == np.uint8) else np.float64)
        labels = np.asarray(labels)
        if X.ndim != 2 or labels.shape != (X.shape[0],):
            raise ValueError("X must be (n, d) and labels (n,)")
        self.classes_ = np.array(sorted(set(labels.tolist()) if classes is None else set(classes)))
        k = len(self.classes_)
        if k < 2:
            raise ValueError(f"one-vs-one needs at least 2 classes, got {k}")
        if k > MAX_CLASSES:
            raise ValueError(f"{k} classes: one-vs-one supports at most {MAX_CLASSES} classes")
        cls = np.searchsorted(self.classes_, labels)
        if np.any(self.classes_[np.minimum(cls, k - 1)] != labels):
            raise ValueError("labels holds a value that `classes` does not list")
        counts = np.bincount(cls, minlength=k)
        if np.any(counts == 0):
            empty = [int(c) for c in self.classes_[counts == 0]]
            raise ValueError(f"classes {empty} have no rows: every one-vs-one pair needs rows of both classes")
        from ..ops.cpu import ovo_pairs

        self._pairs = ovo_pairs(k)
        order = np.argsort(cls, kind="stable").astype(np.int64)  # class-grouped, ids ascending within a class
        cstart = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.probA_ = self.probB_ = self.platt_status_ = self.cv_folds_ = self.cv_decision_ = None
        if self.cv is not None:  # checked before any device work
            folds = check_folds_multiclass(stratified_folds(cls, self.cv, self.cv_seed) if folds is None else folds,
                                           cls, k)
        t0 = time.perf_counter()
        if cuda:
            self._fit_cuda(X, order, cstart, folds)
        else:
            self._fit_cpu(X, order, cstart, folds)
        self.fit_time_ = time.perf_counter() - t0
        return self

    def _pair_label(self, p: int):
        a, b = self._pairs[p]
        return int(self.classes_[a]), int(self.classes_[b])

    def _fit_cpu(self, X, order, cstart, folds=None):
        from ..ops import cpu as C

        Xg, self.scaler_ = scaled_cpu(X)
        Xg = Xg[order]  # scaled, class-grouped
        K = C.rbf_matrix(Xg, Xg, self.params.gamma, self.params.n_threads)
        alphas, results, timings = [], [], {}
        for p, (a, b) in enumerate(self._pairs):
            idx = np.concatenate([np.arange(cstart[a], cstart[a + 1]), np.arange(cstart[b], cstart[b + 1])])
            y = np.where(np.arange(len(idx)) < cstart[a + 1] - cstart[a], 1, -1).astype(np.int32)
            al, r, _ = C.smo_train_gram(np.ascontiguousarray(K[np.ix_(idx, idx)]), y, self.params)
            alphas.append(al)
            results.append(r)
            timings[self._pair_label(p)] = {"smo_ms": r.seconds * 1e3, "gram_path": "host"}
        keep = self._finish(alphas, results, order, cstart)
        self.support_vectors_ = np.ascontiguousarray(Xg[keep])
        self.pair_timings_ = timings
        self.timings_ = {"gram_path": "host", "solver": "smo (cpu oracle)", "pairs": len(self._pairs)}
        self._dev_model = None
        if folds is not None:
            self._calibrate_cpu(Xg, K, order, cstart, folds)

    def _calibrate_cpu(self, Xg, K, order, cstart, folds) -> None:
        """Per pair and fold the pairwise oracle on the block of K of the pair's rows outside the fold, and
        svm_decision on the fold's rows (from -rho over the support vectors); a pair's rows are taken in
        ascending training-row order, the order ``SVC`` sees them in, so that k = 2 is its cross-validation and
        its sigmoid bit for bit."""
        from ..ops import cpu as C

        t0 = time.perf_counter()
        decs, ys, solves = [], [], 0
        for a, b in self._pairs:
            idx = np.concatenate([np.arange(cstart[a], cstart[a + 1]), np.arange(cstart[b], cstart[b + 1])])
            y = np.where(np.arange(len(idx)) < cstart[a + 1] - cstart[a], 1, -1).astype(np.int32)
            by_row = np.argsort(order[idx], kind="stable")
            idx, y = idx[by_row], y[by_row]
            pf = folds[order[idx]]
            dec = np.zeros(len(idx))
            for j in np.unique(pf):
                te = pf == j
                tr = idx[~te]
                al, r, _ = C.smo_train_gram(np.ascontiguousarray(K[np.ix_(tr, tr)]), y[~te], self.params)
                sv = al > self.params.sv_tol
                dec[te] = C.decision(np.ascontiguousarray(Xg[tr[sv]]), y[~te][sv], al[sv],
                                     np.ascontiguousarray(Xg[idx[te]]), self.params.gamma, r.b, self.params.n_threads)
                solves += 1
            decs.append((order[idx], dec, y > 0))
            ys.append(y)
        t1 = time.perf_counter()
        platt = [C.platt_fit(d[1], y) for d, y in zip(decs, ys)]
        t2 = time.perf_counter()
        self._set_calibration(platt, decs, folds)
        self.timings_.update({"cv_ms": (t1 - t0) * 1e3, "platt_ms": (t2 - t1) * 1e3, "fold_solves": solves})

    def _set_calibration(self, platt, decs, folds) -> None:
        """platt: the P sigmoid results; decs: per pair (training-row ids, held-out decisions, row is of the
        pair's first class)."""
        k = len(self.classes_)
        self.probA_ = np.array([pl.A for pl in platt], dtype=np.float64)
        self.probB_ = np.array([pl.B for pl in platt], dtype=np.float64)
        self.platt_status_ = [pl.status for pl in platt]
        self.platt_ = list(platt)
        self.cv_folds_ = folds
        self.cv_decision_ = np.zeros((len(folds), k - 1))
        for (a, b), (ids, dec, is_a) in zip(self._pairs, decs):
            # a row of class a meets b > a in column b - 1; a row of class b meets a < b in column a
            self.cv_decision_[ids, np.where(is_a, b - 1, a)] = dec

    def _fit_cuda(self, X, order, cstart, folds=None):
        import torch

        from .. import _native as N
        from ..ops import device as D
        from .multiclass import _pool, pool_shape, pool_stream

        device = torch.device(self._dev())
        t0 = time.perf_counter()
        rows = TrainRows.upload(X, device)
        mn_h, mx_h = rows.mn_h, rows.mx_h
        grouped = rows.take(order)  # the one row gather
        torch.cuda.synchronize(device)
        t1 = time.perf_counter()
        P = len(self._pairs)
        width = max(1, min(int(self.concurrent_solves or 10), P))
        frac = pool_shape(P, width, *X.shape)[1]

        # Tasks, pair-major: a pair's own solve (j = -1: train_decomp, what cv=None runs), then with folds its
        # fold solves (the held-out mode on the same packed rows; a fold with none of the pair's rows is skipped).
        # The pool takes tasks in this order, so the pairs whose packed rows are resident at one time are those of
        # the running tasks and the one at the head of the queue: at most width + 1 buffers of 2n/k rows.  The
        # task that finishes a pair last sums its folds' held-out vectors (disjoint, zero elsewhere: exact in any
        # order) into the pair's segment of the one concatenated buffer and drops the pair's tensors.
        na = [int(cstart[a + 1] - cstart[a]) for a, _ in self._pairs]
        sizes = [int(na[p] + cstart[b + 1] - cstart[b]) for p, (_, b) in enumerate(self._pairs)]
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        tasks = [(p, -1) for p in range(P)]
        if folds is not None:
            fg_h = folds[order]
            fg = torch.from_numpy(np.ascontiguousarray(fg_h)).to(device)
            tasks = [(p, j) for p, (a, b) in enumerate(self._pairs)
                     for j in [-1] + np.unique(np.concatenate([fg_h[cstart[a]:cstart[a + 1]],
                                                               fg_h[cstart[b]:cstart[b + 1]]])).tolist()]
            y_all = torch.from_numpy(np.concatenate([np.where(np.arange(sizes[p]) < na[p], 1, -1)
                                                     for p in range(P)]).astype(np.int32)).to(device)
            dec_all = torch.zeros(int(offs[-1]), dtype=torch.float64, device=device)
            torch.cuda.synchronize(device)
        left = [sum(1 for t in tasks if t[0] == p) for p in range(P)]
        shared = [ln > 1 for ln in left]
        locks = [threading.Lock() for _ in range(P)]
        state: list = [None] * P

        def packed(p, s):
            a, b = self._pairs[p]
            with locks[p]:
                if state[p] is None:
                    rows = torch.cat([grouped[cstart[a]:cstart[a + 1]], grouped[cstart[b]:cstart[b + 1]]]).contiguous()
                    y = torch.ones(sizes[p], dtype=torch.int32, device=device)
                    y[na[p]:] = -1
                    st = {"rows": rows, "y": y, "decs": []}
                    if folds is not None:
                        st["folds"] = torch.cat([fg[cstart[a]:cstart[a + 1]], fg[cstart[b]:cstart[b + 1]]])
                    if shared[p]:
                        s.synchronize()  # the pair's other tasks read these from their own streams
                    state[p] = st
                return state[p]

        def solve(task):
            p, j = task
            al = dec = None
            with pool_stream(device, frac) as s:
                st = packed(p, s)
                alpha = torch.zeros(sizes[p], dtype=torch.float64, device=device)
                if j < 0:
                    out = D.train_decomp(st["rows"], st["y"], alpha, self.params, mn_h, mx_h,
                                         working_set=self.working_set)
                    al = alpha.cpu().numpy() if out is not None else None
                else:
                    dec = torch.zeros(sizes[p], dtype=torch.float64, device=device)
                    out = D.train_decomp_heldout(st["rows"], st["y"], (st["folds"] == j).to(torch.uint8), alpha, dec,
                                                 self.params, mn_h, mx_h, working_set=self.working_set)
            if out is None:
                raise N.NativeError(f"pair {self._pair_label(p)}: the decomposition solver declined these rows (no "
                                    "exact-integer plan for uint8 rows, or beyond its shapes); pass the rows as "
                                    "float64")
            with locks[p]:
                if dec is not None:
                    st["decs"].append(dec)
                left[p] -= 1
                last = left[p] == 0
            if last:
                if st["decs"]:
                    with torch.cuda.stream(s):
                        dec_all[offs[p]:offs[p + 1]] = torch.stack(st["decs"]).sum(0)
                    s.synchronize()
                state[p] = st = None  # every user of the pair's tensors has synchronised: release them
            return al, out[0], out[1]

        with trace_range(f"svm355.ovo.decomp pairs={P}" + ("" if folds is None else f" tasks={len(tasks)}")):
            every = list(_pool(width).map(solve, tasks))
            torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        outs = [o for t, o in zip(tasks, every) if t[1] < 0]
        keep = self._finish([o[0] for o in outs], [o[1] for o in outs], order, cstart)
        self._dev_model = rows.model(self.support_, self.dual_coef_, start=self._start(), rho=self.rho_)
        self.scaler_ = rows.scaler()
        self.pair_timings_ = {self._pair_label(p): outs[p][2] for p in range(P)}
        paths = sorted({o[2]["gram_path"] for o in outs})
        self.timings_ = {"upload_preprocess_ms": (t1 - t0) * 1e3, "smo_ms_all_pairs": (t2 - t1) * 1e3,
                         "gram_path": paths[0] if len(paths) == 1 else "mixed", "solver": "decomp", "pairs": P,
                         "concurrent_solves": width}
        if folds is not None:
            tp = time.perf_counter()
            platt = D.platt_fit_batch(dec_all, y_all, offs)  # synchronises
            platt_ms = (time.perf_counter() - tp) * 1e3
            dec_h = dec_all.cpu().numpy()
            decs = []
            for p, (a, b) in enumerate(self._pairs):
                pos = np.concatenate([np.arange(cstart[a], cstart[a + 1]), np.arange(cstart[b], cstart[b + 1])])
                decs.append((order[pos], dec_h[offs[p]:offs[p + 1]], np.arange(sizes[p]) < na[p]))
            self._set_calibration(platt, decs, folds)
            fold_ms = [o[2]["total_ms"] for t, o in zip(tasks, every) if t[1] >= 0]
            # cv_ms: the pool's wall time -- the pairs' own solves and their fold solves side by side, as SVC's
            self.timings_.update({"cv_ms": (t2 - t1) * 1e3, "platt_ms": platt_ms, "fold_solves": len(fold_ms),
                                  "fold_solve_ms_sum": float(sum(fold_ms)),
                                  "pair_solve_ms_sum": float(sum(o[2]["total_ms"] for o in outs))})

    def _finish(self, alphas, results, order, cstart) -> np.ndarray:
        """The per-pair alphas (a's rows, then b's) to LIBSVM's layout.  Returns the positions of the support
        vectors in the class-grouped order."""
        k = len(self.classes_)
        per_class = [np.zeros((k - 1, int(cstart[c + 1] - cstart[c]))) for c in range(k)]
        for (a, b), al in zip(self._pairs, alphas):
            na = int(cstart[a + 1] - cstart[a])
            per_class[a][b - 1] = al[:na]     # y = +1
            per_class[b][a] = -al[na:]        # y = -1
        masks = [(np.abs(pc) > self.params.sv_tol).any(0) for pc in per_class]
        keep = np.concatenate([cstart[c] + np.flatnonzero(masks[c]) for c in range(k)]).astype(np.int64)
        self.support_ = order[keep]
        self.n_support_ = np.array([int(mk.sum()) for mk in masks], dtype=np.int64)
        self.dual_coef_ = np.ascontiguousarray(np.concatenate([per_class[c][:, masks[c]] for c in range(k)], axis=1))
        self.rho_ = np.array([r.b for r in results], dtype=np.float64)
        self.intercept_ = -self.rho_
        self.n_iter_ = np.array([r.iterations for r in results])
        self.stop_reasons_ = [r.stop_reason for r in results]
        return keep

    def _start(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.n_support_)]).astype(np.int32)

    # ------------------------------------------------------------------ persistence
    def _host_sv_rows(self) -> np.ndarray:
        if self._dev_model is not None:
            dm = self._dev_model
            return np.ascontiguousarray(dm["Xs"][:, : dm["d"]].cpu().numpy())
        return np.ascontiguousarray(self.support_vectors_)

    def save(self, directory) -> None:
        """``dual_coef.npy``, ``rho.npy``, ``support.npy``, ``n_support.npy``, the support vectors' scaled rows
        (``sv_rows.npy``), the scaler (``scaler.npz``) and ``ovo.json`` -- pickle-free throughout.  A calibrated
        model (``cv=``) also writes the pairs' sigmoids (``prob.npz``: A, B) and records ``cv`` in ``ovo.json``;
        an uncalibrated one writes exactly the files above."""
        import json
        from pathlib import Path

        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        np.save(d / "sv_rows.npy", self._host_sv_rows(), allow_pickle=False)
        np.save(d / "dual_coef.npy", np.ascontiguousarray(self.dual_coef_, dtype=np.float64), allow_pickle=False)
        np.save(d / "rho.npy", np.ascontiguousarray(self.rho_, dtype=np.float64), allow_pickle=False)
        np.save(d / "support.npy", np.ascontiguousarray(self.support_, dtype=np.int64), allow_pickle=False)
        np.save(d / "n_support.npy", np.ascontiguousarray(self.n_support_, dtype=np.int64), allow_pickle=False)
        np.savez(d / "scaler.npz", min=self.scaler_.min_, max=self.scaler_.max_)
        info = {"format": FORMAT, "classes": [int(x) for x in self.classes_], "n_sv_union": int(len(self.support_)),
                "n_iter": [int(x) for x in self.n_iter_], "stop_reasons": list(self.stop_reasons_),
                "params": self.params.as_dict()}
        if getattr(self, "probA_", None) is not None:
            np.savez(d / "prob.npz", A=np.ascontiguousarray(self.probA_, dtype=np.float64),
                     B=np.ascontiguousarray(self.probB_, dtype=np.float64))
            info["cv"] = self.cv
        (d / "ovo.json").write_text(json.dumps(info, indent=2))

    @classmethod
    def load(cls, directory, device: str = "cpu") -> "OneVsOneSVC":
        """The model ``save`` wrote; ``device`` "cuda[:k]" keeps the support vectors on that GPU for prediction."""
        import json
        from pathlib import Path

        d = Path(directory)
        info = json.loads((d / "ovo.json").read_text())
        if info.get("format") != FORMAT:
            raise ValueError(f"{d / 'ovo.json'}: format {info.get('format')!r}, expected {FORMAT!r}")
        p = SVMParams(**info["params"])
        m = cls(C=p.C, gamma=p.gamma, tol=p.tau, eps=p.eps, sv_tol=p.sv_tol, max_iter=p.max_iter, device=device)
        m.classes_ = np.array(info["classes"])
        k = len(m.classes_)
        from ..ops.cpu import ovo_pairs

        m._pairs = ovo_pairs(k)
        m.dual_coef_ = np.load(d / "dual_coef.npy", allow_pickle=False)
        m.rho_ = np.load(d / "rho.npy", allow_pickle=False)
        m.intercept_ = -m.rho_
        m.support_ = np.load(d / "support.npy", allow_pickle=False)
        m.n_support_ = np.load(d / "n_support.npy", allow_pickle=False)
        m.support_vectors_ = np.load(d / "sv_rows.npy", allow_pickle=False)
        S = len(m.support_)
        if (m.dual_coef_.shape != (k - 1, S) or m.rho_.shape != (len(m._pairs),) or m.n_support_.shape != (k,)
                or int(m.n_support_.sum()) != S or m.support_vectors_.shape[0] != S or np.any(m.n_support_ < 0)):
            raise ValueError(f"{d}: the saved arrays do not fit {k} classes and {S} support vectors")
        z = np.load(d / "scaler.npz", allow_pickle=False)
        m.scaler_ = MinMaxScaler(z["min"], z["max"])
        m.probA_ = m.probB_ = m.platt_status_ = m.cv_folds_ = m.cv_decision_ = None
        if (d / "prob.npz").exists():
            z = np.load(d / "prob.npz", allow_pickle=False)
            m.probA_, m.probB_ = np.asarray(z["A"], dtype=np.float64), np.asarray(z["B"], dtype=np.float64)
            if m.probA_.shape != (len(m._pairs),) or m.probB_.shape != (len(m._pairs),):
                raise ValueError(f"{d / 'prob.npz'}: A and B do not fit {len(m._pairs)} pairs")
            m.cv = info.get("cv")
        m.n_iter_ = np.asarray(info.get("n_iter", [0] * len(m._pairs)))
        m.stop_reasons_ = list(info.get("stop_reasons", [""] * len(m._pairs)))
        m._dev_model = None
        if m._dev() != "cpu":
            m._dev_model = device_model_from_host(m.support_vectors_.reshape(S, int(np.size(m.scaler_.min_))), m.scaler_,
                                                  m.dual_coef_, m._dev(), start=m._start(), rho=m.rho_)
        return m

    # ------------------------------------------------------------------ inference
    def _decide(self, X: np.ndarray, want_dec: bool, on_device: bool = False):
        d = int(np.size(self.scaler_.min_))
        check_query_shape(X, d)
        if self._dev_model is not None:
            from ..ops import device as D

            dm = self._dev_model
            Xq, nq = scale_queries(dm, X)
            dec, lab = D.ovo_predict(dm["Xs"], dm["ns"], Xq, nq, self.params.gamma, dm["start"], dm["coef"],
                                     dm["rho"], want_dec=want_dec)
            if on_device:
                return dec, lab
            return (dec.cpu().numpy() if want_dec else None), lab.cpu().numpy()
        from ..ops import cpu as C

        # the CPU oracle's arithmetic, pair by pair: from -rho over the pair's support vectors in ascending
        # training-row order (svm_decision), so that k = 2 is SVC(device="cpu") bit for bit; the vote is
        # ovo_votes' rule
        Xq = self.scaler_.transform(np.ascontiguousarray(X, dtype=np.float64))
        sv = self.support_vectors_.reshape(len(self.support_), d)
        start = self._start()
        dec = np.empty((Xq.shape[0], len(self._pairs)))
        for p, (a, b) in enumerate(self._pairs):
            seg = np.concatenate([np.arange(start[a], start[a + 1]), np.arange(start[b], start[b + 1])])
            coef = np.concatenate([self.dual_coef_[b - 1, start[a]:start[a + 1]],
                                   self.dual_coef_[a, start[b]:start[b + 1]]])
            by_row = np.argsort(self.support_[seg], kind="stable")
            seg, coef = seg[by_row], coef[by_row]
            dec[:, p] = C.decision(sv[seg], np.where(np.signbit(coef), -1, 1), np.abs(coef), Xq, self.params.gamma,
                                   self.rho_[p], self.params.n_threads)
        return dec, C.ovo_labels(dec, len(self.classes_))

    def decision_function(self, X: np.ndarray) -> np.ndarray:
        """(m, P) pair decisions in LIBSVM's pair order; > 0 is a vote for the pair's first class."""
        return self._decide(X, True)[0]

    def predict(self, X: np.ndarray) -> np.ndarray:
        """The one-vs-one vote, calibrated or not: as in scikit-learn, the class with the largest
        ``predict_proba`` may differ from it."""
        return self.classes_[self._decide(X, False)[1]]

    def predict_proba(self, X: np.ndarray) -> np.ndarray:
        """(m, k) class probabilities in the order of ``classes_`` (a model fitted with ``cv=``): the pair
        decisions of ``decision_function`` through the pairs' sigmoids, coupled by Wu, Lin and Weng's second
        method as in LIBSVM -- on the GPU without leaving it (``ops.device.ovo_couple``), on the CPU by the
        kernel's host twin.  ``predict`` stays the vote: its label may differ from the largest probability's."""
        if getattr(self, "probA_", None) is None:
            raise ValueError("predict_proba needs a calibrated model: fit with OneVsOneSVC(cv=K)")
        if self._dev_model is not None:
            import torch

            from ..ops import device as D

            dm = self._dev_model
            if "probA" not in dm:
                dm["probA"] = torch.from_numpy(np.ascontiguousarray(self.probA_)).to(dm["device"])
                dm["probB"] = torch.from_numpy(np.ascontiguousarray(self.probB_)).to(dm["device"])
            dec, _ = self._decide(X, True, on_device=True)
            return D.ovo_couple(dec, dm["probA"], dm["probB"], want_label=False)[0].cpu().numpy()
        from ..ops import cpu as C

        # The pair probabilities P(+1) by SVC.predict_proba's own expression, so that k = 2 gives them bit for
        # bit; the twin takes them as they are (A = B = None).
        z = self._decide(X, True)[0] * self.probA_ + self.probB_
        return C.ovo_couple(np.ascontiguousarray(platt_probability(z)[..., 1]), n_threads=self.params.n_threads)[0]

    def score(self, X: np.ndarray, labels: np.ndarray) -> float:
        return float(np.mean(self.predict(X) == np.asarray(labels)))
