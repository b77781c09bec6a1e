"""L0/L1 data layer: CSV datasets, MNIST-shaped synthetic data, min-max scaling.

``load_csv`` mirrors ``read_CSV`` (main3.cpp:13-54, row-limited gpu_svm_main4.cu:16-59) through
the native parser; ``MinMaxScaler`` mirrors ``find_min_max``/``scale_features`` (main3.cpp:57-89)
including the ``range < 1e-12 -> 1`` rule.  ``synthetic_mnist`` produces a deterministic
MNIST-shaped problem (784 integer pixels, digit labels 0-9) because the reference's MNIST CSVs are
not part of the reference repository.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .. import _native as N

MNIST_D = 784


@dataclass
class Dataset:
    X: np.ndarray  # (n, d) float64 (or uint8 after compact()), C-contiguous
    y: np.ndarray  # (n,) int32 in {+1, -1}
    labels: np.ndarray  # (n,) int32 raw labels

    @property
    def n(self) -> int:
        return int(self.X.shape[0])

    @property
    def d(self) -> int:
        return int(self.X.shape[1])

    def subset(self, start: int, stop: int) -> "Dataset":
        return Dataset(self.X[start:stop], self.y[start:stop], self.labels[start:stop])

    def compact(self) -> "Dataset":
        """The same dataset with uint8 rows when every feature is an integer in [0, 255] (pixels)."""
        Xc = compact_pixels(self.X)
        return self if (Xc is None or Xc is self.X) else Dataset(Xc, self.y, self.labels)


def compact_pixels(X: np.ndarray) -> Optional[np.ndarray]:
    """uint8 copy of X if every value is an integer in [0, 255], else None.

    MNIST-style pixel data are bytes; the reference holds them as FP64 (read_CSV, main3.cpp:13-54)
    and ships 8 bytes per pixel to the GPU.  The device path accepts the uint8 rows directly and
    widens them to FP64 on the device, where every value is exact, so results are unchanged."""
    X = np.asarray(X)
    if X.dtype == np.uint8:
        return X
    if X.size == 0:
        return None
    if X.dtype.kind == "f" and not np.isfinite(X).all():
        return None
    if X.min() < 0 or X.max() > 255:
        return None
    Xc = X.astype(np.uint8)
    return Xc if np.array_equal(Xc, X) else None


def check_labels(y, n: int) -> np.ndarray:
    """y as int32 of shape (n,) with every label +1 or -1 (main3.cpp:49-52 maps the digit labels);
    ValueError otherwise.  A 0 label falls in neither I_high nor I_low, so a solve would 'converge'
    to a wrong model instead of failing."""
    y = np.ascontiguousarray(y)
    if y.shape != (n,):
        raise ValueError(f"y must have shape ({n},), got {y.shape}")
    if not np.all(np.abs(y) == 1):
        raise ValueError("labels must be +1/-1 (use svm355.utils.data.one_vs_rest)")
    return y.astype(np.int32, copy=False)


def resolve_class_weight(class_weight, y: np.ndarray = None):
    """(weight_pos, weight_neg) of a ``class_weight`` option: None -> (1, 1); a dict with exactly the keys
    1 and -1 -> its values; "balanced" -> n / (2 n_c) from the labels y (scikit-learn's rule; an absent
    class is an error).  y = None validates the option's form only (and returns None for "balanced")."""
    if class_weight is None:
        return 1.0, 1.0
    if isinstance(class_weight, str):
        if class_weight != "balanced":
            raise ValueError(f"class_weight must be None, 'balanced' or {{1: w_pos, -1: w_neg}}, got {class_weight!r}")
        if y is None:
            return None
        y = np.asarray(y)
        n, n_pos, n_neg = int(y.shape[0]), int(np.sum(y == 1)), int(np.sum(y == -1))
        for label, cnt in ((1, n_pos), (-1, n_neg)):
            if cnt == 0:
                raise ValueError(f"class_weight='balanced': class {label:+d} is absent from y")
        return n / (2.0 * n_pos), n / (2.0 * n_neg)
    if not isinstance(class_weight, dict) or set(class_weight.keys()) != {1, -1}:
        raise ValueError(f"class_weight must be None, 'balanced' or a dict with exactly the keys 1 and -1, got "
                         f"{class_weight!r}")
    w = (float(class_weight[1]), float(class_weight[-1]))
    if not all(np.isfinite(v) and v > 0 for v in w):
        raise ValueError(f"class weights must be finite and > 0, got {class_weight!r}")
    return w


def check_warm_start(alpha0, y: np.ndarray, C) -> np.ndarray:
    """alpha0 as float64 (n,) that is a feasible point of the dual: finite, inside the box [0, C] (to rounding) and on
    the equality constraint sum(alpha y) = 0 (to rounding).  C: the box constraint, or every row's own (n,)
    under class weights.  ValueError otherwise: the solvers assume a
    feasible start, and from an infeasible one they stop on a "converged" model that is not a solution."""
    a = np.ascontiguousarray(alpha0, dtype=np.float64)
    n = y.shape[0]
    if a.shape != (n,):
        raise ValueError(f"alpha0 must have shape ({n},), got {a.shape}")
    # the solvers' own alphas may sit a few ulps outside the box (a_i moves by the rounded step of a_j,
    # as in the reference's update, gpu_svm_main3.cu:441-448): a previous solution must stay a valid start
    box = np.broadcast_to(np.asarray(C, dtype=np.float64), (n,))
    tol = 1e-9 * np.maximum(1.0, box)
    if not np.all(np.isfinite(a)) or np.any(a < -tol) or np.any(a > box + tol):
        raise ValueError("alpha0 must be finite and inside [0, C = %s]"
                         % (C if np.ndim(C) == 0 else "its class's box, %s" % sorted(set(box.tolist()))))
    s = float(np.dot(a, y.astype(np.float64)))
    if abs(s) > 1e-9 * max(1.0, float(a.sum())):
        raise ValueError(f"alpha0 must satisfy sum(alpha0 * y) = 0 (the dual's equality constraint), got {s:.3g}")
    return a


def check_finite_bounds(mn, mx) -> None:
    """ValueError when a column's min / max is NaN or infinite, i.e. the rows hold a NaN or an infinity
    (numpy's and the device's column bounds propagate NaN): a fit would otherwise find no violating pair
    and return an empty model without saying why."""
    bounds = np.concatenate([np.asarray(mn, dtype=np.float64).ravel(), np.asarray(mx, dtype=np.float64).ravel()])
    if not np.all(np.isfinite(bounds)):
        d = np.asarray(mn).size
        bad = sorted({int(j) for j in np.flatnonzero(~np.isfinite(bounds)) % max(d, 1)})[:8]
        raise ValueError(f"X holds NaN or infinite values (columns {bad}{' ...' if len(bad) == 8 else ''})")


def pixel_rows(X, what: str) -> np.ndarray:
    """X as C-contiguous uint8 (n, d) when every value is an integer in [0, 255]; ValueError naming
    `what` otherwise (never a silent cast: 3.7 or 300 would be truncated or wrapped)."""
    Xc = compact_pixels(X)
    if Xc is None or Xc.ndim != 2:
        raise ValueError(f"{what} needs integer pixel rows (n, d) in [0, 255] (the exact-integer kernel values)")
    return np.ascontiguousarray(Xc)


def stratified_folds(y, k: int, seed: int = 0) -> np.ndarray:
    """Fold ids in [0, k) for k-fold cross-validation, stratified per class: each class's rows are permuted by
    one seeded ``numpy.random.Generator`` (the classes in ascending label order) and dealt round-robin, class
    after class without restarting the deal, so every class's fold sizes differ by at most 1 and so do the folds'.
    Deterministic for (y, k, seed); host only."""
    y = np.asarray(y)
    k = int(k)
    if y.ndim != 1:
        raise ValueError("y must be 1-D")
    if k < 2:
        raise ValueError(f"cross-validation needs k >= 2 folds, got {k}")
    if k > y.shape[0]:
        raise ValueError(f"{k} folds for {y.shape[0]} rows")
    rng = np.random.default_rng(int(seed))
    folds = np.empty(y.shape[0], dtype=np.int32)
    dealt = 0
    for c in np.unique(y):
        idx = np.flatnonzero(y == c)
        idx = idx[rng.permutation(idx.size)]
        folds[idx] = (dealt + np.arange(idx.size)) % k
        dealt += idx.size
    return folds


def check_folds(folds, y: np.ndarray) -> np.ndarray:
    """A fold array for y as int32 (n,): ids 0 .. k - 1 with k >= 2, every id used, and both classes present in
    every fold's training part (all rows outside the fold).  ValueError otherwise."""
    f = np.ascontiguousarray(folds)
    n = y.shape[0]
    if f.shape != (n,) or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"folds must be an integer array of shape ({n},)")
    k = int(f.max()) + 1 if n else 0
    if k < 2 or f.min() < 0:
        raise ValueError(f"cross-validation needs fold ids 0 .. k - 1 with k >= 2, got ids {int(f.min())} .. {k - 1}")
    for j in range(k):
        out = f == j
        if not out.any():
            raise ValueError(f"fold {j} of {k} is empty")
        tr = y[~out]
        if not (np.any(tr == 1) and np.any(tr == -1)):
            raise ValueError(f"fold {j}: its training part (the rows outside it) lacks a class")
    return f.astype(np.int32, copy=False)


def check_folds_multiclass(folds, cls: np.ndarray, n_classes: int) -> np.ndarray:
    """A fold array for the class indices ``cls`` (0 .. n_classes - 1) as int32 (n,): ids 0 .. K - 1 with K >= 2,
    every id used, and every class with rows outside every fold -- so the training part of every one-vs-one pair
    in every fold keeps both of its classes.  ValueError otherwise."""
    f = np.ascontiguousarray(folds)
    cls = np.asarray(cls)
    n = cls.shape[0]
    if f.shape != (n,) or not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"folds must be an integer array of shape ({n},)")
    K = int(f.max()) + 1 if n else 0
    if K < 2 or f.min() < 0:
        raise ValueError(f"cross-validation needs fold ids 0 .. K - 1 with K >= 2, got ids {int(f.min())} .. {K - 1}")
    per = np.zeros((int(n_classes), K), dtype=np.int64)  # rows of class c in fold j
    np.add.at(per, (cls, f), 1)
    empty = np.flatnonzero(per.sum(0) == 0)
    if empty.size:
        raise ValueError(f"fold {int(empty[0])} of {K} is empty")
    c, j = np.nonzero(per == per.sum(1, keepdims=True))
    if c.size:
        raise ValueError(f"class index {int(c[0])} has all its rows in fold {int(j[0])}: that fold's training part "
                         "lacks the class")
    return f.astype(np.int32, copy=False)


def one_vs_rest(labels: np.ndarray, positive_label: int = 1) -> np.ndarray:
    """label == positive_label -> +1, else -1 (main3.cpp:49-52 with positive_label = 1)."""
    return np.where(np.asarray(labels) == positive_label, 1, -1).astype(np.int32)


def load_csv(path: str | os.PathLike, limit: Optional[int] = None, positive_label: int = 1,
             n_threads: int = 0) -> Dataset:
    lib = N.core()
    h = lib.svm_csv_load(os.fsencode(str(path)), -1 if limit is None else int(limit), int(positive_label),
                         int(n_threads))
    if not h:
        raise FileNotFoundError(N.last_error())
    try:
        n, d = ctypes.c_int64(), ctypes.c_int64()
        N.check(lib.svm_dataset_dims(h, ctypes.byref(n), ctypes.byref(d)), "svm_dataset_dims")
        X = np.empty((n.value, d.value), dtype=np.float64)
        y = np.empty(n.value, dtype=np.int32)
        lab = np.empty(n.value, dtype=np.int32)
        N.check(lib.svm_dataset_copy(h, N.ptr(X), N.ptr(y), N.ptr(lab)), "svm_dataset_copy")
    finally:
        lib.svm_dataset_free(h)
    return Dataset(X, y, lab)


def write_csv(path: str | os.PathLike, X: np.ndarray, labels: np.ndarray) -> None:
    X = np.ascontiguousarray(X, dtype=np.float64)
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    N.check(N.core().svm_csv_write(os.fsencode(str(path)), N.ptr(X), N.ptr(labels), X.shape[0], X.shape[1]),
            "svm_csv_write")


def synthetic_mnist(n: int, seed: int = 2024, offset: int = 0, positive_label: int = 1,
                    n_threads: int = 0) -> Dataset:
    """Rows [offset, offset + n) of the deterministic MNIST-shaped generator (see csrc/core/synth.cpp).

    Row i depends only on (seed, i): a train split [0, N) and a test split [N, N + M) are disjoint
    draws of the same distribution, and any rank can generate exactly its own partition.
    """
    X = np.empty((n, MNIST_D), dtype=np.float64)
    lab = np.empty(n, dtype=np.int32)
    N.check(N.core().svm_synth_mnist(int(seed), int(offset), int(n), N.ptr(X), N.ptr(lab), int(n_threads)),
            "svm_synth_mnist")
    return Dataset(X, one_vs_rest(lab, positive_label), lab)


class MinMaxScaler:
    """Column min-max scaling to [0, 1] with the reference's degenerate-range rule."""

    def __init__(self, min_: Optional[np.ndarray] = None, max_: Optional[np.ndarray] = None):
        self.min_ = min_
        self.max_ = max_

    def fit(self, X: np.ndarray) -> "MinMaxScaler":
        X = np.ascontiguousarray(X, dtype=np.float64)
        self.min_ = np.empty(X.shape[1])
        self.max_ = np.empty(X.shape[1])
        N.check(N.core().svm_minmax(N.ptr(X), X.shape[0], X.shape[1], N.ptr(self.min_), N.ptr(self.max_)),
                "svm_minmax")
        return self

    def transform(self, X: np.ndarray, copy: bool = True) -> np.ndarray:
        X = np.array(X, dtype=np.float64, order="C", copy=copy)
        if X.shape[0]:
            N.check(N.core().svm_scale(N.ptr(X), X.shape[0], X.shape[1], N.ptr(self.min_), N.ptr(self.max_)),
                    "svm_scale")
        return X

    def fit_transform(self, X: np.ndarray) -> np.ndarray:
        return self.fit(X).transform(X)
