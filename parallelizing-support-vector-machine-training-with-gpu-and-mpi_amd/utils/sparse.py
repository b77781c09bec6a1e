"""Sparse rows in CSR form: the public input type of ``SVC`` / ``SVR`` beside dense arrays, and its host checks.

Any object with ``data``, ``indices``, ``indptr`` and ``shape`` is taken (``scipy.sparse.csr_matrix`` among them;
scipy is neither imported nor required); :class:`CSR` is that object for callers without it.  Everything a
kernel relies on is checked here, on the host, before anything is uploaded: a kernel never sees an index
outside ``[0, d)``.
"""
from __future__ import annotations

import numpy as np


class CSR:
    """``n`` rows of ``d`` features: row i holds ``data[indptr[i]:indptr[i + 1]]`` at the columns
    ``indices[indptr[i]:indptr[i + 1]]`` (sorted, unique)."""

    def __init__(self, data, indices, indptr, shape):
        self.data, self.indices, self.indptr = data, indices, indptr
        self.shape = (int(shape[0]), int(shape[1]))

    @classmethod
    def from_dense(cls, X) -> "CSR":
        X = np.asarray(X, dtype=np.float64)
        r, c = np.nonzero(X)
        return cls(X[r, c], c.astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(r, minlength=X.shape[0]))]),
                   X.shape)

    def toarray(self) -> np.ndarray:
        return toarray(self)


def is_sparse(X) -> bool:
    return (not isinstance(X, np.ndarray)) and all(hasattr(X, a) for a in ("data", "indices", "indptr", "shape"))


def refuse_sparse(X) -> None:
    """The estimators without a sparse path."""
    if is_sparse(X):
        raise TypeError("sparse rows: SVC and SVR only")


def check_csr(X) -> CSR:
    """X as a CSR of contiguous float64 / int32 / int64 arrays, or ValueError: indptr monotone from 0 to nnz,
    indices in [0, d) and strictly ascending within a row, finite values."""
    if len(X.shape) != 2:
        raise ValueError("sparse X must be 2-D (n, d)")
    n, d = int(X.shape[0]), int(X.shape[1])
    data = np.ascontiguousarray(X.data, dtype=np.float64)
    indices = np.asarray(X.indices)
    indptr = np.ascontiguousarray(X.indptr, dtype=np.int64)
    if data.ndim != 1 or indices.shape != data.shape or indptr.shape != (n + 1,):
        raise ValueError("sparse X: data and indices must be 1-D of one length and indptr of length n + 1")
    if d < 1 or d >= 2**31 - 1 or n >= 2**31 - 1:
        raise ValueError(f"sparse X: shape {X.shape} is outside 1 <= d, n < 2^31 - 1")
    nnz = data.shape[0]
    if indptr[0] != 0 or indptr[-1] != nnz or np.any(np.diff(indptr) < 0):
        raise ValueError("sparse X: indptr must rise monotonically from 0 to nnz")
    if nnz and (indices.min() < 0 or indices.max() >= d):
        bad = int(np.flatnonzero((indices < 0) | (indices >= d))[0])
        raise ValueError(f"sparse X: index {int(indices[bad])} at position {bad} is outside [0, {d})")
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    if nnz > 1:
        row = np.repeat(np.arange(n), np.diff(indptr))
        if np.any((row[1:] == row[:-1]) & (np.diff(indices) <= 0)):
            raise ValueError("sparse X: the indices of a row must be sorted and unique")
    if not np.all(np.isfinite(data)):
        raise ValueError("X holds NaN or infinite values")
    return CSR(data, indices, indptr, (n, d))


def check_zero_min(X: CSR) -> None:
    """Min-max scaling must keep zeros zero: every column's minimum over all n rows, implicit zeros included, is
    0.  ValueError naming the first column with a negative stored value, or stored in every row with a positive
    minimum."""
    n, d = X.shape
    bad = []
    neg = X.data < 0
    if np.any(neg):
        bad.append(int(X.indices[neg].min()))
    count = np.bincount(X.indices, minlength=d)
    full = np.flatnonzero(count == n) if n else np.empty(0, dtype=np.int64)
    if full.size:
        sel = np.isin(X.indices, full)
        mins = np.full(d, np.inf)
        np.minimum.at(mins, X.indices[sel], X.data[sel])
        pos = np.flatnonzero(np.isfinite(mins) & (mins > 0))
        if pos.size:
            bad.append(int(pos[0]))
    if bad:
        raise ValueError(f"sparse X: column {min(bad)} has a nonzero minimum (a negative stored value, or a column "
                         "stored in every row with a positive minimum), so min-max scaling would not keep zeros zero; "
                         "pass the dense array (X.toarray()) instead")


def toarray(X) -> np.ndarray:
    """The dense (n, d) float64 array of checked CSR rows."""
    X = check_csr(X)
    out = np.zeros(X.shape, dtype=np.float64)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    out[rows, X.indices] = X.data
    return out
