"""The estimators' plumbing between host rows and the native solvers: training rows on the device
(``TrainRows``; ``SparseTrainRows`` for CSR input), the byte-rows-then-FP64-rows attempt (``solve_on_rows``), the device model dict
(``device_model*``), the query prologue (``scale_queries``) and the members ``SVC``, ``SVR`` and
``OneClassSVM`` share (``KernelEstimator``).  ``OneVsRestSVC`` and ``OneVsOneSVC`` use the functions."""
from __future__ import annotations

import os
import re
import time
from typing import Optional

import numpy as np

from ..utils.data import MinMaxScaler, check_finite_bounds
from ..utils.sparse import check_csr, check_zero_min, is_sparse


def _resolve_device(device: str) -> str:
    if device == "auto":
        import torch

        return "cuda" if torch.cuda.is_available() else "cpu"
    return device


def _is_u8(X) -> bool:
    return isinstance(X, np.ndarray) and X.dtype == np.uint8


def _to_device(a, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class TrainRows:
    """Training rows on the device in the solvers' format: uint8 pixel rows (n, d) as they are (``sqn`` None), or
    min-max scaled, zero-padded FP64 rows (n, ld) with their squared norms.  ``mn`` / ``mx`` are the two halves of
    one 2 d device buffer, ``mn_h`` / ``mx_h`` its host copy (one D2H, finite or a ValueError); all four are None
    with ``scale=False``.  ``upload_ms``: the host time of ``upload``."""

    def __init__(self, rows, mn, mx, mn_h, mx_h, sqn, d, device, upload_ms):
        self.rows, self.mn, self.mx, self.mn_h, self.mx_h, self.sqn = rows, mn, mx, mn_h, mx_h, sqn
        self.d, self.device, self.upload_ms = d, device, upload_ms

    @property
    def f32(self) -> bool:
        """float32 rows (``row_dtype="float32"``): scaled and rounded once on the device, FP64 norms."""
        import torch

        return self.rows.dtype == torch.float32

    @property
    def f16(self) -> bool:
        """float16 rows (``row_dtype="float16"``): scaled and rounded (to float32, then float16) on the device."""
        import torch

        return self.rows.dtype == torch.float16

    @classmethod
    def upload(cls, X: np.ndarray, device, scale: bool = True, widen: bool = False,
               row_dtype: str = "float64") -> "TrainRows":
        """uint8 host rows stay bytes on the device (min / max from the bytes; no PyTorch kernel runs: a
        process's first one loads PyTorch's code objects, ~95 ms of a cold first fit,
        profiles/r3_cold_fit_probe.txt), unless ``widen``: then they cross PCIe as bytes and are widened there
        into the FP64 rows that float64 host rows become.  ``scale=False`` (FP64 rows only): unscaled rows and
        their norms, through which a NaN / inf anywhere shows.  ``row_dtype="float32"``: the rows cross PCIe and
        stay on the device as float32 (any dtype, uint8 too, cast on the host once), min-max scaled there by
        ``float32((float64(x) - mn) / range)`` with the FP64 norms of the rounded values.  ``row_dtype="float16"``:
        a float16 host array crosses PCIe as it is (2 bytes a value) and is scaled in place; any other dtype crosses as
        float32 and is scaled into a float16 buffer, the float32 staging rows being released before the solve.  The
        rule is ``float16(float32((float64(x) - mn) / range))``, norms again in FP64 of the rounded values."""
        import torch

        from ..ops import device as D

        t0 = time.perf_counter()
        d = X.shape[1]
        mn = mx = mn_h = mx_h = sqn = None
        if row_dtype == "float32":
            if not scale:
                raise ValueError("float32 device rows are min-max scaled rows (scale=True)")
            rows = D.upload_rows_f32(X, device)
            mn, mx, sqn = D.minmax_scale_f32_(rows, d)
        elif row_dtype == "float16":
            if not scale:
                raise ValueError("float16 device rows are min-max scaled rows (scale=True)")
            if X.dtype == np.float16:
                rows = D.upload_rows_f16(X, device)
                mn, mx, sqn = D.minmax_scale_f16_(rows, d)
            else:
                staging = D.upload_rows_f32(X, device)
                rows = D.device_empty((X.shape[0], D.padded_dim_f16(d)), torch.float16, device)
                mn, mx, sqn = D.minmax_scale_f16_(rows, d, src=staging)
                del staging  # released before the solve (stream-ordered: the caller's stream waits for the scaling)
        elif _is_u8(X) and not widen:
            if not scale:
                raise ValueError("uint8 device rows are min-max scaled rows (scale=True)")
            rows = D.upload_u8(X, device)
            mn, mx = D.minmax_u8(rows, out=torch.empty(2 * d, dtype=torch.float64, device=device))
        else:
            rows = D.upload_rows(X, device)
            if scale:
                mn, mx, sqn = D.minmax_scale_(rows, d)
            else:
                sqn = D.row_norms(rows, d)
                if not np.all(np.isfinite(sqn.cpu().numpy())):  # a NaN / inf anywhere makes its row's norm one
                    raise ValueError("X holds NaN or infinite values")
        if scale:
            mm = mn.as_strided((2 * d,), (1,)).cpu().numpy()  # both bounds (one buffer), one copy; synchronises
            mn_h, mx_h = mm[:d].copy(), mm[d:].copy()
            check_finite_bounds(mn_h, mx_h)
        return cls(rows, mn, mx, mn_h, mx_h, sqn, d, torch.device(device), (time.perf_counter() - t0) * 1e3)

    def _index(self, idx):
        import torch

        if not isinstance(idx, torch.Tensor):
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
        return idx.to(self.device)

    def take(self, idx):
        """Rows ``idx`` (host ids or a device int64 tensor) as a contiguous copy in the rows' own format."""
        from ..ops import device as D

        idx = self._index(idx)
        return self.rows[idx].contiguous() if self.sqn is None else D.gather_rows(self.rows, idx)

    def sv(self, idx):
        """(Xs, ns): rows ``idx`` as scaled, padded FP64 rows and their squared norms (a model's support vectors)."""
        from ..ops import device as D

        idx = self._index(idx)
        if self.sqn is None:
            return D.sv_rows_u8(self.rows, idx, self.mn, self.mx)
        if self.f32:  # widened: a model keeps FP64 support vectors, so everything after the fit is the FP64 code
            return D.rows_f32_dense(self.rows, self.sqn, idx)
        if self.f16:
            return D.rows_f16_dense(self.rows, self.sqn, idx, self.d)
        return self.take(idx), self.sqn[idx].contiguous()

    def model(self, support, coef, **extra) -> dict:
        """The device model of the fit on these rows: support vectors ``support`` with coefficients ``coef``."""
        return device_model(self.sv(support), coef, self.mn, self.mx, self.d, self.device, **extra)

    def scaler(self) -> Optional[MinMaxScaler]:
        return MinMaxScaler(self.mn_h, self.mx_h) if self.mn_h is not None else None


class SparseTrainRows:
    """Training rows given in CSR form, on the device as CSR (``csr``: a ``DeviceCSR``), scaled there by their
    column maxima with their squared norms.  Min-max scaling keeps zeros zero only when every column's minimum is
    0 (``check_zero_min``, on the host before the upload), so ``mn`` is all zeros and the scaler an ordinary
    ``MinMaxScaler``: the model is the one the dense FP64 path fits on ``X.toarray()``, up to rounding."""

    def __init__(self, csr, mn, mx, mn_h, mx_h, device, upload_ms):
        self.csr, self.mn, self.mx, self.mn_h, self.mx_h = csr, mn, mx, mn_h, mx_h
        self.d, self.device, self.upload_ms = csr.d, device, upload_ms

    @classmethod
    def upload(cls, X, device) -> "SparseTrainRows":
        import torch

        from ..ops import device as D

        t0 = time.perf_counter()
        X = check_csr(X)
        check_zero_min(X)
        csr = D.upload_csr(X, device)
        mn, mx, _ = D.csr_prepare(csr)
        mm = mn.as_strided((2 * csr.d,), (1,)).cpu().numpy()  # both bounds (one buffer), one copy; synchronises
        mn_h, mx_h = mm[:csr.d].copy(), mm[csr.d:].copy()
        check_finite_bounds(mn_h, mx_h)
        return cls(csr, mn, mx, mn_h, mx_h, torch.device(device), (time.perf_counter() - t0) * 1e3)

    def sv(self, idx):
        """(Xs, ns): rows ``idx`` scattered into dense, padded FP64 rows, and their norms: a model keeps its
        support vectors dense, so the device model, ``support_vectors_`` and save / load are those of dense fits."""
        import torch

        from ..ops import device as D

        if not isinstance(idx, torch.Tensor):
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
        return D.csr_rows_dense(self.csr, idx.to(self.device))

    def model(self, support, coef, **extra) -> dict:
        return device_model(self.sv(support), coef, self.mn, self.mx, self.d, self.device, **extra)

    def scaler(self) -> MinMaxScaler:
        return MinMaxScaler(self.mn_h, self.mx_h)


def solve_on_rows(X: np.ndarray, device, solve, scale: bool = True, bytes_ok: bool = True):
    """``solve(rows)`` on the device rows of X: the byte rows first when X is uint8 (and ``bytes_ok`` and
    ``scale``), and when ``solve`` returns None (nothing ran: no exact-integer plan for these bytes) the FP64 rows
    of the same X.  Returns (rows, what solve returned) of the attempt that ran -- its ``upload_ms`` is that
    attempt's alone -- or (None, None) when both declined."""
    if _is_u8(X) and scale and bytes_ok:
        rows = TrainRows.upload(X, device)
        out = solve(rows)
        if out is not None:
            return rows, out
        del rows  # the bytes leave the device before their FP64 form arrives
    rows = TrainRows.upload(X, device, scale=scale, widen=True)
    out = solve(rows)
    return (rows, out) if out is not None else (None, None)


def device_model(sv, coef, mn, mx, d, device, **extra) -> dict:
    """The one place the device model is built: ``sv`` = (Xs, ns), the scaled, padded FP64 support vectors and
    their squared norms; ``coef`` and ``extra`` (one-vs-rest: ``b``; one-vs-one: ``start``, ``rho``) are host
    arrays, uploaded here; mn / mx: the scaling bounds on the device (None for an unscaled model)."""
    Xs, ns = sv
    return {"Xs": Xs, "ns": ns, "coef": _to_device(coef, device), "mn": mn, "mx": mx, "d": int(d), "device": device,
            **{k: _to_device(v, device) for k, v in extra.items()}}


def _no_rows(d: int, device):
    """(Xs, ns) of a model without support vectors (it predicts -b)."""
    import torch

    from ..ops import device as D

    return (torch.empty((0, D.padded_dim(d)), dtype=torch.float64, device=device),
            torch.empty(0, dtype=torch.float64, device=device))


def _device_bounds(scaler: Optional[MinMaxScaler], d: int, device):
    if scaler is None:
        return None, None
    mm = _to_device(np.concatenate([scaler.min_, scaler.max_]).astype(np.float64), device)
    return mm[:d], mm[d:]


def device_model_from_host(sv_rows: np.ndarray, scaler: Optional[MinMaxScaler], coef, device, **extra) -> dict:
    """The device model of a loaded (or host-assembled) one: ``sv_rows`` (k, d) are scaled FP64 host rows."""
    import torch

    from ..ops import device as D

    device = torch.device(device)
    k, d = sv_rows.shape
    if k:
        Xs = D.upload_rows(sv_rows, device)
        sv = Xs, D.row_norms(Xs, d)
    else:
        sv = _no_rows(d, device)
    return device_model(sv, coef, *_device_bounds(scaler, d, device), d, device, **extra)


def device_model_from_u8(X_sv: np.ndarray, scaler: MinMaxScaler, coef, device, **extra) -> dict:
    """The device model from the support vectors' uint8 pixel rows (the distributed trainers): only their bytes
    cross PCIe, widened and scaled on the device (svmd_sv_rows_u8) -- no host FP64 transform and no FP64 upload
    (~1 MB instead of 8.6 MB at 60k).  No PyTorch kernel runs (copies and the library's own kernels only)."""
    import torch

    from ..ops import device as D

    device = torch.device(device)
    X_sv = np.ascontiguousarray(X_sv, dtype=np.uint8)
    k, d = X_sv.shape
    mn, mx = _device_bounds(scaler, d, device)
    if k:
        sv = D.sv_rows_u8(D.upload_u8(X_sv, device), _to_device(np.arange(k, dtype=np.int64), device), mn, mx)
    else:
        sv = _no_rows(d, device)
    return device_model(sv, coef, mn, mx, d, device, **extra)


def check_query_shape(X, d: Optional[int]) -> None:
    if is_sparse(X):
        if len(X.shape) != 2 or (d is not None and X.shape[1] != d):
            raise ValueError(f"X must be (m, {d}) like the training rows, got shape {tuple(X.shape)}")
        return
    if np.ndim(X) != 2 or (d is not None and np.shape(X)[1] != d):
        raise ValueError(f"X must be (m, {d}) like the training rows, got shape {np.shape(X)}")


def scale_queries(dm: dict, X, scaled: bool = True):
    """(Xq, nq): the query rows on the model's device (uint8 rows cross as bytes), scaled with the model's
    bounds -- or as they are with ``scaled=False`` -- and their squared norms."""
    from ..ops import device as D

    Xq = D.upload_rows(np.ascontiguousarray(X, dtype=np.uint8 if _is_u8(X) else np.float64), dm["device"])
    if scaled:
        return Xq, D.minmax_scale_(Xq, dm["d"], dm["mn"], dm["mx"])[2]
    return Xq, D.row_norms(Xq, dm["d"])


def sparse_queries(dm: dict, X, scaled: bool = True):
    """The CSR query rows on the model's device (a ``DeviceCSR``), scaled by the model's column maxima, with their
    norms.  Zeros stay zeros only under bounds whose minimum is 0 -- those of a fit on sparse rows, or of dense
    rows with such columns; any other model raises (densify the queries)."""
    from ..ops import device as D

    if scaled and bool((dm["mn"] != 0).any().item()):
        raise ValueError("sparse queries need a model whose scaling keeps zeros zero (every column minimum 0); "
                         "pass the dense array (X.toarray()) instead")
    Q = D.upload_csr(X, dm["device"])
    D.csr_prepare(Q, mx=dm["mx"].contiguous() if scaled else None, scale=scaled)
    return Q


def scaled_cpu(X: np.ndarray, scale: bool = True):
    """The CPU backends' prologue: (min-max scaled rows, their scaler), or (X, None) with ``scale=False``;
    ValueError on NaN / inf either way."""
    if scale:
        sc = MinMaxScaler().fit(X)
        check_finite_bounds(sc.min_, sc.max_)
        return sc.transform(X), sc
    if not np.all(np.isfinite(X)):
        raise ValueError("X holds NaN or infinite values")
    return X, None


ROW_DTYPES = ("float64", "float32", "float16")


def check_row_dtype(row_dtype: str) -> str:
    if row_dtype not in ROW_DTYPES:
        raise ValueError(f"row_dtype must be 'float64' (the default), 'float32' or 'float16', got {row_dtype!r}")
    return row_dtype


def check_f32_rows(row_dtype: str = "float32", **off) -> None:
    """What ``row_dtype="float32"`` (or ``"float16"``) does not cover raises here, before any device work: ``off`` maps each
    unsupported option's description to whether it was asked for.  The solver's own limits are the native table's
    (``fused_rows_check`` in decomp.hip, shared with sparse rows); these are the estimator-level options that would
    route a fit elsewhere."""
    for name, on in off.items():
        if on:
            raise ValueError(f"row_dtype='{row_dtype}' is not supported with {name} ({row_dtype} rows run on the RBF "
                             "decomposition solver from a cold start, min-max scaled)")


def newton_polish_on() -> bool:
    """Whether SVM355_DECOMP_NEWTON asks for the Newton polish, read as the native knob reads it (C's atoi != 0)."""
    m = re.match(r"\s*[+-]?\d+", os.environ.get("SVM355_DECOMP_NEWTON", ""))
    return bool(m) and int(m.group()) != 0


def scaled_cpu_f32(X: np.ndarray):
    """``row_dtype="float32"`` on the CPU, the host twin of the device's float32 rows: X rounded to float32, min / max
    of those values, ``float32((float64(x) - mn) / range)`` (the scaler's FP64 arithmetic, one rounding), widened.
    Returns (rows, scaler) as ``scaled_cpu``."""
    Xs, sc = scaled_cpu(np.ascontiguousarray(X, dtype=np.float32).astype(np.float64), True)
    return Xs.astype(np.float32).astype(np.float64), sc


def scaled_cpu_f16(X: np.ndarray):
    """``row_dtype="float16"`` on the CPU, the host twin of the device's float16 rows: a float16 array as it is, any
    other rounded to float32; min / max of those values; ``float16(float32((float64(x) - mn) / range))`` -- the scaler's
    FP64 arithmetic, then the two roundings (subnormal halves kept) -- widened.  Returns (rows, scaler)."""
    X = X if X.dtype == np.float16 else np.ascontiguousarray(X, dtype=np.float32)
    Xs, sc = scaled_cpu(np.ascontiguousarray(X, dtype=np.float64), True)
    return Xs.astype(np.float32).astype(np.float16).astype(np.float64), sc


def platt_probability(z: np.ndarray) -> np.ndarray:
    """Platt's sigmoid of z = A f + B in its overflow-safe form, on the host: P(y = -1) and P(y = +1) =
    1 / (1 + exp(z)) stacked on a new last axis.  The one expression of ``SVC`` and ``OneVsOneSVC`` (numpy's
    exp, which is not libm's): for k = 2 they agree bit for bit."""
    e = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.stack([np.where(z >= 0, big, small), np.where(z >= 0, small, big)], -1)


def check_dot_kernel(params, **off) -> None:
    """What a dot-product kernel (linear, poly, sigmoid) does not cover raises here, before any device work: ``off``
    maps each unsupported option's description to whether it was asked for.  The distance kernels (laplacian, chi2)
    cover the same and refuse the same."""
    if params.gram_kernel:
        for name, on in off.items():
            if on:
                raise ValueError(f"kernel={params.kernel!r} is not supported with {name.replace('_', ' ')} (the RBF only)")


def check_chi2_rows(params, Xs: np.ndarray, what: str = "training rows") -> None:
    """The chi2 kernel's domain: rows >= 0 after scaling (min-max scaled training rows are by construction; unscaled
    rows and queries outside the training range need not be).  ValueError naming the first negative column."""
    if params.kernel == "chi2" and Xs.size and Xs.min() < 0:
        j = int(np.flatnonzero((Xs < 0).any(0))[0])
        raise ValueError(f"kernel='chi2' needs non-negative values: column {j} of the {what} holds {Xs[:, j].min()!r}"
                         + (" after scaling" if what == "queries" else ""))


def check_sample_weight(w, n: int, class_box: np.ndarray, eps: float, y=None, **off) -> np.ndarray:
    """``fit(..., sample_weight=w)`` checked before any device work; returns w as n contiguous float64.  ``off`` maps
    each option a weighted fit does not cover to whether it was asked for.  w: shape (n,), finite, >= 0; with labels
    y at least one positive weight in each class; every positive weight's box ``class_box_i * w_i`` above 2 eps, so a
    point is either frozen at 0 (weight 0) or can be at both bounds (below box - eps, above eps)."""
    for name, on in off.items():
        if on:
            raise ValueError(f"sample_weight is not supported with {name} (sample weights run on the CPU oracles and "
                             "on the one-GPU RBF decomposition solver from a cold start, on dense float64 or uint8 "
                             "rows)")
    w = np.asarray(w)
    if w.shape != (n,):
        raise ValueError(f"sample_weight must have shape ({n},), got {w.shape}")
    w = np.ascontiguousarray(w, dtype=np.float64)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("sample_weight must be finite and >= 0")
    if y is not None and not (np.any(w[y == 1] > 0) and np.any(w[y == -1] > 0)):
        raise ValueError("sample_weight leaves a class without a point of positive weight")
    box = class_box * w
    small = (w > 0) & ~(box > 2 * eps)
    if np.any(small):
        i = int(np.flatnonzero(small)[0])
        raise ValueError(f"sample_weight[{i}] = {w[i]!r} gives a box of {box[i]!r}, not above 2 eps = {2 * eps!r}: use "
                         "0 to leave the row out")
    return w


def host_kernel_decision(est, Xq: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """sum_k coef_k kfun(x_k . q) - b on the host for a dot-product or distance kernel model, summed in
    support-vector order."""
    from ..ops import cpu as C

    if est.params.precomputed:  # Xq is the query Gram: its support columns
        from ._precomputed import _host_f64

        return _host_f64(Xq, "a precomputed kernel's queries")[:, est.support_] @ coef - est.b_
    check_chi2_rows(est.params, Xq, "queries")
    return C.kernel_gram(Xq, est.support_vectors_, est.params) @ coef - est.b_


class KernelEstimator:
    """What ``SVC``, ``SVR`` and ``OneClassSVM`` share: ``scale``, ``scaler_``, the device model ``_dev`` and the
    lazily fetched host copy of the support vectors."""

    scaler_ = None
    row_dtype = "float64"  # SVC / SVR take "float32" (rows_f32.hip) and "float16" (rows_f16.hip); the others keep the default
    _dev = None  # device-side model state (device_model's dict)
    _sv_host = None

    @property
    def support_vectors_(self) -> np.ndarray:
        """Scaled support-vector rows (host copy, fetched lazily from the device model)."""
        if self._sv_host is None and self._dev is not None:
            self._sv_host = self._dev["Xs"][:, : self._dev["d"]].cpu().numpy()
        return self._sv_host

    @support_vectors_.setter
    def support_vectors_(self, value) -> None:
        self._sv_host = value

    def _n_features(self) -> Optional[int]:
        if self.params.precomputed:  # the queries' width: the training points
            return getattr(self, "n_fit_", None)
        if self._dev is not None:
            return int(self._dev["d"])
        if self.scaler_ is not None and self.scaler_.min_ is not None:
            return int(np.size(self.scaler_.min_))
        sv = self.support_vectors_
        return int(sv.shape[1]) if sv is not None and np.ndim(sv) == 2 else None

    def _check_X(self, X) -> None:
        if self.params.precomputed:  # a query Gram (numpy, or a tensor on the model's device)
            from ._precomputed import check_queries

            return check_queries(X, self._n_features(), self._dev is not None)
        check_query_shape(X, self._n_features())

    def _scaled_cpu(self, X: np.ndarray) -> np.ndarray:
        Xs, self.scaler_ = (scaled_cpu_f32(X) if self.row_dtype == "float32" else scaled_cpu_f16(X)
                            if self.row_dtype == "float16" else scaled_cpu(X, self.scale))
        return Xs

    def _adopt_rows(self, rows: TrainRows) -> None:
        """The device model and the scaler of a fit on ``rows`` (support_ and dual_coef_ are set)."""
        self._dev = rows.model(self.support_, self.dual_coef_)
        self.scaler_ = rows.scaler()
        self._sv_host = None  # scaled SV rows stay on the device; copied to the host on first access

    def _upload_model(self, dev: str) -> None:
        if self.params.precomputed:
            from ._precomputed import device_model as gram_model

            self._dev = gram_model(self.support_, self.dual_coef_, self.n_fit_, dev)
            return
        self._dev = device_model_from_host(self.support_vectors_, self.scaler_, self.dual_coef_, dev)

    def _device_model_from_u8(self, X_sv: np.ndarray, dev: str) -> None:
        """The device model of a fit whose rows are uint8 pixels and whose alphas, b and scaler are set."""
        self._dev = device_model_from_u8(X_sv, self.scaler_, self.dual_coef_, dev)
        self._sv_host = None

    def _device_queries(self, X):
        return scale_queries(self._dev, X, self.scale)

    def _linear_w(self):
        """A linear device model's weight vector sum_k coef_k Xs_k (padded, on the device), built once per device
        model by the panel reduce (csr_linear.hip) and kept in it."""
        from ..ops import device as D

        if "w" not in self._dev:
            self._dev["w"] = D.linear_w(self._dev["Xs"], self._dev["coef"])
        return self._dev["w"]

    @property
    def coef_(self) -> np.ndarray:
        """The linear kernel's weight vector in scaled-feature space, shape (d,): ``dual_coef_ @ support_vectors_``
        (the decision function is ``x_scaled @ coef_ - b_``).  AttributeError for any other kernel."""
        if self.params.kernel != "linear":
            raise AttributeError("coef_ is only available when using a linear kernel")
        if self._dev is not None:
            return self._linear_w()[: self._dev["d"]].cpu().numpy()
        return np.asarray(self.dual_coef_, dtype=np.float64) @ self.support_vectors_

    def _device_decide(self, X):
        """sum_k coef_k K(x_k, x) - b_ on the device model, as a device tensor: dense queries on the MFMA cross
        kernel, CSR queries on the CSR x panel kernel against the same dense support vectors."""
        from ..ops import device as D

        dv = self._dev
        if self.params.precomputed:  # X is the query Gram: its support columns gathered (decomp_gram.hip)
            from ._precomputed import decide_device

            return decide_device(self, X)
        if self.params.dist_kernel:  # the fused distance block and sum (decomp_dist.hip)
            if is_sparse(X):
                raise ValueError(f"sparse queries are not supported with kernel={self.params.kernel!r} (densify them)")
            Xq = self._device_queries(X)[0]
            # chi2's domain by one min over the scaled queries (padding is 0, so a negative min is a feature's); the
            # error path alone looks for the column, and words it as the host's check_chi2_rows does
            if self.params.kernel == "chi2" and Xq.numel() and float(Xq.min()) < 0:
                check_chi2_rows(self.params, Xq[:, : dv["d"]].cpu().numpy(), "queries")
            return D.decision_dist(dv["Xs"], dv["coef"], Xq, self.params, self.b_)
        if self.params.dot_kernel:  # the model's kernel: the fused dot-product block and sum
            if is_sparse(X) and self.params.kernel == "linear":  # one sparse dot product per row with w
                return D.decision_csr_linear(self._linear_w(), sparse_queries(dv, X, self.scale), self.b_)
            if is_sparse(X):
                raise ValueError(f"sparse queries are not supported with kernel={self.params.kernel!r} (densify them)")
            return D.decision_kfun(dv["Xs"], dv["coef"], self._device_queries(X)[0], self.params, self.b_)
        if is_sparse(X):
            return D.decision_csr(dv["Xs"], dv["ns"], dv["coef"], sparse_queries(dv, X, self.scale),
                                  self.params.gamma, self.b_)
        Xq, nq = self._device_queries(X)
        return D.decision(dv["Xs"], dv["ns"], dv["coef"], Xq, nq, self.params.gamma, self.b_)
