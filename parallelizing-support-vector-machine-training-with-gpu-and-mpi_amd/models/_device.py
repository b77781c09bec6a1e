"""The estimators' plumbing between host rows and the native solvers: training rows on the device
(``TrainRows``), the byte-rows-then-FP64-rows attempt (``solve_on_rows``), the device model dict
(``device_model*``), the query prologue (``scale_queries``) and the members ``SVC``, ``SVR`` and
``OneClassSVM`` share (``KernelEstimator``).  ``OneVsRestSVC`` and ``OneVsOneSVC`` use the functions."""
from __future__ import annotations

import time
from typing import Optional

import numpy as np

from ..utils.data import MinMaxScaler, check_finite_bounds


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

    @classmethod
    def upload(cls, X: np.ndarray, device, scale: bool = True, widen: bool = False) -> "TrainRows":
        """uint8 host rows stay bytes on the device (min / max from the bytes; no PyTorch kernel runs: a
        process's first one loads PyTorch's code objects, ~95 ms of a cold first fit,
        profiles/r3_cold_fit_probe.txt), unless ``widen``: then they cross PCIe as bytes and are widened there
        into the FP64 rows that float64 host rows become.  ``scale=False`` (FP64 rows only): unscaled rows and
        their norms, through which a NaN / inf anywhere shows."""
        import torch

        from ..ops import device as D

        t0 = time.perf_counter()
        d = X.shape[1]
        mn = mx = mn_h = mx_h = sqn = None
        if _is_u8(X) and not widen:
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
        return self.take(idx), self.sqn[idx].contiguous()

    def model(self, support, coef, **extra) -> dict:
        """The device model of the fit on these rows: support vectors ``support`` with coefficients ``coef``."""
        return device_model(self.sv(support), coef, self.mn, self.mx, self.d, self.device, **extra)

    def scaler(self) -> Optional[MinMaxScaler]:
        return MinMaxScaler(self.mn_h, self.mx_h) if self.mn_h is not None else None


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


def platt_probability(z: np.ndarray) -> np.ndarray:
    """Platt's sigmoid of z = A f + B in its overflow-safe form, on the host: P(y = -1) and P(y = +1) =
    1 / (1 + exp(z)) stacked on a new last axis.  The one expression of ``SVC`` and ``OneVsOneSVC`` (numpy's
    exp, which is not libm's): for k = 2 they agree bit for bit."""
    e = np.exp(-np.abs(z))
    big, small = 1.0 / (1.0 + e), e / (1.0 + e)
    return np.stack([np.where(z >= 0, big, small), np.where(z >= 0, small, big)], -1)


class KernelEstimator:
    """What ``SVC``, ``SVR`` and ``OneClassSVM`` share: ``scale``, ``scaler_``, the device model ``_dev`` and the
    lazily fetched host copy of the support vectors."""

    scaler_ = None
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
        if self._dev is not None:
            return int(self._dev["d"])
        if self.scaler_ is not None and self.scaler_.min_ is not None:
            return int(np.size(self.scaler_.min_))
        sv = self.support_vectors_
        return int(sv.shape[1]) if sv is not None and np.ndim(sv) == 2 else None

    def _check_X(self, X) -> None:
        check_query_shape(X, self._n_features())

    def _scaled_cpu(self, X: np.ndarray) -> np.ndarray:
        Xs, self.scaler_ = scaled_cpu(X, self.scale)
        return Xs

    def _adopt_rows(self, rows: TrainRows) -> None:
        """The device model and the scaler of a fit on ``rows`` (support_ and dual_coef_ are set)."""
        self._dev = rows.model(self.support_, self.dual_coef_)
        self.scaler_ = rows.scaler()
        self._sv_host = None  # scaled SV rows stay on the device; copied to the host on first access

    def _upload_model(self, dev: str) -> None:
        self._dev = device_model_from_host(self.support_vectors_, self.scaler_, self.dual_coef_, dev)

    def _device_model_from_u8(self, X_sv: np.ndarray, dev: str) -> None:
        """The device model of a fit whose rows are uint8 pixels and whose alphas, b and scaler are set."""
        self._dev = device_model_from_u8(X_sv, self.scaler_, self.dual_coef_, dev)
        self._sv_host = None

    def _device_queries(self, X):
        return scale_queries(self._dev, X, self.scale)
