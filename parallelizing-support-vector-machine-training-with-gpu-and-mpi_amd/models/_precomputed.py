"""``kernel="precomputed"`` for ``SVC`` and ``SVR`` (scikit-learn's convention, LIBSVM's ``-t 4``): ``fit`` takes the
(n, n) training Gram, the query methods take (m, n) -- the kernel of each query against all n training points.

The Gram is a float64 numpy array, or a float64 tensor already on the fit's device.  It must be finite and symmetric
to the bit: the GPU solver reads row j of K where the mathematics says column j (decomp_gram.hip) and the CPU oracles
read the same matrix in their own pattern, so exact symmetry is the one rule with no tolerance to choose.  Nothing is
scaled (``scale`` is not read, ``scaler_`` is None), ``gamma`` / ``degree`` / ``coef0`` are not read, and the model is
``support_``, ``dual_coef_``, ``b_`` and ``n_fit_``; ``support_vectors_`` is an empty (0, 0) array."""
from __future__ import annotations

import numpy as np

from ..utils.sparse import is_sparse
from ._device import check_dot_kernel, check_f32_rows, check_sample_weight


def _is_tensor(K) -> bool:
    return hasattr(K, "data_ptr")


def check_options(est, K, sample_weight=None, **off) -> None:
    """What a precomputed kernel does not cover raises here, before any device work: sparse input, sample weights,
    narrow rows, and ``off`` (each unsupported option's description mapped to whether it was asked for)."""
    if is_sparse(K):
        raise ValueError("kernel='precomputed' is not supported with sparse (CSR) input: the Gram is a dense array")
    if sample_weight is not None:
        check_sample_weight(sample_weight, 0, None, 0.0, **{"kernel='precomputed'": True})
    if est.row_dtype != "float64":
        check_f32_rows(est.row_dtype, **{"kernel='precomputed'": True})
    check_dot_kernel(est.params, **off)


def _host_f64(K, what: str) -> np.ndarray:
    """A host Gram as a contiguous float64 array; any other dtype is a ValueError (no silent cast: an integer or
    float32 Gram is the caller's to convert, knowingly)."""
    K = np.asarray(K)
    if K.dtype != np.float64:
        raise ValueError(f"{what} must be a float64 array (or a float64 tensor on the GPU), got dtype {K.dtype}")
    return np.ascontiguousarray(K)


def as_gram(K, n: int, dev: str):
    """The training Gram checked for its form: (n, n) for the n labels or targets; a float64 numpy array (made
    contiguous) or, on a GPU fit, a float64 tensor."""
    if _is_tensor(K):
        if dev == "cpu":
            raise ValueError("a tensor Gram needs a GPU fit (device='cuda'); pass a numpy array to the CPU oracles")
    else:
        K = _host_f64(K, "a precomputed kernel")
    if len(K.shape) != 2 or K.shape[0] != K.shape[1] or K.shape[0] != n:
        raise ValueError(f"a precomputed kernel must be square, (n, n) for the n = {n} labels or targets, got shape "
                         f"{tuple(K.shape)}")
    return K


def raise_bad_entry(K, index: int) -> None:
    """The ValueError for the first offending entry (row-major ``index``) of a Gram that is not finite or not
    symmetric to the bit."""
    i, j = divmod(int(index), K.shape[0])
    a, b = float(K[i, j]), float(K[j, i])
    if not np.isfinite(a):
        raise ValueError(f"the precomputed kernel holds NaN or infinite values: K[{i}, {j}] = {a!r}")
    raise ValueError(f"the precomputed kernel is not symmetric to the bit: K[{i}, {j}] = {a!r} but K[{j}, {i}] = {b!r}; "
                     "symmetrise it with (K + K.T) / 2, which is symmetric to the bit")


def check_host(K: np.ndarray) -> None:
    """Finite and symmetric to the bit, on the host (the CPU fits): the device check's rule and first index."""
    bits = K.view(np.int64)
    bad = np.flatnonzero(~np.isfinite(K).ravel() | (bits != bits.T).ravel())
    if bad.size:
        raise_bad_entry(K, bad[0])


def device_model(support: np.ndarray, coef: np.ndarray, n_fit: int, device) -> dict:
    """The device model of a fit on a Gram: the support columns' ids (int32, ascending) and their coefficients."""
    import torch

    device = torch.device(device)
    return {"gram": True, "sv": torch.from_numpy(np.ascontiguousarray(support, dtype=np.int32)).to(device),
            "coef": torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).to(device), "d": int(n_fit),
            "device": device}


def fit_device(est, K, dev: str, alpha_len: int, **target):
    """The GPU fit: the Gram on the device (uploaded once, or the caller's tensor in place), the symmetry check, the
    decomposition solver.  ``target``: ``y=`` int32 labels or ``z=`` float64 targets and ``epsilon=``, host arrays.
    Returns (alpha on the host, result, timings)."""
    import time

    import torch

    from ..ops import device as D

    device = torch.device(dev)
    t0 = time.perf_counter()
    Kd = D.device_gram(K, device)
    bad = D.gram_check(Kd)
    if bad >= 0:
        raise_bad_entry(Kd, bad)
    upload_ms = (time.perf_counter() - t0) * 1e3
    alpha = torch.empty(alpha_len, dtype=torch.float64, device=device)  # the cold start zeroes it
    kw = {k: (torch.from_numpy(v).to(device) if isinstance(v, np.ndarray) else v) for k, v in target.items()}
    res, tm = D.train_decomp_gram(Kd, alpha, est.params, working_set=est.working_set, **kw)
    return alpha.cpu().numpy(), res, {"upload_preprocess_ms": upload_ms, **tm}


def adopt(est, n_fit: int, dev: str) -> None:
    """The model of a fit on a Gram (support_ and dual_coef_ are set): no scaler, no support-vector rows."""
    est.n_fit_ = int(n_fit)
    est.scaler_ = None
    est.support_vectors_ = np.empty((0, 0))
    est._dev = None if dev == "cpu" else device_model(est.support_, est.dual_coef_, n_fit, dev)


def check_queries(Kq, n_fit, on_device: bool) -> None:
    """The query Gram's form: (m, n_fit), dense; a tensor only for a model on the GPU."""
    shape = tuple(Kq.shape) if hasattr(Kq, "shape") else np.shape(Kq)
    if is_sparse(Kq) or len(shape) != 2 or shape[1] != n_fit:
        raise ValueError(f"X must be (m, {n_fit}) like the training rows, got shape {shape}: a precomputed kernel's "
                         "queries are the kernel of each query against all training points")
    if _is_tensor(Kq) and not on_device:
        raise ValueError("a tensor query Gram needs a model on the GPU; pass a numpy array to a CPU model")


def decide_device(est, Kq):
    """Decision values of a device model as a device tensor: the support columns of Kq gathered on the GPU."""
    from ..ops import device as D

    if not _is_tensor(Kq):
        Kq = _host_f64(Kq, "a precomputed kernel's queries")
    return D.decision_gram(Kq, est._dev["sv"], est._dev["coef"], est.b_)
