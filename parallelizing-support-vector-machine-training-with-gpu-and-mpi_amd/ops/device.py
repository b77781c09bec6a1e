"""Device ops on PyTorch-ROCm tensors backed by the hand-written gfx950 kernels (libsvm355_hip.so).

Every op enqueues on the tensor's device behind PyTorch's current stream (the device context is
re-bound to ``torch.cuda.current_stream()`` on every call), so these compose with ordinary torch
code.  Feature matrices are ``(n, ld)`` float64 with ``ld = padded_dim(d)`` (multiple of 16,
zero-padded).  A missing or unloadable device library raises :class:`svm355._native.NativeError`:
there is no eager/torch fallback for any of these kernels.

Reference kernels these replace (/root/reference/code/gpu_svm_main3.cu): find_min_max :62-95,
scale_features :100-116, calc_kernel_matrix :137-147, init/WSS/update kernels :152-272,
predict + reduce_sum :277-315.
"""
from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from .. import _native as N
from ..utils.config import SVMParams


@dataclass
class SMOResult:
    iterations: int
    b: float
    b_high: float
    b_low: float
    stop_reason: str
    n_sv: int
    seconds: float

    @classmethod
    def from_struct(cls, r: N.SvmResult) -> "SMOResult":
        return cls(int(r.iterations), float(r.b), float(r.b_high), float(r.b_low),
                   N.STOP_NAMES.get(int(r.stop_reason), str(r.stop_reason)), int(r.n_sv), float(r.seconds))


@dataclass
class PlattResult:
    A: float
    B: float
    iterations: int
    status: str  # "converged", "max_iter", "line_search_failed" or "degenerate" (svm355.h)

    @classmethod
    def from_struct(cls, o: N.SvmPlatt) -> "PlattResult":
        return cls(float(o.A), float(o.B), int(o.iterations), N.PLATT_STATUS.get(int(o.status), str(o.status)))


class DeviceContext:
    """One native device context (private HIP stream + workspace) per GPU per host thread
    (thread-ranks sharing a GPU must not share a workspace).  Contexts live in thread-local storage:
    when a worker thread ends, its contexts (and their library-owned Gram) are destroyed with it."""

    _tls = threading.local()

    def __init__(self, index: int):
        self.index = index
        self.lib = N.hip()
        with torch.cuda.device(index):
            self.handle = self.lib.svmd_create(index)
        if not self.handle:
            raise N.NativeError(f"svmd_create({index}) failed: {N.last_error()}")

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            try:
                self.lib.svmd_destroy(h)
            except Exception:  # interpreter shutdown
                pass

    @classmethod
    def get(cls, device) -> "DeviceContext":
        index = torch.device(device).index
        if index is None:
            index = torch.cuda.current_device()
        ctxs = getattr(cls._tls, "ctxs", None)
        if ctxs is None:
            ctxs = cls._tls.ctxs = {}
        ctx = ctxs.get(index)
        if ctx is None:
            ctx = ctxs[index] = DeviceContext(index)
        return ctx

    def bind(self) -> int:
        stream = torch.cuda.current_stream(self.index)
        N.check(self.lib.svmd_set_stream(self.handle, stream.cuda_stream), "svmd_set_stream")
        return self.handle


def _ctx_for(t: torch.Tensor) -> DeviceContext:
    if not t.is_cuda:
        raise ValueError("device op needs a GPU tensor")
    return DeviceContext.get(t.device)


def _check_rows(X: torch.Tensor, name: str = "X") -> None:
    if X.dtype != torch.float64 or X.dim() != 2 or not X.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 2-D float64 tensor, got {X.dtype} {tuple(X.shape)}")
    if X.shape[1] % 16:
        raise ValueError(f"{name} row length must be a multiple of 16 (use padded_dim), got {X.shape[1]}")


def padded_dim(d: int) -> int:
    return (int(d) + 15) // 16 * 16


def available() -> bool:
    """True if a GPU is visible and the device library loads."""
    if not torch.cuda.is_available():
        return False
    N.hip()
    return True


def device_empty(shape, dtype, device) -> torch.Tensor:
    """``torch.empty`` for the library's large device buffers.  On an out-of-memory error the memory the
    library itself holds outside PyTorch's allocator -- the Gram and the row-cache / column-cache slab
    its contexts keep between fits, the grow-only Gram buffers (``release_gram_buffers``), and the
    one-vs-rest pool threads' column-cache slabs (``models.multiclass.release_solver_caches``) -- is handed
    back and the allocation retried once: a cache kept for speed never makes a later allocation fail
    (ADVICE r4, r5).""" 
    try:
        return torch.empty(shape, dtype=dtype, device=device)
    except torch.OutOfMemoryError:
        release_gram_buffers()
        # and the one-vs-rest pool threads' column-cache slabs (their contexts are not this thread's)
        from ..models.multiclass import release_solver_caches

        release_solver_caches(timeout_s=1.0)
        torch.cuda.empty_cache()
        return torch.empty(shape, dtype=dtype, device=device)


def upload_rows(X: np.ndarray, device, ld: Optional[int] = None) -> torch.Tensor:
    """Host (n, d) rows -> device (n, ld) zero-padded FP64 rows.

    float rows go over PCIe as FP64 (hipMemcpy2DAsync).  uint8 rows (pixel data, see
    ``utils.data.compact_pixels``) go over as bytes, 8x less H2D traffic, and are widened to FP64 on
    the device (every value is exact), so everything downstream is identical."""
    if isinstance(X, np.ndarray) and X.dtype == np.uint8:
        X = np.ascontiguousarray(X)
        n, d = X.shape
        ld = padded_dim(d) if ld is None else ld
        out = device_empty((n, ld), torch.float64, device)
        ctx = DeviceContext.get(out.device)
        N.check(ctx.lib.svmd_upload_rows_u8(ctx.bind(), N.ptr(X), n, d, N.ptr(out), ld), "svmd_upload_rows_u8")
        return out
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, d = X.shape
    ld = padded_dim(d) if ld is None else ld
    out = device_empty((n, ld), torch.float64, device)
    ctx = DeviceContext.get(out.device)
    N.check(ctx.lib.svmd_upload_rows(ctx.bind(), N.ptr(X), n, d, N.ptr(out), ld), "svmd_upload_rows")
    return out


def minmax(X: torch.Tensor, d: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Column min/max of the first d columns (one streaming pass, per-block partials)."""
    _check_rows(X)
    ctx = _ctx_for(X)
    mn = torch.empty(d, dtype=torch.float64, device=X.device)
    mx = torch.empty(d, dtype=torch.float64, device=X.device)
    N.check(ctx.lib.svmd_minmax(ctx.bind(), N.ptr(X), X.shape[0], d, X.shape[1], N.ptr(mn), N.ptr(mx)),
            "svmd_minmax")
    return mn, mx


def minmax_scale_(X: torch.Tensor, d: int, mn: Optional[torch.Tensor] = None,
                  mx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """In-place min-max scaling of the first d columns; returns (min, max, squared row norms).

    With mn/mx given they are used as-is (test data scaled with training statistics)."""
    _check_rows(X)
    ctx = _ctx_for(X)
    n = X.shape[0]
    use_given = mn is not None
    if not use_given:  # one buffer: the caller reads both bounds back with one copy (torch.cat-free)
        mm = torch.empty(2 * d, dtype=torch.float64, device=X.device)
        mn, mx = mm[:d], mm[d:]
    sqn = torch.empty(n, dtype=torch.float64, device=X.device)
    N.check(ctx.lib.svmd_preprocess(ctx.bind(), N.ptr(X), n, d, X.shape[1], N.ptr(mn), N.ptr(mx), N.ptr(sqn),
                                    int(use_given)), "svmd_preprocess")
    return mn, mx, sqn


def row_norms(X: torch.Tensor, d: Optional[int] = None) -> torch.Tensor:
    _check_rows(X)
    ctx = _ctx_for(X)
    d = X.shape[1] if d is None else d
    out = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
    N.check(ctx.lib.svmd_row_norms(ctx.bind(), N.ptr(X), X.shape[0], d, X.shape[1], N.ptr(out)), "svmd_row_norms")
    return out


def rbf_gram(A: torch.Tensor, nA: torch.Tensor, B: torch.Tensor, nB: torch.Tensor, gamma: float,
             symmetric: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K[i, j] = exp(-gamma ||A_i - B_j||^2) on MFMA f64 tiles (diagonal forced to 1 if symmetric)."""
    _check_rows(A, "A")
    _check_rows(B, "B")
    if A.shape[1] != B.shape[1]:
        raise ValueError("A and B row lengths differ")
    m, n = A.shape[0], B.shape[0]
    if out is None:
        ldk = (n + 1) // 2 * 2
        out = torch.empty((m, ldk), dtype=torch.float64, device=A.device)
    ctx = _ctx_for(A)
    N.check(ctx.lib.svmd_rbf_gram(ctx.bind(), N.ptr(A), N.ptr(nA), m, A.shape[1], N.ptr(B), N.ptr(nB), n,
                                  B.shape[1], A.shape[1], float(gamma), N.ptr(out), out.stride(0), int(symmetric)),
            "svmd_rbf_gram")
    return out


def smo(K: torch.Tensor, y: torch.Tensor, alpha: torch.Tensor, params: SVMParams, warm: bool = False,
        n: Optional[int] = None, trace_cap: int = 0) -> Tuple[SMOResult, Optional[np.ndarray]]:
    """Device-resident SMO on a kernel matrix; alpha is updated in place."""
    n = K.shape[0] if n is None else n
    if y.dtype != torch.int32 or alpha.dtype != torch.float64:
        raise ValueError("y must be int32 (+-1) and alpha float64")
    ctx = _ctx_for(K)
    r = N.SvmResult()
    trace = np.zeros((max(trace_cap, 0), 2), dtype=np.int64) if trace_cap > 0 else None
    p = params.to_struct()
    N.check(ctx.lib.svmd_smo(ctx.bind(), N.ptr(K), K.stride(0), N.ptr(y), n, N.ptr(alpha), int(warm),
                             ctypes.byref(p), ctypes.byref(r), N.ptr(trace) if trace is not None else None,
                             trace_cap), "svmd_smo")
    res = SMOResult.from_struct(r)
    if trace is not None:
        trace = trace[: max(0, min(trace_cap, res.iterations - 1))]
    return res, trace


def smo_multi(K: torch.Tensor, Y: torch.Tensor, A: torch.Tensor, params: SVMParams,
              n: Optional[int] = None) -> Tuple[List[SMOResult], bool]:
    """``nclass`` cold-start SMO solves on one resident Gram (one-vs-rest): Y (nclass, n) int32 +-1,
    A (nclass, n) float64 receives the alphas.  The classes run concurrently, one XCD-local team per
    XCD (smo.hip, smo_multi_kernel); each result equals the single solve's bit for bit.
    Returns (results, batched) — batched False when the solves ran one by one."""
    n = K.shape[0] if n is None else n
    if Y.dtype != torch.int32 or A.dtype != torch.float64 or Y.shape != A.shape or Y.shape[1] != n:
        raise ValueError("Y must be (nclass, n) int32 and A (nclass, n) float64")
    if not (Y.is_contiguous() and A.is_contiguous()):
        raise ValueError("Y and A must be contiguous (class-major)")
    nclass = Y.shape[0]
    ctx = _ctx_for(K)
    rs = (N.SvmResult * nclass)()
    batched = ctypes.c_int32(0)
    p = params.to_struct()
    N.check(ctx.lib.svmd_smo_multi(ctx.bind(), N.ptr(K), K.stride(0), N.ptr(Y), n, nclass, N.ptr(A),
                                   ctypes.byref(p), rs, ctypes.byref(batched)), "svmd_smo_multi")
    return [SMOResult.from_struct(r) for r in rs], bool(batched.value)


GRAM_MODES = {"auto": 0, "fp64": 1, "int": 2}


def _host_stats(mn, mx):
    if mn is None or mx is None:
        return None, None, 0
    a = np.ascontiguousarray(mn.detach().cpu().numpy() if isinstance(mn, torch.Tensor) else mn, dtype=np.float64)
    b = np.ascontiguousarray(mx.detach().cpu().numpy() if isinstance(mx, torch.Tensor) else mx, dtype=np.float64)
    return a, b, int(a.shape[0])


_GRAM_TLS = threading.local()  # per host thread: {device index: grow-only Gram buffer}


def _gram_bufs() -> dict:
    bufs = getattr(_GRAM_TLS, "bufs", None)
    if bufs is None:
        bufs = _GRAM_TLS.bufs = {}
    return bufs


def gram_buffer(n: int, device) -> torch.Tensor:
    """(n, ldk) float64 scratch Gram for the library's own transient use (SVC fit, one-vs-rest):
    one grow-only buffer per device per host thread, so repeated fits of the same or smaller size
    never go back to the allocator — a fresh multi-GB device allocation can take hundreds of
    milliseconds.  The view is overwritten by the next call on the same thread.  Buffers live in
    thread-local storage (released when the thread ends) and ``release_gram_buffers()`` drops the
    calling thread's."""
    device = torch.device(device)
    ldk = (n + 1) // 2 * 2
    key = device.index if device.index is not None else torch.cuda.current_device()
    bufs = _gram_bufs()
    buf = bufs.get(key)
    if buf is None or buf.numel() < n * ldk:
        bufs.pop(key, None)
        del buf
        buf = bufs[key] = device_empty(n * ldk, torch.float64, device)
    return buf[: n * ldk].view(n, ldk)


def release_gram_buffers() -> None:
    """Drop the calling thread's cached Gram buffers (``gram_buffer``) and the library-owned device
    memory of its contexts (the row-cache slab and Gram the C ABI keeps between fits, which would
    otherwise hold up to 60 % of the HBM and push later fits onto the slower row cache)."""
    _gram_bufs().clear()
    for ctx in list((getattr(DeviceContext._tls, "ctxs", None) or {}).values()):
        if ctx.handle:
            N.check(ctx.lib.svmd_release_cache(ctx.handle), "svmd_release_cache")


def gram_fits(n: int, device, fraction: float = 0.8) -> bool:
    """Does the full n x n float64 Gram fit in `fraction` of the free device memory?  A row-cache slab
    an earlier fit left in this thread's context counts as free: when the Gram fits only with that
    memory the slab is handed back (it is rebuilt on demand), so it cannot push this fit onto the row
    cache; otherwise it is kept for the next row-cache fit."""
    device = torch.device(device)
    need = n * ((n + 1) // 2 * 2) * 8
    free, _ = torch.cuda.mem_get_info(device)
    avail = free + torch.cuda.memory_reserved(device)
    ctx = (getattr(DeviceContext._tls, "ctxs", None) or {}).get(
        device.index if device.index is not None else torch.cuda.current_device())
    if ctx is None or not ctx.handle or need <= fraction * avail:
        return need <= fraction * avail
    slab = ctypes.c_int64(0)
    N.check(ctx.lib.svmd_cache_bytes(ctx.handle, None, ctypes.byref(slab)), "svmd_cache_bytes")
    if slab.value and need <= fraction * (avail + slab.value):
        N.check(ctx.lib.svmd_release_slab(ctx.handle), "svmd_release_slab")
        return True
    return False


def train(X: torch.Tensor, sqn: torch.Tensor, y: torch.Tensor, alpha: torch.Tensor, params: SVMParams,
          warm: bool = False, K: Optional[torch.Tensor] = None, mn=None, mx=None,
          gram: str = "auto", kcache: str = "auto", cache_bytes: int = 0,
          trace_cap: int = 0) -> Tuple[SMOResult, dict]:
    """RBF kernel + SMO.  Returns (result, timing dict in ms).

    ``mn``/``mx`` are the min/max the rows were scaled with; with them the exact-integer Gram
    (int8 MFMA, igram.hip) runs when the rows are integer-valued pixels (``gram="auto"``),
    ``gram="fp64"`` forces the FP64 MFMA Gram, ``gram="int"`` requires the integer path.
    ``kcache="full"`` stores the whole Gram (into K, allocated by torch if None); ``"rows"`` uses
    the on-demand HBM row cache (rowcache.hip) for problems whose Gram does not fit; ``"auto"``
    picks "full" when the Gram fits in 80% of the free memory."""
    _check_rows(X)
    n = X.shape[0]
    if kcache == "auto":
        kcache = "full" if (K is not None or gram_fits(n, X.device)) else "rows"
    ctx = _ctx_for(X)
    r = N.SvmResult()
    p = params.to_struct()
    a, b, d = _host_stats(mn, mx)
    used = ctypes.c_int32(0)
    trace = np.zeros((max(trace_cap, 0), 2), dtype=np.int64) if trace_cap > 0 else None
    if kcache == "rows":
        import time as _t

        # the row cache sizes itself from the free HBM: hand this thread's scratch Gram back first
        if _gram_bufs().pop(X.device.index, None) is not None:
            torch.cuda.empty_cache()

        t0 = _t.perf_counter()
        N.check(ctx.lib.svmd_train_rows(ctx.bind(), N.ptr(X), N.ptr(sqn) if sqn is not None else None, n, X.shape[1],
                                        X.shape[1], N.ptr(y), N.ptr(alpha), int(warm), ctypes.byref(p),
                                        ctypes.byref(r), N.ptr(a), N.ptr(b), GRAM_MODES[gram], int(cache_bytes),
                                        ctypes.byref(used), N.ptr(trace), max(trace_cap, 0)), "svmd_train_rows")
        tms = (_t.perf_counter() - t0) * 1e3
        res = SMOResult.from_struct(r)
        out = {"gram_ms": 0.0, "smo_ms": tms, "total_ms": tms, "kcache": "rows",
               "gram_path": "int8-exact" if used.value else "fp64"}
        if trace is not None:
            out["trace"] = trace[: max(0, min(trace_cap, res.iterations - 1))]
        return res, out
    if trace_cap > 0:
        raise ValueError("trace_cap is supported by the row-cache path only (use smo() on a Gram)")
    import time as _t

    ta = _t.perf_counter()
    if K is None:
        K = gram_buffer(n, X.device)
    alloc_ms = (_t.perf_counter() - ta) * 1e3
    tm = N.SvmdTiming()
    N.check(ctx.lib.svmd_train_q(ctx.bind(), N.ptr(X), N.ptr(sqn) if sqn is not None else None, n, X.shape[1],
                                 X.shape[1], N.ptr(y), N.ptr(alpha), int(warm), ctypes.byref(p), ctypes.byref(r),
                                 N.ptr(K), K.stride(0), ctypes.byref(tm), N.ptr(a), N.ptr(b), d,
                                 GRAM_MODES[gram], ctypes.byref(used)), "svmd_train_q")
    return SMOResult.from_struct(r), {"gram_ms": tm.gram_ms, "smo_ms": tm.smo_ms, "total_ms": tm.total_ms,
                                      "gram_alloc_ms": alloc_ms, "kcache": "full", "gram_path": "int8-exact" if used.value else "fp64"}


# ---- the byte path of SVC.fit for uint8 pixel rows: no FP64 copy of the training rows at all
def upload_u8(X: np.ndarray, device) -> torch.Tensor:
    """Host uint8 pixel rows (n, d) -> the same bytes on the device (n, d) uint8."""
    X = np.ascontiguousarray(X, dtype=np.uint8)
    out = device_empty(X.shape, torch.uint8, device)
    ctx = DeviceContext.get(out.device)
    N.check(ctx.lib.svmd_memcpy_h2d(ctx.bind(), N.ptr(out), N.ptr(X), X.nbytes), "svmd_memcpy_h2d")
    return out


def minmax_u8(Xu: torch.Tensor, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Column min / max (FP64) of device uint8 rows: equal to those of the widened FP64 rows.  With
    ``out`` (2d float64) they are its two halves, so one read-back fetches both."""
    n, d = Xu.shape
    if out is None:
        out = torch.empty(2 * d, dtype=torch.float64, device=Xu.device)
    mn, mx = out[:d], out[d:]
    ctx = _ctx_for(Xu)
    N.check(ctx.lib.svmd_minmax_u8(ctx.bind(), N.ptr(Xu), n, d, N.ptr(mn), N.ptr(mx)), "svmd_minmax_u8")
    return mn, mx


def train_u8(Xu: torch.Tensor, y: torch.Tensor, alpha: torch.Tensor, params: SVMParams, mn: torch.Tensor,
             mx: torch.Tensor, warm: bool = False) -> Optional[Tuple[SMOResult, dict]]:
    """Exact-integer Gram quantised straight from the bytes + SMO (svmd_train_u8): the same Gram,
    trajectory and result as ``train`` on the scaled FP64 rows.  None when the integer plan does not
    apply (the caller takes the FP64-row path)."""
    import time as _t

    n, d = Xu.shape
    ctx = _ctx_for(Xu)
    a, b, _ = _host_stats(mn, mx)  # numpy statistics pass through without a device round trip
    ta = _t.perf_counter()
    K = gram_buffer(n, Xu.device)
    alloc_ms = (_t.perf_counter() - ta) * 1e3
    r, tm, used = N.SvmResult(), N.SvmdTiming(), ctypes.c_int32(0)
    p = params.to_struct()
    N.check(ctx.lib.svmd_train_u8(ctx.bind(), N.ptr(Xu), n, d, N.ptr(a), N.ptr(b), N.ptr(y), N.ptr(alpha), int(warm),
                                  ctypes.byref(p), ctypes.byref(r), N.ptr(K), K.stride(0), ctypes.byref(tm),
                                  ctypes.byref(used)), "svmd_train_u8")
    if not used.value:
        return None
    return SMOResult.from_struct(r), {"gram_ms": tm.gram_ms, "smo_ms": tm.smo_ms, "total_ms": tm.total_ms,
                                      "gram_alloc_ms": alloc_ms, "kcache": "full", "gram_path": "int8-exact",
                                      "rows": "uint8"}


def _decomp_rows(X: torch.Tensor) -> int:
    """The rows of a decomposition solve checked (uint8 pixel rows, or padded FP64 rows); their number."""
    if X.dtype != torch.uint8:
        _check_rows(X)
    return X.shape[0]


def _train_decomp(entry: str, solver: str, X: torch.Tensor, mn, mx, mode_args, params: SVMParams, working_set: int,
                  trace, extra=lambda st: {}, after_ws=()) -> Optional[Tuple[SMOResult, dict]]:
    """The body the ``svmd_train_decomp*`` wrappers share: the rows checked, the host statistics and the out
    structs built, the entry called -- handle, rows and statistics, ``mode_args`` (the entry's own: labels or
    targets, alpha, ...), parameters, working set, ``after_ws``, the out structs, the trace -- and the timing dict
    with the wrapper's ``solver`` name and ``extra(stats)`` keys.  None when nothing ran."""
    n, u8 = _decomp_rows(X), X.dtype == torch.uint8
    ld = X.shape[1]
    ctx = _ctx_for(X)
    a, b, dd = _host_stats(mn, mx)
    d = ld if u8 else dd
    r, tm, used = N.SvmResult(), N.SvmdTiming(), ctypes.c_int32(0)
    st = (ctypes.c_int64 * 16)()
    p = params.to_struct()
    N.check(getattr(ctx.lib, entry)(ctx.bind(), N.ptr(X), int(u8), n, ld, d, N.ptr(a), N.ptr(b), *mode_args,
                                    ctypes.byref(p), int(working_set), *after_ws, ctypes.byref(r), ctypes.byref(tm),
                                    st, ctypes.byref(used),
                                    ctypes.byref(trace.struct) if trace is not None else None), entry)
    if not used.value:
        return None
    return SMOResult.from_struct(r), {"gram_ms": tm.gram_ms, "smo_ms": tm.smo_ms, "total_ms": tm.total_ms,
                                      "kcache": "none", "gram_path": "fp64" if st[6] else "int8-exact",
                                      "rows": "uint8" if u8 else "fp64", "solver": solver,
                                      "outer_iterations": int(st[0]), "inner_iterations": int(st[1]),
                                      "working_set": int(st[2]), "update_columns": int(st[4]),
                                      "inner_threads": int(st[5]), **extra(st)}


def train_decomp(X: torch.Tensor, y: torch.Tensor, alpha: torch.Tensor, params: SVMParams, mn, mx,
                 working_set: int = 1024, warm: bool = False,
                 trace: Optional["N.DecompTrace"] = None) -> Optional[Tuple[SMOResult, dict]]:
    """Working-set decomposition SMO (svmd_train_decomp, decomp.hip): the reference's stop test on all
    n points, reached by SMO on working sets of up to ``working_set`` points; no n x n Gram.  X: device
    uint8 pixel rows (n, d), or min-max scaled FP64 rows (n, ld) with ``d`` columns (the reference's host
    format, d = len(mn); they quantise into the same integers, so trajectory and model are the uint8 path's).
    warm: alpha holds the start (f = K (alpha y) - y over its nonzero entries).  trace: an
    ``N.DecompTrace`` filled per outer iteration (tests).  FP64 rows without an exact-integer plan
    (real-valued data) are solved with FP64-MFMA kernel values (``gram_path`` "fp64"); uint8 rows
    without one return None (the caller widens them)."""
    return _train_decomp("svmd_train_decomp", "decomp", X, mn, mx, (N.ptr(y), N.ptr(alpha)), params, working_set, trace,
                         lambda st: {"warm_start": bool(warm), "warm_columns": int(st[7]), **N.shrink_stats(st)},
                         after_ws=(int(warm),))


def train_decomp_svr(X: torch.Tensor, z: torch.Tensor, alpha: torch.Tensor, params: SVMParams, mn, mx,
                     epsilon: float = 0.1, working_set: int = 1024,
                     trace: Optional["N.DecompTrace"] = None) -> Optional[Tuple[SMOResult, dict]]:
    """epsilon-SVR on the decomposition solver (svmd_train_decomp_svr): twin mode over the n rows of X (device
    uint8 pixel rows (n, d), or min-max scaled FP64 rows (n, ld), as ``train_decomp``) and the n float64 targets
    z on the device.  alpha (2n float64, out): a, then a*; the model is beta = a - a*.  The kernel work of the f
    update runs over the n rows, as a classification of them.  Cold start only; shrinking, the Newton polish and
    class weights raise.  trace: an ``N.DecompTrace`` of 2n-long snapshots (tests).  None when nothing ran
    (uint8 rows without an exact-integer plan; FP64 rows whose workspace does not fit)."""
    n = _decomp_rows(X)
    if z.dtype != torch.float64 or z.shape != (n,) or not z.is_contiguous():
        raise ValueError(f"z must be a contiguous float64 tensor of shape ({n},)")
    if alpha.dtype != torch.float64 or alpha.shape != (2 * n,) or not alpha.is_contiguous():
        raise ValueError(f"alpha must be a contiguous float64 tensor of shape ({2 * n},): a, then a*")
    return _train_decomp("svmd_train_decomp_svr", "decomp-svr", X, mn, mx, (N.ptr(z), float(epsilon), N.ptr(alpha)),
                         params, working_set, trace)


def train_decomp_oneclass(X: torch.Tensor, alpha: torch.Tensor, params: SVMParams, mn, mx, nu: float = 0.5,
                          working_set: int = 1024,
                          trace: Optional["N.DecompTrace"] = None) -> Optional[Tuple[SMOResult, dict]]:
    """One-class SVM on the decomposition solver (svmd_train_decomp_oneclass): the solver's one-class mode over
    the n rows of X (device uint8 pixel rows (n, d), or min-max scaled FP64 rows (n, ld), as ``train_decomp``).
    alpha (n float64, out); the result's b is rho and a decision value is sum_k alpha_k K(x_k, x) - rho.
    params.C is not read (the box is 1).  Shrinking, the Newton polish, class weights and nu outside (0, 1)
    raise.  The timing dict's "start_columns" counts the start's nonzero alphas (one f update per 1,024 of
    them before the first selection).  None when nothing ran (uint8 rows without an exact-integer plan; FP64
    rows whose workspace does not fit)."""
    n = _decomp_rows(X)
    if alpha.dtype != torch.float64 or alpha.shape != (n,) or not alpha.is_contiguous():
        raise ValueError(f"alpha must be a contiguous float64 tensor of shape ({n},)")
    return _train_decomp("svmd_train_decomp_oneclass", "decomp-oneclass", X, mn, mx, (float(nu), N.ptr(alpha)), params,
                         working_set, trace, lambda st: {"start_columns": int(st[7])})


def train_decomp_heldout(X: torch.Tensor, y: torch.Tensor, heldout: torch.Tensor, alpha: torch.Tensor,
                         dec: torch.Tensor, params: SVMParams, mn, mx, working_set: int = 1024,
                         trace: Optional["N.DecompTrace"] = None) -> Optional[Tuple[SMOResult, dict]]:
    """The decomposition solver's held-out mode (svmd_train_decomp_heldout): the ordinary cold-start solve on the
    rows of X (as ``train_decomp``) with the points of ``heldout`` (device uint8 (n,), 1 = held out) taken out of
    the fit: they run with label 0, which no selection takes, so their alpha stays exactly 0 while their f
    collects every update.  alpha (n float64, out); dec (n float64, out): f - b on the held-out points -- their
    decision values under a model that never saw them, from the training's own kernel values -- and 0.0 on the
    others.  Class weights are allowed; shrinking and the Newton polish raise.  The training part must hold both
    classes (check it on the host).  None when nothing ran, as ``train_decomp``."""
    n = _decomp_rows(X)
    for name, t, dt in (("y", y, torch.int32), ("heldout", heldout, torch.uint8), ("alpha", alpha, torch.float64),
                        ("dec", dec, torch.float64)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous() or t.device != X.device:
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({n},) on the rows' device")
    return _train_decomp("svmd_train_decomp_heldout", "decomp-heldout", X, mn, mx,
                         (N.ptr(y), N.ptr(heldout), N.ptr(alpha), N.ptr(dec)), params, working_set, trace)


def platt_fit(dec: torch.Tensor, y: torch.Tensor, use: Optional[torch.Tensor] = None) -> PlattResult:
    """Platt scaling on the device (svmd_platt_fit, platt.hip): P(y = +1 | f) = 1 / (1 + exp(A f + B)) fitted to
    the pairs (dec_i, y_i) by Lin, Lin and Weng's Newton method (LIBSVM's -b 1) in one launch of one workgroup,
    with deterministic sums.  dec (n float64), y (n int32 labels), use: optional (n uint8), nonzero = the pair
    counts.  Synchronises (the result is four numbers on the host)."""
    n = dec.shape[0]
    for name, t, dt in (("dec", dec, torch.float64), ("y", y, torch.int32), ("use", use, torch.uint8)):
        if t is not None and (t.dtype != dt or t.shape != (n,) or not t.is_contiguous() or t.device != dec.device):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({n},) on one device")
    ctx = _ctx_for(dec)
    o = N.SvmPlatt()
    N.check(ctx.lib.svmd_platt_fit(ctx.bind(), N.ptr(dec), N.ptr(y), N.ptr(use), n, ctypes.byref(o)), "svmd_platt_fit")
    return PlattResult.from_struct(o)


def platt_fit_batch(dec: torch.Tensor, y: torch.Tensor, offsets, use: Optional[torch.Tensor] = None
                    ) -> List[PlattResult]:
    """P sigmoid fits in one launch (svmd_platt_fit_batch, platt.hip): segment p of the concatenated dec / y / use
    (as ``platt_fit``) is [offsets[p], offsets[p + 1]); offsets: P + 1 host integers ascending from >= 0 to at
    most len(dec), no empty segment.  One workgroup per segment and one copy back; result p is ``platt_fit`` on
    that segment alone, bit for bit.  Synchronises."""
    n = dec.shape[0]
    for name, t, dt in (("dec", dec, torch.float64), ("y", y, torch.int32), ("use", use, torch.uint8)):
        if t is not None and (t.dtype != dt or t.shape != (n,) or not t.is_contiguous() or t.device != dec.device):
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({n},) on one device")
    off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 2:
        raise ValueError("offsets must hold P + 1 >= 2 segment bounds")
    if off[0] < 0 or off[-1] > n or np.any(np.diff(off) < 1):
        raise ValueError(f"offsets must ascend strictly from >= 0 to at most {n} (no empty segment), got {off.tolist()}")
    P = off.shape[0] - 1
    ctx = _ctx_for(dec)
    out = (N.SvmPlatt * P)()
    N.check(ctx.lib.svmd_platt_fit_batch(ctx.bind(), N.ptr(dec), N.ptr(y), N.ptr(use), N.ptr(off), P, out),
            "svmd_platt_fit_batch")
    return [PlattResult.from_struct(o) for o in out]


def ovo_couple(dec: torch.Tensor, A: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None,
               want_label: bool = True, proba: Optional[torch.Tensor] = None, label: Optional[torch.Tensor] = None,
               iters: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """Pairwise coupling on the device (svmd_ovo_couple, ovo_proba.hip): class probabilities from the (m, P) pair
    decisions of ``ovo_predict`` / ``ovo_votes`` (a row-strided view of a wider tensor is taken as it is), one
    wave per row.  A, B (P,) float64 on the device: the pairs' sigmoids; both None: ``dec`` holds the pair
    probabilities, and the result is ``ops.cpu.ovo_couple``'s bit for bit.  Returns (proba (m, k), label index
    (m,) int32 or None without ``want_label``, iters (m,) int32: max(100, k) means not converged).  proba / label
    / iters: optional tensors to write into (proba may be a row-strided view with at least k columns)."""
    if dec.dtype != torch.float64 or dec.dim() != 2 or (dec.shape[1] > 1 and dec.stride(1) != 1):
        raise ValueError("dec must be a 2-D float64 tensor with unit column stride")
    m, P = dec.shape
    k = int(round((1.0 + (1.0 + 8.0 * P) ** 0.5) / 2.0))
    if k < 2 or k > 64 or k * (k - 1) // 2 != P:
        raise ValueError(f"{P} pair columns are not k (k - 1) / 2 for a k in 2 .. 64")
    if (A is None) != (B is None):
        raise ValueError("A and B come together")
    for name, t in (("A", A), ("B", B)):
        if t is not None and (t.dtype != torch.float64 or t.shape != (P,) or not t.is_contiguous()
                              or t.device != dec.device):
            raise ValueError(f"{name} must be a contiguous float64 tensor of shape ({P},) on the decisions' device")
    if proba is None:
        proba = torch.empty((m, k), dtype=torch.float64, device=dec.device)
    elif (proba.dtype != torch.float64 or proba.dim() != 2 or proba.shape[0] < m or proba.shape[1] != k
          or proba.stride(1) != 1 or proba.device != dec.device):
        raise ValueError(f"proba must be a float64 (>= {m}, {k}) tensor with unit column stride on the decisions' device")
    if label is None and want_label:
        label = torch.empty(m, dtype=torch.int32, device=dec.device)
    if iters is None:
        iters = torch.empty(m, dtype=torch.int32, device=dec.device)
    for name, t in (("label", label), ("iters", iters)):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < m or not t.is_contiguous()
                              or t.device != dec.device):
            raise ValueError(f"{name} must be a contiguous int32 tensor of at least {m} entries on the decisions' device")
    ldd = dec.stride(0) if m > 1 else max(dec.stride(0), P)
    ldp = proba.stride(0) if proba.shape[0] > 1 else max(proba.stride(0), k)
    if ldd < P or ldp < k:
        raise ValueError("dec / proba rows overlap")
    ctx = _ctx_for(dec)
    N.check(ctx.lib.svmd_ovo_couple(ctx.bind(), N.ptr(dec), ldd, m, k, N.ptr(A), N.ptr(B), N.ptr(proba), ldp,
                                    N.ptr(label), N.ptr(iters)), "svmd_ovo_couple")
    return proba, label, iters


def decomp_twin_step_u8(Xu: torch.Tensor, mn, mx, gamma: float, cols: np.ndarray, coef: np.ndarray,
                        f: np.ndarray) -> Optional[np.ndarray]:
    """The twin mode's fold and f update alone (svmd_decomp_twin_step_u8): the moved list ``cols`` (distinct
    virtual ids in [0, 2n): k is a_k, k + n its twin) with ``coef`` is folded on the device to one entry per
    row, and the returned copy of ``f`` (2n) has every row's sum added to both of its points.  None when no
    exact-integer plan applies."""
    n, d = Xu.shape
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    out = np.array(f, dtype=np.float64, copy=True)
    if out.shape != (2 * n,) or cols.shape != coef.shape:
        raise ValueError(f"f must have shape ({2 * n},) and cols / coef one length")
    a, b, _ = _host_stats(mn, mx)
    used = ctypes.c_int32(0)
    ctx = _ctx_for(Xu)
    N.check(ctx.lib.svmd_decomp_twin_step_u8(ctx.bind(), N.ptr(Xu), n, d, N.ptr(a), N.ptr(b), float(gamma), N.ptr(cols),
                                             N.ptr(coef), int(cols.size), N.ptr(out), ctypes.byref(used)),
            "svmd_decomp_twin_step_u8")
    return out if used.value else None


def decomp_gemv_u8(Xu: torch.Tensor, mn, mx, gamma: float, cols: np.ndarray, coef: np.ndarray, lo: int = 0,
                   nloc: Optional[int] = None) -> Optional[np.ndarray]:
    """The decomposition solver's f-update GEMV alone (svmd_decomp_gemv_u8): sum_k coef[k] K(i, cols[k])
    for rows i in [lo, lo + nloc) of the exact-integer kernel, in the solver's summation order.  None
    when no exact-integer plan applies."""
    n, d = Xu.shape
    nloc = n - lo if nloc is None else int(nloc)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    out = np.empty(nloc, dtype=np.float64)
    a, b, _ = _host_stats(mn, mx)
    used = ctypes.c_int32(0)
    ctx = _ctx_for(Xu)
    N.check(ctx.lib.svmd_decomp_gemv_u8(ctx.bind(), N.ptr(Xu), n, d, N.ptr(a), N.ptr(b), float(gamma), int(lo), nloc,
                                        N.ptr(cols), N.ptr(coef), int(cols.size), N.ptr(out), ctypes.byref(used)),
            "svmd_decomp_gemv_u8")
    return out if used.value else None


def decomp_newton_probe(Kw: np.ndarray, y: np.ndarray, a: np.ndarray, f: np.ndarray, C: float = 10.0,
                        eps: float = 1e-12, max_free: int = 1024, reps: int = 1, device="cuda:0", threads: int = 256):
    """One Newton polish step (decomp_newton.h) on the device for a host working set: returns (alpha, f,
    code, phase stamps (100 MHz ticks: free set, K_FF, factorisation, back substitution, step, f; then
    |F|, 0 when the step was refused), mean ms per step).  max_free is capped at kNewtonMaxFree (512): a
    larger free set takes no step.  threads: the workgroup's size, 64, 128, 256 or 512 (the inner solve's
    shapes); any other value is an argument error."""
    Kw = np.ascontiguousarray(Kw, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.int32)
    a = np.array(a, dtype=np.float64)
    f = np.array(f, dtype=np.float64)
    prof = np.zeros(16, dtype=np.int64)
    code, ms = ctypes.c_int32(0), ctypes.c_double(0.0)
    ctx = _ctx_for(torch.empty(1, device=device))
    N.check(ctx.lib.svmd_decomp_newton_probe_nt(ctx.bind(), N.ptr(Kw), N.ptr(y), len(y), N.ptr(a), N.ptr(f), float(C),
                                                float(eps), int(max_free), int(reps), int(threads), ctypes.byref(code),
                                                N.ptr(prof), ctypes.byref(ms)), "svmd_decomp_newton_probe")
    return a, f, int(code.value), prof, float(ms.value)


def rbf_gram_u8(Xu: torch.Tensor, gamma: float, mn, mx, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """Exact-integer RBF Gram straight from device uint8 rows (equal to ``rbf_gram_sym`` on the scaled
    FP64 rows); None when the integer plan does not apply."""
    n, d = Xu.shape
    if out is None:
        out = device_empty((n, (n + 1) // 2 * 2), torch.float64, Xu.device)
    a, b, _ = _host_stats(mn, mx)
    used = ctypes.c_int32(0)
    ctx = _ctx_for(Xu)
    N.check(ctx.lib.svmd_rbf_gram_u8(ctx.bind(), N.ptr(Xu), n, d, N.ptr(a), N.ptr(b), float(gamma), N.ptr(out),
                                     out.stride(0), ctypes.byref(used)), "svmd_rbf_gram_u8")
    return out if used.value else None


def sv_rows_u8(Xu: torch.Tensor, idx: torch.Tensor, mn: torch.Tensor, mx: torch.Tensor, ld: Optional[int] = None,
               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Scaled FP64 rows idx (zero padded to ld) and their squared norms from device uint8 rows.  ``out``: a
    contiguous (len(idx), ld) float64 tensor to write the rows into (every element of it is written)."""
    d = Xu.shape[1]
    ld = padded_dim(d) if ld is None else ld
    idx = idx.to(torch.int64).contiguous()
    k = idx.numel()
    if out is None:
        out = torch.empty((k, ld), dtype=torch.float64, device=Xu.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (k, ld) or not out.is_contiguous() or out.device != Xu.device:
        raise ValueError(f"out must be a contiguous float64 tensor of shape ({k}, {ld}) on {Xu.device}")
    sqn = torch.empty(k, dtype=torch.float64, device=Xu.device)
    ctx = _ctx_for(Xu)
    N.check(ctx.lib.svmd_sv_rows_u8(ctx.bind(), N.ptr(Xu), d, N.ptr(idx) if k else None, k, N.ptr(mn), N.ptr(mx),
                                    N.ptr(out), ld, N.ptr(sqn)), "svmd_sv_rows_u8")
    return out, sqn


def rbf_gram_sym(X: torch.Tensor, sqn: Optional[torch.Tensor], gamma: float, mn=None, mx=None,
                 gram: str = "auto", out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, str]:
    """Symmetric RBF Gram of preprocessed rows with the svmd_train_q path selection.
    Returns (K, path) with path "int8-exact" or "fp64"."""
    _check_rows(X)
    n = X.shape[0]
    if out is None:
        out = device_empty((n, (n + 1) // 2 * 2), torch.float64, X.device)
    ctx = _ctx_for(X)
    a, b, d = _host_stats(mn, mx)
    used = ctypes.c_int32(0)
    N.check(ctx.lib.svmd_rbf_gram_q(ctx.bind(), N.ptr(X), N.ptr(sqn) if sqn is not None else None, n, X.shape[1],
                                    X.shape[1], N.ptr(a), N.ptr(b), d, float(gamma), N.ptr(out), out.stride(0),
                                    GRAM_MODES[gram], ctypes.byref(used)), "svmd_rbf_gram_q")
    return out, ("int8-exact" if used.value else "fp64")


def decision(Xs: torch.Tensor, ns: torch.Tensor, coef: torch.Tensor, Xq: torch.Tensor, nq: torch.Tensor,
             gamma: float, b: float) -> torch.Tensor:
    """out[i] = sum_k coef[k] K(Xq_i, Xs_k) - b (MFMA cross-kernel + deterministic GEMV)."""
    _check_rows(Xq, "Xq")
    m = Xq.shape[0]
    out = torch.empty(m, dtype=torch.float64, device=Xq.device)
    nsv = Xs.shape[0]
    ctx = _ctx_for(Xq)
    N.check(ctx.lib.svmd_decision(ctx.bind(), N.ptr(Xs) if nsv else None, N.ptr(ns) if nsv else None,
                                  N.ptr(coef) if nsv else None, nsv, Xq.shape[1], N.ptr(Xq), N.ptr(nq), m,
                                  Xq.shape[1], Xq.shape[1], float(gamma), float(b), N.ptr(out)), "svmd_decision")
    return out


def decision_int(X: torch.Tensor, d: int, mn: torch.Tensor, mx: torch.Tensor, coef: torch.Tensor, gamma: float):
    """out[i] = sum_{k < nz} coef[k] K(X_i, X_k), nz = len(coef), on the exact-integer path (the
    Gram's own kernel values) for scaled pixel rows X; None when the rows are not integer pixels."""
    _check_rows(X, "X")
    coef = coef.contiguous()
    k, nz = X.shape[0], coef.numel()
    out = torch.empty(k, dtype=torch.float64, device=X.device)
    used = ctypes.c_int32(0)
    mn_h = np.ascontiguousarray(mn.detach().cpu().numpy(), dtype=np.float64)
    mx_h = np.ascontiguousarray(mx.detach().cpu().numpy(), dtype=np.float64)
    ctx = _ctx_for(X)
    N.check(ctx.lib.svmd_decision_int(ctx.bind(), N.ptr(X), k, X.shape[1], int(d), N.ptr(mn_h), N.ptr(mx_h),
                                      N.ptr(coef), nz, float(gamma), N.ptr(out), ctypes.byref(used)),
            "svmd_decision_int")
    return out if used.value else None


def count_correct(dec: torch.Tensor, y, zero_is_positive: bool = False) -> int:
    """#{i : sign(dec[i]) == y[i]} counted on the device (the reference's predict flag + reduce_sum,
    gpu_svm_main3.cu:277-315); s >= 0 -> +1 if zero_is_positive (cascade rule) else s > 0 -> +1."""
    dec = dec.contiguous()
    m = dec.numel()
    yd = torch.as_tensor(np.ascontiguousarray(y, dtype=np.int32) if not torch.is_tensor(y) else y)
    yd = yd.to(device=dec.device, dtype=torch.int32).contiguous()
    if yd.numel() != m:
        raise ValueError(f"count_correct: {m} decision values but {yd.numel()} labels")
    out = ctypes.c_int64(0)
    if m:
        ctx = _ctx_for(dec)
        N.check(ctx.lib.svmd_count_correct(ctx.bind(), N.ptr(dec), N.ptr(yd), m, int(bool(zero_is_positive)),
                                           ctypes.byref(out)), "svmd_count_correct")
    return int(out.value)


def _ovo_args(start: torch.Tensor, coef: torch.Tensor, rho: torch.Tensor, nsv: int, device) -> int:
    """Check the one-vs-one model tensors (device int32 start (k + 1,), float64 coef (k - 1, >= nsv) and
    rho (k (k - 1) / 2,)); returns k."""
    k = start.numel() - 1
    if k < 2 or k > 64:
        raise ValueError(f"one-vs-one prediction takes 2 to 64 classes, got {k}")
    for name, t, dt in (("start", start, torch.int32), ("coef", coef, torch.float64), ("rho", rho, torch.float64)):
        if t.dtype != dt or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{name} must be a contiguous {dt} tensor on {device}")
    if start.dim() != 1 or coef.dim() != 2 or coef.shape[0] != k - 1 or coef.shape[1] < nsv:
        raise ValueError(f"coef must be ({k - 1}, >= {nsv}) for {k} classes, got {tuple(coef.shape)}")
    if rho.shape != (k * (k - 1) // 2,):
        raise ValueError(f"rho must have shape ({k * (k - 1) // 2},), got {tuple(rho.shape)}")
    return k


def ovo_votes(K: torch.Tensor, start: torch.Tensor, coef: torch.Tensor, rho: torch.Tensor, want_dec: bool = True,
              nsv: Optional[int] = None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """One-vs-one pair decisions and votes from a cross-kernel block (svmd_ovo_votes, ovo.hip): K (m, ldk)
    float64 with K[i, s] = K(x_i, sv_s) over the nsv class-grouped support vectors (nsv: default start[-1], read
    back from the device), start int32 (k + 1,) the class segments, coef (k - 1, ldc) LIBSVM's coefficient
    layout, rho (P,).  Returns (dec (m, P) or None without ``want_dec``, label index (m,) int32): a decision
    > 0 votes for the pair's first class, anything else for its second; ties go to the lowest index.  The
    summation order is fixed (``ops.cpu.ovo_votes`` is the host twin)."""
    if K.dtype != torch.float64 or K.dim() != 2 or K.stride(1) != 1:
        raise ValueError("K must be a 2-D float64 tensor with unit column stride")
    nsv = int(start[-1].item()) if nsv is None else int(nsv)
    if nsv < 0 or nsv > K.shape[1]:
        raise ValueError(f"{nsv} support vectors but K has {K.shape[1]} columns")
    k = _ovo_args(start, coef, rho, nsv, K.device)
    m, P = K.shape[0], k * (k - 1) // 2
    dec = torch.empty((m, P), dtype=torch.float64, device=K.device) if want_dec else None
    label = torch.empty(m, dtype=torch.int32, device=K.device)
    ctx = _ctx_for(K)
    N.check(ctx.lib.svmd_ovo_votes(ctx.bind(), N.ptr(K), K.stride(0) if m > 1 else max(K.shape[1], 1), m, nsv, k,
                                   N.ptr(start), N.ptr(coef), coef.stride(0), N.ptr(rho), N.ptr(dec), N.ptr(label)),
            "svmd_ovo_votes")
    return dec, label


def ovo_predict(Xs: torch.Tensor, ns: torch.Tensor, Xq: torch.Tensor, nq: torch.Tensor, gamma: float,
                start: torch.Tensor, coef: torch.Tensor, rho: torch.Tensor, want_dec: bool = True,
                max_rows: int = 0) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """One-vs-one prediction from rows (svmd_ovo_predict): the cross-kernel K(Xq, Xs) in row chunks (at most
    512 MB; ``max_rows`` > 0 caps a chunk at that many rows, rounded up to 128) and ``ovo_votes``' kernel on
    every chunk.  Xs (nsv, ld): the class-grouped support vectors' scaled rows, ns their squared norms; Xq / nq
    the scaled query rows.  Returns (dec (m, P) or None, label index (m,) int32)."""
    _check_rows(Xq, "Xq")
    nsv = Xs.shape[0]
    if nsv:
        _check_rows(Xs, "Xs")
        if Xs.shape[1] != Xq.shape[1]:
            raise ValueError("Xs and Xq row lengths differ")
    k = _ovo_args(start, coef, rho, nsv, Xq.device)
    m, P = Xq.shape[0], k * (k - 1) // 2
    dec = torch.empty((m, P), dtype=torch.float64, device=Xq.device) if want_dec else None
    label = torch.empty(m, dtype=torch.int32, device=Xq.device)
    ctx = _ctx_for(Xq)
    N.check(ctx.lib.svmd_ovo_predict(ctx.bind(), N.ptr(Xs) if nsv else None, N.ptr(ns) if nsv else None, nsv,
                                     Xq.shape[1], N.ptr(Xq), N.ptr(nq), m, Xq.shape[1], Xq.shape[1], float(gamma), k,
                                     N.ptr(start), N.ptr(coef) if nsv else None, coef.stride(0), N.ptr(rho),
                                     int(max_rows), N.ptr(dec), N.ptr(label)), "svmd_ovo_predict")
    return dec, label


def gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """dst[k] = src[idx[k]] (device row gather, idx int64 on the same device)."""
    _check_rows(src, "src")
    idx = idx.to(device=src.device, dtype=torch.int64).contiguous()
    out = torch.empty((idx.numel(), src.shape[1]), dtype=torch.float64, device=src.device)
    if idx.numel():
        ctx = _ctx_for(src)
        N.check(ctx.lib.svmd_gather_rows(ctx.bind(), N.ptr(src), src.shape[1], N.ptr(idx), idx.numel(),
                                         N.ptr(out)), "svmd_gather_rows")
    return out
