"""CPU ops backed by the native core (libsvm355_core.so): the reference-exact oracle.

These implement main3.cpp's serial semantics (SMO_train :162-294, warm start
mpi_svm_main3.cpp:155-290, predict :391-402).  ``n_threads > 1`` parallelises the O(n) loops
without changing any result bit.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from .. import _native as N
from ..utils.config import SVMParams
from .device import PlattResult, SMOResult


def _c64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _c32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _start(alpha, n: int) -> np.ndarray:
    """The solver's alpha buffer: zeros, or a copy of the warm start, which must have n entries (the native
    solvers read n of them)."""
    if alpha is None:
        return np.zeros(n)
    if np.shape(alpha) != (n,):
        raise ValueError(f"alpha must have shape ({n},), got {np.shape(alpha)}")
    return np.array(alpha, dtype=np.float64, copy=True)


def _gram_shape(K: np.ndarray, n: int) -> None:
    if K.ndim != 2 or K.shape[0] < n or K.shape[1] < n:
        raise ValueError(f"K must be at least ({n}, {n}) for {n} labels, got {K.shape}")


def smo_train(X: np.ndarray, y: np.ndarray, params: SVMParams, alpha: Optional[np.ndarray] = None,
              warm: bool = False, trace_cap: int = 0, verbose: int = 0
              ) -> Tuple[np.ndarray, SMOResult, Optional[np.ndarray]]:
    """SMO on (already scaled) rows X with labels y in {+1,-1}.  Returns (alpha, result, trace)."""
    X = _c64(X)
    y = _c32(y)
    n, d = X.shape
    if y.shape != (n,):
        raise ValueError(f"y must have shape ({n},), got {y.shape}")
    a = _start(alpha, n)
    r = N.SvmResult()
    trace = np.zeros((trace_cap, 2), dtype=np.int64) if trace_cap > 0 else None
    p = params.to_struct(verbose)
    N.check(N.core().svm_smo_train(N.ptr(X), N.ptr(y), n, d, N.ptr(a), int(warm), ctypes.byref(p), ctypes.byref(r),
                                   N.ptr(trace) if trace is not None else None, trace_cap), "svm_smo_train")
    res = SMOResult.from_struct(r)
    if trace is not None:
        trace = trace[: max(0, min(trace_cap, res.iterations - 1))]
    return a, res, trace


def smo_train_gram(K: np.ndarray, y: np.ndarray, params: SVMParams, alpha: Optional[np.ndarray] = None,
                   warm: bool = False, trace_cap: int = 0) -> Tuple[np.ndarray, SMOResult, Optional[np.ndarray]]:
    K = _c64(K)
    y = _c32(y)
    n = y.shape[0]
    _gram_shape(K, n)
    a = _start(alpha, n)
    r = N.SvmResult()
    trace = np.zeros((trace_cap, 2), dtype=np.int64) if trace_cap > 0 else None
    p = params.to_struct()
    N.check(N.core().svm_smo_train_gram(N.ptr(K), K.shape[1], N.ptr(y), n, N.ptr(a), int(warm), ctypes.byref(p),
                                        ctypes.byref(r), N.ptr(trace) if trace is not None else None, trace_cap),
            "svm_smo_train_gram")
    res = SMOResult.from_struct(r)
    if trace is not None:
        trace = trace[: max(0, min(trace_cap, res.iterations - 1))]
    return a, res, trace


def decomp_train_gram(K: np.ndarray, y: np.ndarray, params: SVMParams, alpha: Optional[np.ndarray] = None,
                      q: int = 1024, tau_frac: float = 0.1, inner_wss: int = 3, trace_cap: int = 0,
                      snapshots: bool = False, fp64_rows: bool = False):
    """CPU oracle of the device decomposition solver (csrc/core/decomp_cpu.cpp) on a kernel matrix K.
    alpha given = warm start.  Returns (alpha, SMOResult, stats dict, N.DecompTrace or None).  fp64_rows (cold
    start only): the f update sums in the order of the device's FP64-row path (real-valued rows) instead of its
    exact-integer GEMV's."""
    K = _c64(K)
    y = _c32(y)
    n = y.shape[0]
    _gram_shape(K, n)
    a = _start(alpha, n)
    r = N.SvmResult()
    st = (ctypes.c_int64 * 16)()
    tr = N.DecompTrace(trace_cap, n if snapshots else 0) if trace_cap > 0 else None
    p = params.to_struct()
    trp = ctypes.byref(tr.struct) if tr is not None else None
    if alpha is None:  # cold: the entry that takes the f update's summation order
        N.check(N.core().svm_decomp_train_gram_rows(N.ptr(K), K.shape[1], N.ptr(y), n, N.ptr(a), ctypes.byref(p),
                                                    int(q), float(tau_frac), int(inner_wss), int(bool(fp64_rows)),
                                                    ctypes.byref(r), st, trp), "svm_decomp_train_gram_rows")
    elif fp64_rows:
        raise ValueError("fp64_rows: cold start only")
    else:
        N.check(N.core().svm_decomp_train_gram(N.ptr(K), K.shape[1], N.ptr(y), n, N.ptr(a), 1, ctypes.byref(p),
                                               int(q), float(tau_frac), int(inner_wss), ctypes.byref(r), st, trp),
                "svm_decomp_train_gram")
    return a, SMOResult.from_struct(r), _decomp_stats(st), tr


def _targets(z, n: int) -> np.ndarray:
    z = _c64(z)
    if z.shape != (n,):
        raise ValueError(f"z must have shape ({n},), got {z.shape}")
    return z


def smo_train_svr(X: np.ndarray, z: np.ndarray, params: SVMParams, epsilon: float = 0.1
                  ) -> Tuple[np.ndarray, SMOResult]:
    """epsilon-SVR on the pairwise oracle (svm_smo_train_svr: the 2n-variable problem on duplicated rows, for
    small n).  Returns (alpha of 2n entries: a, then a*; result); the model is beta = a - a*."""
    X = _c64(X)
    n, d = X.shape
    z = _targets(z, n)
    a = np.zeros(2 * n)
    r = N.SvmResult()
    p = params.to_struct()
    N.check(N.core().svm_smo_train_svr(N.ptr(X), N.ptr(z), n, d, float(epsilon), N.ptr(a), ctypes.byref(p),
                                       ctypes.byref(r)), "svm_smo_train_svr")
    return a, SMOResult.from_struct(r)


def decomp_train_gram_svr(K: np.ndarray, z: np.ndarray, params: SVMParams, epsilon: float = 0.1, q: int = 1024,
                          tau_frac: float = 0.1, inner_wss: int = 3, trace_cap: int = 0, snapshots: bool = False,
                          fp64_rows: bool = False):
    """The decomposition oracle's twin mode (epsilon-SVR, svm_decomp_train_gram_svr) on the n x n kernel matrix
    K and the n targets z.  Returns (alpha of 2n entries: a, then a*; SMOResult; stats dict; N.DecompTrace or
    None -- its ids are virtual, k and k + n, and its snapshots 2n long).  fp64_rows: the f update sums in the
    order of the device's FP64-row path (real-valued rows) instead of its exact-integer GEMV's."""
    K = _c64(K)
    n = np.shape(z)[0]
    z = _targets(z, n)
    _gram_shape(K, n)
    a = np.zeros(2 * n)
    r = N.SvmResult()
    st = (ctypes.c_int64 * 16)()
    tr = N.DecompTrace(trace_cap, 2 * n if snapshots else 0) if trace_cap > 0 else None
    p = params.to_struct()
    N.check(N.core().svm_decomp_train_gram_svr(N.ptr(K), K.shape[1], N.ptr(z), n, float(epsilon), N.ptr(a),
                                               ctypes.byref(p), int(q), float(tau_frac), int(inner_wss),
                                               int(bool(fp64_rows)), ctypes.byref(r), st,
                                               ctypes.byref(tr.struct) if tr is not None else None),
            "svm_decomp_train_gram_svr")
    return a, SMOResult.from_struct(r), _decomp_stats(st), tr


def twin_fold(cols: np.ndarray, coef: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """The twin mode's moved-column fold (svm_decomp_twin_fold): virtual ids in [0, 2n) and their coefficients
    to one entry per kernel row.  Returns (rows, coefficients)."""
    cols = _c32(cols)
    coef = _c64(coef)
    if cols.shape != coef.shape or cols.ndim != 1:
        raise ValueError("cols and coef must be 1-D arrays of one length")
    oc = np.zeros(max(1, cols.size), dtype=np.int32)
    ov = np.zeros(max(1, cols.size))
    cnt = ctypes.c_int32(0)
    N.check(N.core().svm_decomp_twin_fold(N.ptr(cols), N.ptr(coef), int(cols.size), int(n), N.ptr(oc), N.ptr(ov),
                                          ctypes.byref(cnt)), "svm_decomp_twin_fold")
    return oc[: cnt.value].copy(), ov[: cnt.value].copy()


def smo_train_oneclass(X: np.ndarray, params: SVMParams, nu: float = 0.5) -> Tuple[np.ndarray, SMOResult]:
    """One-class SVM on the pairwise oracle (svm_smo_train_oneclass: y = +1, box 1, no linear term, LIBSVM's
    feasible start).  Returns (alpha of n entries, result); result.b is rho.  params.C is not read."""
    X = _c64(X)
    n, d = X.shape
    a = np.zeros(n)
    r = N.SvmResult()
    p = params.to_struct()
    N.check(N.core().svm_smo_train_oneclass(N.ptr(X), n, d, float(nu), N.ptr(a), ctypes.byref(p), ctypes.byref(r)),
            "svm_smo_train_oneclass")
    return a, SMOResult.from_struct(r)


def decomp_train_gram_oneclass(K: np.ndarray, params: SVMParams, nu: float = 0.5, q: int = 1024,
                               tau_frac: float = 0.1, inner_wss: int = 3, trace_cap: int = 0,
                               snapshots: bool = False, fp64_rows: bool = False):
    """The decomposition oracle's one-class mode (svm_decomp_train_gram_oneclass) on the n x n kernel matrix K.
    Returns (alpha of n entries; SMOResult, b = rho; stats dict, "start_columns" = the start's columns;
    N.DecompTrace or None).  fp64_rows: the start and the f update sum in the order of the device's FP64-row
    path (real-valued rows) instead of its exact-integer GEMV's."""
    K = _c64(K)
    n = K.shape[0]
    _gram_shape(K, n)
    a = np.zeros(n)
    r = N.SvmResult()
    st = (ctypes.c_int64 * 16)()
    tr = N.DecompTrace(trace_cap, n if snapshots else 0) if trace_cap > 0 else None
    p = params.to_struct()
    N.check(N.core().svm_decomp_train_gram_oneclass(N.ptr(K), K.shape[1], n, float(nu), N.ptr(a), ctypes.byref(p),
                                                    int(q), float(tau_frac), int(inner_wss), int(bool(fp64_rows)),
                                                    ctypes.byref(r), st,
                                                    ctypes.byref(tr.struct) if tr is not None else None),
            "svm_decomp_train_gram_oneclass")
    return a, SMOResult.from_struct(r), {**_decomp_stats(st), "start_columns": int(st[7])}, tr


def decomp_train_gram_heldout(K: np.ndarray, y: np.ndarray, heldout: np.ndarray, params: SVMParams, q: int = 1024,
                              tau_frac: float = 0.1, inner_wss: int = 3, trace_cap: int = 0,
                              snapshots: bool = False, fp64_rows: bool = False):
    """The decomposition oracle's held-out mode (svm_decomp_train_gram_heldout) on the n x n kernel matrix K:
    the points with ``heldout[i]`` true run with label 0, which no selection takes, so their alpha stays exactly
    0 while their f collects every update.  Returns (alpha; SMOResult; stats dict; the final f of all n points;
    N.DecompTrace or None): ``f[heldout] - result.b`` are the held-out decision values."""
    K = _c64(K)
    y = _c32(y)
    n = y.shape[0]
    _gram_shape(K, n)
    m = np.ascontiguousarray(np.asarray(heldout).astype(bool), dtype=np.uint8)
    if m.shape != (n,):
        raise ValueError(f"heldout must have shape ({n},), got {m.shape}")
    a = np.zeros(n)
    f = np.zeros(n)
    r = N.SvmResult()
    st = (ctypes.c_int64 * 16)()
    tr = N.DecompTrace(trace_cap, n if snapshots else 0) if trace_cap > 0 else None
    p = params.to_struct()
    N.check(N.core().svm_decomp_train_gram_heldout(N.ptr(K), K.shape[1], N.ptr(y), N.ptr(m), n, N.ptr(a),
                                                   ctypes.byref(p), int(q), float(tau_frac), int(inner_wss),
                                                   int(bool(fp64_rows)), ctypes.byref(r), st, N.ptr(f),
                                                   ctypes.byref(tr.struct) if tr is not None else None),
            "svm_decomp_train_gram_heldout")
    return a, SMOResult.from_struct(r), _decomp_stats(st), f, tr


def platt_fit(dec: np.ndarray, y: np.ndarray, use: Optional[np.ndarray] = None) -> PlattResult:
    """Platt scaling on the host (svm_platt_fit): P(y = +1 | f) = 1 / (1 + exp(A f + B)) fitted to the pairs
    (dec_i, y_i) by Lin, Lin and Weng's Newton method, as LIBSVM's -b 1.  use: optional boolean mask of the pairs
    that count."""
    dec = _c64(dec)
    y = _c32(y)
    if dec.ndim != 1 or y.shape != dec.shape:
        raise ValueError("dec and y must be 1-D arrays of one length")
    u = None if use is None else np.ascontiguousarray(np.asarray(use).astype(bool), dtype=np.uint8)
    if u is not None and u.shape != dec.shape:
        raise ValueError("use must have the shape of dec")
    o = N.SvmPlatt()
    N.check(N.core().svm_platt_fit(N.ptr(dec), N.ptr(y), N.ptr(u), dec.shape[0], ctypes.byref(o)), "svm_platt_fit")
    return PlattResult.from_struct(o)


def _decomp_stats(st) -> dict:
    return {"outer_iterations": int(st[0]), "inner_iterations": int(st[1]), "working_set": int(st[2]),
            "solve_us": int(st[3]), "update_columns": int(st[4]), "chain_iterations": int(st[13]),
            "eta_floor_updates": int(st[14]),  # first-pair updates on a pair with eta <= eps (identical rows)
            **N.shrink_stats(st)}


def decomp_train_gram_dist(K: np.ndarray, y: np.ndarray, params: SVMParams, world: int = 1, comm=None,
                           alpha: Optional[np.ndarray] = None, q: int = 1024, tau_frac: float = 0.1,
                           inner_wss: int = 3, comm_timeout_s: float = 120.0):
    """The distributed form of ``decomp_train_gram`` (decomp.hip's world > 1 solve on the CPU oracle):
    ``comm`` = a ``HostCommRank`` (this process's rank over a gloo group, torchrun), or ``world``
    thread-ranks of this process over the strict loopback transport.  Every rank owns 1/world of the
    selection blocks and of f and all-gathers its candidate records once per outer iteration; for world
    dividing 8 the result is ``decomp_train_gram``'s bit for bit.  Returns (alpha, SMOResult, stats)."""
    K = _c64(K)
    y = _c32(y)
    n = y.shape[0]
    _gram_shape(K, n)
    a = _start(alpha, n)
    r = N.SvmResult()
    st = (ctypes.c_int64 * 16)()
    p = params.to_struct()
    if comm is not None:
        comm.error = None
        rc = N.core().svm_decomp_rank_train_gram(ctypes.addressof(comm.comm), N.ptr(K), K.shape[1], N.ptr(y), n,
                                                 N.ptr(a), int(alpha is not None), ctypes.byref(p), int(q),
                                                 float(tau_frac), int(inner_wss), ctypes.byref(r), st)
        if rc != 0 and comm.error is not None:
            raise N.NativeError(f"{N.last_error()} (collective error: {comm.error!r})") from comm.error
        N.check(rc, "svm_decomp_rank_train_gram")
    else:
        N.check(N.core().svm_decomp_group_train_gram(int(world), N.ptr(K), K.shape[1], N.ptr(y), n, N.ptr(a),
                                                     int(alpha is not None), ctypes.byref(p), int(q), float(tau_frac),
                                                     int(inner_wss), ctypes.byref(r), st, float(comm_timeout_s)),
                "svm_decomp_group_train_gram")
    return a, SMOResult.from_struct(r), _decomp_stats(st)


def rbf_matrix(A: np.ndarray, B: np.ndarray, gamma: float, n_threads: int = 0) -> np.ndarray:
    """Reference-exact RBF kernel matrix (direct sum of squared differences)."""
    A = _c64(A)
    B = _c64(B)
    K = np.empty((A.shape[0], B.shape[0]))
    N.check(N.core().svm_rbf_matrix(N.ptr(A), A.shape[0], N.ptr(B), B.shape[0], A.shape[1], float(gamma), N.ptr(K),
                                    int(n_threads)), "svm_rbf_matrix")
    return K


def decision(Xs: np.ndarray, ys: np.ndarray, alphas: np.ndarray, Xq: np.ndarray, gamma: float, b: float,
             n_threads: int = 0) -> np.ndarray:
    Xs = _c64(Xs).reshape(-1, Xq.shape[1])
    ys = _c32(ys)
    alphas = _c64(alphas)
    Xq = _c64(Xq)
    out = np.empty(Xq.shape[0])
    N.check(N.core().svm_decision(N.ptr(Xs), N.ptr(ys), N.ptr(alphas), Xs.shape[0], N.ptr(Xq), Xq.shape[0],
                                  Xq.shape[1], float(gamma), float(b), N.ptr(out), int(n_threads)), "svm_decision")
    return out


def ovo_pairs(k: int) -> np.ndarray:
    """The k (k - 1) / 2 one-vs-one pairs (a, b), a < b, in LIBSVM's order (0,1), (0,2), ..., (k-2,k-1)."""
    return np.array([(a, b) for a in range(k) for b in range(a + 1, k)], dtype=np.int64).reshape(-1, 2)


def ovo_votes(K: np.ndarray, start: np.ndarray, coef: np.ndarray, rho: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """One-vs-one pair decisions and votes on the host, by the rule of the device kernel (csrc/hip/ovo.hip).
    K (m, >= S): K[i, s] = K(x_i, sv_s) over the class-grouped support vectors; start (k + 1,): class c is
    [start[c], start[c + 1]); coef (k - 1, >= S): LIBSVM's layout (for a support vector of class c, row j is
    its alpha * y in the pair (c, o), o = j for j < c, else j + 1); rho (P,).  For the pair p = (a, b):
    dec[:, p] = (sum over a's segment of coef[b - 1] K) + (sum over b's segment of coef[a] K) - rho[p].
    dec > 0 votes for a, anything else for b; the label index is the first class with the most votes.
    Returns (dec (m, P), label index (m,) int32)."""
    K = np.asarray(K, dtype=np.float64)
    start = np.asarray(start, dtype=np.int64)
    coef = np.asarray(coef, dtype=np.float64)
    rho = np.asarray(rho, dtype=np.float64)
    k = start.shape[0] - 1
    pairs = ovo_pairs(k)
    if k < 2 or rho.shape != (len(pairs),) or coef.ndim != 2 or coef.shape[0] != k - 1 or K.ndim != 2:
        raise ValueError(f"ovo_votes: k = {k} classes need coef ({k - 1}, S) and rho ({len(pairs)},)")
    if start[0] != 0 or np.any(np.diff(start) < 0) or start[-1] > min(K.shape[1], coef.shape[1]):
        raise ValueError("ovo_votes: start must ascend from 0 to at most the columns of K and coef")
    m = K.shape[0]
    part = np.zeros((k, k - 1, m))
    for c in range(k):
        seg = slice(int(start[c]), int(start[c + 1]))
        if seg.stop > seg.start:
            part[c] = coef[:, seg] @ K[:, seg].T
    dec = np.empty((m, len(pairs)))
    for p, (a, b) in enumerate(pairs):
        dec[:, p] = part[a, b - 1] + part[b, a] - rho[p]
    return dec, ovo_labels(dec, k)


def ovo_labels(dec: np.ndarray, k: int) -> np.ndarray:
    """The one-vs-one vote over (m, P) pair decisions in LIBSVM's pair order: dec > 0 votes for the pair's first
    class, anything else (exactly 0 included) for its second; the label index (int32) is the first class with the
    most votes."""
    dec = np.asarray(dec, dtype=np.float64)
    pairs = ovo_pairs(k)
    if dec.ndim != 2 or dec.shape[1] != len(pairs):
        raise ValueError(f"ovo_labels: {k} classes need (m, {len(pairs)}) decisions, got {dec.shape}")
    votes = np.zeros((dec.shape[0], k), dtype=np.int64)
    rows = np.arange(dec.shape[0])
    for p, (a, b) in enumerate(pairs):
        votes[rows, np.where(dec[:, p] > 0.0, a, b)] += 1
    return np.argmax(votes, axis=1).astype(np.int32)


def _couple_k(P: int) -> int:
    """The k of P = k (k - 1) / 2 pair columns (2 .. 64), or ValueError."""
    k = int(round((1.0 + (1.0 + 8.0 * P) ** 0.5) / 2.0))
    if k < 2 or k > 64 or k * (k - 1) // 2 != P:
        raise ValueError(f"ovo_couple: {P} pair columns are not k (k - 1) / 2 for a k in 2 .. 64")
    return k


def ovo_couple(dec: np.ndarray, A: Optional[np.ndarray] = None, B: Optional[np.ndarray] = None,
               n_threads: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pairwise coupling on the host (svm_ovo_couple; the twin of the device kernel in csrc/hip/ovo_proba.hip):
    class probabilities from (m, P) one-vs-one pair decisions in LIBSVM's pair order, Wu, Lin and Weng's second
    method as LIBSVM runs it.  A, B (P,): the pairs' sigmoids, P(first class | dec) = 1 / (1 + exp(A dec + B));
    both None: ``dec`` already holds the pair probabilities r_ab.  Returns (proba (m, k), label index (m,) int32:
    the first largest probability, iters (m,) int32: the sweeps taken -- max(100, k) means not converged)."""
    dec = _c64(dec)
    if dec.ndim != 2:
        raise ValueError("ovo_couple: dec must be (m, P)")
    m, P = dec.shape
    k = _couple_k(P)
    if (A is None) != (B is None):
        raise ValueError("ovo_couple: A and B come together")
    if A is not None:
        A, B = _c64(A), _c64(B)
        if A.shape != (P,) or B.shape != (P,):
            raise ValueError(f"ovo_couple: A and B must have shape ({P},)")
    proba = np.empty((m, k))
    label = np.empty(m, dtype=np.int32)
    iters = np.empty(m, dtype=np.int32)
    N.check(N.core().svm_ovo_couple(N.ptr(dec), P, m, k, N.ptr(A), N.ptr(B), N.ptr(proba), k, N.ptr(label),
                                    N.ptr(iters), int(n_threads)), "svm_ovo_couple")
    return proba, label, iters


def sv_indices(alpha: np.ndarray, tol: float = 1e-8) -> np.ndarray:
    alpha = _c64(alpha)
    out = np.empty(alpha.shape[0], dtype=np.int64)
    k = N.core().svm_sv_indices(N.ptr(alpha), alpha.shape[0], float(tol), N.ptr(out))
    return out[:k].copy()
