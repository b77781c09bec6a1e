"""Sparse (CSR) fit against the dense FP64 fit of the same rows: profiles/sparse.md's numbers.

Generates its own synthetic sparse set from a seed (n rows, d features, a given density, values in (0, 1], labels
from a noisy linear rule), fits SVC on the CSR rows (a cold fit, then the timed warm fits) and, with --dense, on
``toarray()`` of the same rows with the decomposition solver's FP64-row path; reports fit times (host clock around
fits that end in a device-to-host copy), peak device memory of each, the support sets' overlap and the largest
decision difference on held-out rows.  One JSON line on stdout.  For per-kernel times run it under
``rocprofv3 --kernel-trace --stats -- python scripts/sparse_profile.py ...`` in a run of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(n, d, density, seed):
    import svm355

    rng = np.random.default_rng(seed)
    per = max(1, int(round(d * density)))
    stride = d // per  # one index from each of `per` equal strata: sorted and unique by construction
    indices = (np.arange(per) * stride + rng.integers(0, stride, (n, per))).astype(np.int32)
    data = 1.0 - rng.random(n * per)
    X = svm355.CSR(data, indices.ravel(), np.arange(n + 1, dtype=np.int64) * per, (n, d))
    w = rng.normal(size=d)
    s = (data.reshape(n, per) * w[indices]).sum(1) + 0.1 * rng.normal(size=n)
    return X, s


def fit_timed(est, X, y, repeats):
    import torch

    times = []
    for _ in range(repeats + 1):  # the first fit is the warm-up (code objects, workspace growth)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        est.fit(X, y)
        times.append((time.perf_counter() - t0) * 1e3)
        used = free0 - torch.cuda.mem_get_info()[0]  # includes the library's own workspace, outside torch's allocator
    return times[1:], used, torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=20_000)
    ap.add_argument("--density", type=float, default=0.005)
    ap.add_argument("--heldout", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--dense", action="store_true", help="also fit the dense FP64 rows (toarray) of the same set")
    ap.add_argument("--gamma", type=float, default=0.05)
    ap.add_argument("--kernel", default="rbf", choices=("rbf", "linear"),
                    help="linear: the CSR fit runs csr_linear.hip's weight-vector update, the dense one decomp_kfun.hip")
    ap.add_argument("--C", type=float, default=10.0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import svm355

    X, s = make(a.n + a.heldout, a.d, a.density, a.seed)
    per = int(X.indptr[1])
    y = np.where(s > np.median(s), 1, -1).astype(np.int32)
    cut = a.n * per
    Xtr = svm355.CSR(X.data[:cut], X.indices[:cut], X.indptr[:a.n + 1], (a.n, a.d))
    Xte = svm355.CSR(X.data[cut:], X.indices[cut:], X.indptr[a.n:] - cut, (a.heldout, a.d))
    kw = dict(C=a.C, gamma=a.gamma, tol=1e-3, device="cuda:0", solver="decomp", kernel=a.kernel)
    out = {"n": a.n, "d": a.d, "density": a.density, "nnz_per_row": per, "kernel": a.kernel, "C": a.C}
    sp = svm355.SVC(**kw)
    t, used, peak = fit_timed(sp, Xtr, y[:a.n], a.repeats)
    out["sparse"] = {"fit_ms": t, "device_bytes_grown": int(used), "torch_peak_bytes": int(peak),
                     "solve_ms": sp.timings_["total_ms"], "outer": sp.timings_["outer_iterations"],
                     "n_sv": int(len(sp.support_)), "stop": sp.stop_reason_}
    dec_sp = sp.decision_function(Xte)
    if a.dense:
        os.environ["SVM355_DECOMP_F64"] = "1"  # the FP64-row path, the only dense one that takes real-valued rows
        de = svm355.SVC(**kw)
        t, used, peak = fit_timed(de, Xtr.toarray(), y[:a.n], a.repeats)
        dec_de = de.decision_function(Xte.toarray())
        both = np.intersect1d(sp.support_, de.support_).size
        out["dense"] = {"fit_ms": t, "device_bytes_grown": int(used), "torch_peak_bytes": int(peak),
                        "solve_ms": de.timings_["total_ms"], "outer": de.timings_["outer_iterations"],
                        "n_sv": int(len(de.support_)), "stop": de.stop_reason_}
        out["sv_overlap"] = both / max(1, np.union1d(sp.support_, de.support_).size)
        out["max_decision_diff"] = float(np.abs(dec_sp - dec_de).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
