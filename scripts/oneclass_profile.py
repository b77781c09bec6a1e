"""One-GPU one-class SVM fits for profiles/oneclass.md: what the chunked start costs.

    python scripts/oneclass_profile.py [--n 60000] [--nu 0.05 0.1 0.5] [--reps 3]

Input: synthetic_mnist(n, seed=1) uint8 rows (seeded, nothing read from disk), gamma = 0.00125, tol = 1e-5.
Per nu one JSON line: the first fit of the process apart (it loads code objects), then `reps` warm fits timed by
the host clock around fit() (it ends in device-to-host copies of the alphas); the solver's own time (smo_ms), the
start's columns and chunks (one f update per 1,024 columns before the first selection), the outer iterations
and the support vectors.  The start's cost is estimated as chunks x the time of one 1,024-column f update on these
rows: the solver's own f update alone (svmd_decomp_gemv_u8: quantisation, the GEMV and its sum, copies) with
1,024 columns minus the same call with one column, the median of 5.  A last line: the classifier's fit (SVC,
solver="decomp") of the same rows with the generator's one-vs-rest labels, for orientation.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GAMMA = 0.00125


def chunk_ms(X) -> float:
    """One 1,024-column f update over these rows, ms (see the module docstring)."""
    import torch

    from svm355.ops import device as D

    dev = torch.device("cuda:0")
    Xu = D.upload_u8(X, dev)
    mmd = torch.empty(2 * X.shape[1], dtype=torch.float64, device=dev)
    D.minmax_u8(Xu, out=mmd)
    mm = mmd.cpu().numpy()
    mn, mx = mm[: X.shape[1]].copy(), mm[X.shape[1]:].copy()

    def timed(m):
        cols, coef = np.arange(m, dtype=np.int32), np.ones(m)
        ts = []
        for _ in range(6):
            t0 = time.perf_counter()
            assert D.decomp_gemv_u8(Xu, mn, mx, GAMMA, cols, coef) is not None
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts[1:])

    return timed(1024) - timed(1)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--nu", type=float, nargs="+", default=[0.05, 0.1, 0.5])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()

    from svm355 import SVC, OneClassSVM
    from svm355.utils.data import synthetic_mnist

    tr = synthetic_mnist(a.n, seed=1).compact()
    per_chunk = chunk_ms(tr.X)
    for nu in a.nu:
        times = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            m = OneClassSVM(nu=nu, gamma=GAMMA, device="cuda:0", max_iter=10**8).fit(tr.X)
            times.append((time.perf_counter() - t0) * 1e3)
        tm = m.timings_
        chunks = -(-tm["start_columns"] // 1024)
        print(json.dumps({"nu": nu, "n": a.n, "first_fit_ms": round(times[0], 2),
                          "fit_ms": [round(t, 2) for t in times[1:]], "solve_ms": round(tm["smo_ms"], 2),
                          "quantise_ms": round(tm["gram_ms"], 2), "stop": m.stop_reason_,
                          "start_columns": tm["start_columns"], "start_chunks": chunks,
                          "chunk_ms": round(per_chunk, 3), "start_ms_estimate": round(chunks * per_chunk, 2),
                          "outer_iterations": tm["outer_iterations"], "pair_updates": tm["inner_iterations"],
                          "update_columns": tm["update_columns"], "gram_path": tm["gram_path"],
                          "n_sv": int(len(m.support_)), "rho": m.rho_,
                          "train_outliers": int((m.decision_function(tr.X[:5000]) < 0).sum()), "of": 5000}), flush=True)
    times = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        c = SVC(device="cuda:0", solver="decomp", gamma=GAMMA, max_iter=10**8).fit(tr.X, tr.y)
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"mode": "svc", "n": a.n, "first_fit_ms": round(times[0], 2),
                      "fit_ms": [round(t, 2) for t in times[1:]], "solve_ms": round(c.timings_["smo_ms"], 2),
                      "outer_iterations": c.timings_["outer_iterations"], "n_sv": int(len(c.support_))}), flush=True)


if __name__ == "__main__":
    main()
