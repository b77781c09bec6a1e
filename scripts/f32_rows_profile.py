"""row_dtype="float32" against the FP64-row path on the same real-valued rows: profiles/f32_rows.md's numbers; with
``--dtypes float32 float16``, float16 rows against float32 rows by the same protocol: profiles/f16_rows.md's.

The rows are bench.py's --input f64-real rows (the synthetic MNIST-shaped pixels plus a uniform [0, 0.5) offset per
value, the digit-1 one-vs-rest labels) with the headline parameters (C = 10, gamma = 0.00125, tol = 1e-5).  For
each --n it fits SVC with each of --dtypes (default float64 float32) in one process, alternating them: one warm-up fit each,
then --repeats timed fits each (a host clock around fits that end in a device-to-host copy).  Reports fit time,
upload + preprocess time, solve time, the device memory the fit grew (the library's workspace is outside torch's
allocator, so it is read from the free memory), support-vector counts, |b|, and the largest difference of the two
models' decision values on --heldout held-out rows (every dtype against the first of the list).  float32 and float16
fits are both given the float32 array.  One JSON line per n on stdout.  For per-kernel times run one
dtype under ``rocprofv3 --kernel-trace --stats -- python scripts/f32_rows_profile.py --only float32 --repeats 1``
in a run of its own; ``flop`` in the output is the f update's 2 rows x columns x d of the whole fit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def real_rows(n, seed, offset=0):
    from svm355.utils.data import synthetic_mnist

    ds = synthetic_mnist(n, seed=seed, offset=offset)
    return ds.X + np.random.default_rng(seed + 7 + offset).uniform(0.0, 0.5, size=ds.X.shape), ds.y


def fit_once(est, X, y):
    import torch

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    est.fit(X, y)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, free0 - torch.cuda.mem_get_info()[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[60_000, 250_000])
    ap.add_argument("--heldout", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtypes", nargs="+", choices=["float64", "float32", "float16"], default=["float64", "float32"])
    ap.add_argument("--only", choices=["float64", "float32", "float16"], default=None)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    import torch

    import svm355

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    os.environ["SVM355_DECOMP_F64"] = "1"  # float64: the FP64-row path whatever the statistics admit
    for n in a.n:
        X, y = real_rows(n, a.seed)
        Xte, _ = real_rows(a.heldout, a.seed, offset=n)
        d = X.shape[1]
        out = {"n": n, "d": d, "repeats": a.repeats}
        dec = {}
        dtypes = [a.only] if a.only else a.dtypes
        est = {t: svm355.SVC(C=10.0, gamma=0.00125, tol=1e-5, device="cuda:0", solver="decomp", row_dtype=t)
               for t in dtypes}
        rec = {t: {"fit_ms": [], "upload_ms": [], "solve_ms": []} for t in dtypes}
        for rep in range(a.repeats + 1):  # rep 0 warms up; the dtypes alternate
            for t in dtypes:
                Xin = X if t == "float64" else X.astype(np.float32)  # float32 data arrives as float32
                ms, grown = fit_once(est[t], Xin, y)
                if rep == 0:
                    rec[t]["device_bytes_grown_first_fit"] = int(grown)
                    continue
                rec[t]["fit_ms"].append(round(ms, 2))
                rec[t]["upload_ms"].append(round(est[t].timings_["upload_preprocess_ms"], 2))
                rec[t]["solve_ms"].append(round(est[t].timings_["total_ms"], 2))
        for t in dtypes:
            m = est[t]
            cols = m.timings_["update_columns"]
            rec[t].update(n_sv=int(len(m.support_)), b=float(m.b_), stop=m.stop_reason_,
                          outer=m.timings_["outer_iterations"], update_columns=cols, rows=m.timings_["rows"],
                          flop=2.0 * n * cols * d)
            dec[t] = m.decision_function(Xte)
            out[t] = rec[t]
        if len(dtypes) == 2:
            p, q = dtypes
            out["max_decision_diff"] = float(np.abs(dec[p] - dec[q]).max())
            out["b_diff"] = abs(out[p]["b"] - out[q]["b"])
            out["sign_flips"] = int(np.sum(np.sign(dec[p]) != np.sign(dec[q])))
        print(json.dumps(out), flush=True)
        del X, Xte, est
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
