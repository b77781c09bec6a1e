"""One-GPU timings for profiles/probability.md: SVC(probability=True, cv=5) on the headline shape against plain
fits, and the one-workgroup sigmoid fit alone.

    python scripts/probability_profile.py [--n 60000] [--cv 5] [--reps 3] [--plain 6] [--platt-n 60000 1000000]
    python scripts/probability_profile.py --plain-only     # runs on a tree without probability= too (the parent's)

Input: synthetic_mnist(n, seed=1) uint8 rows with the generator's one-vs-rest labels (seeded, nothing read from
disk), C = 10, gamma = 0.00125, tol = 1e-5.  JSON lines:
* "plain": one warm-up fit, then `plain` plain fits back to back, each timed by the host clock around fit(), and
  their sum -- what k fold fits and the final fit cost one after another (each fold fit has 4/5 of the rows, so
  this is an upper bound for k separate fits, and what running the final fit 1 + k times costs).
* "probability": the first fit of the process apart, then `reps` warm fits of SVC(probability=True, cv=cv): the
  whole fit, cv_ms (the pooled final + fold solves), platt_ms, every fold's own solve time, and the sigmoid.
* "platt": svmd_platt_fit alone on n synthetic (decision, label) pairs already on the device, the median of 7 calls
  after a warm-up (host clock around the call: the launch, the kernel, the 24-byte copy back and the
  synchronisation), its Newton iterations, and the host twin (svm_platt_fit) on the same pairs.
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


def timed_fits(make, X, y, count):
    times, m = [], None
    for _ in range(count):
        t0 = time.perf_counter()
        m = make().fit(X, y)
        times.append((time.perf_counter() - t0) * 1e3)
    return times, m


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--cv", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--plain", type=int, default=6)
    ap.add_argument("--platt-n", type=int, nargs="*", default=[60000, 1000000])
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()

    from svm355 import SVC
    from svm355.utils.data import synthetic_mnist

    tr = synthetic_mnist(a.n, seed=1).compact()
    y = np.ascontiguousarray(tr.y, dtype=np.int32)

    def plain():
        return SVC(device="cuda:0", gamma=GAMMA, max_iter=10**8)

    times, m = timed_fits(plain, tr.X, y, a.plain + 1)
    print(json.dumps({"mode": "plain", "n": a.n, "first_fit_ms": round(times[0], 2),
                      "fit_ms": [round(t, 2) for t in times[1:]], "sum_ms": round(sum(times[1:]), 2),
                      "solve_ms": round(m.timings_["smo_ms"], 2), "n_sv": int(len(m.support_)), "b": m.b_}), flush=True)
    if a.plain_only:
        return

    def proba():
        return SVC(device="cuda:0", gamma=GAMMA, max_iter=10**8, probability=True, cv=a.cv)

    times, p = timed_fits(proba, tr.X, y, a.reps + 1)
    tm = p.timings_
    print(json.dumps({"mode": "probability", "n": a.n, "cv": a.cv, "first_fit_ms": round(times[0], 2),
                      "fit_ms": [round(t, 2) for t in times[1:]], "cv_ms": round(tm["cv_ms"], 2),
                      "platt_ms": round(tm["platt_ms"], 3),
                      "upload_preprocess_ms": round(tm["upload_preprocess_ms"], 2),
                      "final_solve_ms": round(tm["total_ms"], 2), "fold_ms": [round(t, 2) for t in tm["fold_ms"]],
                      "concurrent_solves": tm["concurrent_solves"], "same_model_as_plain": bool(
                          np.array_equal(p.alpha_, m.alpha_) and p.b_ == m.b_),
                      "probA": p.probA_, "probB": p.probB_, "platt_iterations": p.platt_.iterations,
                      "platt_status": p.platt_.status,
                      "cv_accuracy": float(np.mean(np.where(p.cv_decision_ > 0, 1, -1) == y))}), flush=True)

    import torch

    from svm355.ops import cpu as C
    from svm355.ops import device as D

    dev = torch.device("cuda:0")
    for n in a.platt_n:
        rng = np.random.default_rng(n)
        lab = np.where(rng.random(n) < 0.1, 1, -1).astype(np.int32)
        dec = 1.5 * lab + 1.2 * rng.standard_normal(n)
        dd, yd = torch.from_numpy(dec).to(dev), torch.from_numpy(lab).to(dev)
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(8):
            t0 = time.perf_counter()
            r = D.platt_fit(dd, yd)
            ts.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        c = C.platt_fit(dec, lab)
        host_ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"mode": "platt", "n": n, "device_ms": round(statistics.median(ts[1:]), 3),
                          "device_first_ms": round(ts[0], 3), "iterations": r.iterations, "status": r.status,
                          "A": r.A, "B": r.B, "host_ms": round(host_ms, 3), "host_iterations": c.iterations,
                          "host_A": c.A, "host_B": c.B}), flush=True)


if __name__ == "__main__":
    main()
