"""Measurements behind profiles/ovo_proba.md (one GPU): the calibrated one-vs-one fit (cv=5) against six plain
fits back to back, the batched sigmoid fit against one launch per pair, and the coupling kernel
(csrc/hip/ovo_proba.hip) against its host twin and as a share of a 10k-row predict_proba.

    python scripts/ovo_proba_profile.py [--n 60000] [--m 10000] [--reps 3] [--kreps 20] [--out ovo_proba_profile.json]

Fits are timed by the host clock around fit() (which ends in a device synchronise), the two variants in turn,
`--reps` times each after one warm-up of each; kernels by device events over `--kreps` launches after 3; calls
that synchronise themselves (the sigmoid fits) by the host clock, the median of `--kreps` after 3.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from svm355 import OneVsOneSVC  # noqa: E402
from svm355.ops import cpu as C  # noqa: E402
from svm355.ops import device as D  # noqa: E402
from svm355.utils.data import synthetic_mnist  # noqa: E402


def _spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return _spread(ts)


def _host(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _spread(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=60000)
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kreps", type=int, default=20)
    ap.add_argument("--out", default="ovo_proba_profile.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ovo_proba_profile.py measures on a GPU: none is visible")
    tr, te = synthetic_mnist(a.n, seed=a.seed), synthetic_mnist(a.m, seed=a.seed, offset=a.n)
    X, Xt = tr.compact().X, te.compact().X
    out = {"n": a.n, "m": a.m, "seed": a.seed, "device": torch.cuda.get_device_name(0)}

    # ---- fit: cv=5 against six plain fits back to back
    fit = {"six_plain_fits_s": [], "cv5_fit_s": [], "one_plain_fit_s": []}
    model = None
    for rep in range(a.reps + 1):  # rep 0 warms both up
        t0 = time.perf_counter()
        singles = []
        for _ in range(6):
            singles.append(OneVsOneSVC(device="cuda:0").fit(X, tr.labels).fit_time_)
        torch.cuda.synchronize()
        six = time.perf_counter() - t0
        model = OneVsOneSVC(device="cuda:0", cv=5).fit(X, tr.labels)
        torch.cuda.synchronize()
        if rep:
            fit["six_plain_fits_s"].append(six)
            fit["one_plain_fit_s"].extend(singles)
            fit["cv5_fit_s"].append(model.fit_time_)
        print("rep", rep, f"six plain {six:.3f} s, cv=5 {model.fit_time_:.3f} s", flush=True)
    fit["cv5_timings"] = dict(model.timings_)
    fit["platt_status"] = sorted(set(model.platt_status_))
    fit["probA_range"] = [float(model.probA_.min()), float(model.probA_.max())]
    out["fit"] = fit

    # ---- the batched sigmoid against one launch and one copy back per pair, on the fit's own held-out decisions
    cls = np.searchsorted(model.classes_, tr.labels)
    decs, ys = [], []
    for a_, b_ in model._pairs:
        rows = np.flatnonzero((cls == a_) | (cls == b_))
        decs.append(np.where(cls[rows] == a_, model.cv_decision_[rows, b_ - 1], model.cv_decision_[rows, a_]))
        ys.append(np.where(cls[rows] == a_, 1, -1).astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(d) for d in decs])])
    dec_d = torch.from_numpy(np.concatenate(decs)).to("cuda:0")
    y_d = torch.from_numpy(np.concatenate(ys)).to("cuda:0")
    segs = [(dec_d[s:e].contiguous(), y_d[s:e].contiguous()) for s, e in zip(off[:-1], off[1:])]
    batch = D.platt_fit_batch(dec_d, y_d, off)
    single = [D.platt_fit(d, y) for d, y in segs]
    out["platt"] = {"pairs": len(segs), "segment_rows": [int(off[1] - off[0]), int(np.diff(off).max())],
                    "identical": batch == single,
                    "newton_iterations": [min(p.iterations for p in batch), max(p.iterations for p in batch)],
                    "batch": _host(lambda: D.platt_fit_batch(dec_d, y_d, off), a.kreps),
                    "single_calls": _host(lambda: [D.platt_fit(d, y) for d, y in segs], a.kreps)}

    # ---- the coupling kernel on the m x P decisions of the query rows
    dm = model._dev_model
    Xq = D.upload_rows(Xt, dm["device"])
    _, _, nq = D.minmax_scale_(Xq, dm["d"], dm["mn"], dm["mx"])
    gamma = model.params.gamma
    dec, _ = D.ovo_predict(dm["Xs"], dm["ns"], Xq, nq, gamma, dm["start"], dm["coef"], dm["rho"])
    A_d, B_d = torch.from_numpy(model.probA_).to("cuda:0"), torch.from_numpy(model.probB_).to("cuda:0")
    proba, _, iters = D.ovo_couple(dec, A_d, B_d)
    dec_h = dec.cpu().numpy()
    twin = C.ovo_couple(dec_h, model.probA_, model.probB_)
    th = []
    for _ in range(5):
        t0 = time.perf_counter()
        C.ovo_couple(dec_h, model.probA_, model.probB_)
        th.append((time.perf_counter() - t0) * 1e3)
    t1 = []
    for _ in range(3):
        t0 = time.perf_counter()
        C.ovo_couple(dec_h, model.probA_, model.probB_, n_threads=1)
        t1.append((time.perf_counter() - t0) * 1e3)
    it = iters.cpu().numpy()
    cp = {"m": int(dec.shape[0]), "P": int(dec.shape[1]), "n_sv_union": int(len(model.support_)),
          "sweeps": {"min": int(it.min()), "median": float(np.median(it)), "max": int(it.max())},
          "max_abs_device_minus_twin": float(np.abs(proba.cpu().numpy() - twin[0]).max()),
          "rows_with_another_sweep_count": int((it != twin[2]).sum()),
          "couple_kernel": _events(lambda: D.ovo_couple(dec, A_d, B_d), a.kreps),
          "couple_kernel_no_label": _events(lambda: D.ovo_couple(dec, A_d, B_d, want_label=False), a.kreps),
          "host_twin_all_threads": _spread(th), "host_twin_one_thread": _spread(t1),
          "cross_kernel": _events(lambda: D.rbf_gram(Xq, nq, dm["Xs"], dm["ns"], gamma), a.kreps),
          "ovo_predict_device": _events(lambda: D.ovo_predict(dm["Xs"], dm["ns"], Xq, nq, gamma, dm["start"], dm["coef"],
                                                              dm["rho"]), a.kreps)}
    t = []
    for _ in range(7):
        t0 = time.perf_counter()
        p = model.predict_proba(Xt)
        t.append((time.perf_counter() - t0) * 1e3)
    cp["predict_proba_end_to_end"] = _spread(t[2:])
    cp["argmax_equals_vote_share"] = float(np.mean(model.classes_[p.argmax(1)] == model.predict(Xt)))
    cp["accuracy_argmax"] = float(np.mean(model.classes_[p.argmax(1)] == te.labels))
    out["couple"] = cp
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
