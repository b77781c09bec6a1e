"""SHA-256 digests of what the five estimators fit on a GPU, to compare two versions of the Python layer on the
same device: every digest must match (profiles/model_plumbing.md).

Rows, labels, query rows, C, gamma and the seed are those of the one-vs-one fixture tests/golden/ovo_n300_seed41.npz
(n = 300, k = 3, d = 16; the first 50 of its query rows).  Each estimator is fitted on three forms of the rows:
the bytes, the same values as FP64 (which quantise into the bytes' integers), and real-valued FP64 rows (the
bytes plus a fixed fraction: no exact-integer plan, the FP64-MFMA kernel values).  SVC is fitted plain, with
probability=True / cv=3, and by the pairwise solver; OneVsRestSVC by the decomposition and the batched solver;
OneVsOneSVC with cv=3.

    python scripts/model_plumbing_digests.py [--out digests.json]
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SEED, CV, QUERIES = 41, 3, 50


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args()
    from svm355 import SVC, SVR, OneClassSVM, OneVsOneSVC, OneVsRestSVC

    g = np.load(ROOT / "tests" / "golden" / f"ovo_n300_seed{SEED}.npz")
    X8, labels, Xq8, C, gamma = g["X"], g["labels"], g["Xt"][:QUERIES], float(g["C"]), float(g["gamma"])
    assert X8.dtype == np.uint8 and X8.shape[0] == 300
    frac = np.random.default_rng(SEED).random(X8.shape[1]) * 0.5  # a fixed fraction per column
    forms = {"u8": (X8, Xq8), "f64": (X8.astype(np.float64), Xq8.astype(np.float64)),
             "real": (X8 + frac, Xq8 + frac)}
    y = np.where(labels == np.unique(labels)[0], 1, -1).astype(np.int32)
    z = np.sin(X8[:, 0] / 40.0) + 0.5 * y
    kw = dict(C=C, gamma=gamma, device=a.device)
    out = {}
    for form, (X, Xq) in forms.items():
        def put(name, **fields):
            for k, v in fields.items():
                out[f"{form}.{name}.{k}"] = digest(*v) if isinstance(v, tuple) else digest(v)

        for name, m in (("svc", SVC(**kw)), ("svc_smo", SVC(solver="smo", **kw)),
                        ("svc_proba", SVC(probability=True, cv=CV, cv_seed=SEED, **kw))):
            m.fit(X, y)
            put(name, alpha=m.alpha_, support=m.support_, b=np.float64(m.b_), decision=m.decision_function(Xq),
                sv=m.support_vectors_)
            if m.probability:
                put(name, prob=(np.float64(m.probA_), np.float64(m.probB_)), cv_decision=m.cv_decision_,
                    proba=m.predict_proba(Xq))
        m = SVR(epsilon=0.1, **kw).fit(X, z)
        put("svr", dual_coef=m.dual_coef_, support=m.support_, b=np.float64(m.b_), decision=m.predict(Xq),
            sv=m.support_vectors_)
        m = OneClassSVM(nu=0.3, gamma=gamma, device=a.device).fit(X)
        put("oneclass", dual_coef=m.dual_coef_, support=m.support_, rho=np.float64(m.rho_),
            decision=m.decision_function(Xq), sv=m.support_vectors_)
        for name, m in (("ovr", OneVsRestSVC(**kw)), ("ovr_batched", OneVsRestSVC(solver="batched", **kw))):
            m.fit(X, labels)
            put(name, dual_coef=m.dual_coef_, support=m.support_, b=m.intercepts_b_,
                decision=m.decision_function(Xq), sv=m._host_sv_rows())
        m = OneVsOneSVC(cv=CV, cv_seed=SEED, **kw).fit(X, labels)
        put("ovo", dual_coef=m.dual_coef_, support=m.support_, rho=m.rho_, prob=(m.probA_, m.probB_),
            cv_decision=m.cv_decision_, decision=m.decision_function(Xq), proba=m.predict_proba(Xq),
            sv=m._host_sv_rows())
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
