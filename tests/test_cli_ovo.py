"""``python -m svm355 multiclass --scheme ovr|ovo`` (CPU): the one-vs-one run and its JSON; the default scheme's
output is what it was without the flag."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _run(args, check=True):
    env = dict(os.environ, MASTER_PORT=str(29600 + os.getpid() % 300))
    r = subprocess.run([sys.executable, "-m", "svm355", "multiclass", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_ovo(tmp_path):
    js = tmp_path / "ovo.json"
    out = _run(["--scheme", "ovo", "--cpu", "--synthetic", "400,100", "--json", str(js),
                "--model-dir", str(tmp_path / "model")]).stdout
    assert "[rank 0] one-vs-one over 10 classes (45 pairs) on 1 rank(s), n = 400" in out
    assert "union SV count = " in out and "support vectors per class = [" in out
    assert "[rank 0] Test accuracy = " in out and "training time = " in out and "prediction time = " in out
    s = json.loads(js.read_text())
    assert s["scheme"] == "ovo" and len(s["rho"]) == 45 and len(s["n_iter"]) == 45 and len(s["n_support"]) == 10
    assert len(s["pairs"]) == 45 and s["pairs"][0] == [0, 1] and s["pairs"][-1] == [8, 9]
    assert sum(s["n_support"]) == s["n_sv_union"] and s["accuracy"] > 0.8
    assert all(r == "converged" for r in s["stop_reasons"])
    from svm355 import OneVsOneSVC

    m = OneVsOneSVC.load(tmp_path / "model")
    assert m.rho_.tolist() == s["rho"] and m.n_support_.tolist() == s["n_support"]


def test_cli_default_scheme_is_unchanged(tmp_path):
    """--scheme ovr is the run without the flag: the same stdout lines (but the times) and the same JSON keys and
    model."""
    outs, summaries = [], []
    for i, flag in enumerate(([], ["--scheme", "ovr"])):
        js = tmp_path / f"ovr{i}.json"
        outs.append(_run([*flag, "--cpu", "--synthetic", "300,100", "--json", str(js)]).stdout)
        summaries.append(json.loads(js.read_text()))
    assert list(summaries[0]) == list(summaries[1])
    assert "scheme" not in summaries[0]
    for key in ("n_sv_union", "n_iter", "b", "stop_reasons", "accuracy", "classes"):
        assert summaries[0][key] == summaries[1][key], key
    lines = [[l for l in o.splitlines() if "training time" not in l] for o in outs]
    assert lines[0] == lines[1] and len(lines[0]) == 3
    assert lines[0][0] == "[rank 0] one-vs-rest over 10 classes on 1 rank(s), n = 300"


def test_cli_ovo_refuses_several_gpus_and_pairwise_solvers():
    r = _run(["--scheme", "ovo", "--cpu", "--synthetic", "100,10", "--gpus", "2"], check=False)
    assert r.returncode == 2 and "--gpus > 1 is not supported" in r.stderr
    r = _run(["--scheme", "ovo", "--cpu", "--synthetic", "100,10", "--solver", "batched"], check=False)
    assert r.returncode == 2 and "decomposition solver" in r.stderr
