#!/usr/bin/env python3
"""The Newton polish step (decomp_newton.h) alone on the device against its host reference: a working set
of m synthetic-MNIST points (the solver's RBF, gamma 0.00125) with exactly nf of them free, the rest at 0 or
C (the tests' case builder, tests/decomp_checks.py: a step cut at a bound).
Prints bit-identity with the reference, the step's code, the mean time per step and its phases."""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from decomp_checks import NEWTON_C, newton_case  # noqa: E402
from svm355 import _native as N  # noqa: E402
from svm355.ops import device as D  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--threads", type=int, default=256, choices=[64, 128, 256, 512],
                help="the probe's workgroup size (the inner solve's shapes)")
ap.add_argument("--kind", default="cut", choices=["cut", "full"], help="the case: cut at a bound, or a full step")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

for m, nf in [(700, 339), (1024, 500), (400, 100)]:
    c = newton_case(m, nf, args.kind)
    ar, fr, cr = N.newton_step_probe(c.K, c.y, c.a, c.f, C=NEWTON_C)
    ad, fd, cd, prof, ms = D.decomp_newton_probe(c.K, c.y, c.a, c.f, C=NEWTON_C, reps=args.reps, threads=args.threads)
    ph = np.diff(np.r_[prof[7], prof[:6]]) / 100.0  # 100 MHz ticks -> us
    print(f"m={m} nf={int(prof[6])} (asked {nf}) threads={args.threads}: code {cd} (ref {cr})  "
          f"alpha bit-identical {np.array_equal(ad, ar)}  "
          f"f bit-identical {np.array_equal(fd, fr)}  {ms * 1e3:.1f} us/step  phases us: free {ph[0]:.1f} "
          f"K_FF {ph[1]:.1f} chol {ph[2]:.1f} (row updates {prof[8] / 100:.1f} block {prof[9] / 100:.1f} "
          f"solve+store {prof[10] / 100:.1f} staging {prof[11] / 100:.1f}) backsub {ph[3]:.1f} step {ph[4]:.1f} "
          f"f {ph[5]:.1f}", flush=True)
