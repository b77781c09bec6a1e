"""One Newton polish step on the device (newton_wg through ws_newton_probe_kernel, csrc/hip/decomp_inner.hip)
against its sequential host reference (newton_step_ref, decomp_newton.h), bit for bit, at the free-set sizes
where the kernel's blocking changes: the 2-point minimum, the 16-column panel and 64-column block boundaries,
the cap of 512 free points, and in workgroups of 64, 128, 256 and 512 threads (the inner solve's shapes).

The cases (decomp_checks.newton_case) have exactly the free count asked for.  The reference itself is checked
against plain mathematics on the CPU (test_decomp_oracle_cpu.py), on the same cases."""
import numpy as np
import pytest

from svm355 import _native as N
from svm355.ops import device as D

from decomp_checks import (NEWTON_C, NEWTON_CAP, NEWTON_SIZES, NEWTON_SIZES_ABOVE_CAP, NEWTON_SIZES_EVERY_NT,
                           newton_case)

pytestmark = pytest.mark.gpu

MATRIX = ([(m, nf, 256) for m, nf in NEWTON_SIZES]
          + [(m, nf, nt) for nt in (64, 128, 512) for m, nf in NEWTON_SIZES_EVERY_NT])


def _both(case, threads=256, **kw):
    """The step on both sides from the same inputs: ((alpha, f, code) of the reference, of the device, prof)."""
    ar, fr, cr = N.newton_step_probe(case.K, case.y, case.a, case.f, C=NEWTON_C, **kw)
    ad, fd, cd, prof, _ = D.decomp_newton_probe(case.K, case.y, case.a, case.f, C=NEWTON_C, threads=threads, **kw)
    return (ar, fr, cr), (ad, fd, cd), prof


def _assert_same_step(case, ref, dev, prof, nf, what):
    (ar, fr, cr), (ad, fd, cd) = ref, dev
    assert cd == cr, f"{what}: device code {cd}, reference {cr}"
    assert np.array_equal(ad, ar), f"{what}: alpha differs at {np.flatnonzero(ad != ar)[:8]}"
    assert np.array_equal(fd, fr), f"{what}: f differs at {np.flatnonzero(fd != fr)[:8]}"
    assert int(prof[6]) == nf, f"{what}: the device saw |F| = {int(prof[6])}"
    bound = np.ones(len(case.a), dtype=bool)
    bound[case.free] = False
    assert np.array_equal(ad[bound], case.a[bound]), f"{what}: a non-free alpha moved"


def _assert_refused(case, ref, dev, what):
    for side, (a, f, code) in (("reference", ref), ("device", dev)):
        assert code == 0, f"{what}: {side} code {code}"
        assert np.array_equal(a, case.a) and np.array_equal(f, case.f), f"{what}: {side} changed alpha or f"


@pytest.mark.parametrize("kind", ["full", "cut"])
@pytest.mark.parametrize("m,nf,threads", MATRIX)
def test_step_is_the_references_bit_for_bit(m, nf, threads, kind):
    case = newton_case(m, nf, kind)
    ref, dev, prof = _both(case, threads)
    # what the case was built for: the full step inside the box; a step cut at a bound from 3 free points
    assert ref[2] == (1 if kind == "full" or nf == 2 else 2)
    _assert_same_step(case, ref, dev, prof, nf, f"m={m} |F|={nf} {kind} threads={threads}")


@pytest.mark.parametrize("threads", [64, 256, 512])
@pytest.mark.parametrize("m,nf", [(64, 17), (600, 257), (1024, 512)])
@pytest.mark.parametrize("where", [0, -1])
def test_cut_at_the_first_and_the_last_free_position(m, nf, where, threads):
    """The step's arg-min (value, then lowest position) crosses threads and waves: the cut is forced at the
    first and at the last free position by an alpha within 1e-9 of the bound it heads for.  Ties are not
    tested: two bound ratios (C - a_k) / d_k that are exactly equal cannot be constructed in floating point
    from a d that comes out of the factorisation."""
    case = newton_case(m, nf, "cut", cut_at=where)
    ref, dev, prof = _both(case, threads)
    k = case.free[where]
    assert ref[2] == 2 and ref[0][k] in (0.0, NEWTON_C) and abs(ref[0][k] - case.a[k]) < 1e-8
    others = np.delete(case.free, where % nf)
    assert np.all((ref[0][others] > 0.0) & (ref[0][others] < NEWTON_C))
    _assert_same_step(case, ref, dev, prof, nf, f"m={m} |F|={nf} cut at F[{where}] threads={threads}")


@pytest.mark.parametrize("max_free", [1024, None])
@pytest.mark.parametrize("kind", ["full", "cut"])
@pytest.mark.parametrize("m,nf", NEWTON_SIZES_ABOVE_CAP)
def test_no_step_above_the_cap_on_either_side(m, nf, kind, max_free):
    """More than kNewtonMaxFree = 512 free points: no step, on the device (its LDS buffers) and in the
    reference (the same cap), whatever max_free asks for."""
    assert nf > NEWTON_CAP
    case = newton_case(m, nf, kind)
    ref, dev, _ = _both(case, **({} if max_free is None else {"max_free": max_free}))
    _assert_refused(case, ref, dev, f"m={m} |F|={nf} {kind} max_free={max_free}")


def test_max_free_below_the_cap():
    case = newton_case(300, 129, "cut")
    ref, dev, _ = _both(case, max_free=128)
    _assert_refused(case, ref, dev, "|F|=129 max_free=128")
    ref, dev, prof = _both(case, max_free=129)
    assert ref[2] == 2
    _assert_same_step(case, ref, dev, prof, 129, "|F|=129 max_free=129")


@pytest.mark.parametrize("dup", [(0, 1), (15, 16), (200, 299)])
def test_singular_free_block_is_refused(dup):
    """A free point duplicated onto another (K_FF singular: the second one's pivot is rounding, below the
    1e-12 refusal): inside the first panel, across the first panel boundary, in the last partial panel."""
    case = newton_case(300, 300, "cut", dup=dup)
    ref, dev, _ = _both(case)
    _assert_refused(case, ref, dev, f"duplicate {dup}")


@pytest.mark.parametrize("nf", [0, 1])
def test_fewer_than_two_free_points_is_refused(nf):
    case = newton_case(40, nf, "cut")
    ref, dev, _ = _both(case)
    _assert_refused(case, ref, dev, f"|F|={nf}")


def test_unbuilt_thread_count_is_an_argument_error():
    case = newton_case(64, 17, "full")
    for threads in (0, 192, 1024):
        with pytest.raises(N.NativeError, match="threads"):
            D.decomp_newton_probe(case.K, case.y, case.a, case.f, C=NEWTON_C, threads=threads)
