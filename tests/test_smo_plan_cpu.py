"""The pairwise SMO drivers' shape rule (csrc/include/smo_plan.h: SmoKnobs, plan_smo, plan_rc) through the CPU
library's svm_smo_plan.  Every shape of the pairwise solver follows the same trajectory by design, so the GPU
tests cannot tell a driver that picks another shape from one that does not: it would only fit slower.  The
rule is integer arithmetic; the values here are what the driver did before it was split into smo_plan.h (its
grid function and decision blocks, run stand-alone on the same table)."""
import pytest

from svm355 import _native as N

KNOBS = ["SVM355_SMO", "SVM355_SMO_SINGLE_MAX", "SVM355_SMO_SINGLE_NT", "SVM355_PSMO_WG", "SVM355_PSMO_NT",
         "SVM355_PSMO_XCD", "SVM355_PSMO_LDS", "SVM355_PSMO_REG_US", "SVM355_PSMO_STAMP", "SVM355_PSMO_STAMP_FROM",
         "SVM355_WARM_U", "SVM355_SMO_MULTI", "SVM355_SMO_MULTI_DEBUG", "SVM355_RC_SMO", "SVM355_RC_MAXG",
         "SVM355_RC_VERBOSE"]


@pytest.fixture
def env(monkeypatch):
    """The environment without any of the drivers' knobs; env(NAME=value, ...) sets some."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
    return set_


def smo(n, wss=1):
    s, _ = N.smo_plan(n, wss=wss)
    return (s["path"], s["NT"], s["E"], s["G"], s["xlocal"]) if s["path"] != "graph" else ("graph",)


def rc(n, **kw):
    _, r = N.smo_plan(n, **kw)
    return r and (r["E"], r["G"], r["rpl"])


@pytest.mark.parametrize("n,plan", [
    (900, ("single", 512, 2, 1, False)),
    (2048, ("single", 512, 4, 1, False)),
    (2049, ("persistent", 256, 1, 9, True)),
    (9000, ("persistent", 256, 2, 18, True)),
    (16000, ("persistent", 256, 2, 32, True)),
    (16001, ("persistent", 512, 1, 32, True)),
    (20000, ("persistent", 512, 2, 20, True)),
    (60000, ("persistent", 512, 4, 30, True)),
    (65536, ("persistent", 512, 4, 32, True)),
    (65537, ("persistent", 512, 4, 33, False)),
    (70000, ("persistent", 512, 4, 35, False)),
])
def test_resident_default_shapes(env, n, plan):
    assert smo(n) == plan


def test_resident_knobs(env):
    env(SVM355_PSMO_XCD=0)
    assert smo(20000) == ("persistent", 512, 1, 40, False)
    env(SVM355_PSMO_XCD=1)  # forced on beyond its default limit: E = 8 is the 512-thread kernels' last
    assert smo(70000) == ("persistent", 512, 8, 18, True)


def test_single_mode_stops_at_8192(env):
    env(SVM355_SMO="single")
    assert smo(3000) == ("single", 512, 8, 1, False)
    assert smo(7000) == ("single", 512, 16, 1, False)
    assert smo(8192) == ("single", 512, 16, 1, False)
    assert smo(9000) == ("persistent", 256, 2, 18, True)
    env(SVM355_SMO_SINGLE_NT=256)
    assert smo(8192) == ("single", 256, 32, 1, False)
    env(SVM355_SMO_SINGLE_NT=300)  # not a workgroup size: 512
    assert smo(3000) == ("single", 512, 8, 1, False)


def test_single_max_moves_the_auto_threshold(env):
    env(SVM355_SMO_SINGLE_MAX=5000)
    assert smo(5000) == ("single", 512, 16, 1, False)
    assert smo(5001)[0] == "persistent"
    env(SVM355_SMO_SINGLE_MAX=100000)  # the kernels still stop at 8,192
    assert smo(8193)[0] == "persistent"


@pytest.mark.parametrize("n", [900, 20000, 70000])
def test_graph_mode_is_for_first_order_only(env, n):
    env(SVM355_SMO="graph")
    assert smo(n) == ("graph",)
    assert smo(n, wss=2)[0] == "persistent"


def test_second_order_is_never_single(env):
    assert smo(900, wss=2) == ("persistent", 256, 1, 4, True)
    env(SVM355_SMO="single")
    assert smo(900, wss=2) == ("persistent", 256, 1, 4, True)


def test_any_other_mode_means_persistent(env):
    for mode in ("persistent", "1", "xcd"):
        env(SVM355_SMO=mode)
        assert smo(900) == ("persistent", 256, 1, 4, True)
    env(SVM355_SMO="auto")
    assert smo(900) == ("single", 512, 2, 1, False)


@pytest.mark.parametrize("n,plan", [(9000, ("persistent", 512, 1, 18, True)), (20000, ("persistent", 512, 2, 20, True))])
def test_invalid_thread_count_is_512(env, n, plan):
    env(SVM355_PSMO_NT=300)  # and, being set, it overrides "256 threads up to 16,000 points"
    assert smo(n) == plan


def test_set_thread_count_overrides_the_size_rule(env):
    env(SVM355_PSMO_NT=1024)
    assert smo(9000) == ("persistent", 1024, 1, 9, True)
    env(SVM355_PSMO_NT=256)
    assert smo(60000) == ("persistent", 256, 8, 30, True)


def test_workgroup_target(env):
    env(SVM355_SMO="persistent", SVM355_PSMO_WG=3)
    assert smo(900) == ("persistent", 256, 2, 2, True)
    env(SVM355_PSMO_WG=1)
    assert smo(900) == ("persistent", 256, 4, 1, True)
    env(SVM355_PSMO_WG=0)  # clamped to 1
    assert smo(900) == ("persistent", 256, 4, 1, True)
    env(SVM355_PSMO_WG=1000, SVM355_PSMO_XCD=0)  # clamped to 64
    assert smo(70000) == ("persistent", 512, 4, 35, False)


def test_no_persistent_shape_leaves_the_graph(env):
    # 64 workgroups x 512 threads x 8 points = 262,144
    assert smo(262144) == ("persistent", 512, 8, 64, False)
    assert smo(262145) == ("graph",)
    assert smo(262145, wss=2) == ("graph",)  # which run_smo refuses: second order has no graph solver


def test_device_wide_replan_of_the_xcd_fallback(env):
    s, _ = N.smo_plan(20000)
    assert (s["NT"], s["E"], s["G"], s["xlocal"]) == (512, 2, 20, True) and s["device_wide"] == (512, 1, 40)
    s, _ = N.smo_plan(9000)
    assert (s["NT"], s["E"], s["G"]) == (256, 2, 18) and s["device_wide"] == (512, 1, 18)
    s, _ = N.smo_plan(60000)
    assert s["device_wide"] == (512, 2, 59)
    env(SVM355_PSMO_XCD=1)
    s, _ = N.smo_plan(300000)  # fits one XCD's 32 x 512 x 8? no: 300,000 > 131,072, and no device-wide shape either
    assert s["path"] == "graph" and s["device_wide"] is None


@pytest.mark.parametrize("n,plan", [
    (2500, (1, 5, 1)),
    (40000, (2, 40, 1)),
    (70000, (4, 35, 1)),
    (250000, (4, 123, 2)),  # the shape docs/DESIGN.md reports
    (1048576, (8, 256, 4)),
    (1048577, None),
])
def test_row_cache_default_shapes(env, n, plan):
    assert rc(n) == plan


def test_row_cache_team_width(env):
    env(SVM355_RC_MAXG=128)
    assert rc(70000) == (2, 69, 2)
    env(SVM355_RC_MAXG=256)
    assert rc(70000) == (1, 137, 4)
    env(SVM355_RC_MAXG=1000)  # clamped to 256
    assert rc(70000) == (1, 137, 4)
    env(SVM355_RC_MAXG=8)  # clamped to 64
    assert rc(70000) == (4, 35, 1)


def test_row_cache_cu_count_caps_the_team(env):
    assert rc(70000, ncu=100) == (4, 35, 1)  # 35 workgroups fit either way
    assert rc(250000, ncu=100) == (8, 62, 1)  # 123 do not fit 100 CUs: twice the points per thread
    env(SVM355_RC_MAXG=128)
    assert rc(70000, ncu=100) == (2, 69, 2)  # 137 x E=1 does not fit, 69 x E=2 does


@pytest.mark.parametrize("n", [2500, 70000, 250000])
def test_row_cache_not_applicable(env, n):
    assert rc(n, wss=2, int_rows=False) is None  # second order: exact-integer rows only
    assert rc(n, wss=2, int_rows=True) is not None
    assert rc(n, kq=4160) is None  # more than 4,096 quantised columns
    assert rc(n, kq=4096) is not None
    assert rc(n, kq=4160, int_rows=False) is not None  # FP64 rows: no such limit
    assert rc(n, nslots=3) is None  # fewer than 4 directory slots
    assert rc(n, nslots=5) is not None
    env(SVM355_RC_SMO="graph")
    assert rc(n) is None


def test_row_cache_directory(env):
    _, r = N.smo_plan(2500, nslots=64)
    assert (r["nd"], r["lds"]) == (64, 288)
    _, r = N.smo_plan(2500, nslots=65)  # an even count
    assert (r["nd"], r["lds"]) == (64, 288)
    _, r = N.smo_plan(250000, nslots=100000)  # at most 16,384 slots: 64 KB of tags + 8 KB of MRU bits
    assert (r["nd"], r["lds"]) == (16384, 73728)
