// Pairwise SMO drivers (hip/smo.hip, hip/rowcache.hip): the environment switches they read and the rule
// that picks a solver and its launch shape from the problem size.  Host-only integer arithmetic with no HIP
// headers, so the CPU library exports it (svm_smo_plan, core/smo_plan.cpp) and the CPU tests pin it: every
// shape follows the same trajectory by design, so a wrong shape shows only as a slower fit.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace svm355 {

// Shape constants host and device must agree on (smo.hip static_asserts the first two against persist.h).
constexpr int kPlanMaxG = 64;                    // persist.h kMaxG: records of one sweep pass
constexpr uint32_t kPlanSentinel = 0x7FFFFFFFu;  // persist.h kSentinel: n must stay below it
constexpr int kRcMaxG = 256;                     // records per epoch parity of the row-cache solver's slot array

constexpr int kDefaultNT = 512;
constexpr int kXcdMaxG = 32;                 // workgroups of the XCD-local solver (one XCD has 32 CUs)
constexpr int64_t kXcdDefaultMax = 65536;    // default n limit of the XCD-local solver (tuned on MI355X)
constexpr int64_t kSingleDefaultMax = 2048;  // auto mode: single workgroup up to this n (tuned on MI355X)
constexpr int64_t kSingleLimit = 8192;       // largest n the single-workgroup kernels are instantiated for
constexpr int kSingleDefaultNT = 512;

// Every environment switch a pairwise solve reads (docs/KNOBS.md), parsed at the top of each solve and
// never kept between solves: the tests change them between fits of one process.
struct SmoKnobs {
  enum Mode { kAuto, kSingle, kGraph, kPersistent };
  Mode mode = kAuto;                     // SVM355_SMO = auto | single | graph; anything else: persistent
  int64_t single_max = kSingleDefaultMax;  // _SMO_SINGLE_MAX
  int single_nt = kSingleDefaultNT;      // _SMO_SINGLE_NT = 256 | 512 | 1024 (else 512)
  int wg = 64;                           // _PSMO_WG: target workgroups, 1..kPlanMaxG
  int nt = 0;                            // _PSMO_NT = 256 | 512 | 1024 (set but else: 512); 0: not set, by size
  int xcd = -1;                          // _PSMO_XCD: 1 / 0 forces the XCD-local exchange on / off; -1: by size
  int64_t lds_pad = -1;                  // _PSMO_LDS: bytes of unused LDS of an XCD-local launch; < 0: default
  unsigned long long reg_ticks = 0;      // _PSMO_REG_US in 10 ns ticks; 0: the kernel's default window
  int stamp = 0;                         // _PSMO_STAMP: nonzero = phase stamps, 2 = and the exchange skew
  unsigned long long stamp_from = 0;     // _PSMO_STAMP_FROM: first stamped epoch (row cache); 0: the default
  int warm_u = 16;                       // _WARM_U = 8 | 16 | 32 (else 16): warm-start f kernel unroll
  bool multi = true, multi_debug = false;  // _SMO_MULTI=0: no batched one-vs-rest; _SMO_MULTI_DEBUG
  bool rc_graph = false, rc_verbose = false;  // _RC_SMO=graph, _RC_VERBOSE
  int rc_maxg = 64;                      // _RC_MAXG: first team width tried, 64..kRcMaxG
};

inline SmoKnobs read_smo_knobs() {
  SmoKnobs k;
  auto valid_nt = [](int nt, int fallback) { return nt == 256 || nt == 512 || nt == 1024 ? nt : fallback; };
  auto flag = [](const char* name) {
    const char* v = getenv(name);
    return v && atoi(v);
  };
  if (const char* m = getenv("SVM355_SMO"))
    k.mode = !strcmp(m, "auto")     ? SmoKnobs::kAuto
             : !strcmp(m, "single") ? SmoKnobs::kSingle
             : !strcmp(m, "graph")  ? SmoKnobs::kGraph
                                    : SmoKnobs::kPersistent;
  if (const char* v = getenv("SVM355_SMO_SINGLE_MAX")) k.single_max = atoll(v);
  if (const char* v = getenv("SVM355_SMO_SINGLE_NT")) k.single_nt = valid_nt(atoi(v), kSingleDefaultNT);
  if (const char* v = getenv("SVM355_PSMO_WG")) k.wg = std::max(1, std::min(kPlanMaxG, atoi(v)));
  if (const char* v = getenv("SVM355_PSMO_NT")) k.nt = valid_nt(atoi(v), kDefaultNT);
  if (const char* v = getenv("SVM355_PSMO_XCD")) k.xcd = atoi(v) != 0;
  if (const char* v = getenv("SVM355_PSMO_LDS")) k.lds_pad = std::max(0, atoi(v));
  if (const char* v = getenv("SVM355_PSMO_REG_US")) k.reg_ticks = std::max(1ull, strtoull(v, nullptr, 10)) * 100ull;
  if (const char* v = getenv("SVM355_PSMO_STAMP")) k.stamp = atoi(v);
  if (const char* v = getenv("SVM355_PSMO_STAMP_FROM")) k.stamp_from = (unsigned long long)std::max(1ll, atoll(v));
  if (const char* v = getenv("SVM355_WARM_U")) k.warm_u = atoi(v);
  if (const char* v = getenv("SVM355_SMO_MULTI")) k.multi = atoi(v) != 0;
  k.multi_debug = flag("SVM355_SMO_MULTI_DEBUG");
  if (const char* m = getenv("SVM355_RC_SMO")) k.rc_graph = !strcmp(m, "graph");
  k.rc_verbose = flag("SVM355_RC_VERBOSE");
  if (const char* v = getenv("SVM355_RC_MAXG")) k.rc_maxg = std::max(64, std::min(kRcMaxG, atoi(v)));
  return k;
}

// ---- resident Gram -------------------------------------------------------------------------------------
struct SmoPlan {
  enum Path { kSingle, kPersistent, kGraph };
  Path path = kGraph;      // kGraph is also "no persistent shape": wss = 2 has no graph solver (run_smo refuses)
  int NT = 0, E = 0, G = 0;  // threads per workgroup, points per thread, workgroups (kGraph: unused)
  bool xlocal = false;     // kPersistent: records exchanged through one XCD's L2
};

// Grid shape of the persistent solver: NT threads per workgroup (_PSMO_NT, default kDefaultNT), the smallest
// E in {1, 2, 4, 8, 16} (capped per NT) with G = ceil(n / (NT*E)) <= target workgroups (_PSMO_WG, default 64;
// all co-resident, one sweep pass).  gcap > 0: the XCD-local solver's cap on G.  False: no shape covers n.
inline bool plan_smo_grid(int64_t n, int gcap, const SmoKnobs& k, SmoPlan* out) {
  int target = k.wg;
  if (gcap > 0) target = std::min(target, gcap);
  // Measured on MI355X (profiles/r1_smo_launch_shape.txt): the XCD-local solver wants 256-thread
  // workgroups up to ~16k points and 512-thread ones above, one per CU (xcd_lds_pad): 2.45-3.44
  // us/iter from 10k to 60k, 4-17 % below the device-wide exchange.
  int nt = kDefaultNT;
  if (gcap > 0 && n <= 16000) nt = 256;
  if (k.nt) nt = k.nt;
  const int emax = nt == 256 ? 16 : nt == 512 ? 8 : 4;
  for (int E = 1; E <= emax; E *= 2) {
    const int64_t per_wg = int64_t(nt) * E;
    const int64_t G = (n + per_wg - 1) / per_wg;
    if (G <= target) {
      out->G = int(std::max<int64_t>(1, G));
      out->E = E;
      out->NT = nt;
      return true;
    }
  }
  return false;
}

// The device-wide shape the persistent solver falls back to when its XCD-local team cannot form.
inline bool replan_smo_device_wide(int64_t n, const SmoKnobs& k, SmoPlan* plan) {
  plan->xlocal = false;
  return plan_smo_grid(n, 0, k, plan);
}

inline SmoPlan plan_smo(int64_t n, int wss, const SmoKnobs& k) {
  SmoPlan pl;
  // Second-order selection (wss == 2, opt-in) exists in the persistent solver only.
  const bool wss2 = wss == 2;
  // Single-workgroup solver for small problems (no cross-workgroup exchange).
  const bool force_single = k.mode == SmoKnobs::kSingle;
  if (!wss2 && (force_single || k.mode == SmoKnobs::kAuto) && (force_single || n <= k.single_max) &&
      n <= kSingleLimit) {
    pl.path = SmoPlan::kSingle;
    pl.NT = k.single_nt;
    pl.E = 1;
    while (int64_t(pl.NT) * pl.E < n) pl.E *= 2;
    pl.G = 1;
    return pl;
  }
  const bool want_persistent = wss2 || k.mode != SmoKnobs::kGraph;
  // XCD-local exchange (all workgroups on one XCD, records through its L2): _PSMO_XCD=1/0 forces it on/off;
  // the default enables it up to kXcdDefaultMax points.
  pl.xlocal = k.xcd >= 0 ? k.xcd != 0 : n <= kXcdDefaultMax;
  if (want_persistent && n < int64_t(kPlanSentinel) && plan_smo_grid(n, pl.xlocal ? kXcdMaxG : 0, k, &pl)) {
    pl.path = SmoPlan::kPersistent;
    return pl;
  }
  pl.xlocal = false;
  return pl;
}

// ---- row cache -----------------------------------------------------------------------------------------
struct RcPlan {
  bool ok = false;   // false: no persistent shape (the caller replays its select / step graph)
  int E = 0, G = 0;  // points per thread of a 512-thread workgroup, workgroups
  int rpl = 0;       // records per sweep lane: 1, 2 or 4
  int64_t nd = 0;    // directory slots held in LDS
  size_t lds = 0;    // dynamic LDS bytes of the directory
};

// Shape: up to 8 register-resident points per thread (E = 16 needs more than 256 VGPRs and spills) and one
// 512-thread workgroup per CU, all co-resident.  Teams of up to 64 workgroups (one record per sweep lane)
// with E <= 4, then 128 and 256 (two / four records per lane, capped by the CU count) with E <= 8: n <= 256
// x 512 x 8 = 1,048,576.  Measured (profiles/r2_rowcache_persistent.txt): at 60k 59 x E=2 beats 118 x E=1
// (98 vs 104 ms); at 250k 123 x E=4 beats 62 x E=8 (465 vs 572 ms: half the miss fill per workgroup);
// 256-wide teams lose to 128 wherever both fit.  _RC_MAXG=128|256 starts at a wider team.  Larger n keep
// the replayed select / step graph.
inline RcPlan plan_rc(int64_t n, int ncu, bool int_rows, int kq, int wss, int64_t nslots, const SmoKnobs& k) {
  RcPlan pl;
  if (k.rc_graph) return pl;
  if (n <= 0 || n >= int64_t(kPlanSentinel)) return pl;
  if (int_rows && kq > 32 * 128) return pl;  // CachedRows::k12: two k-steps per lane
  if (wss == 2 && !int_rows) return pl;      // second order: exact-integer rows only
  int E = 0;
  for (int cap = k.rc_maxg; cap <= kRcMaxG && !E; cap *= 2) {
    const int maxg = std::min(cap, ncu);
    for (int e = 1; e <= (cap == 64 ? 4 : 8) && !E; e *= 2)
      if ((n + 512 * e - 1) / (512 * e) <= maxg) E = e;
  }
  if (!E) return pl;
  pl.E = E;
  pl.G = int((n + 512 * E - 1) / (512 * E));
  pl.rpl = pl.G <= 64 ? 1 : pl.G <= 128 ? 2 : 4;
  // Directory in LDS: up to 16384 slots (64 KB of tags + 8 KB of MRU bits) next to PersistShared.
  pl.nd = std::min<int64_t>(nslots, 16384) / 2 * 2;
  if (pl.nd < 4) return pl;
  pl.lds = (size_t(pl.nd) * 4 + size_t(pl.nd) / 2 + 15) / 16 * 16;
  pl.ok = true;
  return pl;
}

}  // namespace svm355
