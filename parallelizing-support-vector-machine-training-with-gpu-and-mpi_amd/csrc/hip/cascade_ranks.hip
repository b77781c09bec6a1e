// Who runs the device cascade and the distributed decomposition: thread-rank groups, process ranks and their
// C ABI.  The backend is cascade_dev.hip's, the RCCL transport rccl_transport.hip's; no device code here.
//   svmd_cascade_group_* : P thread-ranks over P GPUs of this process (ncclCommInitAll) or a
//                          loopback rehearsal; GroupRun is one fit's set-up and its failure handling;
//   svmd_cascade_rank_*  : one rank per process (ncclCommInitRank with an id the launcher distributes, e.g.
//                          torchrun + a TCP store, or the caller's host collectives); ProcRank::guarded is
//                          its failure handling.
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>

#include "cascade_capi.h"
#include "cascade_dev.h"
#include "decomp.h"

namespace svm355 {
namespace {

// ------------------------------------------------------------------------- thread-rank group
struct Group {
  int world = 0;
  bool rccl = false;
  bool broken = false;
  double timeout_s = 600.0;
  std::vector<int> devices;
  std::vector<std::unique_ptr<HipBackend>> be;
  std::vector<ncclComm_t> comms;
  std::vector<std::unique_ptr<RcclTransport>> rtr;  // persistent (pinned / device scratch)
  std::unique_ptr<RankPool> pool;                   // one persistent host thread per rank
  std::mutex mu;  // one fit at a time
  // loopback rehearsal with SVM355_CASCADE_SERIAL_SOLVES=1: the distributed decomposition's per-rank
  // solo segment times (DecompSolo) and their summary (svmd_cascade_group_decomp_solo)
  std::mutex solo_mu;
  std::vector<double> solo_report;
  std::vector<double> host_wait_ms;  // the last distributed decomposition fit's per-rank host wait
};

// One fit (or exercise) of a group: a fresh abort token and wait policy, and per rank the persistent RCCL
// transport under that policy or a fresh loopback transport on a fresh LoopbackGroup.
class GroupRun {
 public:
  GroupRun(Group& g, double timeout_s) : g_(g), token_(std::make_shared<AbortToken>()), wp_{token_, timeout_s} {
    if (!g.rccl) lg_ = std::make_shared<LoopbackGroup>(g.world, wp_);
    for (int r = 0; r < g.world; ++r) {
      if (g.rccl) {
        g.rtr[size_t(r)]->set_policy(wp_);
        tr_.push_back(g.rtr[size_t(r)].get());
      } else {
        ltr_.push_back(std::make_unique<LoopbackTransport>(lg_, r, g.be[size_t(r)].get()));
        tr_.push_back(ltr_.back().get());
      }
    }
  }
  // job(r, transport, backend) on every rank's thread, the rank's device current.  When a rank throws, the
  // pool raises the token (the others leave their waits), every rank's transport is aborted, an RCCL group
  // is broken for good (ncclCommAbort released its communicators) and the first error is rethrown.
  template <class Job>
  void run(Job&& job) {
    try {
      g_.pool->run(
          token_,
          [&](int r) {
            if (hipSetDevice(g_.devices[size_t(r)]) != hipSuccess) throw CascadeError("hipSetDevice failed");
            job(r, *tr_[size_t(r)], *g_.be[size_t(r)]);
          },
          [&](int r) {
            (void)hipSetDevice(g_.devices[size_t(r)]);
            tr_[size_t(r)]->abort();
          });
    } catch (...) {
      if (g_.rccl) g_.broken = true;
      throw;
    }
  }

 private:
  Group& g_;
  std::shared_ptr<AbortToken> token_;
  const WaitPolicy wp_;
  std::shared_ptr<LoopbackGroup> lg_;
  std::vector<std::unique_ptr<LoopbackTransport>> ltr_;
  std::vector<Transport*> tr_;
};

// ----------------------------------------------------------------------------- process rank
// tr: RCCL over the rank's communicator, or (svmd_cascade_rank_create_hostcomm) the caller's host
// collectives with device buffers staged through host memory -- the per-process launch rehearsed with
// several processes on one GPU, where RCCL refuses to run.
struct ProcRank {
  int device = 0;
  bool broken = false;
  double timeout_s = 600.0;
  std::unique_ptr<HipBackend> be;
  ncclComm_t comm = nullptr;
  std::unique_ptr<Transport> tr;
  RcclTransport* rccl = nullptr;  // tr when it is RCCL (deadline / abort policy per call)
  double host_wait_ms = 0.0;       // the last distributed decomposition fit's host wait
  void set_policy(WaitPolicy wp) {
    if (rccl) rccl->set_policy(std::move(wp));
  }
  // body() on the rank's device under a deadline of timeout_s (the policy stays set afterwards).  When it
  // throws, the communicator is aborted -- the MPI_Abort equivalent: the peers' waits fail too -- the rank
  // is broken for good and the error is rethrown.
  template <class Body>
  void guarded(double timeout_s, Body&& body) {
    (void)hipSetDevice(device);
    set_policy(WaitPolicy{nullptr, timeout_s});
    try {
      body();
    } catch (...) {
      tr->abort();
      broken = true;
      throw;
    }
  }
};

// Runs `script` (exercise.cpp) on every rank of a group; "" on success, else the first error (the
// group is then broken: its communicators were aborted).
std::string group_exercise(Group& g, const std::string& script, double timeout_s) {
  try {
    GroupRun(g, timeout_s).run([&](int, Transport& tr, HipBackend& be) { exercise_transport(tr, be, script); });
  } catch (const std::exception& e) {
    return e.what();
  }
  return "";
}

// One rank of the distributed decomposition SMO (decomp.hip): the rank's GPU gets all n rows and
// labels and runs the solve over its block range with the candidate records all-gathered through `tr`
// (null: one GPU).  u8: uint8 pixel rows (quantised on the device: exact-integer kernel values); else
// FP64 rows (n x d, the reference's format, mpi_svm_main2.cpp:316-402 / mpi_svm_main3.cpp:433-518):
// min-max scaled on the device, then the exact-integer plan when their values admit one, FP64-MFMA kernel
// values otherwise (real-valued data; decomp_fit_rows).
struct DecompIn {
  const void* X;  // host rows, n x d
  bool u8;
  const int32_t* y;
  int64_t n, d;
  const svm_params& p;
  int q;
};
struct DecompOut {  // every member may be null
  double* alpha = nullptr;  // host, n doubles
  svm_result* r = nullptr;
  int64_t* stats = nullptr;  // SVM_DECOMP_STATS int64 (decomp.h)
  double* ms = nullptr;      // the rank's wall time
  double* mm = nullptr;      // 2 d doubles: the column min / max the model's scaling uses
  DecompSolo* solo = nullptr;
  double* host_wait_ms = nullptr;
};

// One attempt: upload, statistics, solve.  False (no result written) when the solver did not take the rows.
// widen: the host bytes widened to doubles on upload and solved as FP64 rows.
bool decomp_attempt(HipBackend& be, Transport* tr, const DecompIn& in, const DecompOut& out, bool widen) {
  const auto check = &HipBackend::check;
  DeviceCtx* ctx = be.device_ctx();
  const int64_t n = in.n, d = in.d;
  const int world = tr ? tr->world() : 1, rank = tr ? tr->rank() : 0;
  // Each GPU copies 1/world of the rows from the host over its own link and the rows are all-gathered
  // over xGMI (in place), instead of every GPU pulling all n rows through the host: world concurrent
  // pageable copies of the whole set would be staged through host memory world times.
  const bool u8dev = in.u8 && !widen;  // the device rows are the host's bytes
  const int64_t ld = u8dev ? d : svmd_padded_dim(d), esz = u8dev ? 1 : 8;
  const int64_t rows_per = (n + world - 1) / world, chunk = rows_per * ld * esz;
  auto* Xd = static_cast<char*>(be.alloc(chunk * world));
  auto* yd = static_cast<int32_t*>(be.alloc(n * 4));
  auto* ad = static_cast<double*>(be.alloc(n * 8));
  auto* mm = static_cast<double*>(be.alloc(2 * d * 8));
  struct Free {
    HipBackend& b;
    std::vector<void*> ptrs;
    ~Free() {
      for (void* q : ptrs) b.free(q);
    }
  } fr{be, {Xd, yd, ad, mm}};
  const int64_t r0 = std::min<int64_t>(n, rank * rows_per), r1 = std::min<int64_t>(n, r0 + rows_per);
  const char* Xh = static_cast<const char*>(in.X);
  auto upload = [&](int64_t a0, int64_t a1, char* dst) {  // host rows [a0, a1) to the device (FP64: padded to ld)
    if (a1 <= a0) return;
    if (u8dev) {
      be.h2d(dst, Xh + a0 * d, (a1 - a0) * d);
    } else if (widen) {  // the bytes widened to doubles on the device (svmd_upload_rows_u8)
      be.upload_rows(Xh + a0 * d, true, a1 - a0, d, reinterpret_cast<double*>(dst));
    } else {
      be.upload_rows(Xh + a0 * d * 8, false, a1 - a0, d, reinterpret_cast<double*>(dst));
    }
  };
  if (world > 1) {
    upload(r0, r1, Xd + rank * chunk);
    tr->allgather(Xd + rank * chunk, chunk, Xd);  // rank r's slice at r * chunk = row r * rows_per
  } else {
    upload(0, n, Xd);
  }
  be.h2d(yd, in.y, n * 4);
  if (u8dev)
    check(svmd_minmax_u8(ctx, reinterpret_cast<uint8_t*>(Xd), n, d, mm, mm + d), "svmd_minmax_u8");
  else  // the single-GPU SVC's scaling (svmd_preprocess: column min / max, then the rows scaled in place)
    check(svmd_preprocess(ctx, reinterpret_cast<double*>(Xd), n, d, ld, mm, mm + d, nullptr, 0), "svmd_preprocess");
  std::vector<double> mmh(size_t(2 * d));
  be.d2h(mmh.data(), mm, 2 * d * 8);
  if (out.mm) std::memcpy(out.mm, mmh.data(), size_t(2 * d) * 8);
  // RCCL: the all-gather is only enqueued; the solver's one host wait per outer iteration (after the
  // working-set build that reads the gathered candidates) polls under the transport's deadline
  DecompOpts o;
  o.world = world;
  o.rank = rank;
  o.solo = out.solo;
  o.host_wait_ms = out.host_wait_ms;
  if (tr)
    o.allgather = {[tr](const void* send, int64_t bytes, void* recv) { tr->allgather_async(send, bytes, recv); },
                   [tr](void* ev) { return tr->event_wait(ev, "decomposition SMO: a batch of outer iterations"); }};
  bool used = false;
  double prep = 0.0;
  svm_result res{};
  // fault injection (tests): SVM355_DECOMP_FAIL_RANK / _OUTER make that rank fail at that outer
  // iteration inside the solve (run_decomp) while the others wait in their candidate all-gather; the
  // group's abort must end every rank with an error, not a hang
  if (u8dev)
    check(decomp_fit_u8(ctx, reinterpret_cast<uint8_t*>(Xd), n, d, mmh.data(), mmh.data() + d, yd, ad, in.p, in.q, &res,
                        out.stats, &used, &prep, o),
          "decomposition SMO");
  else
    check(decomp_fit_rows(ctx, reinterpret_cast<double*>(Xd), n, ld, d, mmh.data(), mmh.data() + d, yd, ad, in.p, in.q,
                          &res, out.stats, &used, &prep, o),
          "decomposition SMO");
  if (!used) return false;
  if (out.alpha) be.d2h(out.alpha, ad, n * 8);
  be.sync();
  if (out.r) *out.r = res;
  return true;
}

// uint8 rows whose column ranges admit no exact-integer plan within the int8 kernels' 4,096 columns (wide
// rows with many distinct ranges) are solved as FP64 rows: a second attempt with the host bytes widened to
// doubles on upload, after the first has released the byte rows' buffers -- the single-GPU SVC's fallback
// (svc.py _fit_cuda_u8 -> train_decomp_rows), taken by every rank alike (the plan is a function of the
// global min / max).  out.ms covers both attempts.
void decomp_on_rank(HipBackend& be, Transport* tr, const DecompIn& in, const DecompOut& out) {
  const auto t0 = std::chrono::steady_clock::now();
  bool used = decomp_attempt(be, tr, in, out, false);
  if (!used && in.u8 && in.n >= 2 && in.n <= (int64_t(1) << 31) - 2) used = decomp_attempt(be, tr, in, out, true);
  if (!used)
    throw CascadeError("decomposition SMO: n = " + std::to_string(in.n) + " is outside 2 .. 2^31 - 2, or the "
                       "FP64-row solve's workspace (n / world x 1,024 doubles per GPU) does not fit");
  if (out.ms) *out.ms = ms_since(t0);
}

// The critical path of P GPUs from the ranks' solo segment times: per outer iteration the slowest rank's
// selection, then the slowest rank's rest (the ranks meet at the candidate all-gather in between); exchanges
// excluded.  [critical path ms, of it selection ms, of it the rest ms, outer iterations, then per rank: its
// selection ms, its rest ms]; empty when the fit was not timed solo.
std::vector<double> solo_summary(const std::vector<DecompSolo>& solo) {
  if (solo.empty()) return {};
  size_t iters = solo[0].sel_ms.size();
  for (const auto& sr : solo) iters = std::min({iters, sr.sel_ms.size(), sr.rest_ms.size()});
  double sel = 0.0, rest = 0.0;
  for (size_t k = 0; k < iters; ++k) {
    double ms_sel = 0.0, ms_rest = 0.0;
    for (const auto& sr : solo) {
      ms_sel = std::max(ms_sel, sr.sel_ms[k]);
      ms_rest = std::max(ms_rest, sr.rest_ms[k]);
    }
    sel += ms_sel;
    rest += ms_rest;
  }
  std::vector<double> report = {sel + rest, sel, rest, double(iters)};
  for (const auto& sr : solo) {
    report.push_back(std::accumulate(sr.sel_ms.begin(), sr.sel_ms.end(), 0.0));
    report.push_back(std::accumulate(sr.rest_ms.begin(), sr.rest_ms.end(), 0.0));
  }
  return report;
}

// The first cap values of v to out; returns how many v holds.
int64_t copy_out(const std::vector<double>& v, double* out, int64_t cap) {
  std::copy_n(v.begin(), std::min<int64_t>(cap, int64_t(v.size())), out);
  return int64_t(v.size());
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" {

SVM_API int svmd_cascade_group_exercise(void* h, const char* script, double timeout_s) {
  auto* g = static_cast<Group*>(h);
  if (!g || !script) {
    set_error("svmd_cascade_group_exercise: bad arguments");
    return SVM_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->broken) {
    set_error("svmd_cascade_group_exercise: the group's communicators were aborted by an earlier failure");
    return SVM_ERR_ARG;
  }
  const std::string err = group_exercise(*g, script, timeout_s > 0 ? timeout_s : kPreflightTimeout);
  if (!err.empty()) {
    set_error("%s", err.c_str());
    return SVM_ERR_DEVICE;
  }
  return SVM_OK;
}

SVM_API int svmd_cascade_group_broken(void* h) { return h && static_cast<Group*>(h)->broken ? 1 : 0; }

SVM_API void* svmd_cascade_group_create(int32_t world, const char* transport, double comm_timeout_s) {
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    if (world < 1) throw CascadeError("world must be >= 1");
    if (ndev < 1) throw CascadeError("no HIP device visible");
    std::string tr = transport ? transport : "auto";
    if (tr == "auto") tr = world <= ndev ? "rccl" : "loopback";
    if (tr != "rccl" && tr != "loopback") throw CascadeError("transport must be auto, rccl or loopback");
    if (tr == "rccl" && world > ndev)
      throw CascadeError("rccl transport needs one GPU per rank (" + std::to_string(world) + " ranks, " +
                         std::to_string(ndev) + " GPUs visible)");
    auto g = std::make_unique<Group>();
    g->world = world;
    g->rccl = tr == "rccl";
    g->timeout_s = timeout_or_default(comm_timeout_s);
    for (int r = 0; r < world; ++r) {
      g->devices.push_back(g->rccl ? r : r % ndev);
      g->be.push_back(std::make_unique<HipBackend>(g->devices.back()));
    }
    if (g->rccl) {
      g->comms.resize(size_t(world));
      const ncclResult_t rc = RC().CommInitAll(g->comms.data(), world, g->devices.data());
      if (rc != ncclSuccess) throw CascadeError(std::string("ncclCommInitAll: ") + RC().GetErrorString(rc));
      for (int r = 0; r < world; ++r)
        g->rtr.push_back(std::make_unique<RcclTransport>(g->comms[size_t(r)], g->devices[size_t(r)],
                                                         g->be[size_t(r)]->stream(), WaitPolicy{}));
    }
    g->pool = std::make_unique<RankPool>(world);
    if (g->rccl) {
      require_rccl_runtime();
      if (preflight_enabled()) {
        const std::string err = group_exercise(*g, preflight_script(world, kPreflightBytes), kPreflightTimeout);
        if (!err.empty()) {
          Group* raw = g.release();
          svmd_cascade_group_destroy(raw);  // communicators were aborted by the failed exercise
          throw CascadeError("RCCL preflight failed: " + err);
        }
      }
    }
    return g.release();
  } catch (const std::exception& e) {
    set_error("svmd_cascade_group_create: %s", e.what());
    return nullptr;
  }
}

SVM_API void svmd_cascade_group_destroy(void* h) {
  auto* g = static_cast<Group*>(h);
  if (!g) return;
  g->pool.reset();
  g->rtr.clear();
  if (!g->broken)
    for (auto c : g->comms) (void)RC().CommDestroy(c);
  g->be.clear();
  delete g;
}

SVM_API int svmd_cascade_group_world(void* h) { return h ? static_cast<Group*>(h)->world : 0; }

SVM_API svm_cascade_out* svmd_cascade_group_fit(void* h, const void* X, int32_t u8, const int32_t* y, int64_t n,
                                                int64_t d, const svm_cascade_cfg* c) {
  auto* g = static_cast<Group*>(h);
  if (!g || n < 0 || d <= 0 || (n && (!X || !y))) {
    set_error("svmd_cascade_group_fit: bad arguments");
    return nullptr;
  }
  if (c && refuse_class_weights(c->params, "svmd_cascade_group_fit")) return nullptr;
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->broken) {
    set_error("svmd_cascade_group_fit: the group's communicators were aborted by an earlier failure; create a new group");
    return nullptr;
  }
  try {
    const char* pe = getenv("SVM355_CASCADE_PROFILE");
    const int prof = pe ? atoi(pe) : 0;
    if (prof >= 3) {
      const auto a = std::chrono::steady_clock::now();
      for (int dv : g->devices) {
        (void)hipSetDevice(dv);
        (void)hipDeviceSynchronize();
      }
      fprintf(stderr, "[svmd_cascade_group_fit] device sync at entry %.3f ms\n", ms_since(a));
    }
    const auto t_setup = std::chrono::steady_clock::now();
    const CascadeConfig cfg = config_from(c);
    const int P = g->world;
    GroupRun run(*g, (c && c->comm_timeout_s > 0) ? c->comm_timeout_s : g->timeout_s);
    const auto t_run = std::chrono::steady_clock::now();
    const size_t row_bytes = u8 ? size_t(d) : size_t(d) * 8;
    std::vector<CascadeOutput> outs(static_cast<size_t>(P));
    std::vector<double> job_in(static_cast<size_t>(P)), job_out(static_cast<size_t>(P));
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    run.run([&](int r, Transport& tr, HipBackend& be) {
      const auto tj = std::chrono::steady_clock::now();
      job_in[size_t(r)] = ms(t_run, tj);
      int64_t lo = 0, hi = 0;
      const std::vector<int64_t> ids = partition_ids(n, P, r, &lo, &hi);
      outs[size_t(r)] = run_cascade(tr, be, static_cast<const char*>(X) + size_t(lo) * row_bytes, u8 != 0, y + lo,
                                    ids.data(), hi - lo, d, n, cfg);
      job_out[size_t(r)] = ms_since(tj);
    });
    std::vector<const CascadeOutput*> ptrs;
    for (const auto& o : outs) ptrs.push_back(&o);
    (void)hipSetDevice(g->devices[0]);
    const auto t_out = std::chrono::steady_clock::now();
    svm_cascade_out* res = build_cascade_out(ptrs, *g->be[0], P, 0, g->rccl ? "rccl" : "loopback", "hip");
    if (prof >= 2)
      fprintf(stderr,
              "[svmd_cascade_group_fit] setup %.3f ms, ranks %.3f ms (rank 0: woke after %.3f ms, job %.3f ms, "
              "driver %.3f ms), output %.3f ms\n",
              ms(t_setup, t_run), ms(t_run, t_out), job_in[0], job_out[0], outs[0].train_ms, ms_since(t_out));
    return res;
  } catch (const std::exception& e) {
    set_error("cascade: %s", e.what());
    return nullptr;
  }
}

// Distributed decomposition SMO over the group's ranks: every rank's GPU holds all n uint8 rows (host
// X, n x d) and owns a block range of f; one candidate all-gather per outer iteration.  alpha_out
// (host, n doubles) and r come from rank 0 (every rank's alpha is the same replica); stats: SVM_DECOMP_STATS int64
// (decomp.h) from rank 0; rank_ms (world doubles, may be null): each rank's wall time; mm_out (2 d
// doubles, may be null): the column min / max the model's scaling uses.
static int group_decomp(void* h, const void* X, bool u8, const int32_t* y, int64_t n, int64_t d, const svm_params* pp,
                        int32_t q, double* alpha_out, svm_result* r, int64_t* stats, double* rank_ms, double* mm_out) {
  auto* g = static_cast<Group*>(h);
  if (!g || !X || !y || n < 2 || d <= 0) {
    set_error("svmd_cascade_group_decomp: bad arguments");
    return SVM_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  if (g->broken) {
    set_error("svmd_cascade_group_decomp: the group's communicators were aborted by an earlier failure");
    return SVM_ERR_ARG;
  }
  const svm_params p = params_or_default(pp);
  if (const int rc = refuse_class_weights(p, "svmd_cascade_group_decomp")) return rc;
  const int P = g->world;
  std::vector<double> ms(static_cast<size_t>(P), 0.0);
  const char* serial = getenv("SVM355_CASCADE_SERIAL_SOLVES");
  std::vector<DecompSolo> solo(static_cast<size_t>(serial && atoi(serial) != 0 && !g->rccl && P > 1 ? P : 0));
  for (auto& sr : solo) sr.mu = &g->solo_mu;
  g->solo_report.clear();
  g->host_wait_ms.assign(size_t(P), 0.0);
  try {
    GroupRun(*g, g->timeout_s).run([&](int rr, Transport& tr, HipBackend& be) {
      DecompOut out;  // the results come from rank 0; every rank reports its times
      if (rr == 0) out = {alpha_out, r, stats, nullptr, mm_out};
      out.ms = &ms[size_t(rr)];
      out.solo = solo.empty() ? nullptr : &solo[size_t(rr)];
      out.host_wait_ms = &g->host_wait_ms[size_t(rr)];
      decomp_on_rank(be, P > 1 ? &tr : nullptr, DecompIn{X, u8, y, n, d, p, q}, out);
    });
  } catch (const std::exception& e) {
    set_error("decomposition SMO: %s", e.what());
    return SVM_ERR_DEVICE;
  }
  if (rank_ms) std::copy(ms.begin(), ms.end(), rank_ms);
  g->solo_report = solo_summary(solo);
  return SVM_OK;
}

SVM_API int svmd_cascade_group_decomp(void* h, const uint8_t* X, const int32_t* y, int64_t n, int64_t d,
                                      const svm_params* pp, int32_t q, double* alpha_out, svm_result* r,
                                      int64_t* stats, double* rank_ms, double* mm_out) {
  return group_decomp(h, X, true, y, n, d, pp, q, alpha_out, r, stats, rank_ms, mm_out);
}

// The same over FP64 rows (host X, n x d, unscaled): real-valued data train with FP64-MFMA kernel values
// (decomp_fit_rows), pixel values held as doubles with the exact-integer plan.
SVM_API int svmd_cascade_group_decomp_rows(void* h, const double* X, const int32_t* y, int64_t n, int64_t d,
                                           const svm_params* pp, int32_t q, double* alpha_out, svm_result* r,
                                           int64_t* stats, double* rank_ms, double* mm_out) {
  return group_decomp(h, X, false, y, n, d, pp, q, alpha_out, r, stats, rank_ms, mm_out);
}

// The last distributed decomposition fit's host time per rank blocked in the per-batch waits (the one
// wait per outer iteration: RCCL's event poll under the deadline, or hipEventSynchronize); returns P.
SVM_API int64_t svmd_cascade_group_decomp_waits(void* h, double* out, int64_t cap) {
  auto* g = static_cast<Group*>(h);
  if (!g) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return copy_out(g->host_wait_ms, out, cap);
}

// The last distributed decomposition fit's solo timing on a loopback rehearsal (SVM355_CASCADE_SERIAL_SOLVES=1):
// out = solo_summary's report; returns the number of values (0: the last fit was not timed solo).
SVM_API int64_t svmd_cascade_group_decomp_solo(void* h, double* out, int64_t cap) {
  auto* g = static_cast<Group*>(h);
  if (!g) return 0;
  std::lock_guard<std::mutex> lk(g->mu);
  return copy_out(g->solo_report, out, cap);
}

// One process rank of the distributed decomposition SMO (every rank passes all n rows and labels).
static int rank_decomp(void* h, const void* X, bool u8, const int32_t* y, int64_t n, int64_t d, const svm_params* pp,
                       int32_t q, double* alpha_out, svm_result* r, int64_t* stats, double* ms_out, double* mm_out) {
  auto* pr = static_cast<ProcRank*>(h);
  if (!pr || !X || !y || n < 2 || d <= 0) {
    set_error("svmd_cascade_rank_decomp: bad arguments");
    return SVM_ERR_ARG;
  }
  if (pr->broken) {
    set_error("svmd_cascade_rank_decomp: the communicator was aborted by an earlier failure");
    return SVM_ERR_ARG;
  }
  const svm_params p = params_or_default(pp);
  if (const int rc = refuse_class_weights(p, "svmd_cascade_rank_decomp")) return rc;
  try {
    pr->guarded(pr->timeout_s, [&] {
      pr->host_wait_ms = 0.0;
      decomp_on_rank(*pr->be, pr->tr->world() > 1 ? pr->tr.get() : nullptr, DecompIn{X, u8, y, n, d, p, q},
                     DecompOut{alpha_out, r, stats, ms_out, mm_out, nullptr, &pr->host_wait_ms});
    });
    return SVM_OK;
  } catch (const std::exception& e) {
    set_error("decomposition SMO: %s", e.what());
    return SVM_ERR_DEVICE;
  }
}

SVM_API int svmd_cascade_rank_decomp(void* h, const uint8_t* X, const int32_t* y, int64_t n, int64_t d,
                                     const svm_params* pp, int32_t q, double* alpha_out, svm_result* r,
                                     int64_t* stats, double* ms_out, double* mm_out) {
  return rank_decomp(h, X, true, y, n, d, pp, q, alpha_out, r, stats, ms_out, mm_out);
}

// The same over FP64 rows (svmd_cascade_group_decomp_rows).
SVM_API int svmd_cascade_rank_decomp_rows(void* h, const double* X, const int32_t* y, int64_t n, int64_t d,
                                          const svm_params* pp, int32_t q, double* alpha_out, svm_result* r,
                                          int64_t* stats, double* ms_out, double* mm_out) {
  return rank_decomp(h, X, false, y, n, d, pp, q, alpha_out, r, stats, ms_out, mm_out);
}

// The last svmd_cascade_rank_decomp fit's host time blocked in the per-batch waits (ms).
SVM_API double svmd_cascade_rank_decomp_wait(void* h) {
  auto* pr = static_cast<ProcRank*>(h);
  return pr ? pr->host_wait_ms : 0.0;
}

SVM_API void* svmd_cascade_rank_create(int32_t device, const uint8_t* uid, int32_t world, int32_t rank,
                                       double comm_timeout_s) {
  try {
    if (!uid || world < 1 || rank < 0 || rank >= world) throw CascadeError("bad arguments");
    auto p = std::make_unique<ProcRank>();
    p->device = device;
    p->timeout_s = timeout_or_default(comm_timeout_s);
    if (hipSetDevice(device) != hipSuccess) throw CascadeError("hipSetDevice(" + std::to_string(device) + ") failed");
    p->be = std::make_unique<HipBackend>(device);
    ncclUniqueId id;
    std::memcpy(&id, uid, sizeof(id));
    const ncclResult_t rc = RC().CommInitRank(&p->comm, world, id, rank);
    if (rc != ncclSuccess) throw CascadeError(std::string("ncclCommInitRank: ") + RC().GetErrorString(rc));
    auto rt = std::make_unique<RcclTransport>(p->comm, device, p->be->stream(), WaitPolicy{nullptr, p->timeout_s});
    p->rccl = rt.get();
    p->tr = std::move(rt);
    require_rccl_runtime();
    if (preflight_enabled()) {
      try {
        p->guarded(kPreflightTimeout,
                   [&] { exercise_transport(*p->tr, *p->be, preflight_script(world, kPreflightBytes)); });
      } catch (const std::exception& e) {
        ProcRank* raw = p.release();
        svmd_cascade_rank_destroy(raw);
        throw CascadeError(std::string("RCCL preflight failed: ") + e.what());
      }
      p->set_policy(WaitPolicy{nullptr, p->timeout_s});
    }
    return p.release();
  } catch (const std::exception& e) {
    set_error("svmd_cascade_rank_create: %s", e.what());
    return nullptr;
  }
}

// A process rank on `device` whose exchanges run through the caller's host collectives (e.g. a gloo
// group under torchrun), device buffers staged through host memory (hostcomm.cpp).  Any number of
// processes may share one GPU: the per-process path of the N-GPU run (the distributed decomposition,
// the cascades) rehearsed on one device.  The callbacks must outlive the rank.  A preflight of the
// driver's op set runs first (collective: every rank creates its rank at the same time); its failure
// aborts nothing.
SVM_API void* svmd_cascade_rank_create_hostcomm(const svm_host_comm* comm, int32_t device, double comm_timeout_s) {
  try {
    if (!host_comm_valid(comm)) throw CascadeError("bad communicator");
    auto p = std::make_unique<ProcRank>();
    p->device = device;
    p->timeout_s = timeout_or_default(comm_timeout_s);
    if (hipSetDevice(device) != hipSuccess) throw CascadeError("hipSetDevice(" + std::to_string(device) + ") failed");
    p->be = std::make_unique<HipBackend>(device);
    p->tr = make_hostcomm_transport(*comm, p->be.get());
    if (preflight_enabled()) {
      try {
        exercise_transport(*p->tr, *p->be, preflight_script(comm->world, kPreflightBytes));
      } catch (const std::exception& e) {
        throw CascadeError(std::string("hostcomm preflight failed: ") + e.what());
      }
    }
    return p.release();
  } catch (const std::exception& e) {
    set_error("svmd_cascade_rank_create_hostcomm: %s", e.what());
    return nullptr;
  }
}

SVM_API void svmd_cascade_rank_destroy(void* h) {
  auto* p = static_cast<ProcRank*>(h);
  if (!p) return;
  (void)hipSetDevice(p->device);
  const bool aborted = p->broken;
  p->tr.reset();
  if (p->comm && !aborted) (void)RC().CommDestroy(p->comm);
  p->be.reset();
  delete p;
}

SVM_API svm_cascade_out* svmd_cascade_rank_fit(void* h, const void* X, int32_t u8, const int32_t* y,
                                               const int64_t* ids, int64_t n_part, int64_t d, int64_t n_total,
                                               const svm_cascade_cfg* c) {
  auto* p = static_cast<ProcRank*>(h);
  if (!p || n_part < 0 || d <= 0 || (n_part && (!X || !y || !ids))) {
    set_error("svmd_cascade_rank_fit: bad arguments");
    return nullptr;
  }
  if (c && refuse_class_weights(c->params, "svmd_cascade_rank_fit")) return nullptr;
  if (p->broken) {
    set_error("svmd_cascade_rank_fit: the communicator was aborted by an earlier failure");
    return nullptr;
  }
  try {
    const CascadeConfig cfg = config_from(c);
    CascadeOutput o;
    p->guarded((c && c->comm_timeout_s > 0) ? c->comm_timeout_s : p->timeout_s,
               [&] { o = run_cascade(*p->tr, *p->be, X, u8 != 0, y, ids, n_part, d, n_total, cfg); });
    return build_cascade_out({&o}, *p->be, p->tr->world(), p->tr->rank(), p->tr->name(), "hip");
  } catch (const std::exception& e) {
    set_error("cascade: %s", e.what());
    return nullptr;
  }
}

SVM_API int svmd_cascade_rank_exercise(void* h, const char* script, double timeout_s) {
  auto* p = static_cast<ProcRank*>(h);
  if (!p || p->broken || !script) {
    set_error("svmd_cascade_rank_exercise: no usable communicator");
    return SVM_ERR_ARG;
  }
  try {
    p->guarded(timeout_s > 0 ? timeout_s : kPreflightTimeout, [&] { exercise_transport(*p->tr, *p->be, script); });
    p->set_policy(WaitPolicy{nullptr, p->timeout_s});
    return SVM_OK;
  } catch (const std::exception& e) {
    set_error("%s", e.what());
    return SVM_ERR_DEVICE;
  }
}

SVM_API int svmd_cascade_rank_barrier(void* h) {
  auto* p = static_cast<ProcRank*>(h);
  if (!p || p->broken) {
    set_error("svmd_cascade_rank_barrier: no usable communicator");
    return SVM_ERR_ARG;
  }
  try {
    (void)hipSetDevice(p->device);
    p->tr->barrier();
    return SVM_OK;
  } catch (const std::exception& e) {
    set_error("svmd_cascade_rank_barrier: %s", e.what());
    return SVM_ERR_DEVICE;
  }
}

}  // extern "C"
