// What the three units of the device cascade share (internal; not part of the C ABI):
//   cascade_dev.hip     the row-copy / selection / KKT kernels and HipBackend's members (the only device code)
//   rccl_transport.hip  RcclTransport, the RCCL runtime identity and the preflight switches
//   cascade_ranks.hip   thread-rank groups, process ranks and their C ABI (svmd_cascade_group_* / _rank_*)
#pragma once
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "cascade.h"
#include "ctx.h"
#include "rccl_api.h"
#include "svm355_device.h"

namespace svm355 {

// SV sets in HBM; assembly / packing are row-copy kernels on the rank's stream; every solve is the device
// trainer (MFMA / exact-integer RBF Gram + device SMO, warm start f from the resident Gram).  A caching
// allocator keeps the per-round sets from going back to hipMalloc / hipFree (hipFree synchronises the device).
class HipBackend final : public Backend {
 public:
  explicit HipBackend(int device);
  ~HipBackend() override;
  HipBackend(const HipBackend&) = delete;
  HipBackend& operator=(const HipBackend&) = delete;

  hipStream_t stream() const { return stream_; }
  DeviceCtx* device_ctx() const { return static_cast<DeviceCtx*>(ctx_); }
  int device() const { return device_; }
  const char* name() const override { return "hip"; }
  int64_t ld(int64_t d) const override { return svmd_padded_dim(d); }

  // Size-class caching allocator: blocks go back to a free list, never to hipFree, until the
  // backend is destroyed.  All users run on this backend's one stream, so reuse is stream-ordered.
  void* alloc(int64_t bytes) override;
  void free(void* p) override;
  void h2d(void* dst, const void* src, int64_t bytes) override {
    if (bytes > 0) check(svmd_memcpy_h2d(ctx_, dst, src, bytes), "svmd_memcpy_h2d");
  }
  void d2h(void* dst, const void* src, int64_t bytes) override {
    if (bytes > 0) check(svmd_memcpy_d2h(ctx_, dst, src, bytes), "svmd_memcpy_d2h");
  }
  void sync() override { check(svmd_synchronize(ctx_), "svmd_synchronize"); }
  void upload_rows(const void* X, bool u8, int64_t n, int64_t d, double* dst) override;
  void minmax(const double* X, int64_t n, int64_t d, double* mn, double* mx) override;
  void scale(double* X, int64_t n, int64_t d, const double* mn, const double* mx) override;
  void assemble(const Segment& s, int64_t ld, DSet& o, int64_t off) override;
  void pack(const DSet& S, int64_t ld, double* rec) override;
  void record_ids(const double* rec, int64_t k, int64_t ld, int64_t* ids) override;
  void record_ids_batch(const std::vector<const double*>& recs, const std::vector<int64_t>& ks, int64_t ld,
                        const std::vector<int64_t*>& ids) override;
  // Device-side SV selection: the indices land in device memory (for the assembly kernel) and in
  // pinned host memory (for the host id mirror) with one synchronisation, instead of an alpha read
  // back, a host scan and an index upload.
  void select_svs(const DSet& S, double tol, std::vector<int64_t>* keep, const int64_t** keep_dev) override;
  SolveStats solve(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h, int solver,
                   int64_t) override;
  bool warm_start_converged(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h,
                            const double* mx_h) override;
  double take_solo_ms() override;
  void trace_push(const char* name) override { svmd_trace_push(name); }
  void trace_pop() override { svmd_trace_pop(); }
  static void check(int rc, const char* what) {  // an svm355 status as a CascadeError
    if (rc != SVM_OK) throw CascadeError(std::string(what) + ": " + svm_last_error());
  }

 private:
  // SVM355_CASCADE_SERIAL_SOLVES=1: solves (and skip checks) of all ranks of this process take one
  // lock, and each is timed from an idle stream to its completion -- the device time the solve
  // would take on a GPU of its own (one-GPU rehearsals of P ranks; bench.py's critical path).
  static std::mutex& solo_mutex() {
    static std::mutex m;
    return m;
  }
  // pre / post run under the lock, outside the timed region.  Defined in cascade_dev.hip, its only user.
  template <class F, class Pre = void (*)(), class Post = void (*)()>
  decltype(std::declval<F&>()()) solo(F&& f, Pre&& pre = [] {}, Post&& post = [] {});
  bool solve_decomp(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h,
                    SolveStats* out);
  SolveStats solve_impl(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h);
  bool kkt_check(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h);
  bool kkt_check_impl(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h);
  static void hipcheck(hipError_t e, const char* what) {
    if (e != hipSuccess) throw CascadeError(std::string(what) + ": " + hipGetErrorString(e));
  }
  void grow(void** p, size_t* cap, size_t bytes);
  void grow_pinned(size_t bytes);
  void wait_staged();
  const int64_t* stage_idx(const std::vector<int64_t>& v);
  void release_cache();

  int device_;
  void* ctx_ = nullptr;
  hipStream_t stream_ = nullptr;
  std::multimap<size_t, void*> cache_;
  std::map<void*, size_t> live_;
  void *idx_ = nullptr, *ids_d_ = nullptr, *sqn_ = nullptr, *kkt_ = nullptr, *sel_d_ = nullptr;
  size_t idx_cap_ = 0, ids_cap_ = 0, sqn_cap_ = 0, kkt_cap_ = 0, sel_cap_ = 0;
  void* pinned_ = nullptr;  // host staging (index uploads, device SV selection results)
  size_t pinned_cap_ = 0;
  hipEvent_t stage_ev_ = nullptr;
  bool staged_ = false;
  const bool serial_ = [] {
    const char* v = getenv("SVM355_CASCADE_SERIAL_SOLVES");
    return v && atoi(v) != 0;
  }();
  const bool release_gram_ = [] {
    const char* v = getenv("SVM355_CASCADE_RELEASE_GRAM");
    return v && atoi(v) != 0;
  }();
  double solo_acc_ = 0.0;
  bool solo_any_ = false;
};

// One communicator per GPU, collectives on the backend's stream (so they are ordered after the kernels
// that produced their buffers); every wait polls hipStreamQuery + ncclCommGetAsyncError against the
// WaitPolicy (abort token and deadline) instead of blocking in hipStreamSynchronize; abort() = ncclCommAbort.
class RcclTransport final : public Transport {
 public:
  RcclTransport(ncclComm_t comm, int device, hipStream_t stream, WaitPolicy wp);
  ~RcclTransport() override;
  bool aborted() const { return aborted_; }
  void set_policy(WaitPolicy wp) { wp_ = std::move(wp); }  // per fit: a fresh abort token
  int rank() const override { return rank_; }
  int world() const override { return world_; }
  const char* name() const override { return "rccl"; }
  int64_t bcast_i64(int64_t v, int root) override;
  std::vector<int64_t> allgather_i64(int64_t v) override;
  void allreduce_min(double* buf, int64_t n) override;
  void allreduce_max(double* buf, int64_t n) override;
  void bcast(void* buf, int64_t bytes, int root) override;
  void gather(const void* send, int64_t bytes, void* recv, int root) override;
  void allgather(const void* send, int64_t bytes, void* recv) override;
  void allgather_async(const void* send, int64_t bytes, void* recv) override;
  bool stream_wait(const char* what) override { return wait(what), true; }
  bool event_wait(void* event, const char* what) override { return wait(what, static_cast<hipEvent_t>(event)), true; }
  void send_i64(int64_t v, int peer) override;
  int64_t recv_i64(int peer) override;
  void send(const void* buf, int64_t bytes, int peer) override;
  void recv(void* buf, int64_t bytes, int peer) override;
  void barrier() override;
  void abort() override;

 private:
  // Poll instead of hipStreamSynchronize: a peer that never arrives must not hang this thread.
  void wait(const char* what, hipEvent_t event = nullptr);
  ncclComm_t comm_;
  int device_, rank_ = 0, world_ = 1;
  hipStream_t stream_;
  WaitPolicy wp_;
  int64_t* scratch_ = nullptr;
  int64_t* pinned_ = nullptr;
  bool aborted_ = false;
};

inline double timeout_or_default(double s) { return s > 0 ? s : 600.0; }
inline const RcclApi& RC() { return rccl_checked(); }  // the explicitly loaded librccl (rccl_api.h)

// ---- RCCL runtime identity.  The entry points come from the librccl loaded explicitly by
// rccl_api.h (the one the headers belong to; inside a PyTorch process a -lrccl link would bind to
// torch's bundled, older copy instead).  The version check stays as a guard for SVM355_RCCL_LIB
// overrides: a runtime of the header's major version and at least kMinRcclCode is accepted, an older
// minor than the header's is reported as a skew, and the preflight (exercise.cpp) checks every op on
// the live communicators anyway.
constexpr int kMinRcclCode = 21200;
struct RcclInfo {
  int header = NCCL_VERSION_CODE;
  int runtime = 0;
  std::string path;
};
const RcclInfo& rccl_info();
void require_rccl_runtime();

// Preflight: the driver's whole op set over the live communicators (SVM355_RCCL_PREFLIGHT=0 skips it).
constexpr double kPreflightTimeout = 20.0;
constexpr int64_t kPreflightBytes = 1 << 20;
bool preflight_enabled();

}  // namespace svm355
