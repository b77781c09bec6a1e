// C ABI of the device library: context management and the end-to-end device training path.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <vector>

#include "ctx.h"
#include "svm355_device.h"
#include "trace.h"

using namespace svm355;

namespace svm355 {
// The solvers without per-class boxes (the pairwise device solvers, the distributed and cascade trainers)
// refuse class weights that differ from 1 -- none solves the unweighted problem in their place.  SVM_OK
// when both weights are 1 (or 0, which reads as 1).
int refuse_class_weights(const svm_params& p, const char* who) {
  double cp, cn;
  const int rc = svm_class_boxes(&p, &cp, &cn);
  if (rc) return rc;
  if (cp != p.C || cn != p.C) {
    set_error("%s: class weights (weight_pos = %g, weight_neg = %g) are supported by the decomposition solver on one "
              "GPU and the CPU solvers only", who, p.weight_pos, p.weight_neg);
    return SVM_ERR_ARG;
  }
  return SVM_OK;
}
// The process's first LARGE host-to-device copy sets up the copy-engine path: ~8 ms, paid by whichever
// copy comes first -- the first fit's 47 MB row upload (profiles/r5_cold_fit_trace.txt: the cold upload
// 8.0 ms against 0.9 ms, and 1.1 ms after a 32 MB copy at start-up, from pinned or pageable memory
// alike).  The context pays it once here with a 32 MB copy into scratch memory.
int warm_copy_engine(DeviceCtx* ctx) {
  constexpr size_t kBytes = size_t(32) << 20;
  void *h = nullptr, *d = nullptr;
  int rc = SVM_OK;
  if (hipHostMalloc(&h, kBytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&d, kBytes) != hipSuccess) {
    rc = SVM_ERR_DEVICE;
  } else {
    std::memset(h, 0, kBytes);
    if (hipMemcpyAsync(d, h, kBytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = SVM_ERR_DEVICE;
  }
  if (d) (void)hipFree(d);
  if (h) (void)hipHostFree(h);
  return rc;
}
int tu_warm_capi(hipStream_t s);
int tu_warm_cascade_dev(hipStream_t s);
int tu_warm_decomp(hipStream_t s);
int tu_warm_decomp_inner(hipStream_t s);
int tu_warm_dsmo(hipStream_t s);
int tu_warm_gram_mfma(hipStream_t s);
int tu_warm_igram(hipStream_t s);
int tu_warm_prep_kernels(hipStream_t s);
int tu_warm_rowcache(hipStream_t s);
int tu_warm_smo(hipStream_t s);
// The first context of the process on `device` (the code objects and the copy engine are the device's,
// not the context's: later contexts -- thread ranks, a one-vs-rest pool -- skip the warm-ups).
static bool first_context_on(int device) {
  static std::mutex mu;
  static std::set<int> seen;
  std::lock_guard<std::mutex> lk(mu);
  return seen.insert(device).second;
}
int tu_warm_all(hipStream_t s) {
  int bad = 0;
  for (auto fn : {tu_warm_capi, tu_warm_cascade_dev, tu_warm_decomp, tu_warm_decomp_inner, tu_warm_dsmo,
                  tu_warm_gram_mfma, tu_warm_igram, tu_warm_prep_kernels, tu_warm_rowcache, tu_warm_smo})
    bad |= fn(s);
  return bad;
}
}  // namespace svm355

extern "C" {

SVM_API int64_t svmd_padded_dim(int64_t d) { return padded_dim(d); }

SVM_API int svmd_device_count(int32_t* count) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  if (count) *count = c;
  return SVM_OK;
}

SVM_API void* svmd_alloc(void* h, int64_t bytes) {
  auto* ctx = static_cast<DeviceCtx*>(h);
  if (!ctx || bytes < 0) return nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, size_t(bytes ? bytes : 1));
  if (e != hipSuccess) {
    set_error("svmd_alloc(%lld): %s", (long long)bytes, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}

SVM_API void svmd_free(void* h, void* ptr) {
  auto* ctx = static_cast<DeviceCtx*>(h);
  if (!ctx || !ptr) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(ptr);
}

SVM_API int svmd_memcpy_h2d(void* h, void* dst_d, const void* src_h, int64_t bytes) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  if (bytes > 0) SVMD_CHECK(hipMemcpyAsync(dst_d, src_h, size_t(bytes), hipMemcpyHostToDevice, ctx->stream));
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

SVM_API int svmd_memcpy_d2h(void* h, void* dst_h, const void* src_d, int64_t bytes) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  if (bytes > 0) SVMD_CHECK(hipMemcpyAsync(dst_h, src_d, size_t(bytes), hipMemcpyDeviceToHost, ctx->stream));
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

SVM_API void svmd_destroy(void* h);


SVM_API void* svmd_create(int32_t device) {
  if (hipSetDevice(device) != hipSuccess) {
    set_error("svmd_create: hipSetDevice(%d) failed", device);
    return nullptr;
  }
  auto* ctx = new DeviceCtx();
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_out, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_ctl[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_ctl[1], hipEventDisableTiming) != hipSuccess) {
    set_error("svmd_create: stream/event creation failed");
    delete ctx;
    return nullptr;
  }
  // Pay the one-time costs here, not inside the first solve: load every code object of the library
  // (one launch per translation unit) and set up the copy engine -- once per device and process --, and
  // allocate the pinned state block and a small solver workspace (grown on demand).
  const bool first = first_context_on(device);
  if ((first && warm_copy_engine(ctx) != SVM_OK) || (first && tu_warm_all(ctx->stream) != 0) ||
      hipGetLastError() != hipSuccess ||
      ctx->ensure_pinned(size_t(1) << 16) != SVM_OK ||
      ctx->ensure_ws(size_t(16) << 20) != SVM_OK || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("svmd_create: warm-up on device %d failed", device);
    svmd_destroy(ctx);
    return nullptr;
  }
  return ctx;
}

SVM_API void svmd_destroy(void* h) {
  auto* ctx = static_cast<DeviceCtx*>(h);
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  ctx->release_graph();
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->gram) (void)hipFree(ctx->gram);
  if (ctx->rc_cache) (void)hipFree(ctx->rc_cache);
  if (ctx->count_d) (void)hipFree(ctx->count_d);

  if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
  if (ctx->ev_out) (void)hipEventDestroy(ctx->ev_out);
  for (hipEvent_t e : ctx->ev_ctl)
    if (e) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

SVM_API int svmd_selftest_exp(void* h, const double* x_d, int64_t n, double* lib_d, double* batch_d) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  rc = exp_selftest(ctx->stream, x_d, n, lib_d, batch_d);
  if (rc) return rc;
  return ctx->end();
}

static int release_gram(DeviceCtx* ctx) {
  if (ctx->gram) {
    ScopedDevice on(ctx->device);
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));
    SVMD_CHECK(hipFree(ctx->gram));
    ctx->gram = nullptr;
    ctx->gram_bytes = 0;
  }
  return SVM_OK;
}

SVM_API int svmd_release_cache(void* h) {  // the library-owned Gram and the row-cache slab
  SVMD_CTX(h);
  int rc = release_gram(ctx);
  if (rc) return rc;
  return svmd_release_slab(h);
}

SVM_API int svmd_cache_bytes(void* h, int64_t* gram, int64_t* slab) {
  SVMD_CTX(h);
  if (gram) *gram = int64_t(ctx->gram_bytes);
  if (slab) *slab = int64_t(ctx->rc_cache_bytes);
  return SVM_OK;
}

SVM_API int svmd_set_ccache_frac(void* h, double frac) {  // < 0: the default quarter of the HBM
  SVMD_CTX(h);
  ctx->ccache_frac = frac < 0.0 ? -1.0 : std::min(0.9, frac);
  return SVM_OK;
}

SVM_API int svmd_release_slab(void* h) {  // the row-cache slab only (the resident Gram stays)
  SVMD_CTX(h);
  if (ctx->rc_cache) {
    ScopedDevice on(ctx->device);
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));
    SVMD_CHECK(hipFree(ctx->rc_cache));
    ctx->rc_cache = nullptr;
    ctx->rc_cache_bytes = 0;
  }
  return SVM_OK;
}

SVM_API int svmd_set_stream(void* h, void* stream) {
  SVMD_CTX(h);
  ctx->ext = static_cast<hipStream_t>(stream);
  ctx->has_ext = true;
  return SVM_OK;
}

SVM_API int svmd_synchronize(void* h) {
  SVMD_CTX(h);
  SVMD_CHECK(hipSetDevice(ctx->device));
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  if (ctx->has_ext) SVMD_CHECK(hipStreamSynchronize(ctx->ext));
  return SVM_OK;
}

SVM_API int svmd_upload_rows(void* h, const double* X_host, int64_t n, int64_t d, double* X_d, int64_t ld) {
  SVMD_CTX(h);
  if (ld < d || n < 0) {
    set_error("svmd_upload_rows: ld < d");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (n > 0) {
    if (ld == d) {
      SVMD_CHECK(hipMemcpyAsync(X_d, X_host, size_t(n * d) * 8, hipMemcpyHostToDevice, ctx->stream));
    } else {
      SVMD_CHECK(hipMemsetAsync(X_d, 0, size_t(n * ld) * 8, ctx->stream));
      SVMD_CHECK(hipMemcpy2DAsync(X_d, size_t(ld) * 8, X_host, size_t(d) * 8, size_t(d) * 8, size_t(n),
                                  hipMemcpyHostToDevice, ctx->stream));
    }
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));  // the host buffer may be released on return
  }
  return ctx->end();
}

SVM_API int svmd_upload_rows_u8(void* h, const uint8_t* X_host, int64_t n, int64_t d, double* X_d,
                                int64_t ld) {
  SVMD_CTX(h);
  if (ld < d || n < 0 || d <= 0) {
    set_error("svmd_upload_rows_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (n > 0) {
    rc = ctx->ensure_ws(size_t(n) * size_t(d));
    if (rc) return rc;
    uint8_t* stage = static_cast<uint8_t*>(ctx->ws);
    SVMD_CHECK(hipMemcpyAsync(stage, X_host, size_t(n) * size_t(d), hipMemcpyHostToDevice, ctx->stream));
    rc = launch_widen_u8(ctx->stream, stage, n, d, ld, X_d);
    if (rc) return rc;
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));  // the host buffer may be released on return
  }
  return ctx->end();
}

SVM_API int svmd_minmax(void* h, const double* X_d, int64_t n, int64_t d, int64_t ld, double* mn_d,
                        double* mx_d) {
  SVMD_CTX(h);
  if (n <= 0 || d <= 0 || ld < d || !mn_d || !mx_d) {
    set_error("svmd_minmax: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  const size_t scratch = size_t(2) * size_t(d) * 2048;
  rc = ctx->ensure_ws(scratch * 8);
  if (rc) return rc;
  rc = launch_minmax(ctx->stream, X_d, n, d, ld, mn_d, mx_d, static_cast<double*>(ctx->ws), scratch);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_preprocess(void* h, double* X_d, int64_t n, int64_t d, int64_t ld, double* mn_d,
                            double* mx_d, double* sqn_d, int32_t use_given) {
  SVMD_CTX(h);
  TraceRange tr("svm355:preprocess");
  if (n <= 0 || d <= 0 || ld < d || !mn_d || !mx_d) {
    set_error("svmd_preprocess: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (!use_given) {
    const size_t scratch = size_t(2) * size_t(d) * 2048;
    rc = ctx->ensure_ws(scratch * 8);
    if (rc) return rc;
    rc = launch_minmax(ctx->stream, X_d, n, d, ld, mn_d, mx_d, static_cast<double*>(ctx->ws), scratch);
    if (rc) return rc;
  }
  rc = launch_scale_norms(ctx->stream, X_d, n, d, ld, mn_d, mx_d, sqn_d);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_row_norms(void* h, const double* X_d, int64_t n, int64_t d, int64_t ld, double* sqn_d) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  rc = launch_scale_norms(ctx->stream, const_cast<double*>(X_d), n, d, ld, nullptr, nullptr, sqn_d);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_rbf_gram(void* h, const double* A_d, const double* nA_d, int64_t m, int64_t lda,
                          const double* B_d, const double* nB_d, int64_t n, int64_t ldb, int64_t kdim,
                          double gamma, double* K_d, int64_t ldk, int32_t sym_diag) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  rc = launch_rbf_gram(ctx->stream, A_d, nA_d, m, lda, B_d, nB_d, n, ldb, kdim, gamma, K_d, ldk, sym_diag != 0);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_smo(void* h, const double* K_d, int64_t ldk, const int32_t* y_d, int64_t n,
                     double* alpha_d, int32_t warm, const svm_params* p, svm_result* r,
                     int64_t* trace_host, int64_t trace_cap) {
  SVMD_CTX(h);
  TraceRange tr("svm355:smo");
  const svm_params q = params_or_default(p);
  int rc = refuse_class_weights(q, "svmd_smo");
  if (rc) return rc;
  if ((rc = ctx->begin())) return rc;
  rc = run_smo(ctx, K_d, ldk, y_d, n, alpha_d, warm, q, r, trace_host, trace_cap);
  if (rc) return rc;
  if (r) {
    int64_t c = 0;
    rc = count_sv(ctx, alpha_d, n, 1, q.sv_tol, &c);
    if (rc) return rc;
    r->n_sv = c;
  }
  return ctx->end();
}

SVM_API int svmd_smo_multi(void* h, const double* K_d, int64_t ldk, const int32_t* Y_d, int64_t n, int32_t nclass,
                           double* A_d, const svm_params* p, svm_result* r, int32_t* batched) {
  SVMD_CTX(h);
  TraceRange tr("svm355:smo_multi");
  const svm_params q = params_or_default(p);
  int rc = refuse_class_weights(q, "svmd_smo_multi");
  if (rc) return rc;
  if ((rc = ctx->begin())) return rc;
  rc = run_smo_multi(ctx, K_d, ldk, Y_d, n, nclass, A_d, q, r, batched);
  if (rc) return rc;
  if (r) {
    std::vector<int64_t> c(static_cast<size_t>(nclass));
    rc = count_sv(ctx, A_d, n, nclass, q.sv_tol, c.data());
    if (rc) return rc;
    for (int k = 0; k < nclass; ++k) r[k].n_sv = c[size_t(k)];
  }
  return ctx->end();
}

// Gram selection: mode 0 = auto (exact-integer path when the scaled rows are integer multiples of
// 1/r_j, else FP64), 1 = FP64 only, 2 = integer path required.  SVM355_GRAM=fp64|int overrides
// the auto mode.  mn/mx (host, d values) are the min-max statistics the rows were scaled with.
static int gram_any(DeviceCtx* ctx, const double* X_d, const double* sqn_d, int64_t n, int64_t ld, int64_t kdim,
                    const double* mn_h, const double* mx_h, int64_t d, int32_t mode, double gamma, double* K,
                    int64_t ldk, int32_t* used_out) {
  if (mode == 0) {
    if (const char* g = getenv("SVM355_GRAM")) {
      if (!strcmp(g, "fp64")) mode = 1;
      if (!strcmp(g, "int")) mode = 2;
    }
  }
  TraceRange tr("svm355:gram");
  bool used = false;
  if (mode != 1 && mn_h && mx_h) {
    QuantPlan P;
    if (plan_quant(mn_h, mx_h, d, &P)) {
      int rc = ctx->ensure_ws(igram_workspace(n, P));
      if (rc) return rc;
      rc = run_igram(ctx->stream, X_d, n, ld, P, gamma, K, ldk, ctx->ws, &used);
      if (rc) return rc;
    }
  }
  if (!used && mode == 2) {
    set_error("integer Gram path requested but the rows are not integer-valued in [0, 255] after scaling");
    return SVM_ERR_ARG;
  }
  if (used_out) *used_out = used ? 1 : 0;
  if (used) return SVM_OK;
  if (!sqn_d) {
    set_error("FP64 Gram path needs the squared row norms");
    return SVM_ERR_ARG;
  }
  return launch_rbf_gram(ctx->stream, X_d, sqn_d, n, ld, X_d, sqn_d, n, ld, kdim, gamma, K, ldk, true);
}

// The library-owned Gram (DeviceCtx::gram, grow-only) sized for n rows; ldk = its row stride.
static int ensure_gram(DeviceCtx* ctx, int64_t n, int64_t* ldk_out) {
  const int64_t ldk = (n + 1) / 2 * 2;  // keep rows 16-byte aligned
  const size_t bytes = size_t(n) * size_t(ldk) * 8;
  *ldk_out = ldk;
  if (bytes <= ctx->gram_bytes) return SVM_OK;
  if (ctx->gram) {
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));
    SVMD_CHECK(hipFree(ctx->gram));
    ctx->gram = nullptr;
    ctx->gram_bytes = 0;
  }
  hipError_t e = hipMalloc(&ctx->gram, bytes);
  if (e != hipSuccess && ctx->rc_cache) {  // give back an idle row-cache slab and retry
    (void)hipGetLastError();
    SVMD_CHECK(hipFree(ctx->rc_cache));
    ctx->rc_cache = nullptr;
    ctx->rc_cache_bytes = 0;
    e = hipMalloc(&ctx->gram, bytes);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("svmd_train: cannot allocate the %.1f GB RBF Gram matrix: %s", double(bytes) * 1e-9,
              hipGetErrorString(e));
    return SVM_ERR_OOM;
  }
  ctx->gram_bytes = bytes;
  return SVM_OK;
}

static int train_impl(DeviceCtx* ctx, const double* X_d, const double* sqn_d, int64_t n, int64_t ld, int64_t kdim,
                      const int32_t* y_d, double* alpha_d, int32_t warm, const svm_params& q, svm_result* r,
                      double* K_d, int64_t ldk, svmd_timing* timing, const double* mn_h, const double* mx_h,
                      int64_t d, int32_t gram_mode, int32_t* gram_used) {
  const auto t0 = std::chrono::steady_clock::now();
  int rc = ctx->begin();
  if (rc) return rc;
  double* K = K_d;
  if (!K) {  // library-owned Gram, cached in the context (see DeviceCtx::gram)
    rc = ensure_gram(ctx, n, &ldk);
    if (rc) return rc;
    K = ctx->gram;
  }
  rc = gram_any(ctx, X_d, sqn_d, n, ld, kdim, mn_h, mx_h, d, gram_mode, q.gamma, K, ldk, gram_used);
  if (!rc && timing) {
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      set_error("svmd_train: gram failed: %s", hipGetErrorString(e));
      rc = SVM_ERR_DEVICE;
    }
  }
  const double t_gram = ms_since(t0);
  if (!rc) {
    TraceRange ts("svm355:smo");
    rc = run_smo(ctx, K, ldk, y_d, n, alpha_d, warm, q, r, nullptr, 0);
  }
  if (!rc && r) {
    int64_t c = 0;
    rc = count_sv(ctx, alpha_d, n, 1, q.sv_tol, &c);
    if (!rc) r->n_sv = c;
  }
  if (rc) return rc;
  if (timing) {
    timing->gram_ms = t_gram;
    timing->total_ms = ms_since(t0);
    timing->smo_ms = timing->total_ms - t_gram;
  }
  return ctx->end();
}

// Size the context's Gram for an n-row solve ahead of it (SVM_ERR_OOM if it does not fit).
SVM_API int svmd_reserve_gram(void* h, int64_t n) {
  SVMD_CTX(h);
  int64_t ldk = 0;
  return n > 0 ? ensure_gram(ctx, n, &ldk) : SVM_OK;
}

SVM_API int svmd_train(void* h, const double* X_d, const double* sqn_d, int64_t n, int64_t ld, int64_t kdim,
                       const int32_t* y_d, double* alpha_d, int32_t warm, const svm_params* p,
                       svm_result* r, double* K_d, int64_t ldk, svmd_timing* timing) {
  SVMD_CTX(h);
  if (const int rc = refuse_class_weights(params_or_default(p), "svmd_train")) return rc;
  return train_impl(ctx, X_d, sqn_d, n, ld, kdim, y_d, alpha_d, warm, params_or_default(p), r, K_d, ldk, timing, nullptr,
                    nullptr, 0, 1, nullptr);
}

SVM_API int svmd_train_q(void* h, const double* X_d, const double* sqn_d, int64_t n, int64_t ld, int64_t kdim,
                         const int32_t* y_d, double* alpha_d, int32_t warm, const svm_params* p, svm_result* r,
                         double* K_d, int64_t ldk, svmd_timing* timing, const double* mn_h, const double* mx_h,
                         int64_t d, int32_t gram_mode, int32_t* gram_used) {
  SVMD_CTX(h);
  if (const int rc = refuse_class_weights(params_or_default(p), "svmd_train_q")) return rc;
  return train_impl(ctx, X_d, sqn_d, n, ld, kdim, y_d, alpha_d, warm, params_or_default(p), r, K_d, ldk, timing, mn_h, mx_h,
                    d, gram_mode, gram_used);
}

// Training straight from uint8 pixel rows (n x d contiguous, device): the exact-integer Gram is
// quantised from the bytes (no FP64 rows), then the SMO.  mn_h / mx_h: the rows' column min / max
// (svmd_minmax_u8).  *used = 0 and nothing trained when the plan does not apply (the caller then
// takes the FP64-row path); K: n x ldk Gram storage.  Same Gram, trajectory and result as
// svmd_train_q on the scaled FP64 rows.
SVM_API int svmd_train_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h, const double* mx_h,
                          const int32_t* y_d, double* alpha_d, int32_t warm, const svm_params* p, svm_result* r,
                          double* K_d, int64_t ldk, svmd_timing* timing, int32_t* used_out) {
  SVMD_CTX(h);
  if (used_out) *used_out = 0;
  if (!Xu_d || n <= 0 || d <= 0 || !mn_h || !mx_h || !K_d || ldk < n) {
    set_error("svmd_train_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  const svm_params q = params_or_default(p);
  int rc = refuse_class_weights(q, "svmd_train_u8");
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = ctx->begin())) return rc;
  QuantPlan P;
  if (!plan_quant(mn_h, mx_h, d, &P)) return ctx->end();
  bool used = false;
  {
    TraceRange tr("svm355:gram");
    rc = ctx->ensure_ws(igram_u8_workspace(n, P));
    if (rc) return rc;
    rc = run_igram_u8(ctx->stream, Xu_d, n, d, mn_h, mx_h, P, q.gamma, K_d, ldk, ctx->ws, &used);
    if (rc) return rc;
  }
  if (!used) return ctx->end();
  if (timing) SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  const double t_gram = ms_since(t0);
  {
    TraceRange ts("svm355:smo");
    rc = run_smo(ctx, K_d, ldk, y_d, n, alpha_d, warm, q, r, nullptr, 0);
  }
  if (!rc && r) {
    int64_t c = 0;
    rc = count_sv(ctx, alpha_d, n, 1, q.sv_tol, &c);
    if (!rc) r->n_sv = c;
  }
  if (rc) return rc;
  if (timing) {
    timing->gram_ms = t_gram;
    timing->total_ms = ms_since(t0);
    timing->smo_ms = timing->total_ms - t_gram;
  }
  if (used_out) *used_out = 1;
  return ctx->end();
}

// The exact-integer RBF Gram of uint8 pixel rows (n x d contiguous, device) straight from the bytes,
// into K (n x ldk).  *used = 0 (nothing written) when the statistics do not admit the integer plan.
SVM_API int svmd_rbf_gram_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h,
                             const double* mx_h, double gamma, double* K_d, int64_t ldk, int32_t* used_out) {
  SVMD_CTX(h);
  if (used_out) *used_out = 0;
  if (!Xu_d || n <= 0 || d <= 0 || !mn_h || !mx_h || !K_d || ldk < n) {
    set_error("svmd_rbf_gram_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  TraceRange tr("svm355:gram");
  int rc = ctx->begin();
  if (rc) return rc;
  QuantPlan P;
  if (!plan_quant(mn_h, mx_h, d, &P)) return ctx->end();
  rc = ctx->ensure_ws(igram_u8_workspace(n, P));
  if (rc) return rc;
  bool used = false;
  rc = run_igram_u8(ctx->stream, Xu_d, n, d, mn_h, mx_h, P, gamma, K_d, ldk, ctx->ws, &used);
  if (rc) return rc;
  if (used_out) *used_out = used ? 1 : 0;
  return ctx->end();
}

SVM_API int svmd_minmax_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, double* mn_d, double* mx_d) {
  SVMD_CTX(h);
  if (n <= 0 || d <= 0 || !Xu_d || !mn_d || !mx_d) {
    set_error("svmd_minmax_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  TraceRange tr("svm355:preprocess");
  int rc = ctx->begin();
  if (rc) return rc;
  const size_t scratch = size_t(2) * size_t(d) * 2048;
  rc = ctx->ensure_ws(scratch * 8);
  if (rc) return rc;
  rc = launch_minmax_u8(ctx->stream, Xu_d, n, d, mn_d, mx_d, static_cast<double*>(ctx->ws), scratch);
  if (rc) return rc;
  return ctx->end();
}

// Scaled FP64 rows idx[0..k) (k x ld, zero padded) and their squared norms from uint8 pixel rows.
SVM_API int svmd_sv_rows_u8(void* h, const uint8_t* Xu_d, int64_t d, const int64_t* idx_d, int64_t k,
                            const double* mn_d, const double* mx_d, double* out_d, int64_t ld, double* sqn_d) {
  SVMD_CTX(h);
  if (k < 0 || d <= 0 || ld < d || (k && (!Xu_d || !idx_d || !mn_d || !mx_d || !out_d || !sqn_d))) {
    set_error("svmd_sv_rows_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  rc = launch_sv_rows_u8(ctx->stream, Xu_d, d, idx_d, k, mn_d, mx_d, out_d, ld, sqn_d);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_train_rows(void* h, const double* X_d, const double* sqn_d, int64_t n, int64_t ld, int64_t d,
                            const int32_t* y_d, double* alpha_d, int32_t warm, const svm_params* p, svm_result* r,
                            const double* mn_h, const double* mx_h, int32_t gram_mode, int64_t cache_bytes,
                            int32_t* gram_used, int64_t* trace_host, int64_t trace_cap) {
  SVMD_CTX(h);
  const svm_params q = params_or_default(p);
  int rc = refuse_class_weights(q, "svmd_train_rows");
  if (rc) return rc;
  if ((rc = ctx->begin())) return rc;
  QuantPlan P;
  if (gram_mode != 1 && mn_h && mx_h) plan_quant(mn_h, mx_h, d, &P);
  if (cache_bytes <= 0) {
    // Default: room for 16384 rows (an SMO touches a few thousand distinct rows at MNIST scale),
    // capped at 60% of the HBM that is free or already this context's slab (after releasing a
    // cached library-owned Gram).
    rc = release_gram(ctx);
    if (rc) return rc;
    size_t fr = 0, tot = 0;
    SVMD_CHECK(hipMemGetInfo(&fr, &tot));
    cache_bytes = std::min<int64_t>(int64_t(double(fr + ctx->rc_cache_bytes) * 0.6),
                                    int64_t(16384) * ((n + 1) / 2 * 2) * 8);
  }
  int32_t used = 0;
  TraceRange tr("svm355:smo:rowcache");
  rc = run_smo_rowcache(ctx, X_d, sqn_d, n, ld, d, P, y_d, alpha_d, warm, q, r, size_t(cache_bytes), trace_host,
                        trace_cap, &used);
  if (rc) return rc;
  if (gram_mode == 2 && !used) {
    set_error("integer kernel rows requested but the rows are not integer-valued in [0, 255] after scaling");
    return SVM_ERR_ARG;
  }
  if (gram_used) *gram_used = used;
  if (r) {
    int64_t c = 0;
    rc = count_sv(ctx, alpha_d, n, 1, q.sv_tol, &c);
    if (rc) return rc;
    r->n_sv = c;
  }
  return ctx->end();
}

SVM_API int svmd_rbf_gram_q(void* h, const double* X_d, const double* sqn_d, int64_t n, int64_t ld,
                            int64_t kdim, const double* mn_h, const double* mx_h, int64_t d, double gamma,
                            double* K_d, int64_t ldk, int32_t gram_mode, int32_t* gram_used) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  rc = gram_any(ctx, X_d, sqn_d, n, ld, kdim, mn_h, mx_h, d, gram_mode, gamma, K_d, ldk, gram_used);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_decision(void* h, const double* Xs_d, const double* ns_d, const double* coef_d, int64_t nsv,
                          int64_t lds, const double* Xq_d, const double* nq_d, int64_t m, int64_t ldq,
                          int64_t kdim, double gamma, double b, double* out_d) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  if (m <= 0) return ctx->end();
  if (nsv <= 0) {
    // No support vectors: decision is -b everywhere.
    std::vector<double> v(size_t(m), -b);
    SVMD_CHECK(hipMemcpyAsync(out_d, v.data(), size_t(m) * 8, hipMemcpyHostToDevice, ctx->stream));
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));
    return ctx->end();
  }
  TraceRange tr("svm355:decision");
  // Cross-kernel block K(Xq, Xs) in row chunks of <= 512 MB scratch, then a deterministic GEMV.
  const int64_t ldk = (nsv + 1) / 2 * 2;
  // tests/test_gpu_predict_kernels.py (test_decision_chunk_size_still_makes_this_two_chunks) recomputes this.
  int64_t rows = std::max<int64_t>(128, (int64_t(512) << 20) / (ldk * 8) / 128 * 128);
  rows = std::min<int64_t>(rows, (m + 127) / 128 * 128);
  rc = ctx->ensure_ws(size_t(rows) * size_t(ldk) * 8);
  if (rc) return rc;
  double* Kq = static_cast<double*>(ctx->ws);
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t mr = std::min(rows, m - r0);
    rc = launch_rbf_gram(ctx->stream, Xq_d + r0 * ldq, nq_d + r0, mr, ldq, Xs_d, ns_d, nsv, lds, kdim, gamma, Kq,
                         ldk, false);
    if (rc) return rc;
    rc = launch_gemv_rows(ctx->stream, Kq, ldk, mr, nsv, coef_d, b, out_d + r0);
    if (rc) return rc;
  }
  return ctx->end();
}

SVM_API int svmd_decision_int(void* h, const double* X_d, int64_t k, int64_t ldx, int64_t d, const double* mn_h,
                              const double* mx_h, const double* coef_d, int64_t nz, double gamma, double* out_d,
                              int32_t* used) {
  SVMD_CTX(h);
  if (used) *used = 0;
  if (k <= 0 || nz <= 0 || nz > k || !used) return SVM_OK;
  QuantPlan P;
  if (!plan_quant(mn_h, mx_h, d, &P)) return SVM_OK;
  int rc = ctx->begin();
  if (rc) return rc;
  TraceRange tr("svm355:decision_int");
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const int64_t ldk = (nz + 1) / 2 * 2;
  const size_t block = al(size_t(k) * size_t(ldk) * 8);
  rc = ctx->ensure_ws(block + igram_workspace(k, P));
  if (rc) return rc;
  double* Kb = static_cast<double*>(ctx->ws);
  bool ok = false;
  rc = run_igram_block(ctx->stream, X_d, k, ldx, nz, P, gamma, Kb, ldk, static_cast<char*>(ctx->ws) + block, &ok);
  if (rc) return rc;
  if (ok) {
    rc = launch_gemv_rows(ctx->stream, Kb, ldk, k, nz, coef_d, 0.0, out_d);
    if (rc) return rc;
    *used = 1;
  }
  return ctx->end();
}

SVM_API int svmd_count_correct(void* h, const double* dec_d, const int32_t* y_d, int64_t m, int32_t zero_positive,
                               int64_t* correct) {
  SVMD_CTX(h);
  if (!correct) {
    set_error("svmd_count_correct: null output");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  rc = count_correct(ctx, dec_d, y_d, m, zero_positive != 0, correct);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_gather_rows(void* h, const double* src_d, int64_t ld, const int64_t* idx_d, int64_t k,
                             double* dst_d) {
  SVMD_CTX(h);
  int rc = ctx->begin();
  if (rc) return rc;
  rc = launch_gather_rows(ctx->stream, src_d, ld, idx_d, k, dst_d);
  if (rc) return rc;
  return ctx->end();
}

SVM_API void svmd_trace_push(const char* name) { roctxRangePushA(name ? name : "svm355"); }
SVM_API void svmd_trace_pop(void) { roctxRangePop(); }

}  // extern "C"

SVMD_TU_WARM(capi)
