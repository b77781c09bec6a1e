// Device side of the native Cascade SVM (csrc/cascade): the gfx950 backend -- its row-copy, selection and
// KKT kernels and HipBackend's members (declared in cascade_dev.h).  The only device code of the device
// cascade: the RCCL transport (rccl_transport.hip) and the groups, process ranks and their C ABI
// (cascade_ranks.hip) launch no kernel of their own, so the library registers one code object for the three.
#include <chrono>
#include <cstring>

#include "cascade_dev.h"
#include "decomp.h"

namespace svm355 {
namespace {

// ------------------------------------------------------------------------------------- kernels
// One workgroup per row (grid-stride); rows of stored sets are 16-byte aligned (ld % 16 == 0), record
// rows (width ld + 3) are only 8-byte aligned.
__global__ __launch_bounds__(256) void assemble_set_kernel(const double* __restrict__ sX,
                                                           const int32_t* __restrict__ sy,
                                                           const double* __restrict__ sa,
                                                           const int64_t* __restrict__ sid,
                                                           const int64_t* __restrict__ idx, int64_t m, int64_t ld,
                                                           double* __restrict__ dX, int32_t* __restrict__ dy,
                                                           double* __restrict__ da, int64_t* __restrict__ did,
                                                           int zero_alpha) {
  for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
    const int64_t src = idx ? idx[i] : i;
    const double2* s = reinterpret_cast<const double2*>(sX + src * ld);
    double2* d = reinterpret_cast<double2*>(dX + i * ld);
    for (int64_t c = threadIdx.x; c < ld / 2; c += blockDim.x) d[c] = s[c];
    if (threadIdx.x == 0) {
      dy[i] = sy[src];
      da[i] = zero_alpha ? 0.0 : sa[src];
      did[i] = sid[src];
    }
  }
}

__global__ __launch_bounds__(256) void assemble_rec_kernel(const double* __restrict__ rec, int64_t w,
                                                           const int64_t* __restrict__ idx, int64_t m, int64_t ld,
                                                           double* __restrict__ dX, int32_t* __restrict__ dy,
                                                           double* __restrict__ da, int64_t* __restrict__ did,
                                                           int zero_alpha) {
  for (int64_t i = blockIdx.x; i < m; i += gridDim.x) {
    const double* r = rec + (idx ? idx[i] : i) * w;
    double* d = dX + i * ld;
    for (int64_t c = threadIdx.x; c < ld; c += blockDim.x) d[c] = r[c];
    if (threadIdx.x == 0) {
      dy[i] = int32_t(r[ld]);
      da[i] = zero_alpha ? 0.0 : r[ld + 1];
      did[i] = int64_t(r[ld + 2]);
    }
  }
}

__global__ __launch_bounds__(256) void pack_kernel(const double* __restrict__ X, const int32_t* __restrict__ y,
                                                   const double* __restrict__ a, const int64_t* __restrict__ id,
                                                   int64_t k, int64_t ld, double* __restrict__ rec) {
  const int64_t w = ld + 3;
  for (int64_t i = blockIdx.x; i < k; i += gridDim.x) {
    const double* s = X + i * ld;
    double* r = rec + i * w;
    for (int64_t c = threadIdx.x; c < ld; c += blockDim.x) r[c] = s[c];
    if (threadIdx.x == 0) {
      r[ld] = double(y[i]);
      r[ld + 1] = a[i];
      r[ld + 2] = double(id[i]);
    }
  }
}

__global__ void record_ids_kernel(const double* __restrict__ rec, int64_t k, int64_t w, int64_t ld,
                                  int64_t* __restrict__ out) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < k) out[i] = int64_t(rec[i * w + ld + 2]);
}

// SV extraction on the device (main3.cpp:297-304): the ascending indices i < k with a[i] > tol, to
// keep_d (device) and keep_h (pinned host), and their count to *count_h.  One 1024-thread workgroup
// walks the set in 1024-element chunks: per wave a ballot + prefix count, per chunk the wave totals.
__global__ __launch_bounds__(1024) void select_svs_kernel(const double* __restrict__ a, int64_t k, double tol,
                                                          int64_t* __restrict__ keep_d, int64_t* __restrict__ keep_h,
                                                          int64_t* __restrict__ count_h) {
  __shared__ int64_t wsum[16];
  __shared__ int64_t base;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t c0 = 0; c0 < k; c0 += 1024) {
    const int64_t i = c0 + threadIdx.x;
    const bool f = i < k && a[i] > tol;
    const unsigned long long m = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int64_t off = base;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (f) {
      const int64_t pos = off + __popcll(m & ((1ull << lane) - 1ull));
      keep_d[pos] = i;
      keep_h[pos] = i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t t = 0;
      for (int q = 0; q < 16; ++q) t += wsum[q];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *count_h = base;
}

__global__ void coef_kernel(const double* __restrict__ a, const int32_t* __restrict__ y, int64_t nz,
                            double* __restrict__ coef) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < nz) coef[i] = a[i] * double(y[i]);
}

// One workgroup: f_i = s_i - y_i, then min f over I_high and max f over I_low (main3.cpp:107-142
// set definitions).  out = {b_high, b_low, #I_high, #I_low}.
__global__ __launch_bounds__(1024) void kkt_bounds_kernel(const double* __restrict__ s,
                                                          const int32_t* __restrict__ y,
                                                          const double* __restrict__ a, int64_t k, double C,
                                                          double eps, double* __restrict__ out) {
  double lo = __builtin_inf(), hi = -__builtin_inf();
  double nh = 0.0, nl = 0.0;
  for (int64_t i = threadIdx.x; i < k; i += blockDim.x) {
    const double f = s[i] - double(y[i]), ai = a[i];
    const bool pos = y[i] == 1;
    if ((pos && ai < C - eps) || (!pos && ai > eps)) {
      lo = fmin(lo, f);
      nh += 1.0;
    }
    if ((pos && ai > eps) || (!pos && ai < C - eps)) {
      hi = fmax(hi, f);
      nl += 1.0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, __shfl_xor(lo, off, kWave));
    hi = fmax(hi, __shfl_xor(hi, off, kWave));
    nh += __shfl_xor(nh, off, kWave);
    nl += __shfl_xor(nl, off, kWave);
  }
  __shared__ double part[16][4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w][0] = lo;
    part[w][1] = hi;
    part[w][2] = nh;
    part[w][3] = nl;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < int(blockDim.x >> 6); ++q) {
      lo = fmin(lo, part[q][0]);
      hi = fmax(hi, part[q][1]);
      nh += part[q][2];
      nl += part[q][3];
    }
    out[0] = lo;
    out[1] = hi;
    out[2] = nh;
    out[3] = nl;
  }
}

unsigned row_grid(int64_t m) { return unsigned(std::min<int64_t>(m, 8192)); }

}  // namespace

// --------------------------------------------------------------------------------- HipBackend
HipBackend::HipBackend(int device) : device_(device) {
  ctx_ = svmd_create(device);
  if (!ctx_) throw CascadeError(std::string("svmd_create: ") + svm_last_error());
  stream_ = static_cast<DeviceCtx*>(ctx_)->stream;
}
HipBackend::~HipBackend() {
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(stream_);
  for (auto& kv : cache_) (void)hipFree(kv.second);
  for (auto& kv : live_) (void)hipFree(kv.first);  // includes the grow() scratch (allocator blocks)
  if (pinned_) (void)hipHostFree(pinned_);
  if (stage_ev_) (void)hipEventDestroy(stage_ev_);
  svmd_destroy(ctx_);
}
void* HipBackend::alloc(int64_t bytes) {
  size_t cls = 256;
  while (cls < size_t(bytes)) cls <<= 1;
  auto it = cache_.find(cls);
  void* p = nullptr;
  if (it != cache_.end()) {
    p = it->second;
    cache_.erase(it);
  } else {
    hipcheck(hipSetDevice(device_), "hipSetDevice");
    if (hipMalloc(&p, cls) != hipSuccess) {
      release_cache();  // retry once with the cached blocks returned
      hipcheck(hipMalloc(&p, cls), "hipMalloc");
    }
  }
  live_[p] = cls;
  return p;
}
void HipBackend::free(void* p) {
  auto it = live_.find(p);
  if (it == live_.end()) return;
  cache_.emplace(it->second, p);
  live_.erase(it);
}
void HipBackend::upload_rows(const void* X, bool u8, int64_t n, int64_t d, double* dst) {
  if (!n) return;
  if (u8)
    check(svmd_upload_rows_u8(ctx_, static_cast<const uint8_t*>(X), n, d, dst, ld(d)), "svmd_upload_rows_u8");
  else
    check(svmd_upload_rows(ctx_, static_cast<const double*>(X), n, d, dst, ld(d)), "svmd_upload_rows");
}
void HipBackend::minmax(const double* X, int64_t n, int64_t d, double* mn, double* mx) {
  if (n == 0) {  // an empty partition contributes the identities of min / max
    const std::vector<double> hi(size_t(d), __builtin_inf()), lo(size_t(d), -__builtin_inf());
    h2d(mn, hi.data(), d * 8);
    h2d(mx, lo.data(), d * 8);
    return;
  }
  check(svmd_minmax(ctx_, X, n, d, ld(d), mn, mx), "svmd_minmax");
}
void HipBackend::scale(double* X, int64_t n, int64_t d, const double* mn, const double* mx) {
  check(svmd_preprocess(ctx_, X, n, d, ld(d), const_cast<double*>(mn), const_cast<double*>(mx), nullptr, 1),
        "svmd_preprocess");
}
void HipBackend::assemble(const Segment& s, int64_t ld, DSet& o, int64_t off) {
  const int64_t m = s.rows();
  if (!m) return;
  const int64_t* idx = nullptr;
  if (s.idx) idx = s.idx_dev ? s.idx_dev : stage_idx(*s.idx);
  if (s.set) {
    hipLaunchKernelGGL(assemble_set_kernel, dim3(row_grid(m)), dim3(256), 0, stream_, s.set->X.as<double>(),
                       s.set->y.as<int32_t>(), s.set->a.as<double>(), s.set->id.as<int64_t>(), idx, m, ld,
                       o.X.as<double>() + off * ld, o.y.as<int32_t>() + off, o.a.as<double>() + off,
                       o.id.as<int64_t>() + off, int(s.zero_alpha));
  } else {
    hipLaunchKernelGGL(assemble_rec_kernel, dim3(row_grid(m)), dim3(256), 0, stream_, s.rec, ld + 3, idx, m, ld,
                       o.X.as<double>() + off * ld, o.y.as<int32_t>() + off, o.a.as<double>() + off,
                       o.id.as<int64_t>() + off, int(s.zero_alpha));
  }
  hipcheck(hipGetLastError(), "assemble kernel");
}
void HipBackend::pack(const DSet& S, int64_t ld, double* rec) {
  if (!S.k) return;
  hipLaunchKernelGGL(pack_kernel, dim3(row_grid(S.k)), dim3(256), 0, stream_, S.X.as<double>(), S.y.as<int32_t>(),
                     S.a.as<double>(), S.id.as<int64_t>(), S.k, ld, rec);
  hipcheck(hipGetLastError(), "pack kernel");
}
void HipBackend::record_ids(const double* rec, int64_t k, int64_t ld, int64_t* ids) {
  if (!k) return;
  grow(&ids_d_, &ids_cap_, size_t(k) * 8);
  hipLaunchKernelGGL(record_ids_kernel, dim3(unsigned((k + 255) / 256)), dim3(256), 0, stream_, rec, k, ld + 3, ld,
                     static_cast<int64_t*>(ids_d_));
  hipcheck(hipGetLastError(), "record_ids kernel");
  d2h(ids, ids_d_, k * 8);
}
void HipBackend::record_ids_batch(const std::vector<const double*>& recs, const std::vector<int64_t>& ks, int64_t ld,
                                  const std::vector<int64_t*>& ids) {
  int64_t tot = 0;
  for (int64_t k : ks) tot += k;
  if (!tot) return;
  grow(&ids_d_, &ids_cap_, size_t(tot) * 8);
  int64_t off = 0;
  for (size_t q = 0; q < recs.size(); ++q) {
    if (!ks[q]) continue;
    hipLaunchKernelGGL(record_ids_kernel, dim3(unsigned((ks[q] + 255) / 256)), dim3(256), 0, stream_, recs[q], ks[q],
                       ld + 3, ld, static_cast<int64_t*>(ids_d_) + off);
    hipcheck(hipGetLastError(), "record_ids kernel");
    off += ks[q];
  }
  std::vector<int64_t> all(static_cast<size_t>(tot));
  d2h(all.data(), ids_d_, tot * 8);  // one round trip for every source
  off = 0;
  for (size_t q = 0; q < recs.size(); ++q) {
    std::copy(all.begin() + off, all.begin() + off + ks[q], ids[q]);
    off += ks[q];
  }
}
void HipBackend::select_svs(const DSet& S, double tol, std::vector<int64_t>* keep, const int64_t** keep_dev) {
  keep->clear();
  *keep_dev = nullptr;
  if (!S.k) return;
  grow(&sel_d_, &sel_cap_, size_t(S.k) * 8);
  grow_pinned(size_t(S.k) * 8 + 64);
  auto* cnt = reinterpret_cast<int64_t*>(pinned_);
  auto* kh = cnt + 8;
  *cnt = -1;
  hipLaunchKernelGGL(select_svs_kernel, dim3(1), dim3(1024), 0, stream_, S.a.as<double>(), S.k, tol,
                     static_cast<int64_t*>(sel_d_), kh, cnt);
  hipcheck(hipGetLastError(), "select kernel");
  hipcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  if (*cnt < 0 || *cnt > S.k) throw CascadeError("device SV selection returned no count");
  keep->assign(kh, kh + *cnt);
  *keep_dev = static_cast<const int64_t*>(sel_d_);
}
SolveStats HipBackend::solve(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h,
                             int solver, int64_t) {
  if (solver == 1) {  // the decomposition solver keeps no Gram: nothing to size or hand back
    SolveStats st;
    if (solo([&] { return solve_decomp(S, d, p, mn_h, mx_h, &st); })) return st;
  }
  if (!(serial_ && release_gram_)) return solo([&] { return solve_impl(S, d, p, mn_h, mx_h); });
  // Large-n rehearsals of P ranks on one GPU (SVM355_CASCADE_RELEASE_GRAM=1 with serial solves):
  // P resident Grams do not fit together, so each solve's Gram is sized before its timed region
  // (the grow-only buffer a rank keeps on its own GPU) and handed back after it, under the lock.
  return solo([&] { return solve_impl(S, d, p, mn_h, mx_h); },
              [&] { (void)svmd_reserve_gram(ctx_, S.k); },
              [&] { check(svmd_release_cache(ctx_), "svmd_release_cache"); });
}
bool HipBackend::warm_start_converged(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h,
                                      const double* mx_h) {
  return solo([&] { return kkt_check(S, nz, d, p, mn_h, mx_h); });
}
double HipBackend::take_solo_ms() {
  if (!solo_any_) return -1.0;
  const double v = solo_acc_;
  solo_acc_ = 0.0;
  solo_any_ = false;
  return v;
}
template <class F, class Pre, class Post>
decltype(std::declval<F&>()()) HipBackend::solo(F&& f, Pre&& pre, Post&& post) {
  if (!serial_) return f();
  std::lock_guard<std::mutex> lk(solo_mutex());
  pre();
  sync();
  const auto t0 = std::chrono::steady_clock::now();
  auto r = f();
  sync();
  solo_acc_ += ms_since(t0);
  solo_any_ = true;
  post();
  return r;
}
// Warm-started working-set decomposition (decomp.hip) on the set's scaled rows: quantised with the
// global statistics into the exact-integer plan, f = K (alpha y) - y from the warm alphas by the
// solver's GEMV, then the decomposition to the reference's stop test.  False (nothing done) when
// the set admits no exact-integer plan or has fewer than 2 rows: the pairwise solve runs instead.
bool HipBackend::solve_decomp(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h,
                              SolveStats* out) {
  if (S.k < 2 || !mn_h || !mx_h) return false;
  svm_result r{};
  int64_t st[kDecompStats] = {};
  bool used = false;
  double prep = 0.0;
  DecompOpts o;
  o.warm = true;
  // A/B probe: SVM355_DECOMP_CASCADE_START=cold starts every solve from alpha = 0 (the same local
  // optimum, another path); the reference warm-starts (mpi_svm_main3.cpp:169-186)
  if (const char* cs = getenv("SVM355_DECOMP_CASCADE_START")) o.warm = strcmp(cs, "cold") != 0;
  check(decomp_fit_rows(device_ctx(), S.X.as<double>(), S.k, ld(d), d, mn_h, mx_h, S.y.as<int32_t>(),
                        S.a.as<double>(), p, 1024, &r, st, &used, &prep, o),
        "decomposition SMO");
  if (!used) return false;
  *out = SolveStats{r.iterations, r.b, r.stop_reason, prep};
  out->solver = 1;
  out->outer = st[0];
  return true;
}
SolveStats HipBackend::solve_impl(DSet& S, int64_t d, const svm_params& p, const double* mn_h, const double* mx_h) {
  const int64_t ldd = ld(d);
  grow(&sqn_, &sqn_cap_, size_t(S.k) * 8);
  auto* sqn = static_cast<double*>(sqn_);
  check(svmd_row_norms(ctx_, S.X.as<double>(), S.k, d, ldd, sqn), "svmd_row_norms");
  svm_result r{};
  svmd_timing tm{};
  int32_t used = 0;
  // A partition whose k x k Gram does not fit (large-n cascades; ranks sharing one GPU in a
  // loopback rehearsal) is solved on the HBM row cache instead: the same exact-integer kernel
  // values, computed on demand (rowcache.hip / smo.hip's persistent row-cache solver).
  // SVM355_CASCADE_GRAM=rows forces that path (tests).
  const char* gm = getenv("SVM355_CASCADE_GRAM");
  int rc = SVM_ERR_OOM;
  if (!(gm && !strcmp(gm, "rows")))
    rc = svmd_train_q(ctx_, S.X.as<double>(), sqn, S.k, ldd, ldd, S.y.as<int32_t>(), S.a.as<double>(), 1, &p, &r,
                      nullptr, 0, &tm, mn_h, mx_h, d, 0, &used);
  const bool on_rows = rc == SVM_ERR_OOM;
  if (on_rows) {
    release_cache();  // unused blocks of this backend's set allocator, then the context's Gram
    check(svmd_release_cache(ctx_), "svmd_release_cache");
    rc = svmd_train_rows(ctx_, S.X.as<double>(), sqn, S.k, ldd, d, S.y.as<int32_t>(), S.a.as<double>(), 1, &p, &r,
                         mn_h, mx_h, 0, 0, &used, nullptr, 0);
  }
  check(rc, "svmd_train");
  return SolveStats{r.iterations, r.b, r.stop_reason, tm.gram_ms, on_rows};
}
// f from the cross-kernel K(S, S[0:nz]): the exact-integer block (int8 MFMA, the very values of
// the Gram the solve would build) for pixel data, else the MFMA f64 decision path, whose values
// agree with the Gram's to a few ulps, so f agrees to ~1e-9 here (nz <= a few thousand,
// alpha <= C); a 1e-7 margin on the stop test covers either.
// The check is an optimisation only: a failure of its own (e.g. its k x nz workspace does not fit
// next to a large partition) answers "not converged" and the normal solve runs.
bool HipBackend::kkt_check(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h,
                           const double* mx_h) {
  try {
    return kkt_check_impl(S, nz, d, p, mn_h, mx_h);
  } catch (const CascadeError&) {
    (void)hipGetLastError();  // clear a sticky launch / allocation error of the failed attempt
    return false;
  }
}
bool HipBackend::kkt_check_impl(DSet& S, int64_t nz, int64_t d, const svm_params& p, const double* mn_h,
                                const double* mx_h) {
  const char* e = getenv("SVM355_CASCADE_SKIP");  // =0 disables the check (A/B runs, tests)
  if ((e && atoi(e) == 0) || nz <= 0 || nz > S.k) return false;
  const int64_t ldd = ld(d), k = S.k;
  grow(&sqn_, &sqn_cap_, size_t(k) * 8);
  grow(&kkt_, &kkt_cap_, size_t(nz + k + 8) * 8);
  auto* sqn = static_cast<double*>(sqn_);
  auto* coef = static_cast<double*>(kkt_);
  double* sum = coef + nz;
  double* res = sum + k;
  check(svmd_row_norms(ctx_, S.X.as<double>(), k, d, ldd, sqn), "svmd_row_norms");
  hipLaunchKernelGGL(coef_kernel, dim3(unsigned((nz + 255) / 256)), dim3(256), 0, stream_, S.a.as<double>(),
                     S.y.as<int32_t>(), nz, coef);
  hipcheck(hipGetLastError(), "coef kernel");
  int32_t used_int = 0;
  const char* ki = getenv("SVM355_CASCADE_SKIP_INT");  // =0: always the f64 cross-kernel (A/B)
  if (!(ki && atoi(ki) == 0) && mn_h && mx_h)
    check(svmd_decision_int(ctx_, S.X.as<double>(), k, ldd, d, mn_h, mx_h, coef, nz, p.gamma, sum, &used_int),
          "svmd_decision_int");
  if (!used_int)
    check(svmd_decision(ctx_, S.X.as<double>(), sqn, coef, nz, ldd, S.X.as<double>(), sqn, k, ldd, ldd, p.gamma,
                        0.0, sum),
          "svmd_decision");
  hipLaunchKernelGGL(kkt_bounds_kernel, dim3(1), dim3(1024), 0, stream_, sum, S.y.as<int32_t>(), S.a.as<double>(), k,
                     p.C, p.eps, res);
  hipcheck(hipGetLastError(), "kkt kernel");
  double h[4];
  d2h(h, res, sizeof(h));
  if (h[2] < 1 || h[3] < 1) return false;  // no candidate: the solve reports it
  constexpr double kMargin = 1e-7;
  return h[1] <= h[0] + 2.0 * p.tau - kMargin;
}
// Grow-only scratch through the size-class caching allocator: the old block goes back to the
// cache (reuse is stream-ordered: every user runs on this backend's one stream), no sync, no
// hipFree.
void HipBackend::grow(void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return;
  if (*p) free(*p);
  *p = nullptr;
  *cap = 0;
  const size_t sz = std::max<size_t>(bytes, 4096) * 2;
  *p = alloc(int64_t(sz));
  *cap = sz;
}
// Pinned host staging area (grow-only; waits for the copy still reading it before it is reused).
void HipBackend::grow_pinned(size_t bytes) {
  wait_staged();
  if (bytes <= pinned_cap_) return;
  if (pinned_) {
    hipcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");  // a kernel may still write it
    hipcheck(hipHostFree(pinned_), "hipHostFree");
  }
  pinned_ = nullptr;
  pinned_cap_ = 0;
  const size_t sz = std::max<size_t>(bytes, 1 << 16) * 2;
  hipcheck(hipHostMalloc(&pinned_, sz, hipHostMallocDefault), "hipHostMalloc");
  pinned_cap_ = sz;
}
void HipBackend::wait_staged() {
  if (staged_) {
    hipcheck(hipEventSynchronize(stage_ev_), "hipEventSynchronize");
    staged_ = false;
  }
}
// Index list -> device through the pinned area with an asynchronous copy: the caller's vector may
// go away at once, and the next staging waits only for this copy (not for the whole stream).
const int64_t* HipBackend::stage_idx(const std::vector<int64_t>& v) {
  grow(&idx_, &idx_cap_, v.size() * 8);
  grow_pinned(v.size() * 8);
  std::memcpy(pinned_, v.data(), v.size() * 8);
  hipcheck(hipMemcpyAsync(idx_, pinned_, v.size() * 8, hipMemcpyHostToDevice, stream_), "hipMemcpyAsync idx");
  if (!stage_ev_) hipcheck(hipEventCreateWithFlags(&stage_ev_, hipEventDisableTiming), "hipEventCreate");
  hipcheck(hipEventRecord(stage_ev_, stream_), "hipEventRecord");
  staged_ = true;
  return static_cast<const int64_t*>(idx_);
}
void HipBackend::release_cache() {
  hipcheck(hipStreamSynchronize(stream_), "hipStreamSynchronize");
  for (auto& kv : cache_) (void)hipFree(kv.second);
  cache_.clear();
}

}  // namespace svm355

SVMD_TU_WARM(cascade_dev)
