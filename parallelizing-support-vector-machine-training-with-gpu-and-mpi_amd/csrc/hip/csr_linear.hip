// The linear kernel on sparse (CSR) rows (gfx950): K(W, W) as a dot block against the transposed panel, the f
// update as a weight-vector delta plus one CSR x vector product, a model's weight vector, and the decision
// function of CSR queries (csr_linear.h has the factoring).  Three kernels, 256-thread workgroups of four waves:
//
//   csr_dot_kernel           one wave per CSR row, csr_rbf_kernel's mapping: lane l owns the panel rows l, l + 64,
//                            ... in up to 16 FP64 accumulators; the row's (index, value) pairs are fetched 64 at a
//                            time, one pair per lane in two coalesced loads, and handed round the wave with readlane,
//                            so index and value travel in scalar registers and every panel read is one coalesced
//                            512-byte run.  The accumulators are the block: no norms, no exp, no diagonal.
//   csr_panel_reduce_kernel  one wave per feature row of the panel; a workgroup walks several feature rows, so a
//                            lane's 16 coefficients coef[l + 64 g] are loaded into registers once.  Every panel read
//                            is a coalesced 512-byte run bounded by the device-side count; the lane's own columns
//                            are summed in ascending order, then the wave_sum butterfly -- a fixed order, where atomic
//                            adds from the moved rows would have none.
//   csr_matvec_kernel        one wave per CSR row: the lanes stride the stored values and gather v[index] (8 bytes
//                            per stored value), the butterfly, and lane 0 adds to f (twin: to both of the row's points).
// No MFMA: as in csr_rbf.hip the rows of a tile share no feature indices, so there is no common k dimension.
#include <algorithm>

#include "csr_linear.h"
#include "svm355_device.h"
#include "trace.h"

namespace svm355 {
namespace {

constexpr int kLinAcc = kCsrPanelCols / kWave;  // accumulators (and coefficients) per lane
constexpr unsigned kLinReduceGrid = 1024;       // workgroups of the reduce at most: 4,096 waves share the feature rows

// Lane t's value in every lane; t is wave-uniform (a loop counter).
__device__ __forceinline__ int32_t lane_bcast(int32_t v, int t) { return __builtin_amdgcn_readlane(v, t); }
__device__ __forceinline__ double lane_bcast(double v, int t) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), t),
                          __builtin_amdgcn_readlane(__double2loint(v), t));
}

__global__ __launch_bounds__(256) void csr_dot_kernel(CsrRows A, const double* __restrict__ PT, int64_t ldp,
                                                      CsrBlock b) {
  if (b.gate && *b.gate != 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int ncols = b.ncount ? min(*b.ncount, b.ncap) : b.ncap;
  const int64_t m = (b.rowcount && int64_t(*b.rowcount) < b.m) ? int64_t(*b.rowcount) : b.m;
  if (i >= m || ncols <= 0) return;  // wave-uniform: a wave is one row
  int64_t r = b.arow0 + i;
  if (b.rowlist) {
    r = b.rowlist[i];
    if (b.twin_nrow > 0 && r >= b.twin_nrow) r -= b.twin_nrow;
  }
  if (r < 0 || r >= A.n) return;
  const int64_t beg = A.indptr[r], end = A.indptr[r + 1];
  double acc[kLinAcc];
#pragma unroll
  for (int g = 0; g < kLinAcc; ++g) acc[g] = 0.0;
  for (int64_t base = beg; base < end; base += kWave) {
    const int cnt = end - base < kWave ? int(end - base) : kWave;
    int32_t ci = 0;
    double cv = 0.0;
    if (lane < cnt) {
      ci = A.indices[base + lane];
      cv = A.values[base + lane];
    }
    for (int t = 0; t < cnt; ++t) {
      const int32_t c = lane_bcast(ci, t);
      const double v = lane_bcast(cv, t);
      if (c < 0 || int64_t(c) >= A.d) continue;  // never read outside the panel (the host has checked the indices)
      const double* __restrict__ p = PT + int64_t(c) * ldp + lane;
#pragma unroll
      for (int g = 0; g < kLinAcc; ++g)
        if (g * kWave < ncols && g * kWave + lane < ncols) acc[g] += v * p[g * kWave];
    }
  }
  double* __restrict__ out = b.K + i * b.ldk + lane;
#pragma unroll
  for (int g = 0; g < kLinAcc; ++g)
    if (g * kWave < ncols && g * kWave + lane < ncols) out[g * kWave] = acc[g];
}

template <bool ACC>
__global__ __launch_bounds__(256) void csr_panel_reduce_kernel(const double* __restrict__ PT, int64_t ldp, int64_t nrows,
                                                               const double* __restrict__ coef, int ncap,
                                                               const int32_t* __restrict__ count,
                                                               double* __restrict__ w) {
  const int lane = threadIdx.x & 63;
  const int cnt = max(0, min(count ? *count : ncap, ncap));
  if (ACC && cnt == 0) return;
  double cf[kLinAcc];
#pragma unroll
  for (int g = 0; g < kLinAcc; ++g) cf[g] = (g * kWave + lane < cnt) ? coef[g * kWave + lane] : 0.0;
  const int64_t stride = int64_t(gridDim.x) * 4;
  for (int64_t c = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); c < nrows; c += stride) {  // wave-uniform
    const double* __restrict__ p = PT + c * ldp + lane;
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < kLinAcc; ++g)
      if (g * kWave < cnt && g * kWave + lane < cnt) sum += cf[g] * p[g * kWave];
    sum = wave_sum(sum);
    if (lane == 0) w[c] = ACC ? w[c] + sum : sum;
  }
}

template <bool TWIN>
__global__ __launch_bounds__(256) void csr_matvec_kernel(CsrRows A, int64_t arow0, int64_t m,
                                                         const double* __restrict__ v,
                                                         const int32_t* __restrict__ count, double* __restrict__ f) {
  if (count && *count <= 0) return;
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= m) return;  // wave-uniform: a wave is one row
  const int64_t r = arow0 + i;
  if (r < 0 || r >= A.n) return;
  const int64_t end = A.indptr[r + 1];
  double sum = 0.0;
  for (int64_t q = A.indptr[r] + lane; q < end; q += kWave) {
    const int32_t c = A.indices[q];
    if (c >= 0 && int64_t(c) < A.d) sum += A.values[q] * v[c];
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    f[i] += sum;
    if (TWIN) f[i + m] += sum;
  }
}

__global__ void lin_fill_kernel(double* __restrict__ v, int64_t n, double x) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) v[i] = x;
}
__global__ void lin_iota_kernel(int32_t* __restrict__ v, int n) {  // v[0 : n] = 0 .. n - 1, v[n] = n (the count)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) v[i] = i;
}

unsigned wave_rows_grid(int64_t rows) { return unsigned((rows + 3) / 4); }

bool lin_rows_ok(const CsrRows& A) {
  return A.indptr && A.indices && A.values && A.n >= 0 && A.n < int64_t(INT32_MAX) && A.d >= 1 &&
         A.d < int64_t(INT32_MAX);
}

}  // namespace

int launch_csr_dot_block(hipStream_t s, const CsrRows& A, const CsrPanel& P, const CsrBlock& b) {
  if (!lin_rows_ok(A) || !P.PT || b.ncap < 0 || b.ncap > kCsrPanelCols || P.ldp < b.ncap || b.m < 0 || !b.K ||
      b.ldk < b.ncap || (!b.rowlist && (b.arow0 < 0 || b.arow0 + b.m > A.n))) {
    set_error("csr dot block: bad arguments");
    return SVM_ERR_ARG;
  }
  if (b.m == 0 || b.ncap == 0) return SVM_OK;
  hipLaunchKernelGGL(csr_dot_kernel, dim3(wave_rows_grid(b.m)), dim3(256), 0, s, A, P.PT, P.ldp, b);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_csr_panel_reduce(hipStream_t s, const double* PT, int64_t ldp, int64_t nrows, const double* coef, int ncap,
                            const int32_t* count, bool accumulate, double* w) {
  if (!PT || !coef || !w || nrows < 0 || ncap < 0 || ncap > kCsrPanelCols || ldp < ncap) {
    set_error("csr panel reduce: bad arguments");
    return SVM_ERR_ARG;
  }
  if (nrows == 0) return SVM_OK;
  const dim3 grid(std::min(wave_rows_grid(nrows), kLinReduceGrid)), block(256);
  if (accumulate)
    hipLaunchKernelGGL(csr_panel_reduce_kernel<true>, grid, block, 0, s, PT, ldp, nrows, coef, ncap, count, w);
  else
    hipLaunchKernelGGL(csr_panel_reduce_kernel<false>, grid, block, 0, s, PT, ldp, nrows, coef, ncap, count, w);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_csr_matvec(hipStream_t s, const CsrRows& A, int64_t arow0, int64_t m, const double* v, bool twin,
                      const int32_t* count, double* f) {
  if (!lin_rows_ok(A) || !v || !f || m < 0 || arow0 < 0 || arow0 + m > A.n) {
    set_error("csr matvec: bad arguments");
    return SVM_ERR_ARG;
  }
  if (m == 0) return SVM_OK;
  const dim3 grid(wave_rows_grid(m)), block(256);
  if (twin)
    hipLaunchKernelGGL(csr_matvec_kernel<true>, grid, block, 0, s, A, arow0, m, v, count, f);
  else
    hipLaunchKernelGGL(csr_matvec_kernel<false>, grid, block, 0, s, A, arow0, m, v, count, f);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_linear_weight_vector(hipStream_t s, const double* Xs, const double* coef, int64_t nsv, int64_t lds,
                                double* PT, int64_t ldp, double* w) {
  if (!PT || !w || lds < 1 || ldp < kCsrPanelCols || nsv < 0 || (nsv > 0 && (!Xs || !coef))) {
    set_error("linear weight vector: bad arguments");
    return SVM_ERR_ARG;
  }
  if (nsv == 0) {
    hipLaunchKernelGGL(lin_fill_kernel, dim3(unsigned((lds + 255) / 256)), dim3(256), 0, s, w, lds, 0.0);
    SVMD_LAUNCH_CHECK();
    return SVM_OK;
  }
  for (int64_t j0 = 0; j0 < nsv; j0 += kCsrPanelCols) {
    const int64_t cnt = std::min<int64_t>(kCsrPanelCols, nsv - j0);
    int rc = launch_csr_panel_from_dense(s, Xs + j0 * lds, lds, cnt, PT, ldp);
    if (rc || (rc = launch_csr_panel_reduce(s, PT, ldp, lds, coef + j0, int(cnt), nullptr, j0 > 0, w))) return rc;
  }
  return SVM_OK;
}

namespace {

// The caller's device arrays as rows; false (the error set) when a pointer or a size is missing.
bool lin_from_args(const char* who, const int64_t* indptr, const int32_t* indices, const double* values,
                   const double* nrm, int64_t n, int64_t d, CsrRows* A) {
  *A = CsrRows{indptr, indices, values, nrm, n, d};
  if (!lin_rows_ok(*A) || n < 1) {
    set_error("%s: bad arguments", who);
    return false;
  }
  return true;
}

// A zeroed d x kCsrPanelCols panel with B's first *cnt rows scattered into positions 0 .. *cnt - 1, in the context's
// workspace; extra doubles follow the panel's parts.  cnt_d: the device-side count (its value is `cnt`).
struct LinPanel {
  CsrPanel P;
  int32_t* cnt_d = nullptr;
  double* extra = nullptr;
};
int lin_panel(DeviceCtx* ctx, const CsrRows& B, int64_t d, int cnt, size_t extra, LinPanel* out) {
  int32_t* ids = nullptr;
  int rc = carve_ws(ctx, [&](WsCarver& c) {
    out->P.PT = c.take<double>(size_t(d) * kCsrPanelCols);
    out->P.ldp = kCsrPanelCols;
    out->P.nrm = c.take<double>(kCsrPanelCols);
    out->P.prev = c.take<int32_t>(kCsrPanelCols);
    out->P.prev_cnt = c.take<int32_t>(64);
    ids = c.take<int32_t>(kCsrPanelCols + 64);
    out->extra = c.take<double>(extra, extra > 0);
  });
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  SVMD_CHECK(hipMemsetAsync(out->P.PT, 0, size_t(d) * kCsrPanelCols * 8, s));
  SVMD_CHECK(hipMemsetAsync(out->P.prev_cnt, 0, 4, s));
  hipLaunchKernelGGL(lin_iota_kernel, dim3((unsigned(cnt) + 256) / 256), dim3(256), 0, s, ids, cnt);
  SVMD_LAUNCH_CHECK();
  out->cnt_d = ids + cnt;
  return launch_csr_panel_scatter(s, B, ids, out->cnt_d, nullptr, 0, out->P);
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" {

// K_d[i * ldk + j] = (CSR row i of A) . (CSR row j of B) for the m rows of A and the 1 <= nb <= 1024 rows of B
// (both with d features, prepared: the scatter copies the norms): B's rows scattered into a zeroed transposed
// panel, then the dot block.
SVM_API int svmd_linear_block_csr(void* h, const int64_t* a_indptr_d, const int32_t* a_indices_d,
                                  const double* a_values_d, const double* a_nrm_d, int64_t m,
                                  const int64_t* b_indptr_d, const int32_t* b_indices_d, const double* b_values_d,
                                  const double* b_nrm_d, int64_t nb, int64_t d, double* K_d, int64_t ldk) {
  const char* who = "svmd_linear_block_csr";
  SVMD_CTX(h);
  CsrRows A, B;
  if (!lin_from_args(who, a_indptr_d, a_indices_d, a_values_d, a_nrm_d, m, d, &A) ||
      !lin_from_args(who, b_indptr_d, b_indices_d, b_values_d, b_nrm_d, nb, d, &B) || !a_nrm_d || !b_nrm_d ||
      nb > kCsrPanelCols || !K_d || ldk < nb) {
    set_error("%s: bad arguments (1 <= nb <= %d, ldk >= nb)", who, kCsrPanelCols);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  LinPanel w;
  if ((rc = lin_panel(ctx, B, d, int(nb), 0, &w))) return rc;
  CsrBlock b;
  b.m = m;
  b.ncap = int(nb);
  b.K = K_d;
  b.ldk = ldk;
  if ((rc = launch_csr_dot_block(ctx->stream, A, w.P, b))) return rc;
  return ctx->end();
}

// f_d[i] += a_i . (B[0 : count]' coef_d) for the m rows of A (twin != 0: f_d holds 2 m values and f_d[i + m] gets
// the same sum), exactly as the solver's f update runs it: B's first `count` rows (count < 0: all nb <= 1024)
// scattered into the panel, the panel reduce under the device-side count, then the CSR x vector product.  A count
// of 0 leaves f_d as it is, bit for bit.
SVM_API int svmd_linear_fupdate_csr(void* h, const int64_t* a_indptr_d, const int32_t* a_indices_d,
                                    const double* a_values_d, const double* a_nrm_d, int64_t m,
                                    const int64_t* b_indptr_d, const int32_t* b_indices_d, const double* b_values_d,
                                    const double* b_nrm_d, int64_t nb, int64_t d, const double* coef_d, int32_t count,
                                    int32_t twin, double* f_d) {
  const char* who = "svmd_linear_fupdate_csr";
  SVMD_CTX(h);
  CsrRows A, B;
  if (!lin_from_args(who, a_indptr_d, a_indices_d, a_values_d, a_nrm_d, m, d, &A) ||
      !lin_from_args(who, b_indptr_d, b_indices_d, b_values_d, b_nrm_d, nb, d, &B) || !a_nrm_d || !b_nrm_d ||
      nb > kCsrPanelCols || count > nb || !coef_d || !f_d) {
    set_error("%s: bad arguments (1 <= nb <= %d, count <= nb)", who, kCsrPanelCols);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  LinPanel w;
  if ((rc = lin_panel(ctx, B, d, count < 0 ? int(nb) : int(count), size_t(d), &w))) return rc;
  hipStream_t s = ctx->stream;
  if ((rc = launch_csr_panel_reduce(s, w.P.PT, w.P.ldp, d, coef_d, kCsrPanelCols, w.cnt_d, false, w.extra)) ||
      (rc = launch_csr_matvec(s, A, 0, m, w.extra, twin != 0, w.cnt_d, f_d)))
    return rc;
  return ctx->end();
}

// w_d[0 : lds] = sum_k coef_d[k] Xs_d[k * lds + :]: a linear model's weight vector from its nsv dense padded support
// vectors, 1024 at a time through the transposed panel, chunk by chunk in order.
SVM_API int svmd_linear_w(void* h, const double* Xs_d, const double* coef_d, int64_t nsv, int64_t lds, double* w_d) {
  SVMD_CTX(h);
  if (!w_d || lds < 1 || nsv < 0 || (nsv > 0 && (!Xs_d || !coef_d))) {
    set_error("svmd_linear_w: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  TraceRange tr("svm355:linear_w");
  double* PT = nullptr;
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { PT = c.take<double>(size_t(lds) * kCsrPanelCols); }))) return rc;
  if ((rc = launch_linear_weight_vector(ctx->stream, Xs_d, coef_d, nsv, lds, PT, kCsrPanelCols, w_d))) return rc;
  return ctx->end();
}

// out_d[i] = (CSR query row i) . w_d - b for m query rows of d features (scaled as the model's rows; w_d: at least d
// doubles): the fill, then the CSR x vector product.
SVM_API int svmd_decision_csr_linear(void* h, const int64_t* indptr_d, const int32_t* indices_d,
                                     const double* values_d, const double* nq_d, int64_t m, int64_t d,
                                     const double* w_d, double b, double* out_d) {
  SVMD_CTX(h);
  if (m <= 0) return SVM_OK;
  CsrRows A;
  if (!lin_from_args("svmd_decision_csr_linear", indptr_d, indices_d, values_d, nq_d, m, d, &A) || !w_d || !out_d) {
    set_error("svmd_decision_csr_linear: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  TraceRange tr("svm355:decision_csr_linear");
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(lin_fill_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, s, out_d, m, -b);
  SVMD_LAUNCH_CHECK();
  if ((rc = launch_csr_matvec(s, A, 0, m, w_d, false, nullptr, out_d))) return rc;
  return ctx->end();
}

}  // extern "C"
