// Sparse (CSR) rows x dense transposed panel -> RBF kernel values (gfx950): the decomposition solver's third
// row source, the decision function of sparse queries, and their C entries (svm355_device.h).
//
//   K_ij = exp(-gamma max(0, |a_i|^2 + |p_j|^2 - 2 a_i . p_j)),  a_i a CSR row, p_j one of <= 1024 panel rows
//
// The panel is dense and transposed, PT[c * ldp + j] = feature c of panel row j, so one nonzero (c, v) of a CSR
// row meets all the panel rows in one contiguous run of doubles.  Work split: 256-thread workgroups, one wave
// per CSR row; lane l owns the panel rows l, l + 64, ... in up to 16 FP64 accumulators; a row's (index, value)
// pairs are fetched 64 at a time, one pair per lane in two coalesced loads, and handed round the wave with
// readlane (the loop counter is wave-uniform, so index and value travel in scalar registers and the panel
// address is a scalar base plus the lane).  Every panel read is one coalesced 512-byte run.  No MFMA: the rows
// of a tile share no feature indices, so there is no common k dimension to feed a matrix instruction without
// densifying, which is what this path exists to avoid.
// Epilogues: `store` writes the block; `sum` / `sum_twin` fold it into f[i] += sum_j coef[j] K_ij in a fixed
// order (the lane's own columns ascending, then the wave_sum butterfly: the same bits on every run) and never
// write the block, so no rows x 1024 workspace exists on this path.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "csr_rbf.h"
#include "svm355_device.h"
#include "trace.h"

namespace svm355 {
namespace {

constexpr int kCsrAcc = kCsrPanelCols / kWave;  // accumulators per lane

// Lane t's value in every lane; t is wave-uniform (a loop counter).
__device__ __forceinline__ int32_t lane_bcast(int32_t v, int t) { return __builtin_amdgcn_readlane(v, t); }
__device__ __forceinline__ double lane_bcast(double v, int t) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), t),
                          __builtin_amdgcn_readlane(__double2loint(v), t));
}

template <CsrEpilogue EPI>
__global__ __launch_bounds__(256) void csr_rbf_kernel(CsrRows A, const double* __restrict__ PT, int64_t ldp,
                                                      const double* __restrict__ nP, CsrBlock b, double neg_gamma) {
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
  double acc[kCsrAcc];
#pragma unroll
  for (int g = 0; g < kCsrAcc; ++g) acc[g] = 0.0;
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
      for (int g = 0; g < kCsrAcc; ++g)
        if (g * kWave < ncols && g * kWave + lane < ncols) acc[g] += v * p[g * kWave];
    }
  }
  const double na = A.nrm[r];
  const int64_t rid = b.rowlist ? r : b.row_off + i;
  double sum = 0.0;
#pragma unroll
  for (int g = 0; g < kCsrAcc; ++g) {
    const int j = g * kWave + lane;
    if (g * kWave < ncols && j < ncols) {
      double dist = na + nP[j] - 2.0 * acc[g];
      dist = dist > 0.0 ? dist : 0.0;
      double kv = exp(neg_gamma * dist);
      if (b.pid && rid == int64_t(b.pid[j])) kv = 1.0;
      if (b.sym && i == j) kv = 1.0;
      if (EPI == CsrEpilogue::store)
        b.K[i * b.ldk + j] = kv;
      else
        sum += b.coef[j] * kv;
    }
  }
  if (EPI != CsrEpilogue::store) {
    sum = wave_sum(sum);
    if (lane == 0) {
      b.f[i] += sum;
      if (EPI == CsrEpilogue::sum_twin) b.f[i + b.m] += sum;
    }
  }
}

// One wave per listed row.  CLEAR: the previous rows' nonzero positions get 0.0; else: the rows ids[0 : *cnt]
// are written into panel positions 0 .. *cnt - 1 with their norms and become the previous rows.
template <bool CLEAR>
__global__ __launch_bounds__(256) void ws_scatter_csr_kernel(CsrRows A, const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ gate, int64_t twin_nrow,
                                                             CsrPanel P) {
  if (gate && *gate != 0) return;
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = max(0, min(CLEAR ? *P.prev_cnt : *cnt, min(kCsrPanelCols, int(P.ldp))));
  if (!CLEAR && k == 0 && lane == 0) *P.prev_cnt = n;  // read by the next CLEAR launch only
  if (k >= n) return;
  int64_t r = CLEAR ? P.prev[k] : ids[k];
  if (!CLEAR && twin_nrow > 0 && r >= twin_nrow) r -= twin_nrow;
  if (r < 0 || r >= A.n) {  // no such row: the position holds nothing (and clears nothing later)
    if (!CLEAR && lane == 0) {
      P.prev[k] = -1;
      P.nrm[k] = 0.0;
    }
    return;
  }
  if (!CLEAR && lane == 0) {
    P.prev[k] = int32_t(r);
    P.nrm[k] = A.nrm[r];
  }
  const int64_t end = A.indptr[r + 1];
  for (int64_t q = A.indptr[r] + lane; q < end; q += kWave) {
    const int32_t c = A.indices[q];
    if (c >= 0 && int64_t(c) < A.d) P.PT[int64_t(c) * P.ldp + k] = CLEAR ? 0.0 : A.values[q];
  }
}

// PT[(c0 + cc) * ldp + jj] = Xs[jj * lds + c0 + cc]: 64 x 64 tiles through LDS (+1 pad), reads coalesced along
// the features, writes along the panel rows.
__global__ __launch_bounds__(256) void csr_panel_transpose_kernel(const double* __restrict__ Xs, int64_t lds,
                                                                  int64_t cnt, double* __restrict__ PT, int64_t ldp) {
  __shared__ double tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j0 = int64_t(blockIdx.x) * 64, c0 = int64_t(blockIdx.y) * 64;
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t j = j0 + rr, c = c0 + tx;
    tile[rr][tx] = (j < cnt && c < lds) ? Xs[j * lds + c] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 64; rr += 4) {
    const int64_t c = c0 + rr, j = j0 + tx;
    if (c < lds && j < cnt) PT[c * ldp + j] = tile[tx][rr];
  }
}

// ---- prepare: column statistics, scaling by the column maximum, row norms ---------------------------------
// The stored values are >= 0 (the host has checked), so a double's bit pattern orders as an unsigned integer and
// min / max are integer atomics on global memory.
__global__ void csr_stats_init_kernel(unsigned long long* __restrict__ mnb, unsigned long long* __restrict__ mxb,
                                      int32_t* __restrict__ cnt, int64_t d) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= d) return;
  mnb[c] = 0x7FF0000000000000ull;  // +inf
  mxb[c] = 0ull;
  cnt[c] = 0;
}

__global__ void csr_stats_kernel(const int32_t* __restrict__ indices, const double* __restrict__ values, int64_t nnz,
                                 int64_t d, unsigned long long* __restrict__ mnb, unsigned long long* __restrict__ mxb,
                                 int32_t* __restrict__ cnt) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < nnz; q += stride) {
    const int32_t c = indices[q];
    if (c < 0 || int64_t(c) >= d) continue;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(values[q]));
    atomicMin(&mnb[c], bits);
    atomicMax(&mxb[c], bits);
    atomicAdd(&cnt[c], 1);
  }
}

// The bit patterns become doubles in place; a column stored in fewer than n rows has the implicit zeros' minimum.
__global__ void csr_stats_finish_kernel(double* __restrict__ mn, double* __restrict__ mx,
                                        const int32_t* __restrict__ cnt, int64_t d, int64_t n) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= d) return;
  const double lo = __longlong_as_double((long long)reinterpret_cast<unsigned long long*>(mn)[c]);
  const double hi = __longlong_as_double((long long)reinterpret_cast<unsigned long long*>(mx)[c]);
  mn[c] = int64_t(cnt[c]) < n ? 0.0 : lo;
  mx[c] = cnt[c] > 0 ? hi : 0.0;
}

// One wave per row: (SCALE) v /= max_c with the dense scaler's rule for a degenerate range (below 1e-12: 1), and
// the row's squared norm, lane-strided then the butterfly.
template <bool SCALE>
__global__ __launch_bounds__(256) void csr_scale_norms_kernel(const int64_t* __restrict__ indptr,
                                                              const int32_t* __restrict__ indices,
                                                              double* __restrict__ values, int64_t n, int64_t d,
                                                              const double* __restrict__ mx, double* __restrict__ nrm) {
  const int lane = threadIdx.x & 63;
  const int64_t r = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t end = indptr[r + 1];
  double s = 0.0;
  for (int64_t q = indptr[r] + lane; q < end; q += kWave) {
    double v = values[q];
    if (SCALE) {
      const int32_t c = indices[q];
      double range = (c >= 0 && int64_t(c) < d) ? mx[c] : 1.0;
      if (range < 1e-12) range = 1.0;
      v = v / range;
      values[q] = v;
    }
    s += v * v;
  }
  s = wave_sum(s);
  if (lane == 0) nrm[r] = s;
}

// Xo[k * ld + c] = the nonzeros of row ids[k] (Xo zeroed by the caller), no[k] = its norm: a model's support
// vectors as the dense padded rows every model holds.
__global__ __launch_bounds__(256) void csr_rows_dense_kernel(CsrRows A, const int64_t* __restrict__ ids, int64_t k,
                                                             double* __restrict__ Xo, int64_t ld,
                                                             double* __restrict__ no) {
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= k) return;
  const int64_t r = ids[i];
  if (r < 0 || r >= A.n) return;
  if (lane == 0) no[i] = A.nrm[r];
  const int64_t end = A.indptr[r + 1];
  for (int64_t q = A.indptr[r] + lane; q < end; q += kWave) {
    const int32_t c = A.indices[q];
    if (c >= 0 && int64_t(c) < A.d && int64_t(c) < ld) Xo[i * ld + c] = A.values[q];
  }
}

__global__ void csr_fill_kernel(double* __restrict__ v, int64_t n, double x) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) v[i] = x;
}
__global__ void csr_iota_kernel(int32_t* __restrict__ v, int n) {  // v[0 : n] = 0 .. n - 1, v[n] = n (the count)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) v[i] = i;
}

unsigned wave_rows_grid(int64_t rows) { return unsigned((rows + 3) / 4); }

bool csr_shape_ok(const CsrRows& A) {
  return A.indptr && A.nrm && A.n >= 0 && A.n < int64_t(INT32_MAX) && A.d >= 1 && A.d < int64_t(INT32_MAX);
}

}  // namespace

int launch_csr_rbf(hipStream_t s, CsrEpilogue e, const CsrRows& A, const CsrPanel& P, const CsrBlock& b) {
  const bool store = e == CsrEpilogue::store;
  if (!csr_shape_ok(A) || !P.PT || !P.nrm || b.ncap < 0 || b.ncap > kCsrPanelCols || P.ldp < b.ncap || b.m < 0 ||
      (store ? (!b.K || b.ldk < b.ncap) : (!b.coef || !b.f)) || (!b.rowlist && (b.arow0 < 0 || b.arow0 + b.m > A.n))) {
    set_error("csr rbf block: bad arguments");
    return SVM_ERR_ARG;
  }
  if (b.m == 0 || b.ncap == 0) return SVM_OK;
  const dim3 grid(wave_rows_grid(b.m)), block(256);
  const double ng = -b.gamma;
  switch (e) {
    case CsrEpilogue::store:
      hipLaunchKernelGGL(csr_rbf_kernel<CsrEpilogue::store>, grid, block, 0, s, A, P.PT, P.ldp, P.nrm, b, ng);
      break;
    case CsrEpilogue::sum:
      hipLaunchKernelGGL(csr_rbf_kernel<CsrEpilogue::sum>, grid, block, 0, s, A, P.PT, P.ldp, P.nrm, b, ng);
      break;
    case CsrEpilogue::sum_twin:
      hipLaunchKernelGGL(csr_rbf_kernel<CsrEpilogue::sum_twin>, grid, block, 0, s, A, P.PT, P.ldp, P.nrm, b, ng);
      break;
  }
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_csr_panel_scatter(hipStream_t s, const CsrRows& A, const int32_t* ids, const int32_t* cnt,
                             const int32_t* gate, int64_t twin_nrow, const CsrPanel& P) {
  if (!csr_shape_ok(A) || !ids || !cnt || !P.PT || !P.nrm || !P.prev || !P.prev_cnt || P.ldp < 1) {
    set_error("csr panel scatter: bad arguments");
    return SVM_ERR_ARG;
  }
  const dim3 grid(kCsrPanelCols / 4), block(256);
  hipLaunchKernelGGL(ws_scatter_csr_kernel<true>, grid, block, 0, s, A, ids, cnt, gate, twin_nrow, P);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ws_scatter_csr_kernel<false>, grid, block, 0, s, A, ids, cnt, gate, twin_nrow, P);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_csr_panel_from_dense(hipStream_t s, const double* Xs, int64_t lds, int64_t cnt, double* PT, int64_t ldp) {
  if (!Xs || !PT || lds < 1 || cnt < 0 || cnt > ldp) {
    set_error("csr panel transpose: bad arguments");
    return SVM_ERR_ARG;
  }
  if (cnt == 0) return SVM_OK;
  hipLaunchKernelGGL(csr_panel_transpose_kernel, dim3(unsigned((cnt + 63) / 64), unsigned((lds + 63) / 64)), dim3(256),
                     0, s, Xs, lds, cnt, PT, ldp);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

namespace {

// The caller's device arrays as rows; false (the error set) when a pointer or a size is missing.
bool csr_from_args(const char* who, const int64_t* indptr, const int32_t* indices, const double* values,
                   const double* nrm, int64_t n, int64_t d, int64_t min_rows, CsrRows* A) {
  *A = CsrRows{indptr, indices, values, nrm, n, d};
  // indices / values may be null only for rows that are all empty, which the callers never upload as null
  if (!csr_shape_ok(*A) || n < min_rows || !indices || !values) {
    set_error("%s: bad arguments", who);
    return false;
  }
  return true;
}

// A panel of d x kCsrPanelCols doubles, its norms, the scatter's bookkeeping and kCsrPanelCols + 1 ids in the
// context's workspace.
struct PanelWs {
  CsrPanel P;
  int32_t* ids = nullptr;
};
int panel_ws(DeviceCtx* ctx, int64_t d, PanelWs* out) {
  return carve_ws(ctx, [&](WsCarver& c) {
    out->P.PT = c.take<double>(size_t(d) * kCsrPanelCols);
    out->P.ldp = kCsrPanelCols;
    out->P.nrm = c.take<double>(kCsrPanelCols);
    out->P.prev = c.take<int32_t>(kCsrPanelCols);
    out->P.prev_cnt = c.take<int32_t>(64);
    out->ids = c.take<int32_t>(kCsrPanelCols + 64);
  });
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" {

// mode 0: the rows' squared norms only.  mode 1: the training prepare -- per column the stored values' minimum
// (0 when a row does not store the column), maximum and stored count into colmin_d / colmax_d / colcnt_d (d
// each), then values /= max_c in place and the norms of the scaled rows.  mode 2: the query prepare -- values
// scaled in place by the given colmax_d, and the norms.
SVM_API int svmd_csr_prepare(void* h, const int64_t* indptr_d, const int32_t* indices_d, double* values_d, int64_t n,
                             int64_t d, int64_t nnz, int32_t mode, double* colmin_d, double* colmax_d,
                             int32_t* colcnt_d, double* nrm_d) {
  SVMD_CTX(h);
  CsrRows A;
  if (!csr_from_args("svmd_csr_prepare", indptr_d, indices_d, values_d, nrm_d, n, d, 0, &A) || nnz < 0 || mode < 0 ||
      mode > 2 || (mode == 1 && (!colmin_d || !colmax_d || !colcnt_d)) || (mode == 2 && !colmax_d)) {
    set_error("svmd_csr_prepare: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  TraceRange tr("svm355:csr_prepare");
  hipStream_t s = ctx->stream;
  if (mode == 1) {
    auto* mnb = reinterpret_cast<unsigned long long*>(colmin_d);
    auto* mxb = reinterpret_cast<unsigned long long*>(colmax_d);
    const unsigned cg = unsigned((d + 255) / 256);
    hipLaunchKernelGGL(csr_stats_init_kernel, dim3(cg), dim3(256), 0, s, mnb, mxb, colcnt_d, d);
    SVMD_LAUNCH_CHECK();
    if (nnz > 0) {
      const unsigned g = unsigned(std::min<int64_t>((nnz + 255) / 256, 4096));
      hipLaunchKernelGGL(csr_stats_kernel, dim3(g), dim3(256), 0, s, indices_d, values_d, nnz, d, mnb, mxb, colcnt_d);
      SVMD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(csr_stats_finish_kernel, dim3(cg), dim3(256), 0, s, colmin_d, colmax_d, colcnt_d, d, n);
    SVMD_LAUNCH_CHECK();
  }
  if (n > 0) {
    if (mode == 0)
      hipLaunchKernelGGL(csr_scale_norms_kernel<false>, dim3(wave_rows_grid(n)), dim3(256), 0, s, indptr_d, indices_d,
                         values_d, n, d, colmax_d, nrm_d);
    else
      hipLaunchKernelGGL(csr_scale_norms_kernel<true>, dim3(wave_rows_grid(n)), dim3(256), 0, s, indptr_d, indices_d,
                         values_d, n, d, colmax_d, nrm_d);
    SVMD_LAUNCH_CHECK();
  }
  return ctx->end();
}

// K_d[i * ldk + j] = K(CSR row i of A, CSR row j of B) for the m rows of A and the nb <= 1024 rows of B (both
// with d features): B's rows scattered into a zeroed transposed panel, then the store kernel.  idsB_d (optional,
// int32[nb]): B row j is training row idsB_d[j], and A row i is training row row_off + i; that pair's value is
// exactly 1.  sym != 0: K[i][i] = 1.
SVM_API int svmd_rbf_block_csr(void* h, const int64_t* a_indptr_d, const int32_t* a_indices_d,
                               const double* a_values_d, const double* a_nrm_d, int64_t m, int64_t row_off,
                               const int64_t* b_indptr_d, const int32_t* b_indices_d, const double* b_values_d,
                               const double* b_nrm_d, int64_t nb, int64_t d, const int32_t* idsB_d, double gamma,
                               int32_t sym, double* K_d, int64_t ldk) {
  SVMD_CTX(h);
  CsrRows A, B;
  if (!csr_from_args("svmd_rbf_block_csr", a_indptr_d, a_indices_d, a_values_d, a_nrm_d, m, d, 1, &A) ||
      !csr_from_args("svmd_rbf_block_csr", b_indptr_d, b_indices_d, b_values_d, b_nrm_d, nb, d, 1, &B) ||
      nb > kCsrPanelCols || !K_d || ldk < nb) {
    set_error("svmd_rbf_block_csr: bad arguments (1 <= nb <= %d, ldk >= nb)", kCsrPanelCols);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  PanelWs w;
  if ((rc = panel_ws(ctx, d, &w))) return rc;
  hipStream_t s = ctx->stream;
  SVMD_CHECK(hipMemsetAsync(w.P.PT, 0, size_t(d) * kCsrPanelCols * 8, s));
  SVMD_CHECK(hipMemsetAsync(w.P.prev_cnt, 0, 4, s));
  hipLaunchKernelGGL(csr_iota_kernel, dim3((unsigned(nb) + 256) / 256), dim3(256), 0, s, w.ids, int(nb));
  SVMD_LAUNCH_CHECK();
  if ((rc = launch_csr_panel_scatter(s, B, w.ids, w.ids + nb, nullptr, 0, w.P))) return rc;
  CsrBlock b;
  b.m = m;
  b.row_off = row_off;
  b.ncap = int(nb);
  b.pid = idsB_d;
  b.gamma = gamma;
  b.K = K_d;
  b.ldk = ldk;
  b.sym = sym != 0;
  if ((rc = launch_csr_rbf(s, CsrEpilogue::store, A, w.P, b))) return rc;
  return ctx->end();
}

// out_d[i] = sum_k coef_d[k] K(query row i, Xs row k) - b for m CSR query rows (scaled as the model's rows, with
// their norms nq_d) against a model's dense support vectors Xs_d (nsv x lds, norms ns_d): chunks of 1024 support
// vectors, each transposed into the panel and folded in by the sum kernel, in order.  The same bits on every run.
SVM_API int svmd_decision_csr(void* h, const int64_t* indptr_d, const int32_t* indices_d, const double* values_d,
                              const double* nq_d, int64_t m, int64_t d, const double* Xs_d, const double* ns_d,
                              const double* coef_d, int64_t nsv, int64_t lds, double gamma, double b, double* out_d) {
  SVMD_CTX(h);
  if (m <= 0) return SVM_OK;
  CsrRows A;
  if (!csr_from_args("svmd_decision_csr", indptr_d, indices_d, values_d, nq_d, m, d, 1, &A) || !out_d || nsv < 0 ||
      (nsv > 0 && (!Xs_d || !ns_d || !coef_d || lds < d))) {
    set_error("svmd_decision_csr: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  TraceRange tr("svm355:decision_csr");
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(csr_fill_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, s, out_d, m, -b);
  SVMD_LAUNCH_CHECK();
  if (nsv == 0) return ctx->end();
  PanelWs w;
  if ((rc = panel_ws(ctx, lds, &w))) return rc;
  for (int64_t j0 = 0; j0 < nsv; j0 += kCsrPanelCols) {
    const int64_t cnt = std::min<int64_t>(kCsrPanelCols, nsv - j0);
    if ((rc = launch_csr_panel_from_dense(s, Xs_d + j0 * lds, lds, cnt, w.P.PT, w.P.ldp))) return rc;
    CsrPanel P = w.P;
    P.nrm = const_cast<double*>(ns_d + j0);
    CsrBlock blk;
    blk.m = m;
    blk.ncap = int(cnt);
    blk.gamma = gamma;
    blk.coef = coef_d + j0;
    blk.f = out_d;
    if ((rc = launch_csr_rbf(s, CsrEpilogue::sum, A, P, blk))) return rc;
  }
  return ctx->end();
}

// Xs_d[k * ld + c] (k x ld, ld >= d, written whole: zeros and the rows' nonzeros) = CSR rows ids_d[0 : k], and
// ns_d[k] their norms: the support vectors of a fit on sparse rows as every model's dense padded rows.
SVM_API int svmd_csr_rows_dense(void* h, const int64_t* indptr_d, const int32_t* indices_d, const double* values_d,
                                const double* nrm_d, int64_t n, int64_t d, const int64_t* ids_d, int64_t k,
                                double* Xs_d, int64_t ld, double* ns_d) {
  SVMD_CTX(h);
  if (k <= 0) return SVM_OK;
  CsrRows A;
  if (!csr_from_args("svmd_csr_rows_dense", indptr_d, indices_d, values_d, nrm_d, n, d, 1, &A) || !ids_d || !Xs_d ||
      !ns_d || ld < d) {
    set_error("svmd_csr_rows_dense: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const int64_t tot = k * ld;
  hipLaunchKernelGGL(csr_fill_kernel, dim3(unsigned((tot + 255) / 256)), dim3(256), 0, s, Xs_d, tot, 0.0);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(csr_rows_dense_kernel, dim3(wave_rows_grid(k)), dim3(256), 0, s, A, ids_d, k, Xs_d, ld, ns_d);
  SVMD_LAUNCH_CHECK();
  return ctx->end();
}

}  // extern "C"
