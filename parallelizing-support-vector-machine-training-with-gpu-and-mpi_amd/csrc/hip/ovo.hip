// One-vs-one multi-class prediction on the device (gfx950): the pair decisions and the votes from one
// cross-kernel block K (m x nsv) against the union of support vectors, which lie grouped by class
// (segment c = [start[c], start[c + 1])), and LIBSVM's (k - 1) x nsv coefficient matrix: for a support vector
// s of class c, row j holds its alpha * y in the pair (c, o), o = j for j < c, else j + 1.  Pair p = (a, b),
// a < b, in the order (0,1), (0,2), ..., (k-2,k-1):
//
//   dec[p] = sum_{s in seg a} coef[b - 1][s] K[s]  +  sum_{s in seg b} coef[a][s] K[s]  -  rho[p]
//
// dec > 0 votes for a, anything else (exactly 0 and NaN included) for b; the label is the class index with
// the most votes, the lowest index on a tie.
//
// One 256-thread workgroup per 4 query rows (per row above 32 classes, where four rows' sums would not fit
// 64 KB of LDS).  Wave w takes the classes w, w + 4, ...; over a class's segment lane l adds the terms
// s = start + l, + 64, ... in ascending order into one running sum per row of coef and query row, at most
// kOvoGroup rows of coef at a time so that the registers stay bounded (the K values of a segment are read once
// per group, the later groups from L1; a coefficient is loaded once for the workgroup's query rows).  The 64
// partials fold by the wave_sum butterfly and lane 0 puts part[c][j] into LDS.  After a barrier thread p forms
// part[a][b-1] + part[b][a] - rho[p], in this order; after a second one a thread per class counts that class's
// votes (integers: no order to fix) and after a third a thread per row takes the first maximum.  No atomics; two
// runs give the same bits, an empty segment adds exactly 0.0, and the rows per workgroup do not enter any sum.
#include <algorithm>

#include "ctx.h"
#include "svm355_device.h"
#include "trace.h"

namespace svm355 {
namespace {

constexpr int kOvoNT = 256, kOvoWaves = kOvoNT / kWave, kOvoGroup = 8, kOvoMaxK = 64;

// index of the pair (a, b), a < b, in LIBSVM's order
__device__ __forceinline__ int ovo_pair(int a, int b, int k) { return a * (k - 1) - a * (a - 1) / 2 + (b - a - 1); }

// R query rows per workgroup: a lane loads a coefficient once and uses it for the R rows, each row with its own
// running sums in the order above (so R does not change a bit of the result).
template <int R>
__global__ __launch_bounds__(kOvoNT) void ovo_votes_kernel(const double* __restrict__ K, int64_t ldk, int64_t m,
                                                           int64_t nsv, int k, const int32_t* __restrict__ start,
                                                           const double* __restrict__ coef, int64_t ldc,
                                                           const double* __restrict__ rho, double* __restrict__ dec,
                                                           int32_t* __restrict__ label) {
  extern __shared__ double ovo_lds[];
  const int km1 = k - 1, P = k * km1 / 2;
  double* part = ovo_lds;                                    // R x k x (k - 1)
  double* dv = part + R * k * km1;                           // R x P
  int32_t* votes = reinterpret_cast<int32_t*>(dv + R * P);   // R x k
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int64_t row0 = int64_t(blockIdx.x) * R;
  const int nrow = int(std::min<int64_t>(R, m - row0));
  const double* Kr[R];  // a row past m reads the block's first row again; nothing of it is written
#pragma unroll
  for (int r = 0; r < R; ++r) Kr[r] = K + (row0 + (r < nrow ? r : 0)) * ldk;

  for (int c = wv; c < k; c += kOvoWaves) {
    // the bounds are the caller's device data: a segment never leaves [0, nsv)
    const int64_t s0 = std::min<int64_t>(std::max<int64_t>(start[c], 0), nsv);
    const int64_t s1 = std::min<int64_t>(std::max<int64_t>(start[c + 1], s0), nsv);
    for (int j0 = 0; j0 < km1; j0 += kOvoGroup) {
      const int nj = min(kOvoGroup, km1 - j0);
      const double* cj = coef + int64_t(j0) * ldc;
      double acc[R][kOvoGroup];
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < kOvoGroup; ++j) acc[r][j] = 0.0;
      for (int64_t s = s0 + lane; s < s1; s += kWave) {
        double kv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) kv[r] = Kr[r][s];
#pragma unroll
        for (int j = 0; j < kOvoGroup; ++j)
          if (j < nj) {
            const double cv = cj[j * ldc + s];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][j] += cv * kv[r];
          }
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < kOvoGroup; ++j) {
          const double v = wave_sum(acc[r][j]);
          if (lane == 0 && j < nj) part[(r * k + c) * km1 + j0 + j] = v;
        }
    }
  }
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += kOvoNT) {
    int a = 0, rem = p;
    while (rem >= km1 - a) {
      rem -= km1 - a;
      ++a;
    }
    const int b = a + 1 + rem;
    const double rp = rho[p];
    for (int r = 0; r < nrow; ++r) {
      const double v = part[(r * k + a) * km1 + (b - 1)] + part[(r * k + b) * km1 + a] - rp;
      dv[r * P + p] = v;
      if (dec) dec[(row0 + r) * P + p] = v;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nrow * k; t += kOvoNT) {
    const int r = t / k, c = t - r * k;
    const double* d = dv + r * P;
    int n = 0;
    for (int o = 0; o < c; ++o) n += d[ovo_pair(o, c, k)] > 0.0 ? 0 : 1;      // c is the pair's b
    for (int o = c + 1; o < k; ++o) n += d[ovo_pair(c, o, k)] > 0.0 ? 1 : 0;  // c is the pair's a
    votes[t] = n;
  }
  __syncthreads();
  if (int(threadIdx.x) < nrow) {
    const int32_t* v = votes + threadIdx.x * k;
    int best = 0;
    for (int c = 1; c < k; ++c)
      if (v[c] > v[best]) best = c;
    label[row0 + threadIdx.x] = best;
  }
}

// 4 rows per workgroup while their sums fit 64 KB of LDS (k <= 32: 47.0 KB), else one (k = 64: 47.5 KB)
constexpr int kOvoRows = 4, kOvoRowsMaxK = 32;
size_t ovo_lds_bytes(int k, int rows) {
  return size_t(rows) * (size_t(k) * (k - 1) * 8 + size_t(k) * (k - 1) / 2 * 8 + size_t(k) * 4);
}

int check_ovo_args(const char* who, int64_t m, int64_t nsv, int64_t k, const void* start_d, const void* coef_d,
                   int64_t ldc, const void* rho_d, const void* label_d) {
  if (k < 2 || k > kOvoMaxK) {
    set_error("%s: k = %lld classes, outside [2, %d]", who, (long long)k, kOvoMaxK);
    return SVM_ERR_ARG;
  }
  if (m < 0 || nsv < 0 || ldc < nsv || !start_d || !rho_d || (m > 0 && !label_d) || (nsv > 0 && !coef_d)) {
    set_error("%s: bad arguments (m = %lld, nsv = %lld, ldc = %lld)", who, (long long)m, (long long)nsv,
              (long long)ldc);
    return SVM_ERR_ARG;
  }
  return SVM_OK;
}

int launch_ovo_votes(hipStream_t s, const double* K, int64_t ldk, int64_t m, int64_t nsv, int k, const int32_t* start,
                     const double* coef, int64_t ldc, const double* rho, double* dec, int32_t* label) {
  if (m <= 0) return SVM_OK;
  if (k <= kOvoRowsMaxK)
    hipLaunchKernelGGL(ovo_votes_kernel<kOvoRows>, dim3(unsigned((m + kOvoRows - 1) / kOvoRows)), dim3(kOvoNT),
                       ovo_lds_bytes(k, kOvoRows), s, K, ldk, m, nsv, k, start, coef, ldc, rho, dec, label);
  else
    hipLaunchKernelGGL(ovo_votes_kernel<1>, dim3(unsigned(m)), dim3(kOvoNT), ovo_lds_bytes(k, 1), s, K, ldk, m, nsv, k,
                       start, coef, ldc, rho, dec, label);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" {

SVM_API int svmd_ovo_votes(void* h, const double* K_d, int64_t ldk, int64_t m, int64_t nsv, int64_t k,
                           const int32_t* start_d, const double* coef_d, int64_t ldc, const double* rho_d,
                           double* dec_d, int32_t* label_d) {
  SVMD_CTX(h);
  int rc = check_ovo_args("svmd_ovo_votes", m, nsv, k, start_d, coef_d, ldc, rho_d, label_d);
  if (rc) return rc;
  if (ldk < nsv || (nsv > 0 && m > 0 && !K_d) || m > INT32_MAX) {
    set_error("svmd_ovo_votes: bad kernel block (m = %lld, nsv = %lld, ldk = %lld)", (long long)m, (long long)nsv,
              (long long)ldk);
    return SVM_ERR_ARG;
  }
  rc = ctx->begin();
  if (rc) return rc;
  rc = launch_ovo_votes(ctx->stream, K_d, ldk, m, nsv, int(k), start_d, coef_d, ldc, rho_d, dec_d, label_d);
  if (rc) return rc;
  return ctx->end();
}

SVM_API int svmd_ovo_predict(void* h, const double* Xs_d, const double* ns_d, int64_t nsv, int64_t lds,
                             const double* Xq_d, const double* nq_d, int64_t m, int64_t ldq, int64_t kdim, double gamma,
                             int64_t k, const int32_t* start_d, const double* coef_d, int64_t ldc, const double* rho_d,
                             int64_t max_rows, double* dec_d, int32_t* label_d) {
  SVMD_CTX(h);
  int rc = check_ovo_args("svmd_ovo_predict", m, nsv, k, start_d, coef_d, ldc, rho_d, label_d);
  if (rc) return rc;
  if (max_rows < 0 || (m > 0 && (!Xq_d || !nq_d)) || (nsv > 0 && (!Xs_d || !ns_d))) {
    set_error("svmd_ovo_predict: bad arguments");
    return SVM_ERR_ARG;
  }
  rc = ctx->begin();
  if (rc) return rc;
  if (m <= 0) return ctx->end();
  TraceRange tr("svm355:ovo_predict");
  // K(Xq, Xs) in row chunks of <= 512 MB scratch as svmd_decision (max_rows > 0: at most that many rows, rounded
  // up to 128), the pair decisions and votes of every chunk behind it.  No support vectors: no block is formed
  // or read, every segment is empty and dec = -rho.
  const int64_t ldk = std::max<int64_t>(2, (nsv + 1) / 2 * 2);
  int64_t rows = std::max<int64_t>(128, (int64_t(512) << 20) / (ldk * 8) / 128 * 128);
  if (max_rows > 0) rows = std::min<int64_t>(rows, (max_rows + 127) / 128 * 128);
  rows = std::min<int64_t>(rows, (m + 127) / 128 * 128);
  rc = ctx->ensure_ws(size_t(rows) * size_t(ldk) * 8);
  if (rc) return rc;
  double* Kq = static_cast<double*>(ctx->ws);
  const int64_t P = k * (k - 1) / 2;
  for (int64_t r0 = 0; r0 < m; r0 += rows) {
    const int64_t mr = std::min(rows, m - r0);
    if (nsv > 0) {
      rc = launch_rbf_gram(ctx->stream, Xq_d + r0 * ldq, nq_d + r0, mr, ldq, Xs_d, ns_d, nsv, lds, kdim, gamma, Kq,
                           ldk, false);
      if (rc) return rc;
    }
    rc = launch_ovo_votes(ctx->stream, Kq, ldk, mr, nsv, int(k), start_d, coef_d, ldc, rho_d,
                          dec_d ? dec_d + r0 * P : nullptr, label_d + r0);
    if (rc) return rc;
  }
  return ctx->end();
}

}  // extern "C"
