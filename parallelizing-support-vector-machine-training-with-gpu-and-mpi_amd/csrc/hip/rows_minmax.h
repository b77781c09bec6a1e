// Column min / max of dense device rows in one streaming pass, on the rows' own element type (float for
// rows_f32.hip, _Float16 for rows_f16.hip): per-block column partials, then a fold in partial order, a NaN anywhere in
// a column making both of its bounds NaN as in the FP64 scaler.  min and max of a set do not depend on the order, so
// the partial count is free to follow the shape.
#pragma once
#include <algorithm>

#include "ctx.h"

namespace svm355 {

constexpr int kMinmaxColsPerBlock = 64, kMinmaxRowLanes = 4;

template <typename T>
__global__ __launch_bounds__(256) void rows_minmax_partial_kernel(const T* __restrict__ X, int64_t n, int64_t d,
                                                                  int64_t ld, double* __restrict__ pmin,
                                                                  double* __restrict__ pmax) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = int64_t(blockIdx.x) * kMinmaxColsPerBlock + lane;
  const int64_t rstride = int64_t(gridDim.y) * kMinmaxRowLanes;
  float lo = __builtin_inff(), hi = -__builtin_inff();  // every element type here widens to float exactly
  bool nan = false;
  if (c < d) {
    for (int64_t r = int64_t(blockIdx.y) * kMinmaxRowLanes + wv; r < n; r += rstride) {
      const float v = float(X[r * ld + c]);
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
      nan |= v != v;
    }
  }
  __shared__ float smin[kMinmaxRowLanes][kMinmaxColsPerBlock], smax[kMinmaxRowLanes][kMinmaxColsPerBlock];
  __shared__ bool snan[kMinmaxRowLanes][kMinmaxColsPerBlock];
  smin[wv][lane] = lo;
  smax[wv][lane] = hi;
  snan[wv][lane] = nan;
  __syncthreads();
  if (wv == 0 && c < d) {
#pragma unroll
    for (int w = 1; w < kMinmaxRowLanes; ++w) {
      nan |= snan[w][lane];
      lo = fminf(lo, smin[w][lane]);
      hi = fmaxf(hi, smax[w][lane]);
    }
    pmin[int64_t(blockIdx.y) * d + c] = nan ? __builtin_nan("") : double(lo);
    pmax[int64_t(blockIdx.y) * d + c] = nan ? __builtin_nan("") : double(hi);
  }
}

static __global__ __launch_bounds__(256) void rows_minmax_final_kernel(const double* __restrict__ pmin,
                                                                       const double* __restrict__ pmax, int parts,
                                                                       int64_t d, double* __restrict__ mn,
                                                                       double* __restrict__ mx) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= d) return;
  double lo = pmin[c], hi = pmax[c];
  bool nan = lo != lo;
  for (int p = 1; p < parts; ++p) {
    const double v = pmin[int64_t(p) * d + c];
    nan |= v != v;
    lo = fmin(lo, v);
    hi = fmax(hi, pmax[int64_t(p) * d + c]);
  }
  mn[c] = nan ? __builtin_nan("") : lo;
  mx[c] = nan ? __builtin_nan("") : hi;
}

// mn_d / mx_d (d doubles each) = the column bounds of X_d (n x ld elements, d of them features); the partials live
// in the context's workspace.  Enqueues on the context's stream.
template <typename T>
int launch_rows_minmax(DeviceCtx* ctx, const T* X_d, int64_t n, int64_t d, int64_t ld, double* mn_d, double* mx_d) {
  const int gx = int((d + kMinmaxColsPerBlock - 1) / kMinmaxColsPerBlock);
  const int parts = int(std::min<int64_t>((n + kMinmaxRowLanes - 1) / kMinmaxRowLanes, std::max(1, 2048 / gx)));
  if (int rc = ctx->ensure_ws(size_t(2) * size_t(d) * size_t(parts) * 8)) return rc;
  double* pmin = static_cast<double*>(ctx->ws);
  double* pmax = pmin + size_t(parts) * size_t(d);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(rows_minmax_partial_kernel<T>, dim3(gx, parts), dim3(256), 0, s, X_d, n, d, ld, pmin, pmax);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(rows_minmax_final_kernel, dim3(unsigned((d + 255) / 256)), dim3(256), 0, s, pmin, pmax, parts, d,
                     mn_d, mx_d);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace svm355
