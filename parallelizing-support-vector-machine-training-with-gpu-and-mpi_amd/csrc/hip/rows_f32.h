// Float32 training rows (rows_f32.hip): RBF kernel values from an FP32-MFMA dot product under an FP64 epilogue.
// The decomposition solver's fourth row source (decomp.hip) and the C entries of svm355_device.h share these
// launchers; all enqueue on `s`.
#pragma once
#include "ctx.h"

namespace svm355 {

// store: K[i, j] = exp(-gamma max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j)).  sum: f[i] += sum_j coef[j] K_ij.
// sum_twin: the same sum also added to f[i + m] (epsilon-SVR: both points of row i).
enum class Rbf32Epilogue { store, sum, sum_twin };

// One block launch: A (m x lda floats) against B (ncap x ldb floats), kdim floats of each row (a multiple of 16;
// zero padding beyond the features), nA / nB the rows' squared norms in FP64.  gate (device, optional): != 0 makes
// the launch a no-op.  ncount (device, optional): only the first min(ncap, *ncount) B rows count; 0 leaves K and f
// untouched.  Ids: B row j is training row idb[j] (optional; none: no pair is the diagonal), A row i is training
// row ida[i] (or row_off + i without a list); with twin_nrow > 0 an id k stands for row k mod twin_nrow.  A pair of
// equal rows gets exactly 1.0, in every epilogue.
struct Rbf32Block {
  const float* A = nullptr;
  const double* nA = nullptr;
  int64_t m = 0, lda = 0;
  const float* B = nullptr;
  const double* nB = nullptr;
  int64_t ncap = 0, ldb = 0, kdim = 0;
  const int32_t* gate = nullptr;
  const int32_t* ncount = nullptr;
  const int32_t* ida = nullptr;
  int64_t row_off = 0;
  const int32_t* idb = nullptr;
  int64_t twin_nrow = 0;
  double gamma = 0.0;
  double* K = nullptr;  // store
  int64_t ldk = 0;
  const double* coef = nullptr;  // sum, sum_twin: ncap coefficients
  double* f = nullptr;           // sum: m values; sum_twin: 2 m
};
int launch_rbf32_block(hipStream_t s, Rbf32Epilogue epi, const Rbf32Block& b);

// Xo[k] = X[ids[k]] (ld floats, a multiple of 4) and no[k] = nrm[ids[k]] for k < min(cap, *count); an id k stands
// for row k mod twin_nrow when that is > 0.  gate: *gate != 0 -> no-op.
int launch_ws_gather_f32(hipStream_t s, const float* X, const double* nrm, int64_t ld, const int32_t* ids,
                         const int32_t* count, const int32_t* gate, int64_t twin_nrow, int cap, float* Xo, double* no);

}  // namespace svm355
