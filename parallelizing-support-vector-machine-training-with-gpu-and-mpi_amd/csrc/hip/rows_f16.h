// Float16 training rows (rows_f16.hip): RBF kernel values from an FP16-MFMA dot product (exact products, float32
// accumulation) under an FP64 epilogue.  The decomposition solver's fifth row source (decomp.hip) and the C entries
// of svm355_device.h share these launchers; all enqueue on `s`.
#pragma once
#include "ctx.h"

namespace svm355 {

typedef _Float16 half_t;

// The k stage of rbf16_block_kernel in halves: every float16 row length (ld, kdim) is a multiple of it.
constexpr int kF16RowQuantum = 64;

// store: K[i, j] = exp(-gamma max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j)).  sum: f[i] += sum_j coef[j] K_ij.
// sum_twin: the same sum also added to f[i + m] (epsilon-SVR: both points of row i).
enum class Rbf16Epilogue { store, sum, sum_twin };

// One block launch: A (m x lda halves) against B (ncap x ldb halves), kdim halves of each row (a multiple of 64;
// zero padding beyond the features), nA / nB the rows' squared norms in FP64.  gate, ncount, ida / row_off, idb and
// twin_nrow are Rbf32Block's (rows_f32.h): a non-zero *gate makes the launch a no-op, only the first
// min(ncap, *ncount) B rows count (0 leaves K and f untouched), and a pair of equal training rows by id -- an id k
// standing for row k mod twin_nrow when that is > 0 -- gets exactly 1.0 in every epilogue.
struct Rbf16Block {
  const half_t* A = nullptr;
  const double* nA = nullptr;
  int64_t m = 0, lda = 0;
  const half_t* B = nullptr;
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
int launch_rbf16_block(hipStream_t s, Rbf16Epilogue epi, const Rbf16Block& b);

// Xo[k] = X[ids[k]] (ld halves, a multiple of 8) and no[k] = nrm[ids[k]] for k < min(cap, *count); an id k stands
// for row k mod twin_nrow when that is > 0.  gate: *gate != 0 -> no-op.
int launch_ws_gather_f16(hipStream_t s, const half_t* X, const double* nrm, int64_t ld, const int32_t* ids,
                         const int32_t* count, const int32_t* gate, int64_t twin_nrow, int cap, half_t* Xo, double* no);

}  // namespace svm355
