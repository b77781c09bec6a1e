// The additive distance kernels (laplacian, chi2: kfun.h) on the device: the launcher of decomp_dist.hip that the
// decomposition solver's driver (decomp.hip) calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kfun.h"

namespace svm355 {

// store: K[i, j] = exp(-gamma D(A_i, B_j)).  sum: f[i] += sum_j coef[j] exp(-gamma D(A_i, B_j)).  sum_twin: the
// same sum also added to f[i + m] (epsilon-SVR: both points of row i).
enum class DistEpilogue { store, sum, sum_twin };

// One block launch, KfunBlock's interface: A (m x lda) against B (ncap x ldb), kdim doubles of each row (a multiple
// of 16; zero padding beyond the features contributes exactly 0).  gate (device, optional): != 0 makes the launch a
// no-op.  ncount (device, optional): only the first min(ncap, *ncount) B rows count; 0 leaves K and f untouched.
struct DistBlock {
  const double* A = nullptr;
  int64_t m = 0, lda = 0;
  const double* B = nullptr;
  int64_t ncap = 0, ldb = 0, kdim = 0;
  int32_t kind = kKernelLaplacian;  // kKernelLaplacian or kKernelChi2
  double gamma = 1.0;
  const int32_t* gate = nullptr;
  const int32_t* ncount = nullptr;
  double* K = nullptr;  // store
  int64_t ldk = 0;
  const double* coef = nullptr;  // sum, sum_twin: ncap coefficients
  double* f = nullptr;           // sum: m values; sum_twin: 2 m
};
int launch_dist_block(hipStream_t s, DistEpilogue epi, const DistBlock& b);

}  // namespace svm355
