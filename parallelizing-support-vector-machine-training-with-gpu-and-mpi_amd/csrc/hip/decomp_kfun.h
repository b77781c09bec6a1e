// The dot-product kernels (linear, polynomial, sigmoid: kfun.h) on the device: the launchers of decomp_kfun.hip
// that the decomposition solver's driver (decomp.hip) calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "decomp_dev.h"
#include "kfun.h"

namespace svm355 {

// store: K[i, j] = kfun(A_i . B_j).  sum: f[i] += sum_j coef[j] kfun(A_i . B_j).  sum_twin: the same sum also
// added to f[i + m] (epsilon-SVR: both points of row i).
enum class KfunEpilogue { store, sum, sum_twin };

// One block launch: A (m x lda) against B (ncap x ldb), kdim doubles of each row (a multiple of 16; zero padding
// beyond the features).  gate (device, optional): != 0 makes the launch a no-op.  ncount (device, optional): only
// the first min(ncap, *ncount) B rows count; 0 leaves K and f untouched.
struct KfunBlock {
  const double* A = nullptr;
  int64_t m = 0, lda = 0;
  const double* B = nullptr;
  int64_t ncap = 0, ldb = 0, kdim = 0;
  KFun kf;
  const int32_t* gate = nullptr;
  const int32_t* ncount = nullptr;
  double* K = nullptr;  // store
  int64_t ldk = 0;
  const double* coef = nullptr;  // sum, sum_twin: ncap coefficients
  double* f = nullptr;           // sum: m values; sum_twin: 2 m
};
int launch_kfun_block(hipStream_t s, KfunEpilogue epi, const KfunBlock& b);

// ws_inner_kfun_kernel: one inner solve on K(W, W) with its own diagonal (one workgroup of 256 threads x 4
// points, second-order j, one pair per iteration, per-class boxes C / Cn).  Of `a` it reads Kw, ldw, W, ctl, y,
// alpha, Wf, C, Cn, eps, cols, coef, mcount and pub.  The caller checks the launch.
void launch_ws_inner_kfun(hipStream_t s, const InnerArgs& a);

}  // namespace svm355
