// The dot-product kernel functions of LIBSVM and scikit-learn (svm_params.kernel = 1, 2, 3): one definition for the
// device kernels (hip/decomp_kfun.hip) and the host.  Plain C++ that also compiles as HIP device code.
//   linear      x.z
//   polynomial  (gamma x.z + coef0)^degree
//   sigmoid     tanh(gamma x.z + coef0)
// The integer power is LIBSVM's powi (repeated squaring): one fixed multiplication order, so the device and the
// host multiply in the same order.  tanh is each side's own library function.
// The additive distance kernels (svm_params.kernel = 4, 5; hip/decomp_dist.hip), K = exp(-gamma D) with a unit diagonal:
//   laplacian   D = sum_k |x_k - z_k|
//   chi2        D = sum_k (x_k - z_k)^2 / (x_k + z_k) over the k with x_k + z_k > 0 (scikit-learn's chi2_kernel;
//               non-negative inputs)
// D accumulates over k ascending in one chain on both sides; exp is each side's own library function.
// A precomputed kernel (svm_params.kernel = 6; hip/decomp_gram.hip): no function at all, the solve reads the caller's
// n x n Gram, which must be symmetric to the bit; gamma, degree and coef0 are not read.
#pragma once
#include <cmath>
#include <cstdint>

#include "svm355.h"

#if defined(__HIPCC__)
#define SVM_KFUN_HD __host__ __device__
#else
#define SVM_KFUN_HD
#endif

namespace svm355 {

enum : int32_t {
  kKernelRbf = 0, kKernelLinear = 1, kKernelPoly = 2, kKernelSigmoid = 3, kKernelLaplacian = 4, kKernelChi2 = 5,
  kKernelPrecomputed = 6
};
constexpr int32_t kMaxDegree = 16;

struct KFun {
  int32_t kind = kKernelLinear, degree = 3;
  double gamma = 1.0, coef0 = 0.0;
};

SVM_KFUN_HD inline double kfun_powi(double base, int32_t times) {
  double tmp = base, ret = 1.0;
  for (int32_t t = times; t > 0; t /= 2) {
    if (t % 2 == 1) ret *= tmp;
    tmp = tmp * tmp;
  }
  return ret;
}

SVM_KFUN_HD inline double kfun_apply(const KFun& k, double dot) {
  if (k.kind == kKernelLinear) return dot;
  const double t = k.gamma * dot + k.coef0;
  return k.kind == kKernelSigmoid ? tanh(t) : kfun_powi(t, k.degree);
}

// The kernels of x.z that kfun_apply evaluates (hip/decomp_kfun.hip's block): linear, polynomial, sigmoid.
inline bool kernel_is_dot(int32_t kind) { return kind >= kKernelLinear && kind <= kKernelSigmoid; }
inline bool kernel_is_dist(int32_t kind) { return kind == kKernelLaplacian || kind == kKernelChi2; }

// One term of D.  |a - b|, (a - b)^2 and a + b commute to the bit, so D(x, z) and D(z, x) are the same bits, equal
// operands (and zero padding) give exactly 0, and the division is IEEE on both sides.
template <bool CHI2>
SVM_KFUN_HD inline double dist_term(double a, double b) {
  const double t = a - b;
  if (!CHI2) return fabs(t);
  const double s = a + b;
  return s > 0.0 ? (t * t) / s : 0.0;
}

// K(a, b) over d features on the host (the host Gram, svm_kernel_gram): the device block's chain and expression.
inline double dist_kernel_value(int32_t kind, double gamma, const double* a, const double* b, int64_t d) {
  double D = 0.0;
  if (kind == kKernelChi2)
    for (int64_t k = 0; k < d; ++k) D += dist_term<true>(a[k], b[k]);
  else
    for (int64_t k = 0; k < d; ++k) D += dist_term<false>(a[k], b[k]);
  return std::exp(-gamma * D);
}

inline KFun kfun_of(const svm_params& p) { return KFun{p.kernel, p.degree, p.gamma, p.coef0}; }

// kernel in 0..6, and for the polynomial 1 <= degree <= 16, a finite coef0 for it and the sigmoid; the distance
// kernels need gamma > 0 and read neither degree nor coef0; a precomputed kernel reads none of the three.
inline bool kfun_params_ok(const svm_params& p) {
  if (p.kernel < kKernelRbf || p.kernel > kKernelPrecomputed) return false;
  if (p.kernel == kKernelPrecomputed) return true;
  if (kernel_is_dist(p.kernel)) return p.gamma > 0.0;
  if (p.kernel == kKernelPoly && (p.degree < 1 || p.degree > kMaxDegree)) return false;
  return p.kernel == kKernelRbf || p.kernel == kKernelLinear || std::isfinite(p.coef0);
}

}  // namespace svm355
