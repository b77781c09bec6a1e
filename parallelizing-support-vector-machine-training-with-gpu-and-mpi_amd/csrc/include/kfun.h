// The dot-product kernel functions of LIBSVM and scikit-learn (svm_params.kernel = 1, 2, 3): one definition for the
// device kernels (hip/decomp_kfun.hip) and the host.  Plain C++ that also compiles as HIP device code.
//   linear      x.z
//   polynomial  (gamma x.z + coef0)^degree
//   sigmoid     tanh(gamma x.z + coef0)
// The integer power is LIBSVM's powi (repeated squaring): one fixed multiplication order, so the device and the
// host multiply in the same order.  tanh is each side's own library function.
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

enum : int32_t { kKernelRbf = 0, kKernelLinear = 1, kKernelPoly = 2, kKernelSigmoid = 3 };
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

inline KFun kfun_of(const svm_params& p) { return KFun{p.kernel, p.degree, p.gamma, p.coef0}; }

// kernel in 0..3, and for the polynomial 1 <= degree <= 16, a finite coef0.
inline bool kfun_params_ok(const svm_params& p) {
  if (p.kernel < kKernelRbf || p.kernel > kKernelSigmoid) return false;
  if (p.kernel == kKernelPoly && (p.degree < 1 || p.degree > kMaxDegree)) return false;
  return p.kernel == kKernelRbf || p.kernel == kKernelLinear || std::isfinite(p.coef0);
}

}  // namespace svm355
