// Platt scaling on the host: P(y = +1 | f) = 1 / (1 + exp(A f + B)) fitted to (decision value, label) pairs by
// Lin, Lin and Weng's Newton method with backtracking ("A note on Platt's probabilistic outputs for support
// vector machines", 2007; the algorithm LIBSVM documents for -b 1).  The CPU twin of platt.hip's
// platt_fit_kernel: the same constants, rules and overflow-safe forms, every sum in plain ascending order.
// Device libm's exp / log are not the host's, so the two agree to the stop rule, not bit for bit.
#include <cmath>

#include "internal.h"

namespace svm355 {
namespace {

constexpr int kMaxIter = 100;
constexpr double kMinStep = 1e-10, kRidge = 1e-12, kGradTol = 1e-5, kDecrease = 1e-4;

struct Pairs {
  const double* dec;
  const int32_t* y;
  const uint8_t* use;  // null: every pair
  int64_t n;
  double hi, lo;  // the targets of the positive / negative labels
  bool on(int64_t i) const { return !use || use[i]; }
  double t(int64_t i) const { return y[i] > 0 ? hi : lo; }
};

// sum_i t_i z_i + log(1 + exp(-z_i)) with z = A f + B, in the form that cannot overflow
double objective(const Pairs& P, double A, double B) {
  double fval = 0.0;
  for (int64_t i = 0; i < P.n; ++i) {
    if (!P.on(i)) continue;
    const double z = P.dec[i] * A + B, t = P.t(i);
    fval += z >= 0.0 ? t * z + std::log(1.0 + std::exp(-z)) : (t - 1.0) * z + std::log(1.0 + std::exp(z));
  }
  return fval;
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" SVM_API int svm_platt_fit(const double* dec, const int32_t* y, const uint8_t* use, int64_t n,
                                     svm_platt* out) {
  if (!dec || !y || !out || n < 1) {
    set_error("svm_platt_fit: bad arguments");
    return SVM_ERR_ARG;
  }
  int64_t np = 0, nn = 0;
  double dmin = INFINITY, dmax = -INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    if (use && !use[i]) continue;
    (y[i] > 0 ? np : nn) += 1;
    dmin = std::fmin(dmin, dec[i]);
    dmax = std::fmax(dmax, dec[i]);
  }
  double A = 0.0, B = std::log(double(nn + 1) / double(np + 1));
  out->A = A;
  out->B = B;
  out->iterations = 0;
  out->status = SVM_PLATT_DEGENERATE;
  if (np == 0 || nn == 0 || !(dmax > dmin)) return SVM_OK;  // one class, or one decision value: the prior alone
  const Pairs P{dec, y, use, n, double(np + 1) / double(np + 2), 1.0 / double(nn + 2)};
  double fval = objective(P, A, B);
  int it = 0, status = SVM_PLATT_MAX_ITER;
  for (; it < kMaxIter; ++it) {
    double h11 = kRidge, h22 = kRidge, h21 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      if (!P.on(i)) continue;
      const double f = dec[i], z = f * A + B;
      double p, q;
      if (z >= 0.0) {
        const double e = std::exp(-z);
        p = e / (1.0 + e);
        q = 1.0 / (1.0 + e);
      } else {
        const double e = std::exp(z);
        p = 1.0 / (1.0 + e);
        q = e / (1.0 + e);
      }
      const double d2 = p * q, d1 = P.t(i) - p;
      h11 += f * f * d2;
      h22 += d2;
      h21 += f * d2;
      g1 += f * d1;
      g2 += d1;
    }
    if (std::fabs(g1) < kGradTol && std::fabs(g2) < kGradTol) {
      status = SVM_PLATT_CONVERGED;
      break;
    }
    const double det = h11 * h22 - h21 * h21;
    const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
    const double gd = g1 * dA + g2 * dB;
    double step = 1.0;
    while (step >= kMinStep) {
      const double nA = A + step * dA, nB = B + step * dB, nf = objective(P, nA, nB);
      if (nf < fval + kDecrease * step * gd) {
        A = nA;
        B = nB;
        fval = nf;
        break;
      }
      step /= 2.0;
    }
    if (step < kMinStep) {
      status = SVM_PLATT_LINE_SEARCH;
      break;
    }
  }
  out->A = A;
  out->B = B;
  out->iterations = it;
  out->status = status;
  return SVM_OK;
}
