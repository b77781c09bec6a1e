// Pairwise coupling on the host: the class probabilities of a query row from its k (k - 1) / 2 one-vs-one pair
// probabilities r_ab, by the second method of Wu, Lin and Weng ("Probability estimates for multi-class
// classification by pairwise coupling", JMLR 2004) -- the one LIBSVM uses for -b 1 with more than two classes.
// The CPU twin of ovo_proba.hip's ovo_couple_kernel: the same arithmetic in the same order, so that the two agree
// bit for bit once r is given (the device's exp is not the host's, so with the sigmoid they agree to its error).
//
// p minimises sum_t sum_{j != t} (r_jt p_t - r_tj p_j)^2 on the simplex, i.e. p' Q p with
//   Q[t][t] = sum_{j != t} r[j][t]^2 (j ascending),   Q[t][j] = -r[j][t] r[t][j],
// by a fixed-point sweep over t that keeps Qp and p' Q p up to date; a sweep starts by forming Q p (j ascending)
// and p' Q p (t ascending) afresh and stops when max_t |(Qp)_t - p' Q p| < 0.005 / k, after at most max(100, k)
// sweeps.  The stop test is "every |(Qp)_t - p' Q p| is below the bound", so a NaN never passes it: a row with a
// NaN decision runs to the cap and comes out NaN.  k = 2: [r_01, r_10], no sweep.
#include <cmath>

#include "internal.h"

namespace svm355 {
namespace {

constexpr int kCoupleMaxK = 64;
constexpr double kCoupleMinProb = 1e-7;

// One row.  r: k x k, Q: k x k, Qp: k scratch; p: k out.  Returns the sweeps taken.
int couple_row(const double* dec, int k, const double* A, const double* B, double* r, double* Q, double* Qp,
               double* p) {
  int pi = 0;
  for (int a = 0; a < k; ++a)
    for (int b = a + 1; b < k; ++b, ++pi) {
      double v = dec[pi];
      if (A) {
        const double z = v * A[pi] + B[pi];
        if (z >= 0.0) {
          const double e = std::exp(-z);
          v = e / (1.0 + e);
        } else {
          v = 1.0 / (1.0 + std::exp(z));
        }
      }
      v = v < kCoupleMinProb ? kCoupleMinProb : (v > 1.0 - kCoupleMinProb ? 1.0 - kCoupleMinProb : v);  // NaN stays
      r[a * k + b] = v;
      r[b * k + a] = 1.0 - v;
    }
  if (k == 2) {
    p[0] = r[1];
    p[1] = r[2];
    return 0;
  }
  for (int t = 0; t < k; ++t) {
    double s = 0.0;
    for (int j = 0; j < k; ++j) {
      if (j == t) continue;
      s += r[j * k + t] * r[j * k + t];
      Q[t * k + j] = -r[j * k + t] * r[t * k + j];
    }
    Q[t * k + t] = s;
    p[t] = 1.0 / double(k);
  }
  const int cap = std::max(100, k);
  const double eps = 0.005 / double(k);
  int it = 0;
  for (; it < cap; ++it) {
    double pQp = 0.0;
    for (int t = 0; t < k; ++t) {
      double s = 0.0;
      for (int j = 0; j < k; ++j) s += Q[t * k + j] * p[j];
      Qp[t] = s;
    }
    for (int t = 0; t < k; ++t) pQp += p[t] * Qp[t];
    bool done = true;
    for (int t = 0; t < k; ++t) done = done && (std::fabs(Qp[t] - pQp) < eps);
    if (done) break;
    for (int t = 0; t < k; ++t) {
      const double qtt = Q[t * k + t];
      const double diff = (-Qp[t] + pQp) / qtt;
      p[t] += diff;
      pQp = (pQp + diff * (diff * qtt + 2.0 * Qp[t])) / (1.0 + diff) / (1.0 + diff);
      for (int j = 0; j < k; ++j) {
        Qp[j] = (Qp[j] + diff * Q[t * k + j]) / (1.0 + diff);
        p[j] /= (1.0 + diff);
      }
    }
  }
  return it;
}

}  // namespace
}  // namespace svm355

using namespace svm355;

extern "C" SVM_API int svm_ovo_couple(const double* dec, int64_t ldd, int64_t m, int64_t k, const double* A,
                                      const double* B, double* proba, int64_t ldp, int32_t* label, int32_t* iters,
                                      int32_t n_threads) {
  if (k < 2 || k > kCoupleMaxK) {
    set_error("svm_ovo_couple: k = %lld classes, outside [2, %d]", (long long)k, kCoupleMaxK);
    return SVM_ERR_ARG;
  }
  const int64_t P = k * (k - 1) / 2;
  if (m < 0 || ldd < P || ldp < k || (m > 0 && (!dec || !proba)) || (A == nullptr) != (B == nullptr)) {
    set_error("svm_ovo_couple: bad arguments (m = %lld, ldd = %lld, ldp = %lld; A and B come together)",
              (long long)m, (long long)ldd, (long long)ldp);
    return SVM_ERR_ARG;
  }
  parallel_for(m, resolve_threads(n_threads), [&](int64_t lo, int64_t hi) {
    const int kk = int(k);
    std::vector<double> buf(size_t(2 * kk * kk + kk));
    double *r = buf.data(), *Q = r + kk * kk, *Qp = Q + kk * kk;
    for (int64_t i = lo; i < hi; ++i) {
      double* p = proba + i * ldp;
      const int it = couple_row(dec + i * ldd, kk, A, B, r, Q, Qp, p);
      if (iters) iters[i] = it;
      if (label) {
        int best = 0;
        for (int c = 1; c < kk; ++c)
          if (p[c] > p[best]) best = c;
        label[i] = best;
      }
    }
  });
  return SVM_OK;
}
