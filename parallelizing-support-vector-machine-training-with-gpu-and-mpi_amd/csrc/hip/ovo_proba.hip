// Pairwise coupling on the device (gfx950): the class probabilities of every query row from its P = k (k - 1) / 2
// one-vs-one pair decisions, by the second method of Wu, Lin and Weng, the one LIBSVM uses.  core/ovo_couple.cpp
// is the CPU twin and states the method; the arithmetic and its order are the twin's, so that the two agree bit
// for bit once the pair probabilities r are given (this file is built without FMA contraction, as every file
// here).  With the sigmoid (A, B given) the device's exp is not the host's, and they agree to its error.
//
// ONE WAVE PER QUERY ROW, lane j owning class j: its p[j], its (Qp)[j], Q[j][j] and row j of Q.  The sweep over
// t is a dependency chain (step t needs the p and Qp that step t - 1 left), and what a step does is k-wide with
// k <= 64, the wave width: step t reads lane t's (Qp)[t] and Q[t][t] by read-lane (t is wave-uniform), every lane
// forms the same diff and the same new p' Q p, and lane j updates its own (Qp)[j] and p[j] with Q[t][j], which
// it reads as Q[j][t] from its own row (Q is symmetric bit for bit: both are -(r_ab (1 - r_ab)) of the pair).
// The order-sensitive sums are done in the twin's order, not by a butterfly: lane t adds Q[t][j] p[j] over
// ascending j (p[j] by read-lane), and p' Q p is added over ascending t by every lane alike.
//
// A workgroup is 4 waves = 4 rows up to 32 classes and one wave = one row above (the rule of ovo.hip's
// kOvoRowsMaxK): a row keeps its P clamped pair probabilities and Q (k rows of k | 1 doubles, the odd stride so
// that the lanes' rows fall on different banks) in LDS, 12.4 KB at k = 32 and 48.3 KB at k = 64.  Rows take
// different numbers of sweeps, so NOTHING in this kernel is a workgroup barrier: a wave touches its own slice of
// LDS only, and the slice's writes are ordered against its reads by wave-level fences.  The stop test is "every
// lane's |(Qp)_t - p' Q p| is below 0.005 / k" (a wave vote), which a NaN never passes: a row with a NaN
// decision leaves the loop at the cap, comes out NaN and disturbs nothing else.  A row past m ends its wave at
// once; columns past P of dec and past k of proba are neither read nor written.  No atomics.
#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

constexpr int kCoupleMaxK = 64, kCoupleRows = 4, kCoupleRowsMaxK = 32;
constexpr double kCoupleMinProb = 1e-7;

// index of the pair (a, b), a < b, in LIBSVM's order
__device__ __forceinline__ int couple_pair(int a, int b, int k) {
  return a * (k - 1) - a * (a - 1) / 2 + (b - a - 1);
}

// lane src's v in every lane; src is wave-uniform
__device__ __forceinline__ double lane_value(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// The wave's LDS writes before this point are visible to its reads after it.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr size_t couple_row_doubles(int k) { return size_t(k) * (k - 1) / 2 + size_t(k) * (k | 1); }

template <int R>
__global__ __launch_bounds__(R * kWave) void ovo_couple_kernel(const double* __restrict__ dec, int64_t ldd, int64_t m,
                                                               int k, const double* __restrict__ A,
                                                               const double* __restrict__ B,
                                                               double* __restrict__ proba, int64_t ldp,
                                                               int32_t* __restrict__ label,
                                                               int32_t* __restrict__ iters) {
  extern __shared__ double couple_lds[];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int64_t row = int64_t(blockIdx.x) * R + wv;
  if (row >= m) return;  // the whole wave: no barrier follows
  const int P = k * (k - 1) / 2, ld = k | 1;
  double* rb = couple_lds + size_t(wv) * couple_row_doubles(k);  // P pair probabilities r_ab, a < b
  double* Q = rb + P;                                            // k x ld
  const double* drow = dec + row * ldd;
  for (int p = lane; p < P; p += kWave) {
    double v = drow[p];
    if (A) {
      const double z = v * A[p] + B[p];
      if (z >= 0.0) {
        const double e = exp(-z);
        v = e / (1.0 + e);
      } else {
        v = 1.0 / (1.0 + exp(z));
      }
    }
    rb[p] = v < kCoupleMinProb ? kCoupleMinProb : (v > 1.0 - kCoupleMinProb ? 1.0 - kCoupleMinProb : v);  // NaN stays
  }
  wave_lds_sync();
  double* prow = proba + row * ldp;
  if (k == 2) {
    if (lane == 0) {
      const double r01 = rb[0], r10 = 1.0 - r01;
      prow[0] = r01;
      prow[1] = r10;
      if (label) label[row] = r10 > r01 ? 1 : 0;
      if (iters) iters[row] = 0;
    }
    return;
  }
  const bool own = lane < k;
  const int me = own ? lane : 0;  // a lane past k walks class 0's row; nothing of it is kept
  double* Qrow = Q + me * ld;
  double qd = 0.0;
  if (own) {
    // row `lane` of Q: Q[t][j] = -r[j][t] r[t][j] = -(r_ab (1 - r_ab)) of the pair {t, j}, and the diagonal
    // sum_{j != t} r[j][t]^2 over ascending j
    for (int j = 0; j < k; ++j) {
      if (j == lane) continue;
      const double rab = j < lane ? rb[couple_pair(j, lane, k)] : rb[couple_pair(lane, j, k)];
      const double rjt = j < lane ? rab : 1.0 - rab, rtj = j < lane ? 1.0 - rab : rab;
      qd += rjt * rjt;
      Qrow[j] = -rjt * rtj;
    }
    Qrow[lane] = qd;
  } else {
    qd = 1.0;
  }
  wave_lds_sync();
  const int cap = max(100, k);
  const double eps = 0.005 / double(k);
  double p = own ? 1.0 / double(k) : 0.0, Qp = 0.0;
  int it = 0;
  for (; it < cap; ++it) {
    Qp = 0.0;
    for (int j = 0; j < k; ++j) Qp += Qrow[j] * lane_value(p, j);
    const double prod = p * Qp;
    double pQp = 0.0;
    for (int t = 0; t < k; ++t) pQp += lane_value(prod, t);
    if (__all(!own || fabs(Qp - pQp) < eps)) break;
    for (int t = 0; t < k; ++t) {
      const double Qpt = lane_value(Qp, t), qtt = lane_value(qd, t);
      const double diff = (-Qpt + pQp) / qtt;
      if (lane == t) p += diff;
      pQp = (pQp + diff * (diff * qtt + 2.0 * Qpt)) / (1.0 + diff) / (1.0 + diff);
      Qp = (Qp + diff * Qrow[t]) / (1.0 + diff);
      p /= (1.0 + diff);
    }
  }
  if (own) prow[lane] = p;
  if (label || iters) {
    int best = 0;
    double bv = lane_value(p, 0);
    for (int c = 1; c < k; ++c) {
      const double v = lane_value(p, c);
      if (v > bv) {
        bv = v;
        best = c;
      }
    }
    if (lane == 0) {
      if (label) label[row] = best;
      if (iters) iters[row] = it;
    }
  }
}

}  // namespace
}  // namespace svm355

using namespace svm355;

// Class probabilities from pair decisions (svm355_device.h has the contract).
extern "C" SVM_API int svmd_ovo_couple(void* h, const double* dec_d, int64_t ldd, int64_t m, int64_t k,
                                       const double* A_d, const double* B_d, double* proba_d, int64_t ldp,
                                       int32_t* label_d, int32_t* iters_d) {
  SVMD_CTX(h);
  if (k < 2 || k > kCoupleMaxK) {
    set_error("svmd_ovo_couple: k = %lld classes, outside [2, %d]", (long long)k, kCoupleMaxK);
    return SVM_ERR_ARG;
  }
  const int64_t P = k * (k - 1) / 2;
  if (m < 0 || m > INT32_MAX || ldd < P || ldp < k || (m > 0 && (!dec_d || !proba_d)) ||
      (A_d == nullptr) != (B_d == nullptr)) {
    set_error("svmd_ovo_couple: bad arguments (m = %lld, ldd = %lld, ldp = %lld; A and B come together)",
              (long long)m, (long long)ldd, (long long)ldp);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (m > 0) {
    const int kk = int(k);
    if (kk <= kCoupleRowsMaxK)
      hipLaunchKernelGGL(ovo_couple_kernel<kCoupleRows>, dim3(unsigned((m + kCoupleRows - 1) / kCoupleRows)),
                         dim3(kCoupleRows * kWave), kCoupleRows * couple_row_doubles(kk) * sizeof(double), ctx->stream,
                         dec_d, ldd, m, kk, A_d, B_d, proba_d, ldp, label_d, iters_d);
    else
      hipLaunchKernelGGL(ovo_couple_kernel<1>, dim3(unsigned(m)), dim3(kWave), couple_row_doubles(kk) * sizeof(double),
                         ctx->stream, dec_d, ldd, m, kk, A_d, B_d, proba_d, ldp, label_d, iters_d);
    SVMD_LAUNCH_CHECK();
  }
  return ctx->end();
}
