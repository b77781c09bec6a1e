// Platt scaling on the device (gfx950): P(y = +1 | f) = 1 / (1 + exp(A f + B)) fitted to n (decision value,
// label) pairs by Lin, Lin and Weng's Newton method with backtracking (the algorithm LIBSVM documents for -b 1;
// core/platt.cpp is the CPU twin and has the reference).
//
// The whole iteration is ONE launch of ONE 1,024-thread workgroup: there is nothing to overlap with -- every
// Newton step needs the five sums of the step before it -- so the cost is launches and host round trips, and
// this has one of the former and none of the latter.  Thread t owns the pairs t, t + 1024, ...; up to
// kPlattRegs of them per thread stay in registers for the whole fit (n <= 1024 kPlattRegs = 8,192), beyond
// that every pass streams them from memory again.  A Newton step's five sums (h11, h22, h21, g1, g2) are one
// pass, a line-search objective one more.  Sums are deterministic: each thread adds its pairs in ascending
// order, a wave folds its 64 partials by a fixed butterfly (every lane ends with the same bits), the 16 wave
// sums go through LDS and every thread adds them in wave order.  So every thread holds the same sums, solves
// the same 2 x 2 system and takes the same branches, and two runs give the same bits.
//
// platt_fit_batch_kernel is the same fit for P segments of concatenated arrays at once, one workgroup each (the
// one-vs-one pairs' sigmoids: P launches with a host round trip each would cost more than the fits).
#include <cmath>

#include "ctx.h"

namespace svm355 {
namespace {

constexpr int kPlattNT = 1024, kPlattWaves = kPlattNT / 64, kPlattRegs = 8;
constexpr int kPlattMaxIter = 100;
constexpr double kPlattMinStep = 1e-10, kPlattRidge = 1e-12, kPlattGradTol = 1e-5, kPlattDecrease = 1e-4;

// v[k] summed over the workgroup, k < K; every thread returns with the same bits in v.
template <int K>
__device__ __forceinline__ void platt_block_sum(double (&v)[K], double* lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
  __syncthreads();  // the readers of the sums before these are done with lds
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k * kPlattWaves + wv] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kPlattWaves; ++w) s += lds[k * kPlattWaves + w];
    v[k] = s;
  }
}

// The pairs of one thread: in registers (RES; a slot past the thread's pairs has w = 0 and adds exact zeros)
// or streamed.  each(fn): fn(f, label > 0) over the thread's used pairs in ascending order.
template <bool RES>
struct PlattPairs {
  const double* dec;
  const int32_t* y;
  const uint8_t* use;
  int64_t n;
  double f[RES ? kPlattRegs : 1];
  int8_t s[RES ? kPlattRegs : 1];  // +1 / -1, 0: no pair
  __device__ __forceinline__ void load() {
    if constexpr (RES) {
#pragma unroll
      for (int k = 0; k < kPlattRegs; ++k) {
        const int64_t i = int64_t(k) * kPlattNT + threadIdx.x;
        const bool on = i < n && (!use || use[i]);
        f[k] = on ? dec[i] : 0.0;
        s[k] = on ? (y[i] > 0 ? 1 : -1) : 0;
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void each(F&& fn) const {
    if constexpr (RES) {
#pragma unroll
      for (int k = 0; k < kPlattRegs; ++k)
        if (s[k] != 0) fn(f[k], s[k] > 0);
    } else {
      for (int64_t i = threadIdx.x; i < n; i += kPlattNT)
        if (!use || use[i]) fn(dec[i], y[i] > 0);
    }
  }
};

// The whole fit of one workgroup: the n pairs at dec / y / use (use may be null) to *out.  lds: 5 kPlattWaves
// doubles of the workgroup's.  Shared by the one-fit kernel and the batched one, so that a segment of a batch
// is fitted by the very code -- and to the very bits -- of a fit of its own.
template <bool RES>
__device__ __forceinline__ void platt_fit_body(const double* __restrict__ dec, const int32_t* __restrict__ y,
                                               const uint8_t* __restrict__ use, int64_t n,
                                               svm_platt* __restrict__ out, double* lds) {
  PlattPairs<RES> P{dec, y, use, n, {}, {}};
  P.load();
  // the class counts (exact in FP64 below 2^53) and the decisions' range
  double cnt[2] = {0.0, 0.0};
  double dmin = __builtin_inf(), dmax = -__builtin_inf();
  P.each([&](double f, bool pos) {
    cnt[pos ? 0 : 1] += 1.0;
    dmin = fmin(dmin, f);
    dmax = fmax(dmax, f);
  });
  platt_block_sum(cnt, lds);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    dmin = fmin(dmin, __shfl_xor(dmin, off, 64));
    dmax = fmax(dmax, __shfl_xor(dmax, off, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    lds[threadIdx.x >> 6] = dmin;
    lds[kPlattWaves + (threadIdx.x >> 6)] = dmax;
  }
  __syncthreads();
  for (int w = 0; w < kPlattWaves; ++w) {
    dmin = fmin(dmin, lds[w]);
    dmax = fmax(dmax, lds[kPlattWaves + w]);
  }
  const double np = cnt[0], nn = cnt[1];
  double A = 0.0, B = log((nn + 1.0) / (np + 1.0));
  int it = 0, status = SVM_PLATT_DEGENERATE;
  if (np > 0.0 && nn > 0.0 && dmax > dmin) {  // else one class, or one decision value: the prior alone
    const double hi = (np + 1.0) / (np + 2.0), lo = 1.0 / (nn + 2.0);
    auto objective = [&](double a, double b) {
      double v[1] = {0.0};
      P.each([&](double f, bool pos) {
        const double z = f * a + b, t = pos ? hi : lo;
        v[0] += z >= 0.0 ? t * z + log(1.0 + exp(-z)) : (t - 1.0) * z + log(1.0 + exp(z));
      });
      platt_block_sum(v, lds);
      return v[0];
    };
    double fval = objective(A, B);
    status = SVM_PLATT_MAX_ITER;
    for (; it < kPlattMaxIter; ++it) {
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // h11, h22, h21, g1, g2
      P.each([&](double f, bool pos) {
        const double z = f * A + B;
        const double e = exp(z >= 0.0 ? -z : z), r = 1.0 / (1.0 + e);
        const double p = z >= 0.0 ? e * r : r, q = z >= 0.0 ? r : e * r;
        const double d2 = p * q, d1 = (pos ? hi : lo) - p;
        v[0] += f * f * d2;
        v[1] += d2;
        v[2] += f * d2;
        v[3] += f * d1;
        v[4] += d1;
      });
      platt_block_sum(v, lds);
      const double h11 = v[0] + kPlattRidge, h22 = v[1] + kPlattRidge, h21 = v[2], g1 = v[3], g2 = v[4];
      if (fabs(g1) < kPlattGradTol && fabs(g2) < kPlattGradTol) {
        status = SVM_PLATT_CONVERGED;
        break;
      }
      const double det = h11 * h22 - h21 * h21;
      const double dA = -(h22 * g1 - h21 * g2) / det, dB = -(-h21 * g1 + h11 * g2) / det;
      const double gd = g1 * dA + g2 * dB;
      double step = 1.0;
      while (step >= kPlattMinStep) {
        const double nA = A + step * dA, nB = B + step * dB, nf = objective(nA, nB);
        if (nf < fval + kPlattDecrease * step * gd) {
          A = nA;
          B = nB;
          fval = nf;
          break;
        }
        step /= 2.0;
      }
      if (step < kPlattMinStep) {
        status = SVM_PLATT_LINE_SEARCH;
        break;
      }
    }
  }
  if (threadIdx.x == 0) {
    out->A = A;
    out->B = B;
    out->iterations = it;
    out->status = status;
  }
}

template <bool RES>
__global__ __launch_bounds__(kPlattNT) void platt_fit_kernel(const double* __restrict__ dec,
                                                             const int32_t* __restrict__ y,
                                                             const uint8_t* __restrict__ use, int64_t n,
                                                             svm_platt* __restrict__ out) {
  __shared__ double lds[5 * kPlattWaves];
  platt_fit_body<RES>(dec, y, use, n, out, lds);
}

// P fits in one launch: workgroup p fits the segment [off[p], off[p + 1]) of the concatenated arrays to out[p],
// register-resident or streamed by its own length (the rule of svmd_platt_fit).  The choice is uniform over the
// workgroup, so the body's barriers are met by all of its threads.
__global__ __launch_bounds__(kPlattNT) void platt_fit_batch_kernel(const double* __restrict__ dec,
                                                                   const int32_t* __restrict__ y,
                                                                   const uint8_t* __restrict__ use,
                                                                   const int64_t* __restrict__ off,
                                                                   svm_platt* __restrict__ out) {
  __shared__ double lds[5 * kPlattWaves];
  const int64_t o = off[blockIdx.x], n = off[blockIdx.x + 1] - o;
  if (n <= int64_t(kPlattNT) * kPlattRegs)
    platt_fit_body<true>(dec + o, y + o, use ? use + o : nullptr, n, out + blockIdx.x, lds);
  else
    platt_fit_body<false>(dec + o, y + o, use ? use + o : nullptr, n, out + blockIdx.x, lds);
}

}  // namespace
}  // namespace svm355

using namespace svm355;

// Fit the sigmoid to the n pairs (dec_d FP64, y_d int32 labels: > 0 is the positive class) on the device;
// use_d: optional uint8[n], nonzero = the pair counts (null: every pair).  *out (host) when the call returns:
// A, B, the Newton iterations and the status (svm355.h).  One workgroup, one launch.
extern "C" SVM_API int svmd_platt_fit(void* h, const double* dec_d, const int32_t* y_d, const uint8_t* use_d, int64_t n,
                                      svm_platt* out) {
  SVMD_CTX(h);
  if (!dec_d || !y_d || !out || n < 1) {
    set_error("svmd_platt_fit: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  svm_platt* out_d = nullptr;
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { out_d = c.take<svm_platt>(1); }))) return rc;
  hipStream_t s = ctx->stream;
  if (n <= int64_t(kPlattNT) * kPlattRegs)
    hipLaunchKernelGGL(platt_fit_kernel<true>, dim3(1), dim3(kPlattNT), 0, s, dec_d, y_d, use_d, n, out_d);
  else
    hipLaunchKernelGGL(platt_fit_kernel<false>, dim3(1), dim3(kPlattNT), 0, s, dec_d, y_d, use_d, n, out_d);
  SVMD_LAUNCH_CHECK();
  SVMD_CHECK(hipMemcpyAsync(out, out_d, sizeof(svm_platt), hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipStreamSynchronize(s));
  return ctx->end();
}

// P sigmoids in one launch (svm355_device.h): segment p of the concatenated dec_d / y_d / use_d is
// [offsets[p], offsets[p + 1]) (host int64[P + 1], ascending, no empty segment); out[p] (host) is what
// svmd_platt_fit gives on that segment alone, bit for bit.  One launch of P workgroups, one copy back.
extern "C" SVM_API int svmd_platt_fit_batch(void* h, const double* dec_d, const int32_t* y_d, const uint8_t* use_d,
                                            const int64_t* offsets, int64_t P, svm_platt* out) {
  SVMD_CTX(h);
  if (!dec_d || !y_d || !offsets || !out || P < 1 || P > INT32_MAX) {
    set_error("svmd_platt_fit_batch: bad arguments");
    return SVM_ERR_ARG;
  }
  if (offsets[0] < 0) {
    set_error("svmd_platt_fit_batch: offsets[0] = %lld is negative", (long long)offsets[0]);
    return SVM_ERR_ARG;
  }
  for (int64_t p = 0; p < P; ++p)
    if (offsets[p + 1] <= offsets[p]) {
      set_error("svmd_platt_fit_batch: segment %lld is empty or descends (offsets %lld, %lld)", (long long)p,
                (long long)offsets[p], (long long)offsets[p + 1]);
      return SVM_ERR_ARG;
    }
  int rc = ctx->begin();
  if (rc) return rc;
  svm_platt* out_d = nullptr;
  int64_t* off_d = nullptr;
  if ((rc = carve_ws(ctx, [&](WsCarver& c) {
         out_d = c.take<svm_platt>(size_t(P));
         off_d = c.take<int64_t>(size_t(P) + 1);
       })))
    return rc;
  hipStream_t s = ctx->stream;
  // offsets is the caller's pageable memory: the copy is complete for the host when the call returns
  SVMD_CHECK(hipMemcpyAsync(off_d, offsets, size_t(P + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(platt_fit_batch_kernel, dim3(unsigned(P)), dim3(kPlattNT), 0, s, dec_d, y_d, use_d, off_d, out_d);
  SVMD_LAUNCH_CHECK();
  SVMD_CHECK(hipMemcpyAsync(out, out_d, size_t(P) * sizeof(svm_platt), hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipStreamSynchronize(s));
  return ctx->end();
}
