// A precomputed kernel on the device (svm_params.kernel = 6): the row source of the decomposition solver is the
// caller's n x n Gram in HBM.  Nothing is computed from features; the driver (decomp.hip) chooses these kernels when
// DecompRows::gram(), and the inner solve is ws_inner_kfun_kernel (decomp_kfun.hip), which reads the diagonal from
// K(W, W).  K is symmetric to the bit (gram_check_kernel), so row j is read wherever the mathematics says column j:
// every access below walks a row of K forward.
//
// ---- gram_rowsum_kernel: f[i] += sum_k coef[k] K[cols[k], i] ------------------------------------------------
// Split.  A workgroup of 256 threads owns 512 adjacent columns i; a thread owns two adjacent ones, so one moved row
// costs it one 16-byte load, a wave reads runs of 1 KB and a workgroup 4 KB of each row.  No thread shares a sum with
// another: there is no cross-lane step and no atomic.
// Staging.  The workgroup copies the moved ids and coefficients (at most 1,024 x 12 bytes) into LDS once, ids clamped
// into [0, n); every later read of them is an LDS broadcast.
// Order (the CPU oracle's rowsum_update_kfun replays it; it is kfun_block_kernel's sum epilogue).  Per column sixteen
// chains: chain l starts from 0.0 and adds coef[k] * K[cols[k], i] for k = l, l + 16, l + 32, ... < count ascending
// (product rounded, then the add: the file is built without contraction).  In this layout the sixteen chains are
// sixteen independent accumulators per column and sixteen row loads in flight per thread -- what a stream bound by HBM
// wants -- so the oracle's order costs nothing.  The chains are folded by the 8, 4, 2, 1 xor butterfly as lane 0 of
// the sum epilogue sees it, v[l] = v[l] + v[l + off] for l < off, then one add into f[i] (and one into f[i + twin]).
// A count of 0 and a non-zero gate return before anything is written: f keeps its bits.
//
// ---- gram_kww_kernel: K(W, W) as a gather -------------------------------------------------------------------
// One wave per working-set row a; its lanes stride b.  W ascends, so a wave's gathers walk row W[a] of K forward.
// A point's kernel row is its id mod n: in twin mode both points of a row get the row's values, its own diagonal
// included, so there is no mirror pass and no twin fix-up.
//
// ---- gram_check_kernel: finite and symmetric to the bit -----------------------------------------------------
// Pairs of 64 x 64 tiles of the upper triangle: tile (bj, bi) goes through an LDS tile padded to 65 doubles and is
// read back transposed against tile (bi, bj), both read from HBM in rows.  Bit patterns are compared (so -0.0 against
// 0.0 offends, and a NaN equals only itself), and the upper entry's exponent is tested for NaN / infinity; a lower
// entry that is not finite differs from a finite upper one.  Each thread keeps its smallest offending row-major
// index and publishes it with one 64-bit vector atomicMin: the answer is the same on every run.  A workgroup whose
// tile pair lies wholly behind the index already published skips its reads.
//
// ---- gram_decision_kernel: dec[q] = sum_s coef[s] Kq[q, sv[s]] - b ------------------------------------------
// One wave per query row.  Lane l sums s = l, l + 64, ... ascending from 0.0, the 64 lanes fold by the butterfly 32,
// 16, 8, 4, 2, 1, lane 0 subtracts b.  sv ascends, so a wave's 64 gathers fall into few cache lines of the row.
#include "decomp_gram.h"

#include <algorithm>
#include <climits>

#include "ctx.h"
#include "decomp_dev.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

constexpr int kGrNT = 256, kGrChains = 16;
constexpr unsigned long long kGramOk = ~0ull;

// One thread's two columns (TWO) or the last column of an odd count of them (an 8-byte load: nothing past a row's
// entries is read): the sixteen chains over the staged list, folded.
template <bool TWO>
__device__ __forceinline__ double2 gram_chains(const double* __restrict__ base, int64_t ld, const int32_t* scol,
                                               const double* scoef, int n) {
  auto load = [&](int k) -> double2 {
    const double* p = base + int64_t(scol[k]) * ld;
    if (TWO) return *reinterpret_cast<const double2*>(p);
    return double2{*p, 0.0};
  };
  double ax[kGrChains], ay[kGrChains];
#pragma unroll
  for (int l = 0; l < kGrChains; ++l) ax[l] = ay[l] = 0.0;
  int k0 = 0;
  for (; k0 + kGrChains <= n; k0 += kGrChains) {  // sixteen rows in flight, then sixteen independent chains
    double2 v[kGrChains];
#pragma unroll
    for (int l = 0; l < kGrChains; ++l) v[l] = load(k0 + l);
#pragma unroll
    for (int l = 0; l < kGrChains; ++l) {
      const double c = scoef[k0 + l];
      const double tx = c * v[l].x, ty = c * v[l].y;
      ax[l] = ax[l] + tx;
      ay[l] = ay[l] + ty;
    }
  }
#pragma unroll
  for (int l = 0; l < kGrChains; ++l)  // the last, partial round: the chains beyond the count add nothing
    if (k0 + l < n) {
      const double2 v = load(k0 + l);
      const double c = scoef[k0 + l];
      const double tx = c * v.x, ty = c * v.y;
      ax[l] = ax[l] + tx;
      ay[l] = ay[l] + ty;
    }
#pragma unroll
  for (int off = kGrChains / 2; off > 0; off >>= 1)
#pragma unroll
    for (int l = 0; l < off; ++l) {
      ax[l] = ax[l] + ax[l + off];
      ay[l] = ay[l] + ay[l + off];
    }
  return double2{ax[0], ay[0]};
}

template <bool TWIN>
__global__ __launch_bounds__(kGrNT) void gram_rowsum_kernel(const double* __restrict__ K, int64_t ld, int64_t nrow,
                                                            int64_t nloc, const int32_t* __restrict__ cols,
                                                            const double* __restrict__ coef,
                                                            const int32_t* __restrict__ cnt,
                                                            const int32_t* __restrict__ gate, double* __restrict__ f) {
  if (gate && *gate != 0) return;
  const int n = min(*cnt, kMaxWS);
  if (n <= 0) return;
  __shared__ int32_t scol[kMaxWS];
  __shared__ double scoef[kMaxWS];
  const int t = threadIdx.x;
  for (int k = t; k < n; k += kGrNT) {
    scol[k] = int32_t(min(max(int64_t(cols[k]), int64_t(0)), nrow - 1));
    scoef[k] = coef[k];
  }
  __syncthreads();
  const int64_t i0 = 2 * (int64_t(blockIdx.x) * kGrNT + t);
  if (i0 >= nloc) return;
  const bool two = i0 + 1 < nloc;
  const double2 r = two ? gram_chains<true>(K + i0, ld, scol, scoef, n) : gram_chains<false>(K + i0, ld, scol, scoef, n);
  f[i0] += r.x;
  if (TWIN) f[i0 + nloc] += r.x;
  if (two) {
    f[i0 + 1] += r.y;
    if (TWIN) f[i0 + 1 + nloc] += r.y;
  }
}

__global__ __launch_bounds__(kGrNT) void gram_kww_kernel(const double* __restrict__ K, int64_t ld, int64_t nrow,
                                                         const int32_t* __restrict__ W, const int32_t* __restrict__ mp,
                                                         int mcap, const int32_t* __restrict__ gate,
                                                         double* __restrict__ Kw, int64_t ldw) {
  if (gate && *gate != 0) return;
  const int m = min(*mp, mcap);
  const int lane = threadIdx.x & 63, a = blockIdx.x * (kGrNT / 64) + (threadIdx.x >> 6);
  if (a >= m) return;
  const double* row = K + int64_t(uint32_t(W[a]) % uint64_t(nrow)) * ld;
  for (int b = lane; b < m; b += 64) Kw[int64_t(a) * ldw + b] = row[uint32_t(W[b]) % uint64_t(nrow)];
}

constexpr int kGcT = 64, kGcLd = 65;

__global__ __launch_bounds__(kGrNT) void gram_check_kernel(const double* __restrict__ K, int64_t n, int64_t ld,
                                                           unsigned long long* __restrict__ bad) {
  const int64_t bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const int64_t r0 = bi * kGcT, c0 = bj * kGcT;
  // every index of this pair is at least r0 n + c0: nothing here can lower an answer already below that
  if (*reinterpret_cast<volatile unsigned long long*>(bad) < static_cast<unsigned long long>(r0 * n + c0)) return;
  __shared__ unsigned long long lower[kGcT * kGcLd];
  const int c = threadIdx.x & 63, rr = threadIdx.x >> 6;
  const unsigned long long* Kb = reinterpret_cast<const unsigned long long*>(K);
  for (int r = rr; r < kGcT; r += kGrNT / 64) {  // tile (bj, bi) in rows: K[c0 + r, r0 + c]
    const int64_t gi = c0 + r, gj = r0 + c;
    lower[r * kGcLd + c] = (gi < n && gj < n) ? Kb[gi * ld + gj] : 0ull;
  }
  __syncthreads();
  unsigned long long best = kGramOk;
  for (int r = rr; r < kGcT; r += kGrNT / 64) {  // tile (bi, bj) in rows against the transposed copy
    const int64_t gi = r0 + r, gj = c0 + c;
    if (gi >= n || gj >= n || gi > gj) continue;
    const unsigned long long up = Kb[gi * ld + gj], lo = lower[c * kGcLd + r];
    const bool finite = ((up >> 52) & 0x7FFull) != 0x7FFull;
    if (!finite || up != lo) best = min(best, static_cast<unsigned long long>(gi * n + gj));
  }
  if (best != kGramOk) atomicMin(bad, best);
}

__global__ __launch_bounds__(kGrNT) void gram_decision_kernel(const double* __restrict__ Kq, int64_t m, int64_t ncol,
                                                              int64_t ldq, const int32_t* __restrict__ sv,
                                                              const double* __restrict__ coef, int64_t nsv, double b,
                                                              double* __restrict__ dec) {
  const int lane = threadIdx.x & 63;
  const int64_t q = int64_t(blockIdx.x) * (kGrNT / 64) + (threadIdx.x >> 6);
  if (q >= m) return;
  const double* row = Kq + q * ldq;
  double v = 0.0;
  for (int64_t s = lane; s < nsv; s += 64) {
    const int64_t j = min(max(int64_t(sv[s]), int64_t(0)), ncol - 1);
    const double term = coef[s] * row[j];
    v = v + term;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
  if (lane == 0) dec[q] = v - b;
}

bool gram_ok(const GramRows& G) {
  return G.K && G.n >= 1 && G.ld >= G.n && G.ld % 2 == 0 && (reinterpret_cast<uintptr_t>(G.K) & 15) == 0;
}

}  // namespace

int launch_gram_rowsum(hipStream_t s, const GramRows& G, int64_t lo, int64_t nloc, const int32_t* cols,
                       const double* coef, const int32_t* cnt, const int32_t* gate, bool twin, double* f) {
  if (nloc <= 0) return SVM_OK;
  if (!gram_ok(G) || lo < 0 || lo % 2 != 0 || lo + nloc > G.n || !cols || !coef || !cnt || !f) {
    set_error("gram row sum: K 16-byte aligned with an even ld >= n, an even first column, columns within n, ids, "
              "coefficients, a count and f");
    return SVM_ERR_ARG;
  }
  const int64_t blocks = (nloc + 2 * kGrNT - 1) / (2 * kGrNT);
  if (blocks > 0x7FFFFFFF) {
    set_error("gram row sum: problem too large for one launch");
    return SVM_ERR_ARG;
  }
  hipLaunchKernelGGL(twin ? gram_rowsum_kernel<true> : gram_rowsum_kernel<false>, dim3(unsigned(blocks)), dim3(kGrNT), 0,
                     s, G.K + lo, G.ld, G.n, nloc, cols, coef, cnt, gate, f);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_gram_kww(hipStream_t s, const GramRows& G, const int32_t* W, const int32_t* m, int mcap,
                    const int32_t* gate, double* Kw, int64_t ldw) {
  if (mcap <= 0) return SVM_OK;
  if (!gram_ok(G) || G.n > int64_t(INT32_MAX) || !W || !m || mcap > kMaxWS || !Kw || ldw < mcap) {
    set_error("gram K(W, W): K 16-byte aligned with an even ld >= n, a working set of at most %d points, its size and "
              "Kw with ldw >= the capacity", kMaxWS);
    return SVM_ERR_ARG;
  }
  const int waves = kGrNT / 64;
  hipLaunchKernelGGL(gram_kww_kernel, dim3(unsigned((mcap + waves - 1) / waves)), dim3(kGrNT), 0, s, G.K, G.ld, G.n, W, m,
                     mcap, gate, Kw, ldw);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_gram_check(hipStream_t s, const GramRows& G, unsigned long long* bad) {
  const int64_t tiles = (G.n + kGcT - 1) / kGcT;
  if (!G.K || G.n < 1 || G.ld < G.n || !bad || tiles > 65535) {
    set_error("gram check: K with ld >= n, n <= %d and a result word", 65535 * kGcT);
    return SVM_ERR_ARG;
  }
  SVMD_CHECK(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(gram_check_kernel, dim3(unsigned(tiles), unsigned(tiles)), dim3(kGrNT), 0, s, G.K, G.n, G.ld, bad);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_gram_decision(hipStream_t s, const double* Kq, int64_t m, int64_t ncol, int64_t ldq, const int32_t* sv,
                         const double* coef, int64_t nsv, double b, double* dec) {
  if (m <= 0) return SVM_OK;
  const int64_t blocks = (m + kGrNT / 64 - 1) / (kGrNT / 64);
  if (!Kq || ncol < 1 || ldq < ncol || nsv < 0 || (nsv > 0 && (!sv || !coef)) || !dec || blocks > 0x7FFFFFFF) {
    set_error("gram decision: a query Gram with ldq >= its columns, support ids and coefficients, an output");
    return SVM_ERR_ARG;
  }
  hipLaunchKernelGGL(gram_decision_kernel, dim3(unsigned(blocks)), dim3(kGrNT), 0, s, Kq, m, ncol, ldq, sv, coef, nsv, b,
                     dec);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace svm355

using namespace svm355;

extern "C" {

SVM_API int svmd_gram_check(void* h, const double* K_d, int64_t n, int64_t ld, int64_t* bad_index) {
  SVMD_CTX(h);
  if (!bad_index) {
    set_error("svmd_gram_check: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  unsigned long long* bad = nullptr;
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { bad = c.take<unsigned long long>(1); }))) return rc;
  if ((rc = launch_gram_check(ctx->stream, GramRows{K_d, n, ld}, bad))) return rc;
  unsigned long long out = 0;
  SVMD_CHECK(hipMemcpyAsync(&out, bad, sizeof(out), hipMemcpyDeviceToHost, ctx->stream));
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  *bad_index = out == kGramOk ? int64_t(-1) : int64_t(out);
  return ctx->end();
}

SVM_API int svmd_decision_gram(void* h, const double* Kq_d, int64_t m, int64_t ncol, int64_t ldq, const int32_t* sv_d,
                               const double* coef_d, int64_t nsv, double b, double* out_d) {
  SVMD_CTX(h);
  if (m < 0) {
    set_error("svmd_decision_gram: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc || (rc = launch_gram_decision(ctx->stream, Kq_d, m, ncol, ldq, sv_d, coef_d, nsv, b, out_d))) return rc;
  return ctx->end();
}

// The two steps as the solver launches them, with a device-side count / size and stop gate of the given values.
SVM_API int svmd_gram_rowsum(void* h, const double* K_d, int64_t n, int64_t ld, const int32_t* cols_d,
                             const double* coef_d, int64_t ncols, int32_t count, int32_t gate, int32_t twin, double* f_d) {
  SVMD_CTX(h);
  if (ncols < 0 || ncols > kMaxWS || count < 0 || count > ncols) {
    set_error("svmd_gram_rowsum: 0 <= count <= ncols <= %d", kMaxWS);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  int32_t* dev = nullptr;  // {gate, count}
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { dev = c.take<int32_t>(16); }))) return rc;
  const int32_t host[2] = {gate, count};
  SVMD_CHECK(hipMemcpyAsync(dev, host, 8, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_gram_rowsum(ctx->stream, GramRows{K_d, n, ld}, 0, n, cols_d, coef_d, dev + 1, dev, twin != 0, f_d)))
    return rc;
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

SVM_API int svmd_gram_kww(void* h, const double* K_d, int64_t n, int64_t ld, const int32_t* W_d, int32_t m,
                          int32_t gate, double* Kw_d, int64_t ldw) {
  SVMD_CTX(h);
  if (m < 0 || m > kMaxWS) {
    set_error("svmd_gram_kww: 0 <= m <= %d", kMaxWS);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  int32_t* dev = nullptr;  // {gate, m}
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { dev = c.take<int32_t>(16); }))) return rc;
  const int32_t host[2] = {gate, m};
  SVMD_CHECK(hipMemcpyAsync(dev, host, 8, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_gram_kww(ctx->stream, GramRows{K_d, n, ld}, W_d, dev + 1, m, dev, Kw_d, ldw))) return rc;
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

}  // extern "C"
