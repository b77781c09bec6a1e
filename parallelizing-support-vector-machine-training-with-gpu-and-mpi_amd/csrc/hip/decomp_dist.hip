// The additive distance kernels on the device (laplacian, chi2: kfun.h): K = exp(-gamma D), D = sum_k term(a_k, b_k)
// with term = |a - b| or (a - b)^2 / (a + b).  There is no matrix instruction for this: the block is FP64 VALU work
// (laplacian: one subtract and one add with the abs source modifier per (i, j, k); chi2 adds a square, a sum and an
// IEEE division under a + b > 0), so the layout is about feeding the VALU.  Both kernels have a unit diagonal, so the
// driver (decomp.hip) runs the RBF inner solve on the stored K(W, W) unchanged.
//
// ---- dist_block_kernel<CHI2, EPI>: K = exp(-gamma D(A, B)) ---------------------------------------------------
// Split.  A workgroup of 4 waves owns 64 A rows; lane l of EVERY wave owns row l of them, so a row's D never crosses
// a lane.  Columns are walked in tiles of 8 (the lane's register block of 8 accumulators): the store epilogue gives
// wave w the one tile 4 blockIdx.y + w, the sum epilogues give it the tiles w, w + 4, w + 8, ... up to the
// device-side count *ncount.  The four waves are there for latency: 60,000 rows are only 938 workgroups, under one
// per SIMD if each were a single wave.
// Data movement.  The A operand is the lane's own row: per k stage of 4 doubles, two 16-byte loads straight from
// global memory into registers, issued one stage ahead; it is re-read per column tile (each loaded double feeds 8
// terms, 16 FP64 VALU instructions for laplacian, so A traffic is ~0.5 byte per VALU cycle of a wave).  The B operand
// is wave-uniform: a tile's 8 rows are read by uniform plain-C++ loads (the wave index comes through readfirstlane),
// which the compiler emits as scalar loads into SGPRs -- 8 columns x 4 doubles x 2 = 64 SGPRs a stage -- and the VALU
// takes each B value as its one scalar source operand.  No LDS and no barrier on the path, so LDS bandwidth is no
// limit; the SGPR file is: the laplacian sum instantiations use all 102 SGPRs (no spill at 8 x 4, none to spare), which
// is why only two scalar loads are in flight per wait.
// Accumulation order of one output element: k ascending in a single chain, acc = acc + term(a_k, b_k), the same for
// every element whatever its tile.  |a - b|, (a - b)^2 and a + b commute to the bit, so a full launch with A = B
// stores a matrix that is symmetric to the bit with no mirror step; identical rows (the diagonal, and the
// epsilon-SVR twins) give D = 0 and exp(-0) = 1.0 exactly; zero padding adds exactly 0.  K = exp(-gamma D) with the
// FP64 library exp; the sum epilogues evaluate the same expression, so their kernel values are the store epilogue's
// bit for bit.
// Summation order of the sum epilogues.  For row i, wave w starts from 0.0 and adds coef[c] * K_ic (product rounded,
// then the add: no FMA) for the columns c of its tiles w, w + 4, ... < count in ascending order; the four partial
// sums go through LDS and wave 0 forms ((p0 + p1) + p2) + p3, adds it to f[i] (and to f[i + m] in the twin form).
// No atomics, no order that depends on timing: two runs give the same bits.  A count of 0 and a non-zero gate return
// before anything is written.  No kernel value goes to HBM.
#include "decomp_dist.h"

#include <algorithm>

#include "ctx.h"
#include "decomp_dev.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

constexpr int kDbM = 64, kDbTN = 8, kDbNW = 4, kDbKS = 4;

template <bool CHI2, int EPI>  // DistEpilogue
__global__ __launch_bounds__(kDbM* kDbNW) void dist_block_kernel(DistBlock a) {
  if (a.gate && *a.gate != 0) return;
  int64_t n = a.ncap;
  if (a.ncount) n = min(n, int64_t(*a.ncount));
  if (n <= 0) return;
  constexpr bool STORE = EPI == int(DistEpilogue::store);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));  // wave-uniform by construction: B stays scalar
  const int64_t tiles = (n + kDbTN - 1) / kDbTN;
  const int64_t ct0 = STORE ? int64_t(blockIdx.y) * kDbNW + w : w;
  const int64_t ct1 = STORE ? min(ct0 + 1, tiles) : tiles;
  const int64_t arow = int64_t(blockIdx.x) * kDbM + lane;
  const bool aok = arow < a.m;
  const double* __restrict__ ap = a.A + (aok ? arow : 0) * a.lda;  // a lane past m computes on row 0 and writes nothing
  const double ng = -a.gamma;
  double part = 0.0;
  for (int64_t ct = ct0; ct < ct1; ct += kDbNW) {
    const int64_t bn = ct * kDbTN;
    const double* __restrict__ bp[kDbTN];  // a column past n reads row n - 1 and is dropped in the epilogue
#pragma unroll
    for (int c = 0; c < kDbTN; ++c) bp[c] = a.B + min(bn + c, n - 1) * a.ldb;
    double acc[kDbTN];
#pragma unroll
    for (int c = 0; c < kDbTN; ++c) acc[c] = 0.0;
    double2 n0 = *reinterpret_cast<const double2*>(ap), n1 = *reinterpret_cast<const double2*>(ap + 2);
    for (int64_t k0 = 0; k0 < a.kdim; k0 += kDbKS) {
      const double a0 = n0.x, a1 = n0.y, a2 = n1.x, a3 = n1.y;
      if (k0 + kDbKS < a.kdim) {  // the next stage: overlaps the VALU work below
        n0 = *reinterpret_cast<const double2*>(ap + k0 + kDbKS);
        n1 = *reinterpret_cast<const double2*>(ap + k0 + kDbKS + 2);
      }
#pragma unroll
      for (int c = 0; c < kDbTN; ++c) {
        const double* __restrict__ b = bp[c] + k0;
        acc[c] += dist_term<CHI2>(a0, b[0]);
        acc[c] += dist_term<CHI2>(a1, b[1]);
        acc[c] += dist_term<CHI2>(a2, b[2]);
        acc[c] += dist_term<CHI2>(a3, b[3]);
      }
    }
#pragma unroll
    for (int c = 0; c < kDbTN; ++c) {
      const int64_t gj = bn + c;
      if (gj < n) {  // uniform
        const double kv = exp(ng * acc[c]);
        if constexpr (STORE) {
          if (aok) a.K[arow * a.ldk + gj] = kv;
        } else {
          const double term = a.coef[gj] * kv;
          part += term;
        }
      }
    }
  }
  if constexpr (!STORE) {
    __shared__ double ps[kDbNW][kDbM];
    ps[w][lane] = part;
    __syncthreads();
    if (w == 0 && aok) {
      const double v = ((ps[0][lane] + ps[1][lane]) + ps[2][lane]) + ps[3][lane];
      a.f[arow] += v;
      if (EPI == int(DistEpilogue::sum_twin)) a.f[arow + a.m] += v;
    }
  }
}

__global__ void dist_fill_kernel(double* __restrict__ out, int64_t m, double v) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < m) out[i] = v;
}

template <bool CHI2>
void launch_dist_term(hipStream_t s, DistEpilogue epi, const DistBlock& b, unsigned tiles_m, unsigned groups_n) {
  switch (epi) {
    case DistEpilogue::store:
      hipLaunchKernelGGL((dist_block_kernel<CHI2, int(DistEpilogue::store)>), dim3(tiles_m, groups_n),
                         dim3(kDbM * kDbNW), 0, s, b);
      break;
    case DistEpilogue::sum:
      hipLaunchKernelGGL((dist_block_kernel<CHI2, int(DistEpilogue::sum)>), dim3(tiles_m), dim3(kDbM * kDbNW), 0, s, b);
      break;
    case DistEpilogue::sum_twin:
      hipLaunchKernelGGL((dist_block_kernel<CHI2, int(DistEpilogue::sum_twin)>), dim3(tiles_m), dim3(kDbM * kDbNW), 0, s,
                         b);
      break;
  }
}

}  // namespace

int launch_dist_block(hipStream_t s, DistEpilogue epi, const DistBlock& b) {
  if (b.m <= 0 || b.ncap <= 0) return SVM_OK;
  const bool store = epi == DistEpilogue::store;
  if (!b.A || !b.B || b.kdim < 16 || b.kdim % 16 || b.lda < b.kdim || b.ldb < b.kdim || (b.lda % 2) ||
      (reinterpret_cast<uintptr_t>(b.A) & 15) || (reinterpret_cast<uintptr_t>(b.B) & 7) ||
      (store ? (!b.K || b.ldk < b.ncap) : (!b.coef || !b.f)) || !kernel_is_dist(b.kind) || !(b.gamma > 0.0)) {
    set_error("dist block: a distance kernel (4 laplacian, 5 chi2) with gamma > 0, kdim a multiple of 16, lda even, "
              "lda / ldb >= kdim, A 16-byte aligned, ldk >= ncap (store) or coef and f (sum)");
    return SVM_ERR_ARG;
  }
  const int64_t tiles_m = (b.m + kDbM - 1) / kDbM, groups_n = (b.ncap + kDbTN * kDbNW - 1) / (kDbTN * kDbNW);
  if (tiles_m > 0x7FFFFFFF || groups_n > 65535) {
    set_error("dist block: problem too large for one launch");
    return SVM_ERR_ARG;
  }
  if (b.kind == kKernelChi2)
    launch_dist_term<true>(s, epi, b, unsigned(tiles_m), unsigned(groups_n));
  else
    launch_dist_term<false>(s, epi, b, unsigned(tiles_m), unsigned(groups_n));
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace svm355

using namespace svm355;

extern "C" {

// The distance block alone on caller-supplied device rows (tests), svmd_kfun_block's arguments: A (m x lda) against
// B (nb x ldb), kdim doubles per row, the kernel of *pp (kernel 4 or 5).  epi 0: K_d (m x ldk).  epi 1 / 2: f_d[i] +=
// sum_j coef_d[j] K_ij (2: also f_d[i + m]).  count >= 0: a device-side column count of that value (count < 0: none,
// all nb columns); gate: the value of the device-side stop gate (non-zero: the launch is a no-op).
SVM_API int svmd_dist_block(void* h, const double* A_d, int64_t m, int64_t lda, const double* B_d, int64_t nb,
                            int64_t ldb, int64_t kdim, const svm_params* pp, int32_t epi, int32_t count, int32_t gate,
                            double* K_d, int64_t ldk, const double* coef_d, double* f_d) {
  SVMD_CTX(h);
  if (!pp || !kfun_params_ok(*pp) || !kernel_is_dist(pp->kernel) || epi < 0 || epi > 2 || m < 1 || nb < 1) {
    set_error("svmd_dist_block: bad arguments (a distance kernel with gamma > 0, epi 0..2, m, nb >= 1)");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  int32_t* dev = nullptr;  // {gate, count}
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { dev = c.take<int32_t>(16); }))) return rc;
  const int32_t host[2] = {gate, count};
  SVMD_CHECK(hipMemcpyAsync(dev, host, 8, hipMemcpyHostToDevice, ctx->stream));
  DistBlock b;
  b.A = A_d;
  b.m = m;
  b.lda = lda;
  b.B = B_d;
  b.ncap = nb;
  b.ldb = ldb;
  b.kdim = kdim;
  b.kind = pp->kernel;
  b.gamma = pp->gamma;
  b.gate = dev;
  b.ncount = count >= 0 ? dev + 1 : nullptr;
  b.K = K_d;
  b.ldk = ldk;
  b.coef = coef_d;
  b.f = f_d;
  if ((rc = launch_dist_block(ctx->stream, DistEpilogue(epi), b))) return rc;
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

// svmd_decision_kfun's sibling for the distance kernels: out_d[i] = sum_k coef_d[k] K(Xs_k, Xq_i) - b over the nsv
// support vectors, the sum epilogue over chunks of 1,024 support vectors taken in order, from out = -b.
SVM_API int svmd_decision_dist(void* h, const double* Xs_d, const double* coef_d, int64_t nsv, int64_t lds,
                               const double* Xq_d, int64_t m, int64_t ldq, int64_t kdim, const svm_params* pp,
                               double b, double* out_d) {
  SVMD_CTX(h);
  if (!pp || !kfun_params_ok(*pp) || !kernel_is_dist(pp->kernel) || !out_d || m < 0 || nsv < 0) {
    set_error("svmd_decision_dist: bad arguments (a distance kernel with gamma > 0)");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (m == 0) return ctx->end();
  hipLaunchKernelGGL(dist_fill_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, ctx->stream, out_d, m, -b);
  SVMD_LAUNCH_CHECK();
  for (int64_t c0 = 0; c0 < nsv; c0 += kMaxWS) {
    DistBlock blk;
    blk.A = Xq_d;
    blk.m = m;
    blk.lda = ldq;
    blk.B = Xs_d + c0 * lds;
    blk.ncap = std::min<int64_t>(kMaxWS, nsv - c0);
    blk.ldb = lds;
    blk.kdim = kdim;
    blk.kind = pp->kernel;
    blk.gamma = pp->gamma;
    blk.coef = coef_d + c0;
    blk.f = out_d;
    if ((rc = launch_dist_block(ctx->stream, DistEpilogue::sum, blk))) return rc;
  }
  return ctx->end();
}

}  // extern "C"
