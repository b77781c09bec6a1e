// Working-set decomposition SMO: the inner solve -- first- / second-order SMO on the working set in ONE
// workgroup (ws_inner_kernel) with the Newton polish of its free variables inlined (newton_wg).  Its own
// translation unit: the instantiations of the inner kernel are most of the solver's compile time.  The
// driver (decomp.hip) reaches it through launch_ws_inner / launch_ws_newton_probe only.
#include "decomp_dev.h"
#include "decomp_newton.h"
#include "persist.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

// ---- Newton polish of the working set's free variables (decomp_newton.h) ---------------------------------
// The inner workgroup's step on W's free set F (positions with c_lo < alpha < c_hi): the Cholesky of
// K_FF with the right-hand sides f_F and 1 as two extra rows, the back substitution, b and u, the step
// cut at the first bound, alpha and f of every position of W updated.  gA / gF: W's alpha and f by
// position (the caller's registers spilled there around the call); Amat: (|F| + 2) x ldA scratch.
// Every entry's arithmetic is newton_step_ref's, in its order (decomp_newton.h):
//   * the factorisation is left-looking in panels of kNwPW columns: a row's panel entries first take the
//     terms of every earlier column (ascending j, from the panel's own rows staged in LDS), then wave 0
//     factors the panel in LDS column by column (the diagonal's sqrt, the divisions, the updates of the
//     panel's later columns) with no workgroup barrier;
//   * the back substitution goes by blocks of 64 columns from the last: wave 0 solves the block's
//     triangle (staged in LDS) one column at a time, then every thread applies the block's 64 x to its
//     entries below, in descending column order;
//   * sums and the step's arg-min in the sequential order (thread 0; wave_arg's value-then-lowest-index).
// Returns 0 (nothing changed), 1 (full step) or 2 (cut at a bound), the same in every thread.
constexpr int kNwPW = 16;      // panel width
constexpr int kNwMax = kNewtonMaxFree;  // |F| bound of the LDS buffers: the cap shared with newton_step_ref,
                                        // which newton_cfg clamps NewtonCfg::max_free to (decomp_newton.h)
static_assert(2 * kNwMax + 64 * 64 <= kNwMax * kNwPW && kNwMax + 127 < kMaxWS,
              "lp also holds the back substitution's s1, s2 and 64 x 64 block; the row updates read 127 columns ahead");
// The factorisation's row updates for one panel (newton_wg): pb[r][c] = A[p0 + r][p0 + c] - sum_{j < p0}
// L[p0 + r][j] L[p0 + c][j] (ascending j) for the panel's rows r < ract and columns c < pw (lower entries;
// the right-hand-side rows nf, nf + 1 take every column), lp[j][c] = L[p0 + c][j] -- on FP64 MFMA
// (v_mfma_f64_16x16x4f64): a wave per 16-row tile of the panel rows,
// 16 columns, k-steps of 4 columns j..j+3.  The instruction sums its four products into the accumulator
// as four fused multiply-adds in k order -- measured bit for bit against the chain c = fma(a0, b0, c);
// ... fma(a3, b3, c) on 512,000 random entries (bench_kernels/mfma_f64_order.hip) -- so with A = -L (exact)
// every entry takes exactly newton_step_ref's ascending fma chain.  Lane l: A = -L[p0 + row0 + (l & 15)]
// [j + (l >> 4)], B = L[p0 + (l & 15)][j + (l >> 4)] (lp[j][c]); D: col = l & 15, row = (l >> 4) + 4 r.
__device__ __forceinline__ void newton_rows_mfma(const double* __restrict__ Amat, int64_t ldA,
                                                 const double* __restrict__ lp, double* __restrict__ pb, int p0, int pw,
                                                 int nf, int ract, int lane, int w, int nw) {
  const int col = lane & 15, g = lane >> 4;
  const int ntile = (ract + 15) / 16;
  for (int tile = w; tile < ntile; tile += nw) {
    const int r0 = tile * 16;
    const int ar = r0 + col;                 // the A operand's row (panel-local)
    const bool arv = ar < ract;
    const double* arow = Amat + int64_t(p0 + (arv ? ar : 0)) * ldA;
    f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = r0 + g + 4 * r, i = p0 + rr;
      acc[r] = rr < ract && col < pw && (i >= nf || p0 + col <= i) ? Amat[int64_t(i) * ldA + p0 + col] : 0.0;
    }
    // A operands 16 k-steps (64 columns) at a time, the next 16 loaded while these run: one wave per SIMD,
    // so only loads in flight hide their latency; k-steps at or beyond p0 are skipped (uniform), never
    // run with zero operands (an added 0 could flip the sign of a zero)
    // (the loads are unconditional -- columns up to p0 + 127 < kMaxWS stay inside Amat's row, and what
    // lies beyond p0 is never used -- so all 16 are in flight together; a branch around each would make
    // the compiler wait for every load before the next)
    double nx[16];
    auto load16 = [&](int j) {
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        const double v = arow[j + 4 * s2 + g];
        nx[s2] = arv ? -v : 0.0;
      }
    };
    load16(0);
    for (int j = 0; j < p0; j += 64) {
      double av[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) av[s2] = nx[s2];
      load16(j + 64);
      if (j + 64 <= p0) {
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], lp[(j + 4 * s2 + g) * kNwPW + col], acc, 0, 0, 0);
      } else {
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2)
          if (j + 4 * s2 < p0)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], lp[(j + 4 * s2 + g) * kNwPW + col], acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = r0 + g + 4 * r;
      if (rr < ract) pb[rr * kNwPW + col] = acc[r];
    }
  }
}

__device__ __forceinline__ int newton_wg(int m, const double* __restrict__ Kw, int64_t ldw, const int8_t* __restrict__ sy,
                                      double* __restrict__ gA, double* __restrict__ gF, double* __restrict__ Amat,
                                      double C, double eps, int max_free, int64_t* __restrict__ prof = nullptr) {
  constexpr int64_t ldA = kMaxWS;
  __shared__ int32_t fidx[kMaxWS];
  __shared__ __attribute__((aligned(16))) double pb[(kNwMax + 2) * kNwPW];  // the panel's rows; later x1, x2, u
  __shared__ __attribute__((aligned(16))) double lp[kNwMax * kNwPW];        // the panel's own rows of L (as [j][c]); later s1, s2, the diagonal blocks
  __shared__ int32_t s_wc[16];
  __shared__ int32_t s_fail, s_blk;
  __shared__ double s_t, s_b;
  __shared__ double s_wv[16];
  __shared__ uint32_t s_wi[16];
  const int t = threadIdx.x, nt = blockDim.x, lane = t & 63, w = t >> 6, nw = nt >> 6;
  const double c_hi = C - eps, c_lo = 0.0 + eps;
  if (prof && t == 0) prof[7] = wall_clock64();
  // 1. the free positions in ascending order
  int base = 0;
  for (int c0 = 0; c0 < m; c0 += nt) {
    const int k = c0 + t;
    const double ak = k < m ? gA[k] : 0.0;
    const bool fr = k < m && ak > c_lo && ak < c_hi;
    const unsigned long long bal = __ballot(fr);
    if (lane == 0) s_wc[w] = __popcll(bal);
    __syncthreads();
    int r = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
    for (int q = 0; q < nw; ++q) {
      if (q < w) r += s_wc[q];
      tot += s_wc[q];
    }
    if (fr) fidx[base + r] = k;
    base += tot;
    __syncthreads();
  }
  const int nf = base;
  if (nf < 2 || nf > min(max_free, kNwMax)) return 0;
  if (prof && threadIdx.x == 0) prof[0] = wall_clock64();
  // 2. A = K_FF (lower) and the right-hand sides f_F, 1 (rows nf, nf + 1); the lower triangle as one flat
  // range of nf (nf + 1) / 2 entries (row i starts at i (i + 1) / 2), 32 independent gathers per thread
  {
    constexpr int U = 32;
    const int64_t ne = int64_t(nf) * (nf + 1) / 2;
    for (int64_t e0 = t; e0 < ne; e0 += U * int64_t(nt)) {
      double v[U];
      int64_t dst[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t e1 = e0 + int64_t(u) * nt, e = min(e1, ne - 1);  // clamped: the gathers are unconditional
        int i = int((__builtin_sqrt(8.0 * double(e) + 1.0) - 1.0) * 0.5);
        i = int64_t(i) * (i + 1) / 2 > e ? i - 1 : int64_t(i + 1) * (i + 2) / 2 <= e ? i + 1 : i;
        const int k = int(e - int64_t(i) * (i + 1) / 2);
        v[u] = Kw[int64_t(fidx[i]) * ldw + fidx[k]];
        dst[u] = e1 < ne ? int64_t(i) * ldA + k : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (dst[u] >= 0) Amat[dst[u]] = v[u];
    }
  }
  for (int k = t; k < nf; k += nt) {
    Amat[int64_t(nf) * ldA + k] = gF[fidx[k]];
    Amat[int64_t(nf + 1) * ldA + k] = 1.0;
  }
  if (t == 0) s_fail = 0;
  __threadfence_block();
  __syncthreads();
  if (prof && threadIdx.x == 0) prof[1] = wall_clock64();
  // 3. the factorisation, a panel of kNwPW columns at a time: every panel row takes the terms of the earlier
  // columns (newton_rows, ascending j; the panel's own rows of L staged in LDS as lp[j][c]) into pb, wave 0
  // factors the panel's diagonal block in registers (a lane per row, readlane broadcasts), and a thread per
  // row then solves the rows below the block against it (ascending kk) and stores the panel to Amat.
  double* dblk = pb;  // the panel's diagonal block, kNwPW x kNwPW
  int64_t pt0 = 0;
  auto pstamp = [&](int k) {
    if (prof && t == 0) {
      const int64_t now = wall_clock64();
      if (pt0) prof[k] += now - pt0;
      pt0 = now;
    }
  };
  if (prof && t == 0) prof[8] = prof[9] = prof[10] = prof[11] = 0;
  for (int p0 = 0; p0 < nf; p0 += kNwPW) {
    const int pw = min(kNwPW, nf - p0);
    pstamp(11);
    for (int e = t; e < kNwPW * p0; e += nt) {  // lp[j][c] = L[p0 + c][j], j < p0
      const int j = e / kNwPW, c = e - j * kNwPW;
      lp[e] = c < pw ? Amat[int64_t(p0 + c) * ldA + j] : 0.0;
    }
    __syncthreads();
    // the earlier columns' terms on the panel's rows [p0, nf + 2), into pb[r][c] (r = row - p0): a thread per
    // row below 129 rows... above 128 rows (up to 3 rows per thread), 2 threads per row (8 columns each)
    // up to 128, 4 (4 columns each) up to 64 -- every lane busy however few rows are left
    const int ract = nf + 2 - p0;
    newton_rows_mfma(Amat, ldA, lp, pb, p0, pw, nf, ract, lane, w, nw);
    pstamp(8);
    __syncthreads();
    if (w == 0) {  // the diagonal block in wave 0's registers: lane r = row p0 + r
      double dr[kNwPW];
#pragma unroll
      for (int c = 0; c < kNwPW; ++c) dr[c] = lane < pw ? dblk[lane * kNwPW + c] : 0.0;
      bool bad = false;
#pragma unroll
      for (int kk = 0; kk < kNwPW; ++kk) {
        if (kk < pw) {
          const double d = read_lane64(dr[kk], kk);  // row kk's updated diagonal
          bad = bad || !(d > 1e-12);
          const double lkk = d > 1e-12 ? __builtin_sqrt(d) : 1.0;
          if (lane == kk) dr[kk] = lkk;
          if (lane > kk) dr[kk] = dr[kk] / lkk;
#pragma unroll
          for (int k2 = kk + 1; k2 < kNwPW; ++k2)
            if (k2 < pw) {
              const double lk2 = read_lane64(dr[kk], k2);  // L[p0 + k2][p0 + kk]
              if (lane >= k2) dr[k2] = __builtin_fma(-dr[kk], lk2, dr[k2]);
            }
        }
      }
      if (lane < pw)
#pragma unroll
        for (int c = 0; c < kNwPW; ++c) dblk[lane * kNwPW + c] = dr[c];
      if (lane == 0 && bad) s_fail = 1;
    }
    __syncthreads();
    pstamp(9);
    if (s_fail) return 0;
    // the rows below the block (and the two right-hand sides) against it, a thread per row; then every
    // row to Amat
    for (int r = t; r < ract; r += nt) {
      const int i = p0 + r;
      double sv[kNwPW];
#pragma unroll
      for (int c2 = 0; c2 < kNwPW / 2; ++c2) {
        const f64x2 v = reinterpret_cast<const f64x2*>(pb + r * kNwPW)[c2];
        sv[2 * c2] = v[0];
        sv[2 * c2 + 1] = v[1];
      }
      if (r >= pw) {
#pragma unroll
        for (int kk = 0; kk < kNwPW; ++kk)
          if (kk < pw) {
            sv[kk] = sv[kk] / dblk[kk * kNwPW + kk];
#pragma unroll
            for (int k2 = kk + 1; k2 < kNwPW; ++k2)
              if (k2 < pw) sv[k2] = __builtin_fma(-sv[kk], dblk[k2 * kNwPW + kk], sv[k2]);
          }
      }
#pragma unroll
      for (int c = 0; c < kNwPW; ++c)
        if (c < pw && (i >= nf || p0 + c <= i)) Amat[int64_t(i) * ldA + p0 + c] = sv[c];
    }
    __threadfence_block();
    __syncthreads();
    pstamp(10);
  }
  if (prof && threadIdx.x == 0) prof[2] = wall_clock64();
  // 4. back substitution: s1 / s2 = z (the right-hand-side rows), x = L^-T z, by blocks of 64 columns
  double* s1 = lp;
  double* s2 = lp + kNwMax;
  double* dB = lp + 2 * kNwMax;  // the block's triangle, 64 x 64
  double* x1 = pb;
  double* x2 = pb + kNwMax;
  for (int k = t; k < nf; k += nt) {
    s1[k] = Amat[int64_t(nf) * ldA + k];
    s2[k] = Amat[int64_t(nf + 1) * ldA + k];
  }
  for (int jb = (nf - 1) / 64 * 64; jb >= 0; jb -= 64) {
    const int je = min(jb + 64, nf), bw = je - jb;
    for (int e = t; e < 64 * 64; e += nt) {
      const int r = e >> 6, c = e & 63;
      dB[e] = r < bw && c <= r ? Amat[int64_t(jb + r) * ldA + jb + c] : 0.0;
    }
    __syncthreads();
    if (w == 0) {  // the block's triangle in registers: lane i holds column i (L_ji, j >= i) and s_i
      double col[64];
#pragma unroll
      for (int r = 0; r < 64; ++r) col[r] = dB[r * 64 + lane];
      const int i = jb + lane;
      double a1 = i < je ? s1[i] : 0.0, a2 = i < je ? s2[i] : 0.0;
#pragma unroll
      for (int r = 63; r >= 0; --r) {
        if (r < bw) {  // j = jb + r, descending
          const double ljj = read_lane64(col[r], r);
          const double xa = read_lane64(a1, r) / ljj, xb = read_lane64(a2, r) / ljj;
          if (lane == r) {
            x1[jb + r] = xa;
            x2[jb + r] = xb;
          }
          if (lane < r) {
            a1 = __builtin_fma(-col[r], xa, a1);
            a2 = __builtin_fma(-col[r], xb, a2);
          }
        }
      }
    }
    __syncthreads();
    for (int i = t; i < jb; i += nt) {  // the block's columns on the entries below it, descending j
      double a1 = s1[i], a2 = s2[i];
      for (int j0 = je - 1; j0 >= jb; j0 -= 32) {
        double l[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) l[u] = Amat[int64_t(max(j0 - u, jb)) * ldA + i];  // unconditional: all in flight
#pragma unroll
        for (int u = 0; u < 32; ++u)
          if (j0 - u >= jb) {
            a1 = __builtin_fma(-l[u], x1[j0 - u], a1);
            a2 = __builtin_fma(-l[u], x2[j0 - u], a2);
          }
      }
      s1[i] = a1;
      s2[i] = a2;
    }
    __syncthreads();
  }
  if (prof && threadIdx.x == 0) prof[3] = wall_clock64();
  // 5. b = sum x1 / sum x2 (ascending)
  if (t == 0) {
    double S1 = 0.0, S2 = 0.0;
    for (int k = 0; k < nf; ++k) {
      S1 += x1[k];
      S2 += x2[k];
    }
    const bool ok = S2 > 0.0 && __builtin_isfinite(S1);
    s_fail = ok ? 0 : 1;
    s_b = ok ? S1 / S2 : 0.0;
  }
  __syncthreads();
  if (s_fail) return 0;
  // 6. the step's cut: min over k of the bound ratios (value, then lowest k)
  const double b = s_b;
  double* dal = lp;  // dalpha by F position (s1 / s2 are consumed)
  VI best{__builtin_inf(), kSentinel};
  for (int k = t; k < nf; k += nt) {
    const double u = __builtin_fma(b, x2[k], -x1[k]);
    const double dk = sy[fidx[k]] == 1 ? u : -u;
    dal[k] = dk;
    const double ak = gA[fidx[k]];
    const double tk = dk > 0.0 ? (C - ak) / dk : dk < 0.0 ? (0.0 - ak) / dk : __builtin_inf();
    if (tk < best.v) best = VI{tk, uint32_t(k)};  // ascending k within a thread: strict keeps the lowest
  }
  const VIL wb = wave_arg<true>(best);
  if (lane == 0) {
    s_wv[w] = wb.v;
    s_wi[w] = wb.i;
  }
  __syncthreads();
  if (t == 0) {
    VI bb{s_wv[0], s_wi[0]};
    for (int q = 1; q < nw; ++q) {
      const VI c{s_wv[q], s_wi[q]};
      if (beats<true>(c, bb)) bb = c;
    }
    s_t = bb.v < 1.0 ? bb.v : 1.0;
    s_blk = bb.v < 1.0 ? int(bb.i) : -1;
  }
  __syncthreads();
  // 7. alpha, and the realised changes (an - a) y
  const double tt = s_t;
  const int blk = s_blk;
  double* ur = x1;  // x1 / x2 are consumed after the reads above
  __syncthreads();
  for (int k = t; k < nf; k += nt) {
    const double ak = gA[fidx[k]], dk = dal[k];
    double an = k == blk ? (dk > 0.0 ? C : 0.0) : __builtin_fma(tt, dk, ak);
    an = fmin(C, fmax(0.0, an));
    ur[k] = sy[fidx[k]] == 1 ? an - ak : ak - an;
    gA[fidx[k]] = an;
  }
  __threadfence_block();
  __syncthreads();
  if (prof && threadIdx.x == 0) prof[4] = wall_clock64();
  // 8. f of every position of W: f_q += sum_k K(F_k, q) ur_k (ascending k), 16 loads per batch
  for (int q0 = 0; q0 < m; q0 += 4 * nt) {  // four positions per thread at once: 4 x 16 loads in flight
    double sacc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < nf; k0 += 16) {
      double kv[4][16];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int q = min(q0 + v * nt + t, m - 1);  // clamped: the loads are unconditional, all in flight
#pragma unroll
        for (int u = 0; u < 16; ++u) kv[v][u] = Kw[int64_t(fidx[min(k0 + u, nf - 1)]) * ldw + q];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (k0 + u < nf) sacc[v] = __builtin_fma(kv[v][u], ur[k0 + u], sacc[v]);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int q = q0 + v * nt + t;
      if (q < m) gF[q] += sacc[v];
    }
  }
  __threadfence_block();
  __syncthreads();
  if (prof && t == 0) {
    prof[5] = wall_clock64();
    prof[6] = nf;
  }
  return blk >= 0 ? 2 : 1;
}

// One Newton step on a given working set (tests / timing, svmd_decomp_newton_probe): K(W, W) in Kw (m x
// m, row stride ldw), alpha and f by position in gA / gF (updated), labels y; *code_out = the step's code.
// One workgroup of NT threads, the inner solve's shapes (launch_ws_inner): newton_wg strides its tiles and
// rows by the NT / 64 waves it runs in.
template <int NT>
__global__ __launch_bounds__(NT) void ws_newton_probe_kernel(int m, const double* __restrict__ Kw, int64_t ldw,
                                                             const int32_t* __restrict__ y, double* __restrict__ gA,
                                                             double* __restrict__ gF, double* __restrict__ Amat,
                                                             double C, double eps, int max_free,
                                                             int32_t* __restrict__ code_out, int64_t* __restrict__ prof) {
  __shared__ int8_t sy[kMaxWS];
  for (int k = threadIdx.x; k < kMaxWS; k += blockDim.x) sy[k] = k < m ? int8_t(y[k]) : int8_t(0);
  __syncthreads();
  const int code = newton_wg(m, Kw, ldw, sy, gA, gF, Amat, C, eps, max_free, prof);
  if (threadIdx.x == 0) *code_out = code;
}

// First-order SMO on the working set in ONE workgroup of NT threads: thread t holds the PER contiguous
// points W[t PER + e] (f, alpha, y in registers; its entries of a K(W, W) row are PER / 2 16-byte loads).
// Per iteration:
//   select   branch-free thread-local (value, lowest position) minimum over I_high and maximum over
//            I_low, carrying the winner's alpha, then the wave64 arg-reductions (wave_arg);
//   publish  lane 0 of every wave writes its two candidates to LDS (double-buffered by iteration
//            parity) -- the iteration's ONE barrier;
//   merge    every lane folds the NW per-wave candidates itself (LDS broadcast reads, the same serial
//            order and tie rule everywhere), so all waves hold the identical (i_high, i_low, b_high,
//            b_low, alpha_h, alpha_l) with no second barrier; the pair's labels come from LDS;
//   rows     K12 and this thread's entries of the two rows of the L2-resident K(W, W);
//   update   the reference's clip / eta / update arithmetic on the same inputs in every thread
//            (persist_solve's sequence, main3.cpp:235-275) and f += ch K(i, .) + cl K(j, .).
// Stops at W's own gap <= 2 tau_in, at max_inner, or on a reference stop reason.  Then the points
// whose alpha changed are compacted in position order: cols[j] = their global ids, coef[j] =
// (alpha_new - alpha_old) y, *mcount = how many -- the f update of all n points reads only those.
// With packed rows (a shrunk solve, pos_of: local row -> packed position or -1), cdiag[j] = column j's
// packed position on this GPU (-1: none), the f update's unit diagonal.
//   DP (second order only): a second pair per iteration from the same selection -- i2 = the best
//            I_high candidate of the waves other than i_high's, j2 = the first-order j (max f over
//            I_low) -- whose rows load beside row i_high; after the first pair's update it is applied
//            if it is still a violating pair (f_j2 > f_i2 + 2 tau_in) and feasible.  32 % fewer
//            iterations of the chain at 60k for ~10 % more work per iteration.
//   J2S (with DP): j2 by the second-order gain of row i2 instead of the first-order j (row i2 loads
//            beside row i before the gains; both gains reduce in the same wave / barrier / fold).
//   CW (class weights): C is the box of the y = +1 points and Cn of the y = -1 points -- an element's own
//            upper bound in the set membership of every selection, and the pair's two boxes in the clip
//            of both pairs (smo_cpu.cpp has the expressions).  Without CW, Cn is not read and the code is
//            the unweighted kernel's.  Not built with the Newton polish (newton_wg is unweighted).
template <int NT, int PER, bool PROF = false, bool W2 = false, bool DP = false, bool J2S = false, bool NWT = false,
          bool CW = false>
__global__ __launch_bounds__(NT) void ws_inner_kernel(const double* __restrict__ Kw, int64_t ldw,
                                                      const int32_t* __restrict__ W, DecompCtl* __restrict__ ctl,
                                                      const int32_t* __restrict__ y, double* __restrict__ alpha,
                                                      const double* __restrict__ Wf, double C, double eps,
                                                      int32_t* __restrict__ cols, double* __restrict__ coef,
                                                      int32_t* __restrict__ mcount, DecompHost* __restrict__ hs,
                                                      DecompCtl* __restrict__ pub, const int32_t* __restrict__ pos_of,
                                                      int64_t lo, int64_t nloc, int32_t* __restrict__ cdiag,
                                                      double* __restrict__ gAw, double* __restrict__ gFw,
                                                      double* __restrict__ nAmat, NwDev nw, double Cn) {
  static_assert(!(CW && NWT), "the Newton polish is unweighted");
  if (ctl->stop != SVM_STOP_RUNNING) return;
  const int m = ctl->m;
  const double tau_in = ctl->tau_in;
  const int64_t max_inner = ctl->max_inner;
  constexpr int NW = NT / 64;
  static_assert(PER % 2 == 0, "row entries are loaded 16 bytes at a time");
  __shared__ double pv[2][2][NW], pa[2][2][NW];
  __shared__ uint32_t pi[2][2][NW];
  __shared__ double qv[2][NW], qa[2][NW], qf[2][NW], qk[2][NW];  // W2: the second index's candidates
  __shared__ uint32_t qi[2][NW];
  __shared__ double rv[2][NW], ra[2][NW], rf[2][NW], rk[2][NW];  // J2S: the second pair's j candidates
  __shared__ uint32_t ri2[2][NW];
  __shared__ int8_t sy[NT * PER];
  __shared__ int32_t wcnt[PER][NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  // position of this thread's element e: pair h = e / 2 of every lane is one 16-byte piece; a wave's 64
  // pieces of pair h are one contiguous kilobyte, and the NT / 64 waves' kilobytes of pair h are adjacent
  const int pbase = w * 128 + 2 * lane;
  auto pos = [&](int e) { return pbase + (e >> 1) * (2 * NT) + (e & 1); };
  double a[PER], a0[PER], ft[PER];
  bool yp[PER], yn[PER];  // y = +1 / y = -1 (padding: neither, so in neither set)
  int64_t gid[PER];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    const int k = pos(e);
    const bool valid = k < m;
    gid[e] = valid ? W[k] : 0;
    a[e] = valid ? alpha[gid[e]] : 0.0;
    a0[e] = a[e];
    const int32_t yk = valid ? y[gid[e]] : 0;
    yp[e] = yk == 1;
    yn[e] = yk == -1;
    sy[k] = int8_t(yk);
    ft[e] = valid ? Wf[k] : 0.0;
  }
  const double c_hi = C - eps, c_lo = 0.0 + eps, inf = __builtin_inf();
  const double c_hin = CW ? Cn - eps : c_hi;  // CW: c_hi is the y = +1 points' bound, c_hin the y = -1 points'
  // element e's upper bound (padding has neither label and is in neither set)
  auto chi = [&](int e) {
    if constexpr (CW)
      return yp[e] ? c_hi : c_hin;
    else
      return c_hi;
  };
  // the box of a point of W by its label
  auto box = [&](int32_t yk) {
    if constexpr (CW)
      return yk == 1 ? C : Cn;
    else
      return C;
  };
  int64_t it = 0;
  int32_t reason = SVM_STOP_CONVERGED;
  // the Newton polish (decomp_newton.h): chain iterations with no bound-status change, starting at `every`
  // after a long last inner solve (newton_since0)
  int32_t since = NWT && ctl->last_m > 0 && double(ctl->last_inner_it) >= nw.frac * double(ctl->last_m) ? nw.every : 0;
  int32_t ntrig = 0;
  int64_t nsteps = 0;
  // PROF: wave 0's clock at the phase boundaries (select | publish+barrier | merge | row loads | update)
  int64_t pacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int64_t pt = PROF ? int64_t(clock64()) : 0;
  const int64_t pc0 = pt, pw0 = PROF ? int64_t(wall_clock64()) : 0;
  // this thread's PER contiguous entries of row r of K(W, W) as 16-byte loads (in bounds: t PER + e <
  // NT PER <= ldw; the row base is 16-byte aligned: ldw even), zero beyond m
  auto row = [&](int r, double* out) {
    const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(r) * ldw + pbase);
#pragma unroll
    for (int h = 0; h < PER / 2; ++h) {
      const double2 v = src[NT * h];
      out[2 * h] = pos(2 * h) < m ? v.x : 0.0;
      out[2 * h + 1] = pos(2 * h + 1) < m ? v.y : 0.0;
    }
  };
  // a wave-uniform element of K(W, W) through a VECTOR load (in order with the row loads on vmcnt): a
  // scalar load would share lgkmcnt with the folds' LDS reads, which would then wait for it
  auto kval = [&](int r, int c) {
    int64_t off = int64_t(r) * ldw + c;
    asm volatile("" : "+v"(off));
    return Kw[off];
  };
  auto stamp = [&](int k) {
    if constexpr (PROF) {
      const int64_t now = int64_t(clock64());
      pacc[k] += now - pt;
      pt = now;
    }
  };
  for (int par = 0;; par ^= 1) {
    double hv = inf, lv = -inf, ha = 0.0, la = 0.0;
    uint32_t hi = kSentinel, li = kSentinel;
#pragma unroll
    for (int e = 0; e < PER; ++e) {  // ascending position within a thread: strict compares keep the lowest
      const bool below = a[e] < chi(e), above = a[e] > c_lo;
      const bool in_high = (yp[e] && below) || (yn[e] && above);
      const bool in_low = (yp[e] && above) || (yn[e] && below);
      const bool ch = in_high && ft[e] < hv, cl = in_low && ft[e] > lv;
      const uint32_t k = uint32_t(pos(e));
      hv = ch ? ft[e] : hv;
      ha = ch ? a[e] : ha;
      hi = ch ? k : hi;
      lv = cl ? ft[e] : lv;
      la = cl ? a[e] : la;
      li = cl ? k : li;
    }
    int lmn, lmx;  // the lanes holding the wave's winners publish them (no cross-lane reads)
    wave_arg_pair_lanes(VI{hv, hi}, VI{lv, li}, lmn, lmx);
    stamp(0);
    if (lane == lmn) {
      pv[par][0][w] = hv;
      pi[par][0][w] = hi;
      pa[par][0][w] = ha;
    }
    if (lane == lmx) {
      pv[par][1][w] = lv;
      pi[par][1][w] = li;
      pa[par][1][w] = la;
    }
    __syncthreads();
    stamp(1);
    // the same pairwise tree fold in every lane (value, then lowest position): log2(NW) dependent steps
    // fold (value, position) only, tracking the winning wave; its alpha is read from LDS afterwards
    double fv[2][NW];
    uint32_t fi[2][NW];
    int fw[2][NW];
#pragma unroll
    for (int q = 0; q < NW; ++q)
#pragma unroll
      for (int sd = 0; sd < 2; ++sd) {
        fv[sd][q] = pv[par][sd][q];
        fi[sd][q] = pi[par][sd][q];
        fw[sd][q] = q;
      }
#pragma unroll
    for (int st = 1; st < NW; st <<= 1)
#pragma unroll
      for (int q = 0; q + st < NW; q += 2 * st) {
        // bitwise, not short-circuit: the compiler turned || / && on these uniform values into branches
        const bool th = (fv[0][q + st] < fv[0][q]) | ((fv[0][q + st] == fv[0][q]) & (fi[0][q + st] < fi[0][q]));
        const bool tl = (fv[1][q + st] > fv[1][q]) | ((fv[1][q + st] == fv[1][q]) & (fi[1][q + st] < fi[1][q]));
        fv[0][q] = th ? fv[0][q + st] : fv[0][q];
        fi[0][q] = th ? fi[0][q + st] : fi[0][q];
        fw[0][q] = th ? fw[0][q + st] : fw[0][q];
        fv[1][q] = tl ? fv[1][q + st] : fv[1][q];
        fi[1][q] = tl ? fi[1][q + st] : fi[1][q];
        fw[1][q] = tl ? fw[1][q + st] : fw[1][q];
      }
    double bh = fv[0][0], bl = fv[1][0];
    uint32_t uih = fi[0][0], uil = fi[1][0];
    stamp(2);
    if (uih == kSentinel || uil == kSentinel) {
      reason = SVM_STOP_NO_CANDIDATE;
      break;
    }
    if (bl <= bh + 2.0 * tau_in) break;  // W's own optimum (reason stays CONVERGED)
    if (it >= max_inner) {
      reason = SVM_STOP_MAX_ITER;
      break;
    }
    if (NWT && since >= nw.every && ntrig < nw.per_solve) {  // uniform: the polish, then select again
      ++ntrig;
      since = 0;
#pragma unroll
      for (int e = 0; e < PER; ++e)
        if (pos(e) < m) {
          gAw[pos(e)] = a[e];
          gFw[pos(e)] = ft[e];
        }
      __threadfence_block();
      __syncthreads();
      int steps = 0;
      while (NWT && steps < nw.repeat) {
        const int code = newton_wg(m, Kw, ldw, sy, gAw, gFw, nAmat, C, eps, nw.max_free);
        if (code == 0) break;
        ++steps;
        if (code == 1) break;
      }
      if (steps > 0) {
#pragma unroll
        for (int e = 0; e < PER; ++e)
          if (pos(e) < m) {
            a[e] = gAw[pos(e)];
            ft[e] = gFw[pos(e)];
          }
        it += steps;
        nsteps += steps;
        continue;
      }
    }
    int ih = int(uih), il = int(uil);
    double K12, bl_upd = bl, al;  // the second index's f in the update (first order: b_low)
    double kh[PER], kl[PER];
    // DP: the second pair (i2, j2) and what its update needs, from the same selection
    int i2 = -1;
    double f2h = 0.0, a2h = 0.0, f2l = bl, a2l = 0.0;
    double2 r2h[PER / 2], r2l[PER / 2];  // DP: rows i2 and j2, raw, consumed by the second pair only
    double Kh_i2 = 0.0, Kh_j2 = 0.0, Kl_i2 = 0.0, Kl_j2 = 0.0, K2_12 = 0.0;
    bool dp_ok = false;
    if constexpr (DP) {
      const int wih = fw[0][0];
      double bv = inf;
      uint32_t bi = kSentinel;
      int bq = 0;
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        const double v = pv[par][0][q];
        const uint32_t ix = pi[par][0][q];
        const bool take = (q != wih) & ((v < bv) | ((v == bv) & (ix < bi)));
        bv = take ? v : bv;
        bi = take ? ix : bi;
        bq = take ? q : bq;
      }
      i2 = bi != kSentinel ? int(bi) : -1;
      f2h = bv;
      a2h = pa[par][0][bq];
      a2l = pa[par][1][fw[1][0]];
      dp_ok = J2S ? i2 >= 0 : i2 >= 0 && il != ih && i2 != il;  // (not J2S) il is still the first-order j = j2
    }
    int j2 = il;
    double2 rj[PER / 2];  // second order: row j's raw pieces, consumed only after the clip arithmetic
    if constexpr (!W2) {
      // one memory round trip: K12 and this thread's entries of the two rows; the labels from LDS
      K12 = Kw[int64_t(ih) * ldw + il];
      row(ih, kh);
      row(il, kl);
      al = pa[par][1][fw[1][0]];
    } else {
      // second-order choice of the second index (smo_cpu.cpp / persist_solve WSS2): row i_high, then
      // the maximum of (f_t - b_high)^2 / a_t over I_low points above b_high (a_t = 2 - 2 K(i, t),
      // floored at eps; reciprocal approximation: only the choice depends on it), a second barrier
      // and fold, then row j
      row(ih, kh);  // unconditional loads (no exec-mask branch per load)
      if constexpr (J2S) {  // row i2 now (its gains need it); row j2 and the K values after the fold
        const int ri = dp_ok ? i2 : ih;
        const double2* s2h = reinterpret_cast<const double2*>(Kw + int64_t(ri) * ldw + pbase);
#pragma unroll
        for (int h = 0; h < PER / 2; ++h) r2h[h] = s2h[NT * h];
        Kh_i2 = kval(ih, ri);
      } else if constexpr (DP) {
        {  // issued after row i (unconditionally -- row i again when there is no second pair: no branch
           // around loads, whose merge made the compiler wait for all of them before the gains)
          const int ri = dp_ok ? i2 : ih, rj2 = dp_ok ? j2 : ih;
          const double2* s2h = reinterpret_cast<const double2*>(Kw + int64_t(ri) * ldw + pbase);
          const double2* s2l = reinterpret_cast<const double2*>(Kw + int64_t(rj2) * ldw + pbase);
#pragma unroll
          for (int h = 0; h < PER / 2; ++h) r2h[h] = s2h[NT * h];
#pragma unroll
          for (int h = 0; h < PER / 2; ++h) r2l[h] = s2l[NT * h];
          Kh_i2 = kval(ih, ri);
          Kh_j2 = kval(ih, rj2);
          K2_12 = kval(ri, rj2);
        }
      }
      if constexpr (PROF) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        stamp(8);
      }
      double gv = inf;
      int ge = 0;  // the element of the thread's best gain: its alpha, f and K(i, j) are read by the winner
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const bool below = a[e] < chi(e), above = a[e] > c_lo;
        const bool in_low = (yp[e] && above) || (yn[e] && below);
        const double bb = ft[e] - bh;
        double at = 2.0 - 2.0 * kh[e];
        at = at <= 0.0 ? eps : at;
        // IEEE division (not v_rcp_f64): the choice is then reproducible on the host bit for bit
        // (svm_decomp_train_gram, the CPU oracle)
        const double gain = -(bb * bb) / at;
        const bool c = in_low && ft[e] > bh && gain < gv;
        gv = c ? gain : gv;
        ge = c ? e : ge;
      }
      const uint32_t gi = gv < inf ? uint32_t(pos(ge)) : kSentinel;
      double gv2 = inf;
      int ge2 = 0;
      if constexpr (J2S) {  // the same gain over I_low points above f(i2), on row i2 (f2h = inf: none)
#pragma unroll
        for (int e = 0; e < PER; ++e) {
          const bool below = a[e] < chi(e), above = a[e] > c_lo;
          const bool in_low = (yp[e] && above) || (yn[e] && below);
          const double bb = ft[e] - f2h;
          const double k2 = pos(e) < m ? ((e & 1) ? r2h[e >> 1].y : r2h[e >> 1].x) : 0.0;
          double at = 2.0 - 2.0 * k2;
          at = at <= 0.0 ? eps : at;
          const double gain = -(bb * bb) / at;
          const bool c = in_low && ft[e] > f2h && gain < gv2;
          gv2 = c ? gain : gv2;
          ge2 = c ? e : ge2;
        }
      }
      const uint32_t gi2 = gv2 < inf ? uint32_t(pos(ge2)) : kSentinel;
      const int lc = wave_arg_lane<true>(VI{gv, gi});
      const int lc2 = J2S ? wave_arg_lane<true>(VI{gv2, gi2}) : -1;
      stamp(9);
      if (lane == lc) {
        double ga = a[0], gf = ft[0], gk = kh[0];
#pragma unroll
        for (int e = 1; e < PER; ++e) {
          ga = ge == e ? a[e] : ga;
          gf = ge == e ? ft[e] : gf;
          gk = ge == e ? kh[e] : gk;
        }
        qv[par][w] = gv;
        qi[par][w] = gi;
        qa[par][w] = ga;
        qf[par][w] = gf;
        qk[par][w] = gk;
      }
      if (J2S && lane == lc2) {
        double ga = a[0], gf = ft[0], gk = r2h[0].x;
#pragma unroll
        for (int e = 1; e < PER; ++e) {
          ga = ge2 == e ? a[e] : ga;
          gf = ge2 == e ? ft[e] : gf;
          gk = ge2 == e ? ((e & 1) ? r2h[e >> 1].y : r2h[e >> 1].x) : gk;
        }
        rv[par][w] = gv2;
        ri2[par][w] = gi2;
        ra[par][w] = ga;
        rf[par][w] = gf;
        rk[par][w] = gk;
      }
      __syncthreads();
      stamp(10);
      // the same (value, lowest position) order as a serial fold, as a tree over (value, position);
      // the winner's alpha, f and K(i, j) are read from its wave's slot afterwards
      double cv[NW];
      uint32_t cj[NW];
      int cw[NW];
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        cv[q] = qv[par][q];
        cj[q] = qi[par][q];
        cw[q] = q;
      }
#pragma unroll
      for (int st = 1; st < NW; st <<= 1)
#pragma unroll
        for (int q = 0; q + st < NW; q += 2 * st) {
          const bool tk = (cv[q + st] < cv[q]) | ((cv[q + st] == cv[q]) & (cj[q + st] < cj[q]));
          cv[q] = tk ? cv[q + st] : cv[q];
          cj[q] = tk ? cj[q + st] : cj[q];
          cw[q] = tk ? cw[q + st] : cw[q];
        }
      if (cj[0] == kSentinel) {  // no I_low point above b_high (cannot happen while the gap is open)
        reason = SVM_STOP_NO_CANDIDATE;
        break;
      }
      il = int(cj[0]);
      stamp(11);
      {  // issued now, consumed after the clip / division below, which then runs under the loads' latency
        const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(il) * ldw + pbase);
#pragma unroll
        for (int h = 0; h < PER / 2; ++h) rj[h] = src[NT * h];
      }
      if constexpr (J2S) {  // the second pair's j: the same fold over the second gains
        double dv[NW];
        uint32_t dj[NW];
        int dw[NW];
#pragma unroll
        for (int q = 0; q < NW; ++q) {
          dv[q] = rv[par][q];
          dj[q] = ri2[par][q];
          dw[q] = q;
        }
#pragma unroll
        for (int st = 1; st < NW; st <<= 1)
#pragma unroll
          for (int q = 0; q + st < NW; q += 2 * st) {
            const bool tk = (dv[q + st] < dv[q]) | ((dv[q + st] == dv[q]) & (dj[q + st] < dj[q]));
            dv[q] = tk ? dv[q + st] : dv[q];
            dj[q] = tk ? dj[q + st] : dj[q];
            dw[q] = tk ? dw[q + st] : dw[q];
          }
        const bool jok = dj[0] != kSentinel;
        j2 = jok ? int(dj[0]) : ih;
        dp_ok = dp_ok && jok && j2 != ih && il != j2 && il != i2;
        f2l = rf[par][dw[0]];
        a2l = ra[par][dw[0]];
        K2_12 = rk[par][dw[0]];
        const int rj2 = dp_ok ? j2 : ih;
        const double2* s2l = reinterpret_cast<const double2*>(Kw + int64_t(rj2) * ldw + pbase);
#pragma unroll
        for (int h = 0; h < PER / 2; ++h) r2l[h] = s2l[NT * h];
        Kh_j2 = kval(ih, rj2);
        Kl_i2 = kval(il, dp_ok ? i2 : il);
        Kl_j2 = kval(il, rj2);
      } else if constexpr (DP) {
        dp_ok = dp_ok && il != j2 && il != i2;  // the second-order j must leave the second pair alone
        Kl_i2 = kval(il, dp_ok ? i2 : il);
        Kl_j2 = kval(il, dp_ok ? j2 : il);
      }
      al = qa[par][cw[0]];
      bl_upd = qf[par][cw[0]];
      K12 = qk[par][cw[0]];
    }
    const double ah = pa[par][0][fw[0][0]];
    const int32_t yh = sy[ih], yl = sy[il];
    if constexpr (PROF) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      stamp(3);
    }
    const double K11 = 1.0, K22 = 1.0;  // the Gram's unit diagonal
    const int s = yh * yl;
    double eta = K11 + K22 - 2.0 * K12;
    const double Ch = box(yh), Cl = box(yl);
    double U, V;
    if (s == -1) {
      U = fmax(0.0, al - ah);
      V = fmin(Cl, Ch + al - ah);
    } else {
      U = fmax(0.0, al + ah - Ch);
      V = fmin(Cl, al + ah);
    }
    if (!(U <= V + 1e-12)) {
      reason = SVM_STOP_INFEASIBLE;
      break;
    }
    // Identical rows (K12 = 1, or 1 - ulp from the FP64 Gram) with conflicting labels or targets: a violating
    // pair without curvature.  LIBSVM's rule, not the reference's stop: eta is floored at eps and the box clips
    // the step.  high is in I_high and low in I_low, so the step has room of more than eps in its direction;
    // with eta = eps it lands on U or V, which are finite.  (The second pair below still skips: the next
    // selection picks it up as a first pair.)
    eta = eta <= eps ? eps : eta;
    double al_new = al + double(yl) * (bh - bl_upd) / eta;
    if (al_new > V) al_new = V;
    if (al_new < U) al_new = U;
    const double ah_new = ah + double(s) * (al - al_new);
    const double ch = (ah_new - ah) * double(yh);
    const double cl = (al_new - al) * double(yl);
    // a bound-status change of an updated point (bound_status): the Newton polish waits for a settled set
    auto bst = [&](double v) { return v <= c_lo ? 0 : v >= c_hi ? 2 : 1; };
    bool moved_status = NWT && (bst(ah_new) != bst(ah) || bst(al_new) != bst(al));
    if constexpr (W2) {
#pragma unroll
      for (int h = 0; h < PER / 2; ++h) {
        double x = rj[h].x, z = rj[h].y;
        // an empty asm reading cl: the wait for row j's data lands here, after the division, not inside it
        asm volatile("" : "+v"(x), "+v"(z) : "v"(cl));
        kl[2 * h] = pos(2 * h) < m ? x : 0.0;
        kl[2 * h + 1] = pos(2 * h + 1) < m ? z : 0.0;
      }
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int k = pos(e);
      ft[e] += ch * kh[e] + cl * kl[e];  // main3.cpp:274 operation order
      a[e] = k == ih ? ah_new : k == il ? al_new : a[e];
    }
    ++it;
    if constexpr (DP) {
      if (dp_ok && it < max_inner) {
        // the second pair's f after the first update, as its owner thread computed it just now
        const double fi2 = f2h + (ch * Kh_i2 + cl * Kl_i2);
        const double fj2 = f2l + (ch * Kh_j2 + cl * Kl_j2);
        const int32_t yh2 = sy[i2], yl2 = sy[j2];
        const int s2 = yh2 * yl2;
        const double eta2 = K11 + K22 - 2.0 * K2_12;
        const double Ch2 = box(yh2), Cl2 = box(yl2);
        double U2, V2;
        if (s2 == -1) {
          U2 = fmax(0.0, a2l - a2h);
          V2 = fmin(Cl2, Ch2 + a2l - a2h);
        } else {
          U2 = fmax(0.0, a2l + a2h - Ch2);
          V2 = fmin(Cl2, a2l + a2h);
        }
        if (fj2 > fi2 + 2.0 * tau_in && U2 <= V2 + 1e-12 && !(eta2 <= eps)) {  // still violating, feasible
          double al2 = a2l + double(yl2) * (fi2 - fj2) / eta2;
          if (al2 > V2) al2 = V2;
          if (al2 < U2) al2 = U2;
          const double ah2 = a2h + double(s2) * (a2l - al2);
          const double ch2 = (ah2 - a2h) * double(yh2);
          const double cl2 = (al2 - a2l) * double(yl2);
          double k2h[PER], k2l[PER];
#pragma unroll
          for (int h = 0; h < PER / 2; ++h) {
            double x = r2h[h].x, z = r2h[h].y, u = r2l[h].x, v = r2l[h].y;
            asm volatile("" : "+v"(x), "+v"(z), "+v"(u), "+v"(v) : "v"(cl2));  // consumed here, not at the load
            k2h[2 * h] = pos(2 * h) < m ? x : 0.0;
            k2h[2 * h + 1] = pos(2 * h + 1) < m ? z : 0.0;
            k2l[2 * h] = pos(2 * h) < m ? u : 0.0;
            k2l[2 * h + 1] = pos(2 * h + 1) < m ? v : 0.0;
          }
#pragma unroll
          for (int e = 0; e < PER; ++e) {
            const int k = pos(e);
            ft[e] += ch2 * k2h[e] + cl2 * k2l[e];
            a[e] = k == i2 ? ah2 : k == j2 ? al2 : a[e];
          }
          ++it;
          if constexpr (NWT) moved_status = moved_status || bst(ah2) != bst(a2h) || bst(al2) != bst(a2l);
        }
      }
    }
    if constexpr (NWT) since = moved_status ? 0 : since + 1;
    stamp(4);
  }
  // compaction in position order: pair h, then wave, then lane, then e & 1
  bool chg[PER];
  int below[PER / 2];
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    chg[e] = pos(e) < m && a[e] != a0[e];
    if (chg[e]) alpha[gid[e]] = a[e];
  }
#pragma unroll
  for (int h = 0; h < PER / 2; ++h) {
    const unsigned long long b0 = __ballot(chg[2 * h]), b1 = __ballot(chg[2 * h + 1]);
    const unsigned long long lt = (1ull << lane) - 1ull;
    below[h] = __popcll(b0 & lt) + __popcll(b1 & lt);
    if (lane == 0) wcnt[h][w] = __popcll(b0) + __popcll(b1);
  }
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int h = 0; h < PER / 2; ++h) {
    int j = base + below[h];
    for (int q = 0; q < NW; ++q) {
      if (q < w) j += wcnt[h][q];
      base += wcnt[h][q];
    }
#pragma unroll
    for (int e = 2 * h; e < 2 * h + 2; ++e)
      if (chg[e]) {
        cols[j] = int32_t(gid[e]);
        coef[j] = (a[e] - a0[e]) * (yp[e] ? 1.0 : -1.0);
        // packed rows (shrinking): the column's row in the packed list, for the unit diagonal of the update
        if (cdiag) cdiag[j] = gid[e] >= lo && gid[e] < lo + nloc ? pos_of[gid[e] - lo] : -1;
        ++j;
      }
  }
  if (PROF && t == 0) {
    for (int k = 0; k < 5; ++k) hs->prof[k] += pacc[k];
    for (int k = 8; k < 12; ++k) hs->prof[k] += pacc[k];
    hs->prof[6] += int64_t(clock64()) - pc0;
    hs->prof[7] += int64_t(wall_clock64()) - pw0;
  }
  if (t == 0) {
    *mcount = base;
    ctl->outer += 1;
    ctl->inner_total += it;
    ctl->changed_total += base;
    ctl->last_inner_it = it;
    ctl->last_m = m;
    ctl->newton_steps += nsteps;
    ctl->last_inner_reason = reason;
    publish_ctl(*ctl, pub);
  }
}

// The instantiation for v's selection rule at one workgroup shape and build, in this precedence: the second
// pair's j by gain (j2s), the second pair with the Newton polish, the second pair, one pair; all but the
// last need second-order selection (S2).
template <int NT, int PER, bool PR, bool S2>
void launch_rule(hipStream_t s, const InnerVariant& v, const InnerArgs& a) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, s, a.Kw, a.ldw, a.W, a.ctl, a.y, a.alpha, a.Wf, a.C, a.eps, a.cols,
                       a.coef, a.mcount, a.hs, a.pub, a.pos_of, a.lo, a.nloc, a.cdiag, a.gAw, a.gFw, a.nAmat, a.nw, a.Cn);
  };
  if (v.j2s && S2)
    go(ws_inner_kernel<NT, PER, PR, S2, S2, S2>);
  else if (v.dp && S2 && v.newton)
    go(ws_inner_kernel<NT, PER, PR, S2, S2, false, true>);
  else if (v.dp && S2)
    go(ws_inner_kernel<NT, PER, PR, S2, S2>);
  else
    go(ws_inner_kernel<NT, PER, PR, S2>);
}

template <int NT, int PER>
void launch_shape(hipStream_t s, const InnerVariant& v, const InnerArgs& a) {
  if (v.prof && v.wss2)
    launch_rule<NT, PER, true, true>(s, v, a);
  else if (v.prof)
    launch_rule<NT, PER, true, false>(s, v, a);
  else if (v.wss2)
    launch_rule<NT, PER, false, true>(s, v, a);
  else
    launch_rule<NT, PER, false, false>(s, v, a);
}

// The weighted instantiations (per-class boxes): 256 x 4 under the second-order rule with the second pair
// (the default), the second-order rule alone and the first-order rule.
void launch_weighted(hipStream_t s, const InnerVariant& v, const InnerArgs& a) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(256), 0, s, a.Kw, a.ldw, a.W, a.ctl, a.y, a.alpha, a.Wf, a.C, a.eps, a.cols,
                       a.coef, a.mcount, a.hs, a.pub, a.pos_of, a.lo, a.nloc, a.cdiag, a.gAw, a.gFw, a.nAmat, a.nw, a.Cn);
  };
  if (v.wss2 && v.dp)
    go(ws_inner_kernel<256, 4, false, true, true, false, false, true>);
  else if (v.wss2)
    go(ws_inner_kernel<256, 4, false, true, false, false, false, true>);
  else
    go(ws_inner_kernel<256, 4, false, false, false, false, false, true>);
}

}  // namespace

bool ws_inner_weighted_built(const InnerVariant& v) { return v.nt == 256 && !v.prof && !v.j2s && !v.newton; }

int launch_ws_inner(hipStream_t s, const InnerVariant& v, const InnerArgs& a) {
  if (v.weighted) {
    if (!ws_inner_weighted_built(v)) {
      set_error("decomposition SMO: the weighted inner solve is not built for this variant");
      return SVM_ERR_ARG;
    }
    launch_weighted(s, v, a);
    return SVM_OK;
  }
  if (v.nt == 65)  // one wave x 6 points (a working set of <= 384)
    launch_shape<64, 6>(s, v, a);
  else if (v.nt == 64)
    launch_shape<64, 16>(s, v, a);
  else if (v.nt == 128)
    launch_shape<128, 8>(s, v, a);
  else if (v.nt == 256)
    launch_shape<256, 4>(s, v, a);
  else
    launch_shape<512, 2>(s, v, a);
  return SVM_OK;
}

bool ws_newton_probe_built(int nt) { return nt == 64 || nt == 128 || nt == 256 || nt == 512; }

int launch_ws_newton_probe(hipStream_t s, int nt, int m, const double* Kw, int64_t ldw, const int32_t* y, double* gA,
                           double* gF, double* Amat, double C, double eps, int max_free, int32_t* code_out, int64_t* prof) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(1), dim3(unsigned(nt)), 0, s, m, Kw, ldw, y, gA, gF, Amat, C, eps, max_free, code_out,
                       prof);
  };
  if (nt == 64)
    go(ws_newton_probe_kernel<64>);
  else if (nt == 128)
    go(ws_newton_probe_kernel<128>);
  else if (nt == 256)
    go(ws_newton_probe_kernel<256>);
  else if (nt == 512)
    go(ws_newton_probe_kernel<512>);
  else {
    set_error("decomposition SMO: the Newton probe is built for 64, 128, 256 or 512 threads, not %d", nt);
    return SVM_ERR_ARG;
  }
  return SVM_OK;
}

}  // namespace svm355

SVMD_TU_WARM(decomp_inner)
