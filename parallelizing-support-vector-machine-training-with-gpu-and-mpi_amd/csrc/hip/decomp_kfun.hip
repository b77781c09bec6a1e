// The dot-product kernels on the device (linear, polynomial, sigmoid: kfun.h): a kernel block on FP64 MFMA with no
// norms and no diagonal rule, and an inner solve that carries the diagonal K_ii in its curvature terms.  The RBF
// paths (gram_mfma.hip, decomp_inner.hip) have the unit diagonal in their arithmetic and are not touched; the
// driver (decomp.hip) chooses these kernels when svm_params.kernel != 0.
//
// ---- kfun_block_kernel: K = kfun(A B') ----------------------------------------------------------------------
// Split.  A workgroup of 4 waves owns 64 A rows; wave w owns rows 16 w .. 16 w + 15 of them for the WHOLE column
// range, so no sum ever crosses a wave.  Columns are walked in tiles of 64 (4 MFMA blocks of 16 per wave): the
// store epilogue takes the one tile blockIdx.y names, the sum epilogues walk the tiles 0, 1, ... in ascending
// order up to the device-side count *ncount.
// Data movement.  Lane (lr = lane & 15, lg = lane >> 4) supplies v_mfma_f64_16x16x4_f64's A operand for row lr of
// its wave: per k stage of 16 doubles it needs A[row][k0 + 4 lg .. k0 + 4 lg + 3], 32 contiguous bytes, which it
// loads straight from global memory into registers (two 16-byte loads, prefetched one stage ahead).  The A tile
// never goes through LDS and needs no barrier; it is re-read per column tile (64 rows x d doubles per workgroup, L2
// traffic).  The B tile (64 columns x 16 doubles, shared by the four waves) is staged through LDS, rows padded to
// 18 doubles, register-prefetched one stage ahead.  k-permutation: at sub-step s of a stage, lane group lg feeds
// k = k0 + 4 lg + s to both operands, so each lane reads its four B values with two ds_read_b128.
// Accumulation order of one output element: stages k0 ascending, sub-steps s = 0..3, the MFMA's four k slots in
// the hardware's fixed order.  It is the same for every element and does not depend on the tile's position, and
// the products commute, so kfun(A_i . B_j) and kfun(A_j . B_i) are the same bits: a full launch with A = B stores a
// matrix that is symmetric to the bit, with no mirror step, and two ids on one row (the epsilon-SVR twins) get
// that row's diagonal value.  The sum epilogues evaluate the same expression, so their kernel values are the
// store epilogue's bit for bit.
// Summation order of the sum epilogues (the CPU oracle's rowsum_update_kfun replays it).  For row i, lane lr
// starts from 0.0 and adds coef[c] * kfun(x_i . x_c) for the columns c = lr, lr + 16, lr + 32, ... < count in
// ascending order (product rounded, then the add: no FMA); a column >= count adds +0.0.  The 16 lanes are then
// folded by the xor butterfly 8, 4, 2, 1 (v[l] = v[l] + v[l ^ off]), lane 0 adds the result to f[i] (and to
// f[i + m] in the twin form).  No atomics, no order that depends on timing: two runs give the same bits.  A count
// of 0 and a non-zero gate return before anything is written.  No kernel value goes to HBM.
//
// ---- ws_inner_kfun_kernel -----------------------------------------------------------------------------------
// One workgroup of 256 threads x 4 points (decomp_nu.hip's layout: alpha and f in registers, labels in LDS, rows
// of K(W, W) read from L2).  The rule is SVM355_DECOMP_WSS=2's: i_high first order; j by the gain -(f_t - b_high)^2
// / a_t over the I_low points above b_high, a_t = K_ii + K_tt - 2 K_it (<= 0: eps), IEEE division, ties to the
// lowest position; the classifier's clip with the pair's boxes; eta = K_ii + K_jj - 2 K_ij floored at eps (the
// sigmoid kernel's negative curvature as LIBSVM handles it); main3.cpp:274's update order; the stop test on W's
// own gap.  The diagonal is read once per solve: each thread keeps its 4 entries in registers, K_ii of the chosen i
// comes from a 1,024-double LDS copy and K_jj travels with the published candidate.
#include "decomp_kfun.h"

#include "ctx.h"
#include "persist.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

constexpr int kKbM = 64, kKbN = 64, kKbK = 16, kKbLS = 18;

template <int EPI>  // KfunEpilogue
__global__ __launch_bounds__(256) void kfun_block_kernel(KfunBlock a) {
  if (a.gate && *a.gate != 0) return;
  int64_t n = a.ncap;
  if (a.ncount) n = min(n, int64_t(*a.ncount));
  if (n <= 0) return;
  constexpr bool STORE = EPI == int(KfunEpilogue::store);
  const int64_t tiles = (n + kKbN - 1) / kKbN;
  const int64_t ct0 = STORE ? int64_t(blockIdx.y) : 0, ct1 = STORE ? ct0 + 1 : tiles;
  if (ct0 >= tiles) return;
  __shared__ __attribute__((aligned(16))) double Bs[kKbN * kKbLS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 15, lg = lane >> 4;
  const int64_t bm = int64_t(blockIdx.x) * kKbM;
  const int64_t arow = bm + 16 * w + lr;
  const bool aok = arow < a.m;
  const double* ap = a.A + (aok ? arow * a.lda : 0) + 4 * lg;
  const int srow = t >> 2, scol = (t & 3) * 4;  // B staging: thread t copies 4 doubles of tile row t / 4
  const double2 z2 = {0.0, 0.0};
  double part[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t bn = ct * kKbN;
    const bool bok = bn + srow < n;
    const double* bp = a.B + (bok ? (bn + srow) * a.ldb : 0) + scol;
    double2 ra0, ra1, rb0, rb1;
#define KFUN_GLOAD(k0)                                                      \
  do {                                                                      \
    ra0 = aok ? *reinterpret_cast<const double2*>(ap + (k0)) : z2;          \
    ra1 = aok ? *reinterpret_cast<const double2*>(ap + (k0) + 2) : z2;      \
    rb0 = bok ? *reinterpret_cast<const double2*>(bp + (k0)) : z2;          \
    rb1 = bok ? *reinterpret_cast<const double2*>(bp + (k0) + 2) : z2;      \
  } while (0)
    KFUN_GLOAD(0);
    f64x4 acc[4];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) acc[nj] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t k0 = 0; k0 < a.kdim; k0 += kKbK) {
      __syncthreads();  // the previous stage (or tile) fully consumed
      *reinterpret_cast<double2*>(&Bs[srow * kKbLS + scol]) = rb0;
      *reinterpret_cast<double2*>(&Bs[srow * kKbLS + scol + 2]) = rb1;
      __syncthreads();
      const double av0 = ra0.x, av1 = ra0.y, av2 = ra1.x, av3 = ra1.y;
      if (k0 + kKbK < a.kdim) KFUN_GLOAD(k0 + kKbK);  // overlaps the MFMAs below
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        const double* p = &Bs[(nj * 16 + lr) * kKbLS + 4 * lg];
        const double2 y0 = *reinterpret_cast<const double2*>(p);
        const double2 y1 = *reinterpret_cast<const double2*>(p + 2);
        acc[nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av0, y0.x, acc[nj], 0, 0, 0);  // sub-steps s = 0..3
        acc[nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av1, y0.y, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av2, y1.x, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av3, y1.y, acc[nj], 0, 0, 0);
      }
    }
#undef KFUN_GLOAD
    // C / D layout of the f64 16x16x4 MFMA: column = lane & 15, row = (lane >> 4) + 4 r
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int64_t gj = bn + nj * 16 + lr;
      const bool jok = gj < n;
      const double cj = (!STORE && jok) ? a.coef[gj] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double kv = kfun_apply(a.kf, acc[nj][r]);
        if (STORE) {
          const int64_t gi = bm + 16 * w + lg + 4 * r;
          if (gi < a.m && jok) a.K[gi * a.ldk + gj] = kv;
        } else {
          const double term = cj * kv;
          part[r] += jok ? term : 0.0;
        }
      }
    }
  }
  if (!STORE) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = part[r];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
      const int64_t gi = bm + 16 * w + lg + 4 * r;
      if (lr == 0 && gi < a.m) {
        a.f[gi] += v;
        if (EPI == int(KfunEpilogue::sum_twin)) a.f[gi + a.m] += v;
      }
    }
  }
}

__global__ void kfun_fill_kernel(double* __restrict__ out, int64_t m, double v) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < m) out[i] = v;
}

// ---- inner solve ----------------------------------------------------------------------------------------
constexpr int kKfNT = 256, kKfPER = 4;

__global__ __launch_bounds__(kKfNT) void ws_inner_kfun_kernel(const double* __restrict__ Kw, int64_t ldw,
                                                              const int32_t* __restrict__ W, DecompCtl* __restrict__ ctl,
                                                              const int32_t* __restrict__ y, double* __restrict__ alpha,
                                                              const double* __restrict__ Wf, double Cp, double Cn,
                                                              double eps, int32_t* __restrict__ cols,
                                                              double* __restrict__ coef, int32_t* __restrict__ mcount,
                                                              DecompCtl* __restrict__ pub) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  constexpr int NT = kKfNT, PER = kKfPER, NW = NT / 64;
  const int m = min(ctl->m, kMaxWS);
  const double tau_in = ctl->tau_in;
  const int64_t max_inner = ctl->max_inner;
  __shared__ double pv[2][2][NW], pa[2][NW];  // the sides' extremes per wave (0 = I_high, 1 = I_low), I_high's alpha
  __shared__ uint32_t pi[2][2][NW];
  __shared__ double qv[2][NW], qa[2][NW], qf[2][NW], qk[2][NW], qd[2][NW];  // the second index's candidates
  __shared__ uint32_t qi[2][NW];
  __shared__ double sdiag[NT * PER];
  __shared__ int8_t sy[NT * PER];
  __shared__ int32_t wcnt[PER / 2][NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int pbase = w * 128 + 2 * lane;
  auto pos = [&](int e) { return pbase + (e >> 1) * (2 * NT) + (e & 1); };
  double a[PER], a0[PER], ft[PER], dg[PER], chi[PER];
  bool yp[PER], yn[PER];
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
    dg[e] = valid ? Kw[int64_t(k) * ldw + k] : 0.0;  // the diagonal: once per solve
    sdiag[k] = dg[e];
    chi[e] = (yp[e] ? Cp : Cn) - eps;  // the point's own box, less eps
  }
  const double c_lo = 0.0 + eps, inf = __builtin_inf();
  int64_t it = 0;
  int32_t reason = SVM_STOP_CONVERGED;
  for (int par = 0;; par ^= 1) {
    // 1. per-thread extremes: min f over I_high (with its alpha), max f over I_low; ascending position, strict
    double hv = inf, ha = 0.0, lv = -inf;
    uint32_t hi = kSentinel, li = kSentinel;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const bool below = a[e] < chi[e], above = a[e] > c_lo;
      const bool ih_ = ((yp[e] && below) || (yn[e] && above)) && ft[e] < hv;
      const bool il_ = ((yp[e] && above) || (yn[e] && below)) && ft[e] > lv;
      hv = ih_ ? ft[e] : hv;
      ha = ih_ ? a[e] : ha;
      hi = ih_ ? uint32_t(pos(e)) : hi;
      lv = il_ ? ft[e] : lv;
      li = il_ ? uint32_t(pos(e)) : li;
    }
    int wl0, wl1;
    wave_arg_pair_lanes(VI{hv, hi}, VI{lv, li}, wl0, wl1);
    if (lane == wl0) {
      pv[par][0][w] = hv;
      pi[par][0][w] = hi;
      pa[par][w] = ha;
    }
    if (lane == wl1) {
      pv[par][1][w] = lv;
      pi[par][1][w] = li;
    }
    __syncthreads();  // (the first one also covers sy and sdiag)
    // 2. the same fold in every lane: (value, then lowest position)
    double bh = pv[par][0][0], bl = pv[par][1][0], ah = pa[par][0];
    uint32_t uih = pi[par][0][0], uil = pi[par][1][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      const double v0 = pv[par][0][q], v1 = pv[par][1][q];
      const uint32_t i0 = pi[par][0][q], i1 = pi[par][1][q];
      const bool t0 = (v0 < bh) | ((v0 == bh) & (i0 < uih));
      const bool t1 = (v1 > bl) | ((v1 == bl) & (i1 < uil));
      ah = t0 ? pa[par][q] : ah;
      bh = t0 ? v0 : bh;
      uih = t0 ? i0 : uih;
      bl = t1 ? v1 : bl;
      uil = t1 ? i1 : uil;
    }
    if (uih == kSentinel || uil == kSentinel) {
      reason = SVM_STOP_NO_CANDIDATE;
      break;
    }
    if (bl <= bh + 2.0 * tau_in) break;  // W's own optimum (reason stays CONVERGED)
    if (it >= max_inner) {
      reason = SVM_STOP_MAX_ITER;
      break;
    }
    // 3. row i and its diagonal entry; every I_low point above b_high gets its gain
    const int ih = int(uih);
    const double Kii = sdiag[ih];
    double kh[PER];
    {
      const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(ih) * ldw + pbase);
#pragma unroll
      for (int h = 0; h < PER / 2; ++h) {
        const double2 v = src[NT * h];
        kh[2 * h] = pos(2 * h) < m ? v.x : 0.0;
        kh[2 * h + 1] = pos(2 * h + 1) < m ? v.y : 0.0;
      }
    }
    double gv = inf;
    int ge = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const bool in_low = (yp[e] && a[e] > c_lo) || (yn[e] && a[e] < chi[e]);
      const double bb = ft[e] - bh;
      double at = Kii + dg[e] - 2.0 * kh[e];
      at = at <= 0.0 ? eps : at;
      // IEEE division (not v_rcp_f64): the choice is reproducible on the host bit for bit (the CPU oracle)
      const double gain = -(bb * bb) / at;
      const bool c = in_low && ft[e] > bh && gain < gv;
      gv = c ? gain : gv;
      ge = c ? e : ge;
    }
    const uint32_t gi = gv < inf ? uint32_t(pos(ge)) : kSentinel;
    const int lc = wave_arg_lane<true>(VI{gv, gi});
    if (lane == lc) {
      double ga = a[0], gf = ft[0], gk = kh[0], gd = dg[0];
#pragma unroll
      for (int e = 1; e < PER; ++e) {
        ga = ge == e ? a[e] : ga;
        gf = ge == e ? ft[e] : gf;
        gk = ge == e ? kh[e] : gk;
        gd = ge == e ? dg[e] : gd;
      }
      qv[par][w] = gv;
      qi[par][w] = gi;
      qa[par][w] = ga;
      qf[par][w] = gf;
      qk[par][w] = gk;
      qd[par][w] = gd;
    }
    __syncthreads();
    double cv = qv[par][0];
    uint32_t cj = qi[par][0];
    int cw = 0;
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      const bool tk = (qv[par][q] < cv) | ((qv[par][q] == cv) & (qi[par][q] < cj));
      cv = tk ? qv[par][q] : cv;
      cj = tk ? qi[par][q] : cj;
      cw = tk ? q : cw;
    }
    if (cj == kSentinel) {
      reason = SVM_STOP_NO_CANDIDATE;
      break;
    }
    // 4. row j issued now, consumed after the clip and the division
    const int il = int(cj);
    double2 rj[PER / 2];
    {
      const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(il) * ldw + pbase);
#pragma unroll
      for (int h = 0; h < PER / 2; ++h) rj[h] = src[NT * h];
    }
    const double al = qa[par][cw], bl_upd = qf[par][cw], K12 = qk[par][cw], Kjj = qd[par][cw];
    const int32_t yh = sy[ih], yl = sy[il];
    const int s = yh * yl;
    double eta = Kii + Kjj - 2.0 * K12;
    const double Ch = yh == 1 ? Cp : Cn, Cl = yl == 1 ? Cp : Cn;
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
    eta = eta <= eps ? eps : eta;  // no (or negative) curvature: LIBSVM's floor, the box clips the step
    double al_new = al + double(yl) * (bh - bl_upd) / eta;
    if (al_new > V) al_new = V;
    if (al_new < U) al_new = U;
    const double ah_new = ah + double(s) * (al - al_new);
    const double ch = (ah_new - ah) * double(yh);
    const double cl = (al_new - al) * double(yl);
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int k = pos(e);
      const double kj = (e & 1) ? rj[e >> 1].y : rj[e >> 1].x;
      const double kle = k < m ? kj : 0.0;
      ft[e] += ch * kh[e] + cl * kle;
      a[e] = k == ih ? ah_new : a[e];
      a[e] = k == il ? al_new : a[e];
    }
    ++it;
  }
  // compaction in position order (ws_inner_kernel's): pair h, then wave, then lane, then e & 1
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
        ++j;
      }
  }
  if (t == 0) {
    *mcount = base;
    ctl->outer += 1;
    ctl->inner_total += it;
    ctl->changed_total += base;
    ctl->last_inner_it = it;
    ctl->last_m = m;
    ctl->last_inner_reason = reason;
    publish_ctl(*ctl, pub);
  }
}

}  // namespace

int launch_kfun_block(hipStream_t s, KfunEpilogue epi, const KfunBlock& b) {
  if (b.m <= 0 || b.ncap <= 0) return SVM_OK;
  const bool store = epi == KfunEpilogue::store;
  if (!b.A || !b.B || b.kdim < kKbK || b.kdim % kKbK || b.lda < b.kdim || b.ldb < b.kdim || (b.lda % 2) || (b.ldb % 2) ||
      (reinterpret_cast<uintptr_t>(b.A) & 15) || (reinterpret_cast<uintptr_t>(b.B) & 15) ||
      (store ? (!b.K || b.ldk < b.ncap) : (!b.coef || !b.f)) || b.kf.kind < kKernelLinear ||
      b.kf.kind > kKernelSigmoid || (b.kf.kind == kKernelPoly && (b.kf.degree < 1 || b.kf.degree > kMaxDegree))) {
    set_error("kfun block: a dot-product kernel (1..3, degree 1..%d), kdim a multiple of %d, lda / ldb even and >= "
              "kdim, A / B 16-byte aligned, ldk >= ncap (store) or coef and f (sum)", kMaxDegree, kKbK);
    return SVM_ERR_ARG;
  }
  const int64_t tiles_m = (b.m + kKbM - 1) / kKbM, tiles_n = (b.ncap + kKbN - 1) / kKbN;
  if (tiles_m > 0x7FFFFFFF || tiles_n > 65535) {
    set_error("kfun block: problem too large for one launch");
    return SVM_ERR_ARG;
  }
  switch (epi) {
    case KfunEpilogue::store:
      hipLaunchKernelGGL(kfun_block_kernel<int(KfunEpilogue::store)>, dim3(unsigned(tiles_m), unsigned(tiles_n)),
                         dim3(256), 0, s, b);
      break;
    case KfunEpilogue::sum:
      hipLaunchKernelGGL(kfun_block_kernel<int(KfunEpilogue::sum)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
    case KfunEpilogue::sum_twin:
      hipLaunchKernelGGL(kfun_block_kernel<int(KfunEpilogue::sum_twin)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
  }
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

void launch_ws_inner_kfun(hipStream_t s, const InnerArgs& a) {
  hipLaunchKernelGGL(ws_inner_kfun_kernel, dim3(1), dim3(kKfNT), 0, s, a.Kw, a.ldw, a.W, a.ctl, a.y, a.alpha, a.Wf, a.C,
                     a.Cn, a.eps, a.cols, a.coef, a.mcount, a.pub);
}

}  // namespace svm355

using namespace svm355;

extern "C" {

// The kernel block alone on caller-supplied device rows (tests): A (m x lda) against B (nb x ldb), kdim doubles per
// row, the kernel of *pp (kernel 1..3).  epi 0: K_d (m x ldk) = kfun(A B').  epi 1 / 2: f_d[i] += sum_j coef_d[j]
// kfun(A_i . B_j) (2: also f_d[i + m]).  count >= 0: a device-side column count of that value (count < 0: none,
// all nb columns); gate: the value of the device-side stop gate (non-zero: the launch is a no-op).
SVM_API int svmd_kfun_block(void* h, const double* A_d, int64_t m, int64_t lda, const double* B_d, int64_t nb,
                            int64_t ldb, int64_t kdim, const svm_params* pp, int32_t epi, int32_t count, int32_t gate,
                            double* K_d, int64_t ldk, const double* coef_d, double* f_d) {
  SVMD_CTX(h);
  if (!pp || !kfun_params_ok(*pp) || !kernel_is_dot(pp->kernel) || epi < 0 || epi > 2 || m < 1 || nb < 1) {
    set_error("svmd_kfun_block: bad arguments (a dot-product kernel: 1 linear, 2 poly or 3 sigmoid; epi 0..2; m, nb >= 1)");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  int32_t* dev = nullptr;  // {gate, count}
  if ((rc = carve_ws(ctx, [&](WsCarver& c) { dev = c.take<int32_t>(16); }))) return rc;
  const int32_t host[2] = {gate, count};
  SVMD_CHECK(hipMemcpyAsync(dev, host, 8, hipMemcpyHostToDevice, ctx->stream));
  KfunBlock b;
  b.A = A_d;
  b.m = m;
  b.lda = lda;
  b.B = B_d;
  b.ncap = nb;
  b.ldb = ldb;
  b.kdim = kdim;
  b.kf = kfun_of(*pp);
  b.gate = dev;
  b.ncount = count >= 0 ? dev + 1 : nullptr;
  b.K = K_d;
  b.ldk = ldk;
  b.coef = coef_d;
  b.f = f_d;
  if ((rc = launch_kfun_block(ctx->stream, KfunEpilogue(epi), b))) return rc;
  SVMD_CHECK(hipStreamSynchronize(ctx->stream));
  return ctx->end();
}

// svmd_decision's sibling for the dot-product kernels: out_d[i] = sum_k coef_d[k] kfun(Xs_k . Xq_i) - b over the
// nsv support vectors, the sum epilogue over chunks of 1,024 support vectors taken in order, from out = -b.
SVM_API int svmd_decision_kfun(void* h, const double* Xs_d, const double* coef_d, int64_t nsv, int64_t lds,
                               const double* Xq_d, int64_t m, int64_t ldq, int64_t kdim, const svm_params* pp,
                               double b, double* out_d) {
  SVMD_CTX(h);
  if (!pp || !kfun_params_ok(*pp) || !kernel_is_dot(pp->kernel) || !out_d || m < 0 || nsv < 0) {
    set_error("svmd_decision_kfun: bad arguments (a dot-product kernel: 1 linear, 2 poly or 3 sigmoid)");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (m == 0) return ctx->end();
  hipLaunchKernelGGL(kfun_fill_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, ctx->stream, out_d, m, -b);
  SVMD_LAUNCH_CHECK();
  for (int64_t c0 = 0; c0 < nsv; c0 += kMaxWS) {
    KfunBlock blk;
    blk.A = Xq_d;
    blk.m = m;
    blk.lda = ldq;
    blk.B = Xs_d + c0 * lds;
    blk.ncap = std::min<int64_t>(kMaxWS, nsv - c0);
    blk.ldb = lds;
    blk.kdim = kdim;
    blk.kf = kfun_of(*pp);
    blk.coef = coef_d + c0;
    blk.f = out_d;
    if ((rc = launch_kfun_block(ctx->stream, KfunEpilogue::sum, blk))) return rc;
  }
  return ctx->end();
}

}  // extern "C"
