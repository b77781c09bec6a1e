// Working-set decomposition SMO with a box per point (sample weights; decomp_mode.h, svm355_device.h): 0 <= alpha_i
// <= C_i with C_i = (C w_class(y_i)) w_i for the classifier, and 0 <= a_k, a*_k <= C w_k for the regression (twin)
// solve, whose two points of row k share box[k].  ws_select_kernel and ws_inner_kernel (decomp.hip,
// decomp_inner.hip) take the box as two scalars picked by label and cannot express that; their text is untouched
// and the driver chooses the kernels below when a solve brings weights.  ws_build_kernel never reads a box and is
// used as it is, as are K(W, W), the f update, the column cache, the twin fold and the stop gate.
//
//   ws_box_kernel         box[k] = Cc(y_k) * w_k over the n kernel rows, once per fit, in FP64: Cc is the class box
//                         svm_class_boxes computed on the host (C * weight), so the value is (C w_class) w_i with one
//                         multiply here -- the CPU oracle's expression.  A weight of 0 gives a box of exactly 0.
//   ws_select_box_kernel  ws_select_kernel's scheme: 256 threads x 16 points in registers, every wave's T best per
//                         side by wave arg-reductions (the winner masked by its owner), the merge of the four sorted
//                         wave lists in LDS, (value, lowest index) order.  The box is one more coalesced 8-byte load
//                         beside alpha (twin mode: row k's box for the points k and k + nrow, 256 consecutive points
//                         of a thread step read 256 consecutive boxes on either side of nrow).  It is consumed at once:
//                         membership is a < box - eps / a > eps by sign, after which only the two key arrays (f or
//                         +-inf) and the ids stay live, the classifier's register budget.  A box of 0 gives box - eps
//                         < 0 <= a and a = 0 <= eps: the point is on neither side and is never picked.
//   ws_inner_box_kernel   one workgroup of 256 threads x 4 points (decomp_kfun.hip's layout: alpha, f and the boxes in
//                         registers, labels in LDS, rows of K(W, W) read from L2), SVM355_DECOMP_WSS=2's rule with the
//                         RBF's unit diagonal: i_high first order; j by the gain -(f_t - b_high)^2 / (2 - 2 K_it)
//                         over the I_low points above b_high (<= 0: eps), IEEE division, ties to the lowest position;
//                         smo_cpu.cpp's two-box clip with C_i, C_j; eta = 1 + 1 - 2 K_ij floored at eps; main3.cpp:274's
//                         update order; the stop test on W's own gap.
//                         The pair's boxes travel with the published candidates, as alpha does: the lane that holds a
//                         wave's I_high extreme writes its box beside its alpha (pc), the lane that holds a wave's
//                         best gain writes its box beside alpha, f and K_ij (qc), and every lane reads both in the
//                         folds it already runs after the barriers it already waits at.  The alternative, a
//                         1,024-double LDS copy filled once per solve, costs 8 KB and puts a dependent LDS read
//                         (address = the folded position) after each fold; the carried box adds 64 bytes of LDS, no
//                         barrier and no address that depends on a reduction's result.
#include "decomp_dev.h"
#include "persist.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

// ---- the boxes ------------------------------------------------------------------------------------------
__global__ void ws_box_kernel(const int32_t* __restrict__ y, const double* __restrict__ w, int64_t nrow, double Cp,
                              double Cn, double* __restrict__ box) {
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= nrow) return;
  const double cc = (y && y[k] != 1) ? Cn : Cp;  // twin mode: no labels, one box C
  box[k] = cc * w[k];
}

// ---- select ---------------------------------------------------------------------------------------------
constexpr int kBoxTMax = 64;  // T <= q / (2 * 8 blocks)

__global__ __launch_bounds__(kSelNT) void ws_select_box_kernel(const double* __restrict__ f,
                                                               const double* __restrict__ alpha,
                                                               const int32_t* __restrict__ y,
                                                               const double* __restrict__ box, int64_t n, int64_t nrow,
                                                               int64_t per, int T, double eps,
                                                               CandRec* __restrict__ cand_h, CandRec* __restrict__ cand_l,
                                                               const DecompCtl* __restrict__ ctl) {
  if (ctl->stop != SVM_STOP_RUNNING || T > kBoxTMax) return;
  constexpr int NW = kSelNT / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t b0 = int64_t(blockIdx.x) * per, b1 = std::min<int64_t>(n, b0 + per);
  const double c_lo = 0.0 + eps, inf = __builtin_inf();
  double fh[kSelE], fl[kSelE];
  uint32_t gi[kSelE];  // point ids, ascending in e
#pragma unroll
  for (int e = 0; e < kSelE; ++e) {
    const int64_t k = b0 + t + int64_t(kSelNT) * e;
    fh[e] = inf;
    fl[e] = -inf;
    gi[e] = uint32_t(k);
    if (k < b1) {
      const double a = alpha[k], fi = f[k];
      const double c_hi = box[k >= nrow ? k - nrow : k] - eps;  // the point's own box, dead after the two tests
      const int32_t yi = y[k];
      if ((yi == 1 && a < c_hi) || (yi == -1 && a > c_lo)) fh[e] = fi;
      if ((yi == 1 && a > c_lo) || (yi == -1 && a < c_hi)) fl[e] = fi;
    }
  }
  __shared__ double lv[2][NW][kBoxTMax];
  __shared__ uint32_t li[2][NW][kBoxTMax];
  for (int k = 0; k < T; ++k) {
    VI mn{inf, kSentinel}, mx{-inf, kSentinel};
#pragma unroll
    for (int e = 0; e < kSelE; ++e) {  // ascending index within a thread: strict compares keep the lowest
      const uint32_t i = gi[e];
      const bool ch = fh[e] < mn.v, cl = fl[e] > mx.v;
      mn = ch ? VI{fh[e], i} : mn;
      mx = cl ? VI{fl[e], i} : mx;
    }
    VIL a, b;
    wave_arg_pair(mn, mx, a, b);
    if (lane == 0) {
      lv[0][w][k] = a.v;
      li[0][w][k] = a.i;
      lv[1][w][k] = b.v;
      li[1][w][k] = b.i;
    }
#pragma unroll
    for (int e = 0; e < kSelE; ++e) {
      if (gi[e] == a.i) fh[e] = inf;
      if (gi[e] == b.i) fl[e] = -inf;
    }
  }
  __syncthreads();
  if (t == 0 || t == 64) {  // wave 0 merges I_high, wave 1 I_low
    const int sd = t == 0 ? 0 : 1;
    int ptr[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) ptr[q] = 0;
    CandRec* out = (sd == 0 ? cand_h : cand_l) + int64_t(blockIdx.x) * T;
    for (int k = 0; k < T; ++k) {
      int bq = 0;
      VI best{lv[sd][0][ptr[0]], li[sd][0][ptr[0]]};
#pragma unroll
      for (int q = 1; q < NW; ++q) {
        const VI c{lv[sd][q][ptr[q]], li[sd][q][ptr[q]]};
        const bool take = sd == 0 ? beats<true>(c, best) : beats<false>(c, best);
        if (take) {
          best = c;
          bq = q;
        }
      }
      ++ptr[bq];  // a wave's list holds T entries: no list runs out before T picks
      const bool ok = best.i != kSentinel && (sd == 0 ? best.v < inf : best.v > -inf);
      out[k] = CandRec{ok ? best.v : 0.0, ok ? int32_t(best.i) : -1, 0};
    }
  }
}

// ---- inner solve ----------------------------------------------------------------------------------------
constexpr int kBxNT = 256, kBxPER = 4;
static_assert(kBxNT * kBxPER == kMaxWS, "one workgroup holds a full working set");

__global__ __launch_bounds__(kBxNT) void ws_inner_box_kernel(const double* __restrict__ Kw, int64_t ldw,
                                                             const int32_t* __restrict__ W, DecompCtl* __restrict__ ctl,
                                                             const int32_t* __restrict__ y, double* __restrict__ alpha,
                                                             const double* __restrict__ Wf,
                                                             const double* __restrict__ box, int64_t nrow, double eps,
                                                             int32_t* __restrict__ cols, double* __restrict__ coef,
                                                             int32_t* __restrict__ mcount, DecompCtl* __restrict__ pub) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  constexpr int NT = kBxNT, PER = kBxPER, NW = NT / 64;
  const int m = min(ctl->m, kMaxWS);
  const double tau_in = ctl->tau_in;
  const int64_t max_inner = ctl->max_inner;
  // the sides' extremes per wave (0 = I_high, 1 = I_low), I_high's alpha and box
  __shared__ double pv[2][2][NW], pa[2][NW], pc[2][NW];
  __shared__ uint32_t pi[2][2][NW];
  __shared__ double qv[2][NW], qa[2][NW], qf[2][NW], qk[2][NW], qc[2][NW];  // the second index's candidates
  __shared__ uint32_t qi[2][NW];
  __shared__ int8_t sy[NT * PER];
  __shared__ int32_t wcnt[PER / 2][NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int pbase = w * 128 + 2 * lane;
  auto pos = [&](int e) { return pbase + (e >> 1) * (2 * NT) + (e & 1); };
  double a[PER], a0[PER], ft[PER], bx[PER], chi[PER];
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
    bx[e] = valid ? box[gid[e] >= nrow ? gid[e] - nrow : gid[e]] : 0.0;  // the point's own box: once per solve
    chi[e] = bx[e] - eps;
  }
  const double c_lo = 0.0 + eps, inf = __builtin_inf();
  int64_t it = 0;
  int32_t reason = SVM_STOP_CONVERGED;
  for (int par = 0;; par ^= 1) {
    // 1. per-thread extremes: min f over I_high (with its alpha and box), max f over I_low; ascending position
    double hv = inf, ha = 0.0, hc = 0.0, lv = -inf;
    uint32_t hi = kSentinel, li = kSentinel;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const bool below = a[e] < chi[e], above = a[e] > c_lo;
      const bool ih_ = ((yp[e] && below) || (yn[e] && above)) && ft[e] < hv;
      const bool il_ = ((yp[e] && above) || (yn[e] && below)) && ft[e] > lv;
      hv = ih_ ? ft[e] : hv;
      ha = ih_ ? a[e] : ha;
      hc = ih_ ? bx[e] : hc;
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
      pc[par][w] = hc;
    }
    if (lane == wl1) {
      pv[par][1][w] = lv;
      pi[par][1][w] = li;
    }
    __syncthreads();  // (the first one also covers sy)
    // 2. the same fold in every lane: (value, then lowest position)
    double bh = pv[par][0][0], bl = pv[par][1][0], ah = pa[par][0], Ch = pc[par][0];
    uint32_t uih = pi[par][0][0], uil = pi[par][1][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      const double v0 = pv[par][0][q], v1 = pv[par][1][q];
      const uint32_t i0 = pi[par][0][q], i1 = pi[par][1][q];
      const bool t0 = (v0 < bh) | ((v0 == bh) & (i0 < uih));
      const bool t1 = (v1 > bl) | ((v1 == bl) & (i1 < uil));
      ah = t0 ? pa[par][q] : ah;
      Ch = t0 ? pc[par][q] : Ch;
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
    // 3. row i; every I_low point above b_high gets its gain
    const int ih = int(uih);  // < m: a position some lane published for a valid point
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
      double at = 2.0 - 2.0 * kh[e];
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
      double ga = a[0], gf = ft[0], gk = kh[0], gc = bx[0];
#pragma unroll
      for (int e = 1; e < PER; ++e) {
        ga = ge == e ? a[e] : ga;
        gf = ge == e ? ft[e] : gf;
        gk = ge == e ? kh[e] : gk;
        gc = ge == e ? bx[e] : gc;
      }
      qv[par][w] = gv;
      qi[par][w] = gi;
      qa[par][w] = ga;
      qf[par][w] = gf;
      qk[par][w] = gk;
      qc[par][w] = gc;
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
    const double al = qa[par][cw], bl_upd = qf[par][cw], K12 = qk[par][cw], Cl = qc[par][cw];
    const int32_t yh = sy[ih], yl = sy[il];
    const int s = yh * yl;
    double eta = 1.0 + 1.0 - 2.0 * K12;
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
    eta = eta <= eps ? eps : eta;  // identical rows: LIBSVM's floor, the box clips the step
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

void launch_ws_box(hipStream_t s, const int32_t* y, const double* w, int64_t nrow, double Cp, double Cn, double* box) {
  hipLaunchKernelGGL(ws_box_kernel, dim3(unsigned((nrow + 255) / 256)), dim3(256), 0, s, y, w, nrow, Cp, Cn, box);
}

void launch_ws_select_box(hipStream_t s, const BoxSelectArgs& a) {
  hipLaunchKernelGGL(ws_select_box_kernel, dim3(unsigned(a.NB)), dim3(kSelNT), 0, s, a.f, a.alpha, a.y, a.box, a.n,
                     a.nrow, a.per, a.T, a.eps, a.cand_h, a.cand_l, a.ctl);
}

void launch_ws_inner_box(hipStream_t s, const InnerArgs& a, const double* box, int64_t nrow) {
  hipLaunchKernelGGL(ws_inner_box_kernel, dim3(1), dim3(kBxNT), 0, s, a.Kw, a.ldw, a.W, a.ctl, a.y, a.alpha, a.Wf, box,
                     nrow, a.eps, a.cols, a.coef, a.mcount, a.pub);
}

}  // namespace svm355
