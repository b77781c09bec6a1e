// Working-set decomposition SMO, the nu modes (nu-SVC and nu-SVR; decomp_mode.h, svm355.h): the kernels of an
// outer iteration for problems with TWO equality constraints, y'a = 0 and e'a = const.  A feasible step moves a
// pair of points of one sign, so every selection runs per sign class c in {+, -}: I_high and I_low are the
// classifier's sets (smo_cpu.cpp) intersected with the class, b_high_c = min f over I_high of c, b_low_c = max f
// over I_low of c, and the stop test is max_c (b_low_c - b_high_c) <= 2 tau; a class with an empty side has no
// gap.  ws_select_kernel, ws_build_kernel and ws_inner_kernel (decomp.hip, decomp_inner.hip) pick one pair over
// all points and cannot express that; their text is untouched and the driver chooses this trio by mode.  K(W, W),
// the f update, the column cache, the twin fold and the chunked start are the classifier's.
//
//   ws_select_nu_kernel  per block of <= 4,096 points, Tc picks for each of four sorted lists (I_high +, I_high -,
//                        I_low +, I_low -).  The scheme is ws_select_kernel's -- 256 threads x 16 points in
//                        registers, per-wave picks by wave arg-reductions, a merge of the sorted wave lists,
//                        (value, lowest index) order -- but the four keys per point do NOT cost four register
//                        arrays: a point has one sign, so of its four keys two are always "none".  A thread keeps
//                        the classifier's two arrays (f where the point is in I_high, f where it is in I_low: 64
//                        VGPRs) plus ONE 16-bit sign mask, and the thread-local pass routes each point's two keys
//                        to its class's two running extremes: 4 (value, index) candidates = 12 VGPRs live across
//                        the wave passes, against 128 + 16 for four key arrays (which would halve the occupancy).
//                        The kernel compiles to 107 VGPRs and no scratch.
//                        The four wave reductions run as two wave_arg_pair calls (min and max high-word
//                        butterflies interleaved, as in the classifier's), + class then - class.  The LDS merge is
//                        [list][wave][pick] and the block's four waves merge one list each, concurrently: the
//                        merge's serial chain is Tc long, not 4 Tc.
//   ws_build_nu_kernel   one workgroup over the L = 4 NB Tc candidates: the four extremes, the stop test on the
//                        larger class gap, and W by the no-sort placement (a block now has 4 Tc picks; a point may
//                        be in its class's two lists).
//   ws_inner_nu_kernel   one workgroup of 256 threads x 4 points: LIBSVM's Solver_NU rule.  Per iteration the
//                        per-class minima / maxima in registers, ONE publish and barrier for all four sides (the
//                        double-buffered slots are 4 wide), the fold in every lane, the stop test, BOTH rows i_+
//                        and i_- issued together, every I_low point's second-order gain against its own class's
//                        row -- again one gain per point, so one reduction, barrier and fold give the (i, j) of
//                        smallest gain over both classes --, row j, and the classifier's update with s = +1.
#include "decomp_dev.h"
#include "persist.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

constexpr int kNuLists = 4;               // I_high +, I_high -, I_low +, I_low -
constexpr int kNuTMax = kMaxWS / 4 / 8;   // Tc <= q / (4 x 8 blocks) = 32

// ---- select ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSelNT) void ws_select_nu_kernel(const double* __restrict__ f,
                                                              const double* __restrict__ alpha,
                                                              const int32_t* __restrict__ sgn, int64_t n, int64_t per,
                                                              int Tc, double C, double eps, CandRec* __restrict__ cand,
                                                              const DecompCtl* __restrict__ ctl) {
  if (ctl->stop != SVM_STOP_RUNNING || Tc > kNuTMax) return;
  constexpr int NW = kSelNT / 64;
  static_assert(NW == kNuLists, "one wave merges one list");
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t NB = gridDim.x;
  const int64_t b0 = int64_t(blockIdx.x) * per, b1 = std::min<int64_t>(n, b0 + per);
  const double c_hi = C - eps, c_lo = 0.0 + eps, inf = __builtin_inf();
  double fh[kSelE], fl[kSelE];
  uint32_t gi[kSelE];  // point ids, ascending in e
  uint32_t up = 0;     // bit e: point e has sign +1
#pragma unroll
  for (int e = 0; e < kSelE; ++e) {
    const int64_t k = b0 + t + int64_t(kSelNT) * e;
    fh[e] = inf;
    fl[e] = -inf;
    gi[e] = uint32_t(k);
    if (k < b1) {
      const double a = alpha[k], fi = f[k];
      const bool p = sgn[k] == 1, below = a < c_hi, above = a > c_lo;
      if (p ? below : above) fh[e] = fi;
      if (p ? above : below) fl[e] = fi;
      up |= p ? (1u << e) : 0u;
    }
  }
  __shared__ double lv[kNuLists][NW][kNuTMax];
  __shared__ uint32_t li[kNuLists][NW][kNuTMax];
  for (int k = 0; k < Tc; ++k) {
    VI hp{inf, kSentinel}, hn{inf, kSentinel}, lp{-inf, kSentinel}, ln{-inf, kSentinel};
#pragma unroll
    for (int e = 0; e < kSelE; ++e) {  // ascending index within a thread: strict compares keep the lowest
      const uint32_t i = gi[e];
      const bool p = (up >> e) & 1u;
      const bool chp = p & (fh[e] < hp.v), chn = !p & (fh[e] < hn.v);
      const bool clp = p & (fl[e] > lp.v), cln = !p & (fl[e] > ln.v);
      hp = chp ? VI{fh[e], i} : hp;
      hn = chn ? VI{fh[e], i} : hn;
      lp = clp ? VI{fl[e], i} : lp;
      ln = cln ? VI{fl[e], i} : ln;
    }
    VIL ahp, alp, ahn, aln;
    wave_arg_pair(hp, lp, ahp, alp);
    wave_arg_pair(hn, ln, ahn, aln);
    if (lane == 0) {
      lv[0][w][k] = ahp.v;
      li[0][w][k] = ahp.i;
      lv[1][w][k] = ahn.v;
      li[1][w][k] = ahn.i;
      lv[2][w][k] = alp.v;
      li[2][w][k] = alp.i;
      lv[3][w][k] = aln.v;
      li[3][w][k] = aln.i;
    }
#pragma unroll
    for (int e = 0; e < kSelE; ++e) {  // ids are distinct across the classes: the winner's id names its key
      if (gi[e] == ahp.i || gi[e] == ahn.i) fh[e] = inf;
      if (gi[e] == alp.i || gi[e] == aln.i) fl[e] = -inf;
    }
  }
  __syncthreads();
  if (lane == 0) {  // wave w merges list w: the first Tc of the merge of the four sorted wave lists
    const int list = w;
    const bool mn = list < 2;
    int ptr[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) ptr[q] = 0;
    CandRec* out = cand + (int64_t(list) * NB + blockIdx.x) * Tc;
    for (int k = 0; k < Tc; ++k) {
      int bq = 0;
      VI best{lv[list][0][ptr[0]], li[list][0][ptr[0]]};
#pragma unroll
      for (int q = 1; q < NW; ++q) {
        const VI c{lv[list][q][ptr[q]], li[list][q][ptr[q]]};
        const bool take = mn ? beats<true>(c, best) : beats<false>(c, best);
        if (take) {
          best = c;
          bq = q;
        }
      }
      ++ptr[bq];  // a wave's list holds Tc entries: no list runs out before Tc picks
      const bool ok = best.i != kSentinel && (mn ? best.v < inf : best.v > -inf);
      out[k] = CandRec{ok ? best.v : 0.0, ok ? int32_t(best.i) : -1, 0};
    }
  }
}

// ---- build ----------------------------------------------------------------------------------------------
// One workgroup over the L = 4 NB Tc candidates (list-major, then block, then pick): per class the extremes
// over its two lists (every block's first pick is its own extreme), the stop test on the larger class gap, and
// W = the ids sorted without duplicates, with their f.  No sort, as ws_build_kernel: blocks are disjoint
// ascending id ranges, so a candidate's place is its block's offset plus the distinct ids of its own block's
// 4 Tc picks below it.
__global__ __launch_bounds__(kMaxWS) void ws_build_nu_kernel(const CandRec* __restrict__ cand, int NB, int Tc, double tau,
                                                             double tau_frac, int64_t max_iter, int32_t* __restrict__ W,
                                                             double* __restrict__ Wf, DecompCtl* __restrict__ ctl,
                                                             int32_t* __restrict__ mcount, DecompCtl* __restrict__ pub) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  __shared__ int32_t s[kMaxWS];
  __shared__ int8_t kf[kMaxWS];
  __shared__ int32_t bcnt[kMaxWS / kNuLists];
  __shared__ int32_t wsum[kMaxWS / 64];
  __shared__ double red[kNuLists][kMaxWS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int Ll = NB * Tc, L = kNuLists * Ll;
  if (NB < 1 || Tc < 1 || L > kMaxWS) {  // the host refuses these shapes; never index past the lists
    if (t == 0) {
      ctl->stop = kStopInternal;
      *mcount = 0;
      publish_ctl(*ctl, pub);
    }
    return;
  }
  const double inf = __builtin_inf();
  const CandRec c = t < L ? cand[t] : CandRec{0.0, -1, 0};
  const int list = t < L ? t / Ll : 0, blk = t < L ? (t - list * Ll) / Tc : 0;
  const bool has = c.id >= 0;
  double v[kNuLists] = {has && list == 0 ? c.f : inf, has && list == 1 ? c.f : inf, has && list == 2 ? c.f : -inf,
                        has && list == 3 ? c.f : -inf};
  for (int off = 32; off > 0; off >>= 1) {
    v[0] = fmin(v[0], __shfl_xor(v[0], off, 64));
    v[1] = fmin(v[1], __shfl_xor(v[1], off, 64));
    v[2] = fmax(v[2], __shfl_xor(v[2], off, 64));
    v[3] = fmax(v[3], __shfl_xor(v[3], off, 64));
  }
  if (lane == 0)
    for (int q = 0; q < kNuLists; ++q) red[q][w] = v[q];
  s[t] = c.id;
  if (t < kMaxWS / kNuLists) bcnt[t] = 0;
  __syncthreads();
  // the block's first occurrence of an id (in candidate order) is the one kept
  bool keep = c.id >= 0;
  if (keep)
    for (int q = 0; q < kNuLists; ++q)
      for (int j = q * Ll + blk * Tc, je = j + Tc; j < je; ++j)
        if (j < t && s[j] == c.id) keep = false;
  kf[t] = keep;
  if (keep) atomicAdd(&bcnt[blk], 1);
  __syncthreads();
  // exclusive scan of the blocks' distinct counts (NB <= 256 blocks)
  const int bv = t < NB ? bcnt[t] : 0;
  const int incl = wave_incl_scan(bv);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int wpre = 0;
  for (int q = 0; q < w; ++q) wpre += wsum[q];
  if (t < NB) bcnt[t] = wpre + incl - bv;
  __syncthreads();
  if (keep) {
    int j = bcnt[blk];
    for (int q = 0; q < kNuLists; ++q)
      for (int i = q * Ll + blk * Tc, ie = i + Tc; i < ie; ++i) j += (kf[i] != 0 && s[i] < c.id) ? 1 : 0;
    if (j < kMaxWS) {
      W[j] = c.id;
      Wf[j] = c.f;  // duplicates of an id carry the same f
    }
  }
  if (t == 0) {
    int m = 0;
    double b[kNuLists] = {inf, inf, -inf, -inf};
    for (int q = 0; q < kMaxWS / 64; ++q) {
      m += wsum[q];
      b[0] = fmin(b[0], red[0][q]);
      b[1] = fmin(b[1], red[1][q]);
      b[2] = fmax(b[2], red[2][q]);
      b[3] = fmax(b[3], red[3][q]);
    }
    ctl->b_high = b[0];
    ctl->b_high_n = b[1];
    ctl->b_low = b[2];
    ctl->b_low_n = b[3];
    // a class with an empty side contributes no gap
    const double gp = b[0] < inf && b[2] > -inf ? b[2] - b[0] : -inf;
    const double gn = b[1] < inf && b[3] > -inf ? b[3] - b[1] : -inf;
    const double gap = gp > gn ? gp : gn;
    int32_t st = SVM_STOP_RUNNING;
    if (ctl->outer > 0 && ctl->last_inner_it == 0)  // no progress on the last W
      st = ctl->last_inner_reason == SVM_STOP_CONVERGED ? SVM_STOP_NO_CANDIDATE : ctl->last_inner_reason;
    else if (gap <= 2.0 * tau)
      st = SVM_STOP_CONVERGED;
    else if (ctl->inner_total + 1 > max_iter)
      st = SVM_STOP_MAX_ITER;
    else if (m < 2 || m > kMaxWS)
      st = kStopInternal;
    if (st != SVM_STOP_RUNNING) {
      ctl->stop = st;
      *mcount = 0;  // the rest of the batch's f updates are no-ops
      publish_ctl(*ctl, pub);
    } else {
      ctl->m = m;
      ctl->tau_in = fmax(tau, tau_frac * gap);
      ctl->max_inner = min(int64_t(20) * m, max_iter - ctl->inner_total);
    }
  }
}

// ---- inner solve ----------------------------------------------------------------------------------------
// Thread t holds 4 points of W in ws_inner_kernel<256, 4>'s layout (pair h of every lane is one 16-byte piece of
// a K(W, W) row).  Sides: 0 = I_high +, 1 = I_high -, 2 = I_low +, 3 = I_low -.  A class without a violating
// pair does not stop the solve while the other has one: a side without a candidate holds the sentinel (value
// +-inf), its class then has no gap, and no point of it passes the gain's f_t > b_high_c test.
constexpr int kNuNT = 256, kNuPER = 4;

__global__ __launch_bounds__(kNuNT) void ws_inner_nu_kernel(const double* __restrict__ Kw, int64_t ldw,
                                                            const int32_t* __restrict__ W, DecompCtl* __restrict__ ctl,
                                                            const int32_t* __restrict__ y, double* __restrict__ alpha,
                                                            const double* __restrict__ Wf, double C, double eps,
                                                            int32_t* __restrict__ cols, double* __restrict__ coef,
                                                            int32_t* __restrict__ mcount, DecompCtl* __restrict__ pub) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  constexpr int NT = kNuNT, PER = kNuPER, NW = NT / 64;
  const int m = min(ctl->m, kMaxWS);
  const double tau_in = ctl->tau_in;
  const int64_t max_inner = ctl->max_inner;
  __shared__ double pv[2][kNuLists][NW], pa[2][kNuLists][NW];
  __shared__ uint32_t pi[2][kNuLists][NW];
  __shared__ double qv[2][NW], qa[2][NW], qf[2][NW], qk[2][NW];  // the second index's candidates
  __shared__ uint32_t qi[2][NW];
  __shared__ int8_t sy[NT * PER];
  __shared__ int32_t wcnt[PER / 2][NW];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int pbase = w * 128 + 2 * lane;
  auto pos = [&](int e) { return pbase + (e >> 1) * (2 * NT) + (e & 1); };
  double a[PER], a0[PER], ft[PER];
  bool yp[PER], yn[PER];  // sign +1 / -1 (padding: neither, so in no set)
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
  int64_t it = 0;
  int32_t reason = SVM_STOP_CONVERGED;
  // this thread's entries of row r of K(W, W) as 16-byte loads (in bounds: NT PER <= ldw; ldw even), zero beyond m
  auto row = [&](int r, double* out) {
    const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(r) * ldw + pbase);
#pragma unroll
    for (int h = 0; h < PER / 2; ++h) {
      const double2 v = src[NT * h];
      out[2 * h] = pos(2 * h) < m ? v.x : 0.0;
      out[2 * h + 1] = pos(2 * h + 1) < m ? v.y : 0.0;
    }
  };
  for (int par = 0;; par ^= 1) {
    // 1. per-thread extremes per side, with the winner's alpha
    double sv[kNuLists] = {inf, inf, -inf, -inf}, sa[kNuLists] = {0.0, 0.0, 0.0, 0.0};
    uint32_t si[kNuLists] = {kSentinel, kSentinel, kSentinel, kSentinel};
#pragma unroll
    for (int e = 0; e < PER; ++e) {  // ascending position within a thread: strict compares keep the lowest
      const bool below = a[e] < c_hi, above = a[e] > c_lo;
      const bool c0 = yp[e] && below && ft[e] < sv[0], c1 = yn[e] && above && ft[e] < sv[1];
      const bool c2 = yp[e] && above && ft[e] > sv[2], c3 = yn[e] && below && ft[e] > sv[3];
      const bool cc[kNuLists] = {c0, c1, c2, c3};
      const uint32_t k = uint32_t(pos(e));
#pragma unroll
      for (int sd = 0; sd < kNuLists; ++sd) {
        sv[sd] = cc[sd] ? ft[e] : sv[sd];
        sa[sd] = cc[sd] ? a[e] : sa[sd];
        si[sd] = cc[sd] ? k : si[sd];
      }
    }
    // 2. the four wave reductions (two interleaved pairs); the winning lanes publish; ONE barrier
    int wl[kNuLists];
    wave_arg_pair_lanes(VI{sv[0], si[0]}, VI{sv[2], si[2]}, wl[0], wl[2]);
    wave_arg_pair_lanes(VI{sv[1], si[1]}, VI{sv[3], si[3]}, wl[1], wl[3]);
#pragma unroll
    for (int sd = 0; sd < kNuLists; ++sd)
      if (lane == wl[sd]) {
        pv[par][sd][w] = sv[sd];
        pi[par][sd][w] = si[sd];
        pa[par][sd][w] = sa[sd];
      }
    __syncthreads();
    // 3. the same pairwise tree fold in every lane (value, then lowest position), tracking the winning wave
    double fv[kNuLists][NW];
    uint32_t fi[kNuLists][NW];
    int fw[kNuLists][NW];
#pragma unroll
    for (int sd = 0; sd < kNuLists; ++sd)
#pragma unroll
      for (int q = 0; q < NW; ++q) {
        fv[sd][q] = pv[par][sd][q];
        fi[sd][q] = pi[par][sd][q];
        fw[sd][q] = q;
      }
#pragma unroll
    for (int st = 1; st < NW; st <<= 1)
#pragma unroll
      for (int q = 0; q + st < NW; q += 2 * st)
#pragma unroll
        for (int sd = 0; sd < kNuLists; ++sd) {
          const bool lt = sd < 2 ? fv[sd][q + st] < fv[sd][q] : fv[sd][q + st] > fv[sd][q];
          const bool tk = lt | ((fv[sd][q + st] == fv[sd][q]) & (fi[sd][q + st] < fi[sd][q]));
          fv[sd][q] = tk ? fv[sd][q + st] : fv[sd][q];
          fi[sd][q] = tk ? fi[sd][q + st] : fi[sd][q];
          fw[sd][q] = tk ? fw[sd][q + st] : fw[sd][q];
        }
    const double bhp = fv[0][0], bhn = fv[1][0], blp = fv[2][0], bln = fv[3][0];
    const uint32_t ihp = fi[0][0], ihn = fi[1][0];
    // 4. the stop test on the larger class gap; a class without both sides has none
    const bool has_p = (ihp != kSentinel) & (fi[2][0] != kSentinel), has_n = (ihn != kSentinel) & (fi[3][0] != kSentinel);
    if (!has_p && !has_n) {
      reason = SVM_STOP_NO_CANDIDATE;
      break;
    }
    const double gp = has_p ? blp - bhp : -inf, gn = has_n ? bln - bhn : -inf;
    const double gap = gp > gn ? gp : gn;
    if (gap <= 2.0 * tau_in) break;  // W's own optimum (reason stays CONVERGED)
    if (it >= max_inner) {
      reason = SVM_STOP_MAX_ITER;
      break;
    }
    // 5. both classes' rows i issued together (unconditional loads: a class without an i reads the other's row,
    // which no gain then uses)
    const int rp = ihp != kSentinel ? int(ihp) : int(ihn), rn = ihn != kSentinel ? int(ihn) : int(ihp);
    double kp[PER], kn[PER];
    row(rp, kp);
    row(rn, kn);
    // 6. every I_low point's gain on its own class's row: one gain per point, so one running minimum
    double gv = inf;
    int ge = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const bool below = a[e] < c_hi, above = a[e] > c_lo;
      const bool in_low = (yp[e] && above) || (yn[e] && below);
      const double bhe = yp[e] ? bhp : bhn, ke = yp[e] ? kp[e] : kn[e];
      const double bb = ft[e] - bhe;
      double at = 2.0 - 2.0 * ke;
      at = at < eps ? eps : at;
      // IEEE division (not v_rcp_f64): the choice is reproducible on the host bit for bit (the CPU oracle)
      const double gain = -(bb * bb) / at;
      const bool c = in_low && ft[e] > bhe && gain < gv;
      gv = c ? gain : gv;
      ge = c ? e : ge;
    }
    const uint32_t gi = gv < inf ? uint32_t(pos(ge)) : kSentinel;
    const int lc = wave_arg_lane<true>(VI{gv, gi});
    if (lane == lc) {
      double ga = a[0], gf = ft[0], gk = yp[0] ? kp[0] : kn[0];
#pragma unroll
      for (int e = 1; e < PER; ++e) {
        ga = ge == e ? a[e] : ga;
        gf = ge == e ? ft[e] : gf;
        gk = ge == e ? (yp[e] ? kp[e] : kn[e]) : gk;
      }
      qv[par][w] = gv;
      qi[par][w] = gi;
      qa[par][w] = ga;
      qf[par][w] = gf;
      qk[par][w] = gk;
    }
    // 7. the second barrier and the fold over both classes' gains
    __syncthreads();
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
    if (cj[0] == kSentinel) {  // no I_low point above its class's b_high (cannot happen while a gap is open)
      reason = SVM_STOP_NO_CANDIDATE;
      break;
    }
    // 8. row j, issued now and consumed after the clip / division below
    const int il = int(cj[0]);
    double2 rj[PER / 2];
    {
      const double2* src = reinterpret_cast<const double2*>(Kw + int64_t(il) * ldw + pbase);
#pragma unroll
      for (int h = 0; h < PER / 2; ++h) rj[h] = src[NT * h];
    }
    const double al = qa[par][cw[0]], bl_upd = qf[par][cw[0]], K12 = qk[par][cw[0]];
    const int32_t yl = sy[il];
    const bool cp = yl == 1;  // the pair's class: i is that class's i
    const int ih = cp ? int(ihp) : int(ihn);
    const double bh = cp ? bhp : bhn;
    const double ah = pa[par][cp ? 0 : 1][cp ? fw[0][0] : fw[1][0]];
    // 9. the classifier's clip / eta floor / update with both labels yl (s = +1)
    double eta = 1.0 + 1.0 - 2.0 * K12;
    const double U = fmax(0.0, al + ah - C), V = fmin(C, al + ah);
    if (!(U <= V + 1e-12)) {
      reason = SVM_STOP_INFEASIBLE;
      break;
    }
    eta = eta <= eps ? eps : eta;  // identical rows: LIBSVM's floor, the box clips the step
    double al_new = al + double(yl) * (bh - bl_upd) / eta;
    if (al_new > V) al_new = V;
    if (al_new < U) al_new = U;
    const double ah_new = ah + (al - al_new);
    const double ch = (ah_new - ah) * double(yl);
    const double cl = (al_new - al) * double(yl);
    double kl[PER];
#pragma unroll
    for (int h = 0; h < PER / 2; ++h) {
      double x = rj[h].x, z = rj[h].y;
      // an empty asm reading cl: the wait for row j's data lands here, after the division, not inside it
      asm volatile("" : "+v"(x), "+v"(z) : "v"(cl));
      kl[2 * h] = pos(2 * h) < m ? x : 0.0;
      kl[2 * h + 1] = pos(2 * h + 1) < m ? z : 0.0;
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
      const int k = pos(e);
      const double khe = cp ? kp[e] : kn[e];
      ft[e] += ch * khe + cl * kl[e];
      a[e] = k == ih ? ah_new : k == il ? al_new : a[e];
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

// ---- starts and finish ----------------------------------------------------------------------------------
// nu-SVC's start (one workgroup): a point's rank within its class by a running scan over chunks of 1024 x 8
// points; the class's first `full` points get 1, the next `frac`, the rest 0.
__global__ __launch_bounds__(1024) void ws_nu_start_svc_kernel(const int32_t* __restrict__ y, int64_t n, int64_t full,
                                                               double frac, int32_t* __restrict__ sgn,
                                                               double* __restrict__ alpha, double* __restrict__ f,
                                                               DecompCtl* __restrict__ ctl) {
  constexpr int E = 8, NW = 1024 / 64;
  __shared__ int32_t wtot[NW];
  __shared__ int64_t base_p;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) base_p = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += int64_t(1024) * E) {
    const int64_t i0 = c0 + int64_t(t) * E;
    int cnt = 0;  // this thread's +1 points
#pragma unroll
    for (int e = 0; e < E; ++e) cnt += (i0 + e < n && y[i0 + e] == 1) ? 1 : 0;
    const int incl = wave_incl_scan(cnt);
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int64_t rp = base_p + incl - cnt;  // +1 points before i0
    for (int q = 0; q < w; ++q) rp += wtot[q];
    int64_t rn = i0 - rp;  // -1 points before i0
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t i = i0 + e;
      if (i < n) {
        const bool p = y[i] == 1;
        const int64_t r = p ? rp : rn;
        alpha[i] = r < full ? 1.0 : (r == full ? frac : 0.0);
        f[i] = 0.0;
        sgn[i] = p ? 1 : -1;
        rp += p ? 1 : 0;
        rn += p ? 0 : 1;
      }
    }
    __syncthreads();
    if (t == 0) {
      int64_t tot = 0;
      for (int q = 0; q < NW; ++q) tot += wtot[q];
      base_p += tot;
    }
    __syncthreads();
  }
  if (t == 0) ctl->n_active = n;
}

// nu-SVR's start: a_k = a*_k, f_k = f_{k+nrow} = -z_k (the twin init with epsilon 0), signs +1 and -1.
__global__ void ws_nu_start_twin_kernel(const double* __restrict__ z, int64_t nrow, double C, int64_t full, double frac,
                                        int32_t* __restrict__ sgn, double* __restrict__ alpha, double* __restrict__ f,
                                        DecompCtl* __restrict__ ctl) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < nrow) {
    const double a = i < full ? C : (i == full ? frac : 0.0), fi = -z[i];
    alpha[i] = a;
    alpha[i + nrow] = a;
    f[i] = fi;
    f[i + nrow] = fi;
    sgn[i] = 1;
    sgn[i + nrow] = -1;
  }
  if (i == 0) ctl->n_active = 2 * nrow;
}

// A class's multiplier from its two bounds: the midpoint, or the side that exists.
__device__ __forceinline__ double nu_mid(double bh, double bl) {
  const double inf = __builtin_inf();
  return bh < inf && bl > -inf ? (bh + bl) / 2 : (bh < inf ? bh : bl);
}

__global__ __launch_bounds__(1024) void ws_nu_finish_kernel(const DecompCtl* __restrict__ ctl, double* __restrict__ alpha,
                                                            int64_t n, int rescale, double* __restrict__ out) {
  const double bp = nu_mid(ctl->b_high, ctl->b_low), bn = nu_mid(ctl->b_high_n, ctl->b_low_n);
  const double r = (bp - bn) / 2, rho = (bp + bn) / 2;
  if (rescale && r > 0.0)
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) alpha[i] = alpha[i] / r;
  if (threadIdx.x == 0) {
    out[0] = r;
    out[1] = rho;
  }
}

}  // namespace

void launch_ws_select_nu(hipStream_t s, const NuArgs& a) {
  hipLaunchKernelGGL(ws_select_nu_kernel, dim3(unsigned(a.NB)), dim3(kSelNT), 0, s, a.f, a.alpha, a.sgn, a.n, a.per,
                     a.Tc, a.C, a.eps, a.cand, a.ctl);
}

void launch_ws_build_nu(hipStream_t s, const NuArgs& a) {
  hipLaunchKernelGGL(ws_build_nu_kernel, dim3(1), dim3(kMaxWS), 0, s, a.cand, a.NB, a.Tc, a.tau, a.tau_frac,
                     a.max_iter, a.W, a.Wf, a.ctl, a.mcount, a.pub);
}

void launch_ws_inner_nu(hipStream_t s, const InnerArgs& a) {
  hipLaunchKernelGGL(ws_inner_nu_kernel, dim3(1), dim3(kNuNT), 0, s, a.Kw, a.ldw, a.W, a.ctl, a.y, a.alpha, a.Wf, a.C,
                     a.eps, a.cols, a.coef, a.mcount, a.pub);
}

void launch_ws_nu_start_svc(hipStream_t s, const NuArgs& a, double* f, const int32_t* y, int64_t full, double frac) {
  hipLaunchKernelGGL(ws_nu_start_svc_kernel, dim3(1), dim3(1024), 0, s, y, a.n, full, frac, a.sgn, a.alpha, f, a.ctl);
}

void launch_ws_nu_start_twin(hipStream_t s, const NuArgs& a, double* f, const double* z, int64_t full, double frac) {
  const int64_t nrow = a.n / 2;
  hipLaunchKernelGGL(ws_nu_start_twin_kernel, dim3(unsigned((nrow + 255) / 256)), dim3(256), 0, s, z, nrow, a.C, full,
                     frac, a.sgn, a.alpha, f, a.ctl);
}

void launch_ws_nu_finish(hipStream_t s, const NuArgs& a, int rescale, double* out) {
  hipLaunchKernelGGL(ws_nu_finish_kernel, dim3(1), dim3(1024), 0, s, a.ctl, a.alpha, a.n, rescale, out);
}

}  // namespace svm355
