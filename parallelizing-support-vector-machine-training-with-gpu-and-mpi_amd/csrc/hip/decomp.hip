// Working-set decomposition SMO (opt-in, SVC(solver="decomp")): the reference's first-order SMO
// semantics per pair, but on a WORKING SET of up to q points at a time -- the SMO-type decomposition
// of LIBSVM / ThunderSVM re-designed for MI355X.
//
// The reference (main3.cpp:162-294, gpu_svm_main3.cu:318-483) updates ONE pair per iteration over
// all n points, so a GPU iteration is bound by a grid-wide exchange (~3.4 us at 60k even
// persistent).  Here one outer iteration is:
//   1. ws_select_kernel   per block of the points, its T most violating of I_high (smallest f) and
//                         of I_low (largest f), lowest index on ties -- the union always holds the
//                         globally maximal violating pair, so every outer iteration makes progress;
//   2. ws_build_kernel    one workgroup: the stop test on the global extremes (b_low <= b_high + 2 tau,
//                         main3.cpp:213), then the sorted, de-duplicated working set W (m <= q);
//   3. K(W, W)            the working set's rows gathered, its m x m Gram on the exact-integer path
//                         (the same kernel values as the full Gram, igram.hip);
//   4. ws_inner_kernel    (decomp_inner.hip) ONE workgroup runs first-order SMO on W with the reference's update
//                         arithmetic (clip bounds, eta, stop reasons) -- an iteration is a workgroup
//                         reduction and two L2-resident row reads, no grid exchange -- until W's own
//                         gap is below max(tau, gap / 10);
//   5. f update           f += K(:, W) (delta alpha * y): the exact-integer kernel values of all n
//                         rows against W computed on int8 MFMA and reduced in the epilogue
//                         (igram_tri_kernel GEMV mode), never stored -- no n x n Gram at all.
// The stop test is the reference's, on all n points, so the model meets the same optimality bound
// (tests: the same support-vector set as the pairwise solve, b within the stop tolerance); the
// sequence of pair updates differs, so iteration counts and b differ in the last digits.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "decomp.h"
#include "decomp_dev.h"
#include "decomp_newton.h"
#include "decomp_shrink.h"
#include "persist.h"
#include "svm355_device.h"
#include "trace.h"

namespace svm355 {
namespace {

// ---- select ---------------------------------------------------------------------------------------------
// Per block b of `per` points of this GPU's slice (local rows [b per, (b + 1) per), global ids lo +
// local): the T most violating points of I_high (smallest f) and of I_low (largest f) in wave_arg's
// order (value, then lowest index): every wave's own T best by T wave arg-reductions (the winner
// masked out by its owner after each), then a 4-way merge of the sorted wave lists.  f is the slice's
// (local index); alpha and y are global.
// Shrinking (decomp_shrink.h): shr[i] = 1 excludes local row i; with a packed list (act: the rows in
// the active order, boff: selection block b's rows are act[boff[b] .. boff[b + 1])) the block walks its
// packed rows instead of [b per, (b + 1) per) -- the same points in the same ascending order, so the picks
// are those of the masked full block.
__global__ __launch_bounds__(kSelNT) void ws_select_kernel(const double* __restrict__ f,
                                                           const double* __restrict__ alpha,
                                                           const int32_t* __restrict__ y, int64_t lo, int64_t nloc,
                                                           int64_t per, int T, double C, double Cn, double eps,
                                                           CandRec* __restrict__ cand_h, CandRec* __restrict__ cand_l,
                                                           const DecompCtl* __restrict__ ctl,
                                                           const int32_t* __restrict__ act,
                                                           const int32_t* __restrict__ boff,
                                                           const uint8_t* __restrict__ shr) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  constexpr int NW = kSelNT / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t b0 = act ? int64_t(boff[blockIdx.x]) : int64_t(blockIdx.x) * per;
  const int64_t b1 = act ? int64_t(boff[blockIdx.x + 1]) : std::min<int64_t>(nloc, b0 + per);
  // class weights: C is the box of the y = +1 rows, Cn of the y = -1 rows (equal without weights)
  const double c_hi = C - eps, c_hin = Cn - eps, c_lo = 0.0 + eps, inf = __builtin_inf();
  double fh[kSelE], fl[kSelE];
  uint32_t gi[kSelE];  // global ids, ascending in e
#pragma unroll
  for (int e = 0; e < kSelE; ++e) {
    const int64_t k = b0 + t + int64_t(kSelNT) * e;
    fh[e] = inf;
    fl[e] = -inf;
    const int64_t i = k < b1 ? (act ? int64_t(act[k]) : k) : k;
    gi[e] = uint32_t(lo + i);
    if (k < b1 && !(shr && shr[i])) {
      const double a = alpha[lo + i], fi = f[i];
      const int32_t yi = y[lo + i];
      if ((yi == 1 && a < c_hi) || (yi == -1 && a > c_lo)) fh[e] = fi;
      if ((yi == 1 && a > c_lo) || (yi == -1 && a < c_hin)) fl[e] = fi;
    }
  }
  // Every wave takes its own T best of each side with wave reductions only (no barrier per pick), then
  // the block's T best are the first T of the merge of the four sorted wave lists: the same picks in
  // the same order as T rounds of a block arg-reduction (the keys (value, index) are distinct).
  constexpr int kTMax = 64;  // T <= q / (2 * 8 blocks)
  __shared__ double lv[2][NW][kTMax];
  __shared__ uint32_t li[2][NW][kTMax];
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

// ws_select_kernel's picks for blocks of any size, streamed from memory: past 2,097,152 rows the block
// count is capped at kMaxWS / 2 (the candidates must fit one working set, so T = 1) and a block holds
// more than the kSelNT x kSelE points the register-resident kernel takes (SVM355_DECOMP_WIDE_SELECT=1
// runs it at any n, for the equivalence tests).  Round k takes, per side, the best point strictly after
// round k - 1's block pick in (value, lowest index) order: the keys are distinct, so that is the next
// entry of the sorted list the T arg-reductions of ws_select_kernel (and the CPU oracle) produce.  One
// pass over the block per round; every thread merges the four wave winners itself.
__global__ __launch_bounds__(kSelNT) void ws_select_wide_kernel(const double* __restrict__ f,
                                                                const double* __restrict__ alpha,
                                                                const int32_t* __restrict__ y, int64_t lo,
                                                                int64_t nloc, int64_t per, int T, double C, double Cn,
                                                                double eps,
                                                                CandRec* __restrict__ cand_h,
                                                                CandRec* __restrict__ cand_l,
                                                                const DecompCtl* __restrict__ ctl,
                                                                const int32_t* __restrict__ act,
                                                                const int32_t* __restrict__ boff,
                                                                const uint8_t* __restrict__ shr) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  constexpr int NW = kSelNT / 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t b0 = act ? int64_t(boff[blockIdx.x]) : int64_t(blockIdx.x) * per;
  const int64_t b1 = act ? int64_t(boff[blockIdx.x + 1]) : std::min<int64_t>(nloc, b0 + per);
  const double c_hi = C - eps, c_hin = Cn - eps, c_lo = 0.0 + eps, inf = __builtin_inf();
  __shared__ double wv[2][NW];
  __shared__ uint32_t wi[2][NW];
  VI ph{-inf, 0}, pl{inf, 0};  // the previous round's block picks (round 0: nothing excluded)
  for (int k = 0; k < T; ++k) {
    VI mn{inf, kSentinel}, mx{-inf, kSentinel};
    for (int64_t kk = b0 + t; kk < b1; kk += kSelNT) {  // ascending index within a thread
      const int64_t i = act ? int64_t(act[kk]) : kk;
      if (shr && shr[i]) continue;
      const double a = alpha[lo + i], fi = f[i];
      const int32_t yi = y[lo + i];
      const uint32_t gi = uint32_t(lo + i);
      const bool up = (yi == 1 && a < c_hi) || (yi == -1 && a > c_lo);
      const bool dn = (yi == 1 && a > c_lo) || (yi == -1 && a < c_hin);
      const bool eh = k == 0 || fi > ph.v || (fi == ph.v && gi > ph.i);
      const bool el = k == 0 || fi < pl.v || (fi == pl.v && gi > pl.i);
      if (up && eh && fi < mn.v) mn = VI{fi, gi};
      if (dn && el && fi > mx.v) mx = VI{fi, gi};
    }
    VIL a, b;
    wave_arg_pair(mn, mx, a, b);
    if (lane == 0) {
      wv[0][w] = a.v;
      wi[0][w] = a.i;
      wv[1][w] = b.v;
      wi[1][w] = b.i;
    }
    __syncthreads();
    VI bh{wv[0][0], wi[0][0]}, bl{wv[1][0], wi[1][0]};
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      const VI ch{wv[0][q], wi[0][q]}, cl{wv[1][q], wi[1][q]};
      if (beats<true>(ch, bh)) bh = ch;
      if (beats<false>(cl, bl)) bl = cl;
    }
    __syncthreads();  // every thread has read the wave winners before the next round writes them
    if (t == 0) {
      const bool ok = bh.i != kSentinel && bh.v < inf;
      cand_h[int64_t(blockIdx.x) * T + k] = CandRec{ok ? bh.v : 0.0, ok ? int32_t(bh.i) : -1, 0};
    } else if (t == 64) {
      const bool ok = bl.i != kSentinel && bl.v > -inf;
      cand_l[int64_t(blockIdx.x) * T + k] = CandRec{ok ? bl.v : 0.0, ok ? int32_t(bl.i) : -1, 0};
    }
    ph = bh;
    pl = bl;
  }
}

// ---- build and gather -----------------------------------------------------------------------------------
// One workgroup over the L gathered candidates (Lr per GPU, GPU-major; the first Lh of each GPU's
// are I_high picks, T per selection block, the rest I_low): b_high = min f over the I_high
// candidates, b_low = max f over the I_low ones (the global extremes: every block's first pick is its
// own extreme), the stop test, and the working set = the candidates' ids sorted, without duplicates (a
// free SV may be in both lists), with their f (Wf).  No sort: selection blocks are disjoint id ranges
// in candidate order (GPU-major, block-major), so a candidate's place in W is its block's offset (a
// scan of the blocks' distinct counts) plus the number of distinct ids of its own block (2T picks)
// below it -- four barriers instead of a 55-stage bitonic network.
__global__ __launch_bounds__(kMaxWS) void ws_build_kernel(const CandRec* __restrict__ cand, int L, int Lr, int Lh, int T,
                                                          double tau, double tau_frac, int64_t max_iter,
                                                          int32_t* __restrict__ W, double* __restrict__ Wf,
                                                          DecompCtl* __restrict__ ctl, int32_t* __restrict__ mcount,
                                                          DecompCtl* __restrict__ pub) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  __shared__ int32_t s[kMaxWS];
  __shared__ int8_t kf[kMaxWS];
  __shared__ int32_t bcnt[kMaxWS / 2];
  __shared__ int32_t wsum[kMaxWS / 64];
  __shared__ double red[2][kMaxWS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const CandRec c = t < L ? cand[t] : CandRec{0.0, -1, 0};
  double vh = __builtin_inf(), vl = -__builtin_inf();
  if (c.id >= 0) {
    if (t % Lr < Lh)
      vh = c.f;
    else
      vl = c.f;
  }
  for (int off = 32; off > 0; off >>= 1) {
    vh = fmin(vh, __shfl_xor(vh, off, 64));
    vl = fmax(vl, __shfl_xor(vl, off, 64));
  }
  if (lane == 0) {
    red[0][w] = vh;
    red[1][w] = vl;
  }
  // this candidate's selection block: its T high picks start at hb, its T low picks at hb + Lh
  const int nb = L / (2 * T), nbr = Lh / T;
  int blk = 0, hb = 0;
  if (t < L) {
    const int r = t / Lr, o = t - r * Lr, lb = (o < Lh ? o : o - Lh) / T;
    blk = r * nbr + lb;
    hb = r * Lr + lb * T;
  }
  s[t] = c.id;
  if (t < kMaxWS / 2) bcnt[t] = 0;
  __syncthreads();
  // the block's first occurrence of an id is the one kept
  bool keep = c.id >= 0;
  if (keep)
    for (int half = 0; half < 2; ++half)
      for (int j = hb + half * Lh, je = j + T; j < je; ++j)
        if (j < t && s[j] == c.id) keep = false;
  kf[t] = keep;
  if (keep) atomicAdd(&bcnt[blk], 1);
  __syncthreads();
  // exclusive scan of the blocks' distinct counts (nb <= 512 blocks)
  const int bv = t < nb ? bcnt[t] : 0;
  const int incl = wave_incl_scan(bv);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int wpre = 0;
  for (int q = 0; q < w; ++q) wpre += wsum[q];
  if (t < nb) bcnt[t] = wpre + incl - bv;
  __syncthreads();
  if (keep) {
    int j = bcnt[blk];
    for (int half = 0; half < 2; ++half)
      for (int i = hb + half * Lh, ie = i + T; i < ie; ++i) j += (kf[i] != 0 && s[i] < c.id) ? 1 : 0;
    W[j] = c.id;
    Wf[j] = c.f;  // duplicates of an id carry the same f
  }
  if (t == 0) {
    int m = 0;
    double bh = __builtin_inf(), bl = -__builtin_inf();
    for (int q = 0; q < kMaxWS / 64; ++q) {
      m += wsum[q];
      bh = fmin(bh, red[0][q]);
      bl = fmax(bl, red[1][q]);
    }
    ctl->b_high = bh;
    ctl->b_low = bl;
    int32_t st = SVM_STOP_RUNNING;
    if (ctl->outer > 0 && ctl->last_inner_it == 0)  // no progress on the last W (a reference stop reason in it)
      st = ctl->last_inner_reason == SVM_STOP_CONVERGED ? SVM_STOP_NO_CANDIDATE : ctl->last_inner_reason;
    else if (!(bh < __builtin_inf()) || !(bl > -__builtin_inf()))  // "i_high or i_low not found" (main3.cpp:205-209)
      st = SVM_STOP_NO_CANDIDATE;
    else if (bl <= bh + 2.0 * tau)
      st = SVM_STOP_CONVERGED;
    else if (ctl->inner_total + 1 > max_iter)  // the reference counts num_iter from 1 (main3.cpp:283-287)
      st = SVM_STOP_MAX_ITER;
    else if (m < 2 || m > kMaxWS)
      st = kStopInternal;
    // the ACTIVE problem stopped while points are shrunk: not a stop -- the host unshrinks (f recomputed
    // from alpha, every point active) and the next build tests all n points (decomp_shrink.h)
    if (st != SVM_STOP_RUNNING && st != SVM_STOP_MAX_ITER && st != kStopInternal && ctl->shrunk) st = kStopUnshrink;
    if (st != SVM_STOP_RUNNING) {
      ctl->stop = st;
      *mcount = 0;  // the rest of the batch's f updates are no-ops
      publish_ctl(*ctl, pub);
    } else {
      ctl->m = m;
      ctl->tau_in = fmax(tau, tau_frac * (bl - bh));
      ctl->max_inner = min(int64_t(20) * m, max_iter - ctl->inner_total);
    }
  }
}

// Qw[k] = Q[W[k]] (kq bytes), N0w[k], WNw[k]: one workgroup per working-set row.
__global__ __launch_bounds__(64) void ws_gather_kernel(const int8_t* __restrict__ Q, const int32_t* __restrict__ N0,
                                                       const double* __restrict__ WN, int kq,
                                                       const int32_t* __restrict__ W, const DecompCtl* __restrict__ ctl,
                                                       int8_t* __restrict__ Qw, int32_t* __restrict__ N0w,
                                                       double* __restrict__ WNw) {
  const int k = blockIdx.x;
  if (ctl->stop != SVM_STOP_RUNNING || k >= ctl->m) return;
  const int64_t src = W[k];
  const int4* s = reinterpret_cast<const int4*>(Q + src * int64_t(kq));
  int4* d = reinterpret_cast<int4*>(Qw + int64_t(k) * kq);
  for (int c = threadIdx.x; c < kq / 16; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) {
    N0w[k] = N0[src];
    WNw[k] = WN[src];
  }
}

// FP64 rows (real-valued data): Xo[k] = X[ids[k]] (ld doubles) and no[k] = nrm[ids[k]] for k < *count,
// one workgroup per row; no-op when gated (a stopped solve's remaining launches).
__global__ __launch_bounds__(64) void ws_gather_f64_kernel(const double* __restrict__ X, const double* __restrict__ nrm,
                                                           int64_t ld, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ gate, double* __restrict__ Xo,
                                                           double* __restrict__ no) {
  const int k = blockIdx.x;
  if ((gate && *gate != 0) || k >= *count) return;
  const int64_t src = ids[k];
  const double2* s = reinterpret_cast<const double2*>(X + src * ld);
  double2* d = reinterpret_cast<double2*>(Xo + int64_t(k) * ld);
  for (int64_t c = threadIdx.x; c < ld / 2; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) no[k] = nrm[src];
}

// Twin mode (epsilon-SVR, DecompOpts): a point id in [0, 2 nrow) reads kernel row id mod nrow.  The two
// gathers above for a working set of such points (kernels of their own: the classifier's keep their arguments).
__device__ __forceinline__ int64_t twin_row(int32_t id, int64_t nrow) { return id >= nrow ? id - nrow : id; }

__global__ __launch_bounds__(64) void ws_gather_twin_kernel(const int8_t* __restrict__ Q,
                                                            const int32_t* __restrict__ N0,
                                                            const double* __restrict__ WN, int kq,
                                                            const int32_t* __restrict__ W,
                                                            const DecompCtl* __restrict__ ctl, int8_t* __restrict__ Qw,
                                                            int32_t* __restrict__ N0w, double* __restrict__ WNw,
                                                            int64_t nrow) {
  const int k = blockIdx.x;
  if (ctl->stop != SVM_STOP_RUNNING || k >= ctl->m) return;
  const int64_t src = twin_row(W[k], nrow);
  const int4* s = reinterpret_cast<const int4*>(Q + src * int64_t(kq));
  int4* d = reinterpret_cast<int4*>(Qw + int64_t(k) * kq);
  for (int c = threadIdx.x; c < kq / 16; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) {
    N0w[k] = N0[src];
    WNw[k] = WN[src];
  }
}

__global__ __launch_bounds__(64) void ws_gather_f64_twin_kernel(const double* __restrict__ X,
                                                                const double* __restrict__ nrm, int64_t ld,
                                                                const int32_t* __restrict__ ids,
                                                                const int32_t* __restrict__ count,
                                                                const int32_t* __restrict__ gate,
                                                                double* __restrict__ Xo, double* __restrict__ no,
                                                                int64_t nrow) {
  const int k = blockIdx.x;
  if ((gate && *gate != 0) || k >= *count) return;
  const int64_t src = twin_row(ids[k], nrow);
  const double2* s = reinterpret_cast<const double2*>(X + src * ld);
  double2* d = reinterpret_cast<double2*>(Xo + int64_t(k) * ld);
  for (int64_t c = threadIdx.x; c < ld / 2; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) no[k] = nrm[src];
}

// Twin mode: two twins in one working set (W is ascending, so k sits before k + nrow) are the same kernel
// row, and K(W, W) between their positions is the diagonal's 1 -- as the f update has it for that row -- not
// the off-diagonal arithmetic's value for a zero distance.  One workgroup after the K(W, W) build: every
// position holding a point k + nrow looks k up by bisection and sets both mirrored entries.
__global__ __launch_bounds__(kMaxWS) void ws_twin_kww_kernel(const int32_t* __restrict__ W,
                                                             const DecompCtl* __restrict__ ctl, int64_t nrow,
                                                             double* __restrict__ Kw, int64_t ldw) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  __shared__ int32_t s[kMaxWS];
  const int k = threadIdx.x, m = min(ctl->m, kMaxWS);
  const int32_t id = k < m ? W[k] : -1;
  s[k] = id;
  __syncthreads();
  if (id < nrow) return;  // a point of the first half (or none): its twin, if present, does the work
  const int32_t want = int32_t(id - nrow);
  int a = 0, b = m;  // the first position whose id is >= want
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (s[mid] < want)
      a = mid + 1;
    else
      b = mid;
  }
  if (a < m && s[a] == want) {
    Kw[int64_t(k) * ldw + a] = 1.0;
    Kw[int64_t(a) * ldw + k] = 1.0;
  }
}

// ---- cache plan and sums --------------------------------------------------------------------------------
// FP64 rows: f[i] += sum_{k < *count} coef[k] Kc[i][k] (the block K(rows, moved columns)), one wave
// per row, lane-strided then a fixed butterfly (deterministic).
// TWIN (twin mode; also ws_cache_fsum_kernel and ws_fsum_count_kernel below): a row's sum is computed once,
// exactly as otherwise, and added to both of the row's points, f[row] and f[row + nloc] (nloc = the kernel
// rows, all on this GPU; no packed rows in twin mode).
template <bool TWIN>
__global__ __launch_bounds__(256) void ws_rowsum_f64_kernel(const double* __restrict__ Kc, int64_t ldc,
                                                            const double* __restrict__ coef,
                                                            const int32_t* __restrict__ count, double* __restrict__ f,
                                                            int64_t nloc) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int cnt = *count;
  if (row >= nloc || cnt <= 0) return;
  const double* kr = Kc + row * ldc;
  double acc = 0.0;
  for (int k = lane; k < cnt; k += 64) acc += coef[k] * kr[k];
  acc = wave_sum(acc);
  if (lane == 0) f[row] += acc;
  if (TWIN && lane == 0) f[row + nloc] += acc;
}

// Column cache bookkeeping of one f update (one 1024-thread workgroup): the moved columns cols[0..*count)
// the cache lacks get slots -- free persistent ones in moved order while the cache has room (slot_of
// keeps them for the rest of the fit), then, with `meta`, slots evicted by a CLOCK sweep, then scratch
// slots cap + position -- and are listed for the column store (miss_ids / miss_slots, state[1] of them);
// rd_slot[k] = every moved column's slot.  state[0] = the next free persistent slot; state[2] = 1 when
// the narrow column store takes the misses (at most 64: the tiled store's gate); state[3] = the clock
// hand, state[4] = the update's stamp.  meta (nullptr: fill-only) = owner[cap] (point id, -1 none),
// last[cap] (stamp of the last update that used the slot), ref[cap] (the CLOCK bit, set on every use):
// past ~2M rows the distinct moved columns outnumber the slots a quarter of the HBM holds, and the
// columns the solve moves late are not the ones it moved first.  A victim is a slot this update does not
// read whose bit the hand finds clear (the hand clears the bits it passes); a cached column is the
// recomputed one bit for bit, so the policy never changes a result.
__device__ __forceinline__ int block_excl_scan_1024(bool v, int32_t* wsum, int& total) {
  const int k = threadIdx.x, lane = k & 63, w = k >> 6;
  const unsigned long long bal = __ballot(v);
  if (lane == 0) wsum[w] = __popcll(bal);
  __syncthreads();
  int r = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
  for (int q = 0; q < 16; ++q) {
    if (q < w) r += wsum[q];
    tot += wsum[q];
  }
  __syncthreads();  // wsum is reused by the next scan
  total = tot;
  return r;
}

__global__ __launch_bounds__(1024) void ws_cache_plan_kernel(const int32_t* __restrict__ cols,
                                                             const int32_t* __restrict__ count,
                                                             int32_t* __restrict__ slot_of, int32_t cap,
                                                             int32_t* __restrict__ state, int32_t* __restrict__ rd_slot,
                                                             int32_t* __restrict__ miss_ids,
                                                             int32_t* __restrict__ miss_slots,
                                                             int32_t* __restrict__ meta,
                                                             const int32_t* __restrict__ cdiag,
                                                             int32_t* __restrict__ miss_diag) {
  __shared__ int32_t wsum[16];
  __shared__ int32_t vict[kMaxWS];
  __shared__ int32_t s_nv, s_hand, s_stop;
  const int k = threadIdx.x;
  const int cnt = *count;
  const bool valid = k < cnt;
  const int32_t id = valid ? cols[k] : -1;
  int32_t sl = valid ? slot_of[id] : 0;
  const bool miss = valid && sl < 0;
  int32_t* owner = meta;
  int32_t* last = meta ? meta + cap : nullptr;
  int32_t* ref = meta ? meta + 2 * int64_t(cap) : nullptr;
  const int32_t E = state[4] + 1;
  if (meta && valid && !miss) {  // hits: read by this update (never a victim now) and referenced
    last[sl] = E;
    ref[sl] = 1;
  }
  int tot = 0;
  const int r = block_excl_scan_1024(miss, wsum, tot);  // its barriers publish the hits' stamps
  const int32_t next = state[0];
  const int fresh = max(0, min(tot, cap - next));
  const int need = meta ? tot - fresh : 0;
  if (k == 0) {
    s_nv = 0;
    s_hand = state[3];
  }
  __syncthreads();
  if (need > 0) {
    const int win = min(cap, kMaxWS);
    const int max_sweeps = 2 * ((cap + win - 1) / win) + 1;  // one full turn clears every unpinned bit
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
      const int have = s_nv, hand = s_hand;
      if (have >= need) break;  // uniform: read after a barrier
      const int32_t sx = int32_t((int64_t(hand) + k) % cap);
      // slots from `next` on are this update's fresh fills (the cache fills up in this very update)
      const bool cand = k < win && sx < next && last[sx] != E && ref[sx] == 0;
      int vtot = 0;
      const int vr = block_excl_scan_1024(cand, wsum, vtot);
      const bool take = cand && have + vr < need;
      if (take) {
        vict[have + vr] = sx;
        last[sx] = E;  // taken: not a candidate again when a small cache's next window wraps onto it
      }
      if (take && have + vr == need - 1) s_stop = k;  // the hand stops after the last victim it needs
      __syncthreads();
      const bool done = have + vtot >= need;
      const int passed = done ? s_stop + 1 : win;
      if (k < passed && !take && last[sx] != E) ref[sx] = 0;  // second chance used up
      __syncthreads();
      if (k == 0) {
        s_nv = min(need, have + vtot);
        s_hand = int32_t((int64_t(hand) + passed) % cap);
      }
      __syncthreads();
    }
  }
  const int nv = s_nv;
  if (miss) {
    if (r < fresh) {
      sl = next + r;
    } else if (r - fresh < nv) {
      sl = vict[r - fresh];
      const int32_t old = owner[sl];
      if (old >= 0) slot_of[old] = -1;  // not a column of this update: its slot would be pinned
    } else {
      sl = cap + k;  // no slot free or evictable: a scratch slot for this update only
    }
    if (sl < cap) {
      slot_of[id] = sl;
      if (meta) {
        owner[sl] = id;
        last[sl] = E;
        ref[sl] = 1;
      }
    }
    miss_ids[r] = id;
    miss_slots[r] = sl;
    if (cdiag) miss_diag[r] = cdiag[k];  // packed rows: the column's packed position (the unit diagonal)
  }
  if (valid) rd_slot[k] = sl;
  __syncthreads();  // every thread has read state[0] / state[3] / state[4]
  if (k == 0) {
    state[0] = next + fresh;
    state[1] = tot;
    state[2] = tot <= 64 ? 1 : 0;
    state[3] = s_hand;
    state[4] = E;
  }
}

// f[i] += sum_k coef[k] K(i, cols[k]) from the column cache, in the GEMV + half-sum order, bit for bit
// (igram GEMV epilogue + ws_fsum_count_kernel): per 64-column half, lane l's two terms (columns l and
// 32 + l) summed from 0, the 32-lane xor butterfly (16, 8, 4, 2, 1) as seen by lane 0 -- a binary tree
// whose leaves in evaluation order are the 5-bit bit-reversed lanes, so a 6-deep stack of completed
// subtrees replaces the 32 lane values --, the halves added in index order, then one add into f.
// A thread per RPT rows (16-byte loads: ldc is a multiple of 4); the 32 leaves of a half run as 4
// rolled groups of 8 (8 column pairs of loads in flight per group; unrolled, the compiler hoisted all
// 64 and ran at 3 waves / SIMD: 4.3 against 5.9 TB/s), the level of a group's last leaf depending on g.
// Packed rows (a shrunk solve): row i of the cache is f[act[i]], i < *nrows.
template <int RPT, bool TWIN>
__global__ __launch_bounds__(256) void ws_cache_fsum_kernel(const double* __restrict__ cache, int64_t ldc,
                                                             const int32_t* __restrict__ rd_slot,
                                                             const double* __restrict__ coef,
                                                             const int32_t* __restrict__ count, double* __restrict__ f,
                                                             int64_t nloc, const int32_t* __restrict__ act = nullptr,
                                                             const int32_t* __restrict__ nrows = nullptr) {
  const int64_t i = RPT * (int64_t(blockIdx.x) * blockDim.x + threadIdx.x);
  const int cnt = *count;
  if (nrows) nloc = std::min<int64_t>(nloc, *nrows);
  if (i >= nloc || cnt <= 0) return;
  const int halves = (cnt + 63) / 64;
  const double* base = cache + i;
  double s[RPT];
#pragma unroll
  for (int r = 0; r < RPT; ++r) s[r] = 0.0;
  for (int c = 0; c < halves; ++c) {
    double st[6][RPT];
#pragma unroll 1
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = 8 * g + jj;
        const int l = ((j & 1) << 4) | ((j & 2) << 2) | (j & 4) | ((j & 8) >> 2) | ((j & 16) >> 4);
        const int k0 = c * 64 + l, k1 = k0 + 32;
        double x[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) x[r] = 0.0;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int k = kk ? k1 : k0;
          if (k < cnt) {
            const double cf = coef[k];
            const f64x2* src = reinterpret_cast<const f64x2*>(base + int64_t(rd_slot[k]) * ldc);
#pragma unroll
            for (int r2 = 0; r2 < RPT / 2; ++r2) {
              const f64x2 v = src[r2];
              x[2 * r2] += cf * v[0];
              x[2 * r2 + 1] += cf * v[1];
            }
          }
        }
        int lev = 0;
#pragma unroll
        for (int t = jj; t & 1; t >>= 1, ++lev)
#pragma unroll
          for (int r = 0; r < RPT; ++r) x[r] = st[lev][r] + x[r];
        if (jj == 7) {  // lev == 3: continue up through the trailing ones of g
          if (g & 1) {
#pragma unroll
            for (int r = 0; r < RPT; ++r) x[r] = st[3][r] + x[r];
            if (g & 2) {
#pragma unroll
              for (int r = 0; r < RPT; ++r) x[r] = st[4][r] + x[r];
#pragma unroll
              for (int r = 0; r < RPT; ++r) st[5][r] = x[r];
            } else {
#pragma unroll
              for (int r = 0; r < RPT; ++r) st[4][r] = x[r];
            }
          } else {
#pragma unroll
            for (int r = 0; r < RPT; ++r) st[3][r] = x[r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < RPT; ++r) st[lev][r] = x[r];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) s[r] += st[5][r];
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r)
    if (i + r < nloc) f[act ? int64_t(act[i + r]) : i + r] += s[r];
  if (TWIN) {
#pragma unroll
    for (int r = 0; r < RPT; ++r)
      if (i + r < nloc) f[nloc + i + r] += s[r];
  }
}

// f[i] += the first ceil(*mcount / 64) column halves of part (the ones the GEMV wrote).  Packed rows
// (a shrunk solve): part row i is f[act[i]], i < *nrows.
template <bool TWIN>
__global__ __launch_bounds__(256) void ws_fsum_count_kernel(const double* __restrict__ part, int64_t ldp,
                                                            const int32_t* __restrict__ mcount,
                                                            double* __restrict__ f, int64_t n,
                                                            const int32_t* __restrict__ act = nullptr,
                                                            const int32_t* __restrict__ nrows = nullptr) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int npart = (*mcount + 63) / 64;
  if (nrows) n = std::min<int64_t>(n, *nrows);
  if (i >= n || npart == 0) return;
  const double* p = part + i * ldp;
  double s = 0.0;
  for (int c = 0; c < npart; ++c) s += p[c];
  f[act ? int64_t(act[i]) : i] += s;
  if (TWIN) f[n + i] += s;
}

// Twin mode's moved-column fold, between the inner solve and the f update (one workgroup): the moved list
// (cols: virtual ids k / k + nrow, coef: the change of alpha times the sign, *mcount <= kMaxWS of them) becomes
// one entry per kernel row -- fcols: the row, at the position order of the rows' first occurrences; fcoef:
// the point's coefficient, or coef_k + coef_{k+nrow} when both twins moved; *fcount: the rows.  The column
// cache and the column store key on the column id and must never see one twice, so the merge is not optional.
__global__ __launch_bounds__(kMaxWS) void ws_twin_fold_kernel(const int32_t* __restrict__ cols,
                                                              const double* __restrict__ coef,
                                                              const int32_t* __restrict__ mcount, int64_t nrow,
                                                              int32_t* __restrict__ fcols, double* __restrict__ fcoef,
                                                              int32_t* __restrict__ fcount) {
  __shared__ int32_t s[kMaxWS];
  __shared__ int32_t wsum[16];
  const int k = threadIdx.x, cnt = max(0, min(*mcount, kMaxWS));
  const int32_t id = k < cnt ? cols[k] : -1;
  s[k] = id;
  __syncthreads();
  const int32_t twin = id < 0 ? -2 : (id < nrow ? int32_t(id + nrow) : int32_t(id - nrow));
  int at = -1;  // the twin's position in the list (a point is listed once)
  for (int q = 0; q < cnt; ++q)
    if (s[q] == twin) at = q;
  const bool keep = id >= 0 && (at < 0 || at > k);
  int tot = 0;
  const int r = block_excl_scan_1024(keep, wsum, tot);
  if (keep) {
    double c = coef[k];
    if (at >= 0) c = id < nrow ? c + coef[at] : coef[at] + c;
    fcols[r] = int32_t(twin_row(id, nrow));
    fcoef[r] = c;
  }
  if (k == 0) *fcount = tot;
}

// ---- init and warm start --------------------------------------------------------------------------------
// pos_of = the identity (the packed list before any repack, or after an unshrink).
__global__ void ws_iota_kernel(int32_t* __restrict__ v, int64_t n) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) v[i] = int32_t(i);
}

__global__ void ws_init_kernel(const int32_t* __restrict__ y, double* __restrict__ alpha, double* __restrict__ f,
                               int64_t lo, int64_t nloc, int64_t n, int warm, DecompCtl* __restrict__ ctl) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n && !warm) alpha[i] = 0.0;
  if (i < nloc) f[i] = -static_cast<double>(y[lo + i]);  // main3.cpp:165-172
  if (i == 0 && ctl) ctl->n_active = nloc;
}

// Twin mode's (cold) start over the nrow targets z: f_k = eps - z_k, f_{k+nrow} = -eps - z_k, alpha = 0, and the
// 2 nrow points' signs (the solve's y): +1 for a_k, -1 for its twin a*_k.
__global__ void ws_twin_init_kernel(const double* __restrict__ z, double eps, int64_t nrow, int32_t* __restrict__ sgn,
                                    double* __restrict__ alpha, double* __restrict__ f, DecompCtl* __restrict__ ctl) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < nrow) {
    const double zi = z[i];
    f[i] = eps - zi;
    f[i + nrow] = -eps - zi;
    alpha[i] = 0.0;
    alpha[i + nrow] = 0.0;
    sgn[i] = 1;
    sgn[i + nrow] = -1;
  }
  if (i == 0) ctl->n_active = 2 * nrow;
}

// One-class mode's start over the n points: LIBSVM's feasible alpha (full ones, then frac at point `full`, zeros
// beyond; svm_oneclass_start), f = 0 (no linear term: nz_update adds K[:, nz] alpha_nz), and the signs (the
// solve's y), all +1.
__global__ void ws_oneclass_init_kernel(int64_t full, double frac, int64_t n, int32_t* __restrict__ sgn,
                                        double* __restrict__ alpha, double* __restrict__ f,
                                        DecompCtl* __restrict__ ctl) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) {
    alpha[i] = i < full ? 1.0 : (i == full ? frac : 0.0);
    f[i] = 0.0;
    sgn[i] = 1;
  }
  if (i == 0) ctl->n_active = n;
}

// Held-out mode's start over the n points: the solve's own signs -- 0 for a held-out point, which no selection
// takes (ws_select_kernel, ws_select_wide_kernel and ws_inner_kernel test y == 1 / y == -1), so its alpha stays 0
// -- alpha = 0 and f = -sgn.
__global__ void ws_heldout_init_kernel(const int32_t* __restrict__ y, const uint8_t* __restrict__ mask, int64_t n,
                                       int32_t* __restrict__ sgn, double* __restrict__ alpha,
                                       double* __restrict__ f, DecompCtl* __restrict__ ctl) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) {
    const int32_t sg = mask[i] ? 0 : y[i];
    sgn[i] = sg;
    alpha[i] = 0.0;
    f[i] = -static_cast<double>(sg);
  }
  if (i == 0) ctl->n_active = n;
}

// Held-out mode's result after the last outer iteration: a held-out point's f has received every f update from
// -0, so it is sum_j alpha_j y_j K_ij, and f - b (b as finish_solve computes it from the same two bounds, so the
// same bits) is its decision value under a model that never saw it.  0.0 for the training part.
__global__ void ws_heldout_dec_kernel(const double* __restrict__ f, const uint8_t* __restrict__ mask, int64_t n,
                                      const DecompCtl* __restrict__ ctl, double* __restrict__ dec) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) dec[i] = mask[i] ? f[i] - (ctl->b_high + ctl->b_low) / 2 : 0.0;
}

// Warm start: the ascending ids j with alpha_j != 0 into cols, alpha_j y_j into coef, their number to
// *count (device) and *count_h (pinned host).  One 1024-thread workgroup; each thread takes 8
// consecutive points of a 8192-point chunk, a workgroup exclusive scan of the per-thread counts
// places them (ascending order preserved).
__global__ __launch_bounds__(1024) void ws_nz_compact_kernel(const double* __restrict__ alpha,
                                                             const int32_t* __restrict__ y, int64_t n,
                                                             int32_t* __restrict__ cols, double* __restrict__ coef,
                                                             int32_t* __restrict__ count, int64_t* __restrict__ count_h) {
  constexpr int E = 8, NW = 1024 / 64;
  __shared__ int32_t wtot[NW];
  __shared__ int64_t base;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t == 0) base = 0;
  __syncthreads();
  for (int64_t c0 = 0; c0 < n; c0 += int64_t(1024) * E) {
    const int64_t i0 = c0 + int64_t(t) * E;
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) cnt += (i0 + e < n && alpha[i0 + e] != 0.0) ? 1 : 0;
    int incl = cnt;  // inclusive wave scan
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    int64_t pos = base + incl - cnt;
    for (int q = 0; q < w; ++q) pos += wtot[q];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int64_t i = i0 + e;
      if (i < n && alpha[i] != 0.0) {
        cols[pos] = int32_t(i);
        coef[pos] = alpha[i] * double(y[i]);
        ++pos;
      }
    }
    __syncthreads();
    if (t == 0) {
      int64_t tot = 0;
      for (int q = 0; q < NW; ++q) tot += wtot[q];
      base += tot;
    }
    __syncthreads();
  }
  if (t == 0) {
    *count = int32_t(base);
    *count_h = base;
  }
}

// counts[c] = the columns of warm-start chunk c (kMaxWS per chunk; the last one partial).
__global__ void ws_chunk_counts_kernel(const int32_t* __restrict__ count, int32_t* __restrict__ counts, int nchunks) {
  const int c = int(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c < nchunks) counts[c] = max(0, min(kMaxWS, *count - c * kMaxWS));
}

// ---- shrinking (decomp_shrink.h) ----------------------------------------------------------------------
// The shrink pass after an outer iteration: every active row of this GPU (the packed list act[0 ..
// *nrows), or all nloc rows) that the rule drops gets shr = 1; ctl->n_active counts what is left and
// ctl->shrunk records that a pass ran (the build then unshrinks instead of stopping).  The bounds are the
// outer iteration's build's.
__global__ __launch_bounds__(256) void ws_shrink_pass_kernel(const double* __restrict__ f,
                                                             const double* __restrict__ alpha,
                                                             const int32_t* __restrict__ y, int64_t lo, int64_t nloc,
                                                             const int32_t* __restrict__ act,
                                                             const int32_t* __restrict__ nrows,
                                                             uint8_t* __restrict__ shr, double C, double eps,
                                                             double margin, DecompCtl* __restrict__ ctl) {
  if (ctl->stop != SVM_STOP_RUNNING) return;
  __shared__ int32_t wdrop[4];
  const int64_t k = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t nr = act ? std::min<int64_t>(nloc, *nrows) : nloc;
  const double g = margin * (ctl->b_low - ctl->b_high);  // shrink_cuts
  const double hi_cut = ctl->b_low + g, lo_cut = ctl->b_high - g;
  const double c_hi = C - eps, c_lo = 0.0 + eps;
  bool drop = false;
  if (k < nr) {
    const int64_t i = act ? int64_t(act[k]) : k;
    if (!shr[i]) {
      const int32_t yi = y[lo + i];
      const double a = alpha[lo + i], fi = f[i];
      const bool up = (yi == 1 && a < c_hi) || (yi == -1 && a > c_lo);
      const bool dn = (yi == 1 && a > c_lo) || (yi == -1 && a < c_hi);
      drop = (up && !dn && fi > hi_cut) || (dn && !up && fi < lo_cut);  // shrinkable()
      if (drop) shr[i] = 1;
    }
  }
  const unsigned long long b = __ballot(drop);
  if ((threadIdx.x & 63) == 0) wdrop[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int d = wdrop[0] + wdrop[1] + wdrop[2] + wdrop[3];
    if (d) atomicAdd(reinterpret_cast<unsigned long long*>(&ctl->n_active), static_cast<unsigned long long>(-int64_t(d)));
    if (blockIdx.x == 0) {
      ctl->shrunk = 1;
      ctl->passes += 1;
    }
  }
}

// Repacking the active rows, 1 of 2 (one workgroup per selection block of this GPU): the block's rows
// still active -- its packed rows [boff[b], boff[b + 1]) of the current list act, or its full range
// [b per, (b + 1) per) before the first repack (act null) -- counted into bcnt[b].
__global__ __launch_bounds__(256) void ws_pack_count_kernel(const int32_t* __restrict__ act,
                                                            const int32_t* __restrict__ boff, int64_t per,
                                                            int64_t nloc, const uint8_t* __restrict__ shr,
                                                            int32_t* __restrict__ bcnt) {
  __shared__ int32_t wsum[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t b0 = act ? int64_t(boff[blockIdx.x]) : int64_t(blockIdx.x) * per;
  const int64_t b1 = act ? int64_t(boff[blockIdx.x + 1]) : std::min<int64_t>(nloc, b0 + per);
  int c = 0;
  for (int64_t k = b0 + t; k < b1; k += 256) c += shr[act ? int64_t(act[k]) : k] ? 0 : 1;
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0) wsum[w] = c;
  __syncthreads();
  if (t == 0) bcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Repacking, 2 of 2 (one workgroup per selection block): the block's new offset (the sum of the counts
// before it; the last block also writes the total to nboff[nb] and *nrows), then its active rows in
// order to the new list nact, pos_of[row] = the new position (-1 for the rows dropped), and the packed
// copies of their quantised rows (Qa, N0a, WNa: the GEMV / column store's row operand).  It reads the old
// list (act, boff) and writes the other buffer of the pair, so no block overwrites a list another reads.
__global__ __launch_bounds__(256) void ws_pack_write_kernel(const int32_t* __restrict__ act,
                                                            const int32_t* __restrict__ boff, int64_t per,
                                                            int64_t nloc, const uint8_t* __restrict__ shr,
                                                            const int32_t* __restrict__ bcnt,
                                                            int32_t* __restrict__ nboff, int32_t* __restrict__ nrows,
                                                            int32_t* __restrict__ nact, int32_t* __restrict__ pos_of,
                                                            const int8_t* __restrict__ Q, const int32_t* __restrict__ N0,
                                                            const double* __restrict__ WN, int64_t lo, int kq,
                                                            int8_t* __restrict__ Qa, int32_t* __restrict__ N0a,
                                                            double* __restrict__ WNa) {
  __shared__ int32_t wsum[4];
  __shared__ int32_t rows[256], dst[256];
  __shared__ int32_t s_n;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nb = int(gridDim.x), b = int(blockIdx.x);
  {  // this block's offset: the counts of the blocks before it (nb <= 512)
    int v = 0;
    for (int q = t; q < b; q += 256) v += bcnt[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) wsum[w] = v;
    __syncthreads();
    if (t == 0) {
      const int base = wsum[0] + wsum[1] + wsum[2] + wsum[3];
      nboff[b] = base;
      s_n = base;
      if (b == nb - 1) {
        nboff[nb] = base + bcnt[b];
        *nrows = base + bcnt[b];
      }
    }
    __syncthreads();
  }
  int base = s_n;
  const int64_t b0 = act ? int64_t(boff[b]) : int64_t(b) * per;
  const int64_t b1 = act ? int64_t(boff[b + 1]) : std::min<int64_t>(nloc, b0 + per);
  const int cpr = kq / 16;  // 16-byte chunks per quantised row
  for (int64_t c0 = b0; c0 < b1; c0 += 256) {
    const int64_t k = c0 + t;
    const int64_t i = k < b1 ? (act ? int64_t(act[k]) : k) : -1;
    const bool keep = i >= 0 && !shr[i];
    const unsigned long long bal = __ballot(keep);
    __syncthreads();  // the previous chunk is done with wsum / s_n / rows / dst
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int r = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
    for (int q = 0; q < 4; ++q) {
      if (q < w) r += wsum[q];
      tot += wsum[q];
    }
    if (keep) {
      nact[base + r] = int32_t(i);
      pos_of[i] = base + r;
      rows[r] = int32_t(i);
      dst[r] = base + r;
      N0a[base + r] = N0[lo + i];
      WNa[base + r] = WN[lo + i];
    } else if (i >= 0) {
      pos_of[i] = -1;
    }
    __syncthreads();  // rows / dst complete
    for (int64_t c = t; c < int64_t(tot) * cpr; c += 256) {  // the kept rows' bytes, 16 at a time
      const int rr = int(c / cpr), ch = int(c - int64_t(rr) * cpr);
      reinterpret_cast<int4*>(Qa + int64_t(dst[rr]) * kq)[ch] =
          reinterpret_cast<const int4*>(Q + (lo + int64_t(rows[rr])) * kq)[ch];
    }
    base += tot;
  }
}

// Unshrink, on the device side: every row active again (shr = 0; the host resets the packed list to the
// identity), the control block running with no shrink pass since (origin = now), and the no-progress test
// disarmed for the next working set (last_inner_it = -1: the last inner solve ran on the active problem).
__global__ void ws_unshrink_ctl_kernel(DecompCtl* __restrict__ ctl, int64_t nloc) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    ctl->stop = SVM_STOP_RUNNING;
    ctl->shrunk = 0;
    ctl->n_active = nloc;
    ctl->last_inner_it = -1;
    ctl->last_m = 0;
  }
}

}  // namespace

DecompShape decomp_shape(int64_t n, int qws, int world) {
  DecompShape d;
  d.q = std::max(4, std::min(qws, kMaxWS));
  // blocks of <= 4096 points, at least 64 blocks (each gives its own top-T picks), a multiple of 8 so
  // 1, 2, 4 or 8 GPUs own whole blocks and the distributed trajectory is the one-GPU one (another
  // world rounds to a multiple of it)
  const int64_t nb0 = std::max<int64_t>((n + kSelNT * kSelE - 1) / (kSelNT * kSelE), std::min<int64_t>(64, (n + 63) / 64));
  const int64_t mult = (8 % world == 0) ? 8 : int64_t(8) * world;
  d.NB = (nb0 + mult - 1) / mult * mult;
  // at most kMaxWS / 2 blocks (past 2,097,152 rows): their extreme pairs fill one working set, and the
  // blocks grow beyond kSelNT x kSelE points (ws_select_wide_kernel)
  d.NB = std::min<int64_t>(d.NB, int64_t(kMaxWS / 2) / mult * mult);
  d.per = d.NB > 0 ? (n + d.NB - 1) / d.NB : 0;
  // T picks per block and side; at least one, so the working-set capacity L = 2 NB T is the
  // requested q rounded down to the blocks, or 2 NB when q < 2 NB (every block contributes its extreme
  // pair: the union must hold the globally maximal violating pair).  stats[2] reports L.
  d.T = d.NB > 0 ? int(std::max<int64_t>(1, d.q / (2 * d.NB))) : 0;
  d.L = 2 * d.NB * d.T;
  d.ok = n >= 2 && n < int64_t(kSentinel) && d.NB >= 1 && d.L <= kMaxWS && world >= 1;
  return d;
}

// ---- the driver -----------------------------------------------------------------------------------------
namespace {

constexpr int64_t kLdw = kMaxWS;              // K(W, W) row stride
constexpr int64_t kLdp = 2 * (kMaxWS / 128);  // column halves of the f update

// Every environment switch a solve reads (docs/KNOBS.md), parsed at the top of each solve and never kept
// between solves: the tests change them between fits of one process.
struct DecompKnobs {
  bool wide_select = false, prof = false, kww_sym = false, shrink_log = false;  // _WIDE_SELECT, _PROF, _KWW, _SHRINK_LOG
  bool wss2 = true, dp = true, j2s = false;                                     // _WSS = 1 | 2 | 3 | 4
  bool pack = true, cache_evict = true;                                         // _PACK=0, _CCACHE_EVICT=0
  int inner_nt = 256, batch = 1;                                                // _NT, _BATCH
  double tau_frac = 0.1, repack_frac = 0.75;                                    // _TAU_FRAC, _REPACK
  int fail_rank = -1;                                                           // _FAIL_RANK (-1: none)
  int64_t fail_outer = 0;                                                       // _FAIL_OUTER
  int ccache = -1;                                                              // _CCACHE: 0 off, 1 on, -1 by size
  double ccache_frac = -1.0;                                                    // _CCACHE_FRAC (< 0: not set)
  bool ccache_slots_set = false;                                                // _CCACHE_SLOTS
  int64_t ccache_slots = 0;
  int local_world = 0;                                                          // LOCAL_WORLD_SIZE (0: not set)
};

int read_knobs(const DecompShape& sh, DecompKnobs* out) {
  DecompKnobs k;
  auto is1 = [](const char* name) {
    const char* v = getenv(name);
    return v && atoi(v) == 1;
  };
  k.wide_select = is1("SVM355_DECOMP_WIDE_SELECT");
  // inner workgroup: NT threads x PER points (NT * PER = 1024); SVM355_DECOMP_NT = 64 | 128 | 256 | 512
  if (const char* v = getenv("SVM355_DECOMP_NT")) k.inner_nt = atoi(v);
  if (k.inner_nt != 64 && k.inner_nt != 128 && k.inner_nt != 512 && k.inner_nt != 65) k.inner_nt = 256;
  // 65: one wave x 6 points (A/B probe of a one-wave inner solve; needs a working set of <= 384)
  if (k.inner_nt == 65 && sh.L > 384) {
    set_error("decomposition SMO: SVM355_DECOMP_NT=65 needs a working set of <= 384 points");
    return SVM_ERR_ARG;
  }
  // inner stop: the working set's own gap <= max(2 tau, 2 tau_frac gap) (SVM355_DECOMP_TAU_FRAC)
  if (const char* v = getenv("SVM355_DECOMP_TAU_FRAC")) k.tau_frac = atof(v);
  // at 0.5 and above the working set's stop (its gap <= tau_frac x 2 gap) holds before any update, so the
  // solve could make no progress (it would stop at once with a zero model)
  if (!(k.tau_frac >= 0.0 && k.tau_frac < 0.5)) {
    set_error("decomposition SMO: SVM355_DECOMP_TAU_FRAC must be in [0, 0.5), got %g", k.tau_frac);
    return SVM_ERR_ARG;
  }
  // SVM355_DECOMP_PROF=1: clock64 phase totals of the inner solves on stderr (diagnostic build)
  k.prof = is1("SVM355_DECOMP_PROF");
  // inner pair selection: second order for j (default; fewer, longer iterations: 8,206 vs 14,334 at
  // 60k, 12% faster) or first order (SVM355_DECOMP_WSS=1)
  k.wss2 = !is1("SVM355_DECOMP_WSS");
  // SVM355_DECOMP_WSS = 3 (the default): second order plus the second pair per iteration (DP); 2: one
  // pair (40k 17.0 -> 15.5 ms, 60k 20.8 -> 19.2, 120k 43.9 -> 42.7, 250k 84.9 -> 83.1, 1M 296 -> 289)
  const char* wss = getenv("SVM355_DECOMP_WSS");
  k.dp = k.wss2 && (wss ? atoi(wss) >= 3 : true);
  // SVM355_DECOMP_WSS = 4: the second pair's j by the second-order gain of row i2 (opt-in)
  k.j2s = k.dp && wss && atoi(wss) == 4;
  // with one batch always queued ahead, 1 already hides the host; more only adds no-op tail
  if (const char* v = getenv("SVM355_DECOMP_BATCH")) k.batch = std::max(1, atoi(v));
  const char* kww = getenv("SVM355_DECOMP_KWW");  // "sym": the triangular Gram launch (A/B)
  k.kww_sym = kww && std::strcmp(kww, "sym") == 0;
  const char* pk = getenv("SVM355_DECOMP_PACK");
  k.pack = !(pk && atoi(pk) == 0);
  // repack when the active rows are at most this share of the packed ones
  if (const char* v = getenv("SVM355_DECOMP_REPACK")) k.repack_frac = std::min(1.0, std::max(0.0, atof(v)));
  k.shrink_log = is1("SVM355_DECOMP_SHRINK_LOG");
  // fault injection (tests, world > 1): rank SVM355_DECOMP_FAIL_RANK fails when it is about to enqueue
  // outer iteration SVM355_DECOMP_FAIL_OUTER (default 0: before the first selection), while its peers
  // wait in their candidate all-gathers (decomp_cpu.cpp has the same hook)
  if (const char* fr = getenv("SVM355_DECOMP_FAIL_RANK")) {
    const char* fo = getenv("SVM355_DECOMP_FAIL_OUTER");
    k.fail_rank = atoi(fr);
    k.fail_outer = fo ? std::max(0, atoi(fo)) : 0;
  }
  if (const char* cc = getenv("SVM355_DECOMP_CCACHE")) k.ccache = atoi(cc) != 0 ? 1 : 0;
  // evict by CLOCK once the slots are taken (SVM355_DECOMP_CCACHE_EVICT=0: fill-only, the round-4 cache)
  const char* ev = getenv("SVM355_DECOMP_CCACHE_EVICT");
  k.cache_evict = !(ev && atoi(ev) == 0);
  if (const char* v = getenv("SVM355_DECOMP_CCACHE_FRAC")) k.ccache_frac = std::min(0.9, std::max(0.0, atof(v)));
  if (const char* v = getenv("SVM355_DECOMP_CCACHE_SLOTS")) {  // tests: a small cache (its scratch path)
    k.ccache_slots_set = true;
    k.ccache_slots = atoll(v);
  }
  if (const char* lw = getenv("LOCAL_WORLD_SIZE")) k.local_world = std::max(1, atoi(lw));
  *out = k;
  return SVM_OK;
}

// A solve's buffers in the context's workspace (nullptr: not part of this solve).
struct DecompWs {
  double* f = nullptr;                     // this GPU's rows
  CandRec *own = nullptr, *all = nullptr;  // this GPU's candidate records, every GPU's
  int32_t* W = nullptr;
  double *Wf = nullptr, *Kw = nullptr;  // the working set's f (the inner solve's, the Newton polish's), K(W, W)
  double* coef = nullptr;               // the moved columns: (alpha_new - alpha_old) y, ids, their number
  int32_t *cols = nullptr, *mcount = nullptr;
  DecompCtl* ctl = nullptr;
  // exact-integer rows: the working set's quantised rows and the GEMV's column-half partials;
  // FP64 rows: the working set's and the moved columns' rows (+ norms) and the block K(rows, columns)
  int8_t* Qw = nullptr;
  int32_t* N0w = nullptr;
  double *WNw = nullptr, *part = nullptr, *Xw = nullptr, *nw = nullptr, *Xc = nullptr, *nc = nullptr, *Kc = nullptr;
  // column cache state: slot per point (-1 = none), the update's slots, its misses, {next free, misses},
  // the CLOCK metadata (fill-only: none)
  int32_t *cslot = nullptr, *crd = nullptr, *cmid = nullptr, *cmsl = nullptr, *cst = nullptr, *cmeta = nullptr;
  int32_t* wid = nullptr;  // K(W, W) through the narrow column store: the ids 0 .. kMaxWS - 1, then the count kMaxWS
  // warm start (and the recomputation of f when a shrunk solve unshrinks): the nonzero alphas' ids and
  // alpha y (all n at most), the per-chunk column counts
  int32_t *wcols = nullptr, *wcnt = nullptr;
  double* wcoef = nullptr;
  uint8_t* shr = nullptr;  // shrinking (decomp_shrink.h): the per-row flags
  // the Newton polish (decomp_newton.h): W's alpha by position and the factorisation's scratch
  double *gAw = nullptr, *nAmat = nullptr;
  // packing (shrinking on exact-integer rows): the packed lists of active rows (two buffers), the selection
  // blocks' offsets into them (two), the blocks' counts, the rows' packed positions, the device-side packed
  // row count, the moved columns' (and misses') packed positions for the unit diagonal, and the packed
  // copies of the quantised rows
  int32_t *act[2] = {nullptr, nullptr}, *boff[2] = {nullptr, nullptr};
  int32_t *bcnt = nullptr, *pos_of = nullptr, *nrows = nullptr, *cdiag = nullptr, *mdiag = nullptr, *N0a = nullptr;
  int8_t* Qa = nullptr;
  double* WNa = nullptr;
  // twin mode (epsilon-SVR): the 2n points' signs (the solve's y) and the folded moved list (one entry per row)
  int32_t *sgn = nullptr, *fcols = nullptr, *fcount = nullptr;
  double* fcoef = nullptr;
};

// The f update's kernel columns K(this GPU's rows, j) kept in HBM (size_col_cache); slab null: no cache.
struct ColCache {
  double* slab = nullptr;
  int32_t cap = 0;  // persistent slots (kMaxWS scratch slots follow them)
  int64_t ld = 0;   // slot stride in doubles
};

// What every stage of a solve reads: the problem, this GPU's slice of it, the knobs, the buffers.
struct Solve {
  DeviceCtx* ctx = nullptr;
  hipStream_t s = nullptr;
  DecompRows R;
  bool f64 = false;
  int kq = 0;  // the quantised rows' bytes (exact-integer rows)
  const int32_t* y = nullptr;
  double* alpha = nullptr;
  svm_params p{};
  double Cp = 0.0, Cn = 0.0;  // the boxes of the y = +1 / y = -1 rows (svm_class_boxes)
  DecompShape sh;
  int world = 1, rank = 0;
  // all rows; this GPU's selection blocks, rows [lo, lo + nloc) and candidate records; warm-start chunks
  int64_t n = 0, NBr = 0, lo = 0, nloc = 0, Lr = 0, nchunks = 0;
  DecompKnobs k;
  bool wide_select = false, kww_narrow = false, pack_on = false;
  // the mode (decomp_mode.h).  With its own signs, y is the workspace's (alloc_solve) and y_in the caller's labels.
  // twin mode: n, lo, nloc and the selection shape are those of the 2 nrow virtual points; the kernel rows -- what
  // the GEMV, the column store and the column cache run over -- are the nrow rows.  one-class mode: the boxes are
  // 1, and the start is (oc_full, oc_frac) followed by the chunked start (nz_update)
  DecompMode mode;
  int64_t nrow = 0;
  int64_t rows() const { return mode.twin() ? nrow : nloc; }  // this GPU's kernel rows
  int64_t cols() const { return mode.twin() ? nrow : n; }     // the kernel columns
  int64_t oc_full = 0;
  double oc_frac = 0.0;
  const int32_t* y_in = nullptr;
  ShrinkCfg shc;
  InnerVariant inner;
  NwDev nwd{};
  const DecompAllGather* allgather = nullptr;
  svm_decomp_trace* tr = nullptr;
  ColCache cc;
  DecompWs w;
  // pinned: the PROF totals, the two published control blocks (and their device address), the warm start's count
  DecompHost* hs = nullptr;
  DecompCtl *ctl_h = nullptr, *ctl_pub = nullptr;
  int64_t* nz_h = nullptr;
  std::chrono::steady_clock::time_point t0;
};

// The packed rows of a shrunk solve and the host's view of the shrinking: pk = the current list's buffer
// (-1: none, the rows in place -- before the first repack and after an unshrink), pk_bound = an upper bound
// of the device's packed row count (the active count the host last read: passes only drop rows); o_dev =
// the device's outer-iteration count when the next enqueued one runs (exact: only a stop or an unshrink
// turns launches into no-ops, and the host re-reads the count at an unshrink), origin = the outer count at
// the start or the last unshrink, seen_active = the active rows the host last read back.
struct PackState {
  int pk = -1;
  int64_t pk_bound = 0, seen_active = 0, min_active = 0;
  int64_t o_dev = 0, origin = 0, unshrinks = 0, repacks = 0;
  explicit PackState(int64_t nloc) : pk_bound(nloc), seen_active(nloc), min_active(nloc) {}
};

// Column cache (exact-integer rows): the f update's kernel columns K(this GPU's rows, j) stay in HBM
// per point for the rest of the fit, so a column moved again is a read, not an int8-MFMA
// recomputation (64 / 75 / 85 % of the column uses at 60k / 250k / 1M repeat an earlier one,
// profiles/r4_decomp_column_cache.txt); bit-identical to the GEMV path (ws_cache_fsum_kernel).
// SVM355_DECOMP_CCACHE = 0 off, 1 on; default on once this GPU's int8 rows (nloc x kq bytes, read by
// every recomputation) outgrow the 256 MB last-level cache: the recomputation then streams them from
// HBM (192 MiB: 60k MNIST rows, 46 MB, are 4 % faster without the cache, 250k rows 2 % with it).
// Runs under the lock that also covers the workspace allocation (alloc_solve).
int size_col_cache(const Solve& S, bool warm, ColCache* out) {
  DeviceCtx* ctx = S.ctx;
  const DecompKnobs& k = S.k;
  const int64_t n = S.cols(), nloc = S.rows();  // slots per kernel row
  *out = ColCache{};
  if (S.f64 || nloc <= 0) return SVM_OK;
  if (!(k.ccache >= 0 ? k.ccache != 0 : nloc * int64_t(S.kq) > (int64_t(192) << 20))) return SVM_OK;
  // slots: twice the distinct columns measured per fit (~1,686 (n / 60k)^0.46), within half the free
  // HBM, plus kMaxWS scratch slots (moved columns beyond a full cache, this update only)
  int64_t cap = int64_t(2.0 * 1686.0 * std::pow(double(n) / 60000.0, 0.46));
  cap = std::min<int64_t>(std::max<int64_t>(cap, 1024), n);
  size_t free_b = 0, total_b = 0;
  SVMD_CHECK(hipMemGetInfo(&free_b, &total_b));
  const int64_t ld = (nloc + 3) & ~int64_t(3);  // a multiple of 4: 16-byte row pairs (or quads) in the reader
  const size_t slot_b = size_t(ld) * 8;
  // the workspace allocated next (f, the GEMV partials, the per-point slot map, a warm start's columns
  // and ~64 MB of fixed parts) comes out of the same free memory
  const size_t ws_need = size_t(nloc + 1) * 8 * size_t(1 + kLdp) + size_t(n) * (warm ? 16 : 4) + (size_t(64) << 20);
  const size_t ws_grow = ws_need > ctx->ws_bytes ? ws_need - ctx->ws_bytes : 0;
  const size_t avail = free_b + ctx->rc_cache_bytes > ws_grow ? free_b + ctx->rc_cache_bytes - ws_grow : 0;
  cap = std::min<int64_t>(cap, int64_t(avail / 2 / slot_b) - kMaxWS);
  // and at most a quarter of the GPU's HBM (SVM355_DECOMP_CCACHE_FRAC): the slab is a grow-only
  // buffer of the context, kept for the next fit, that PyTorch's allocator cannot see -- it must leave
  // room for the caller's tensors and other contexts on the device.  At 1M rows that is
  // ~8,000 slots of 8 MB for ~6,100 distinct columns a fit moves, so no fit of n <= 1M loses a hit.
  // (a context's own share when several solve side by side, svmd_set_ccache_frac; the env var overrides)
  double frac = ctx->ccache_frac >= 0.0 ? ctx->ccache_frac : 0.25;
  // processes sharing this GPU (torchrun ranks over host-staged gloo on one device; the lock orders the
  // sizing within a process only): each takes its share of the quarter
  if (ctx->ccache_frac < 0.0 && k.local_world > 0) {
    int ndev = 1;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) ndev = 1;
    const int sharing = (k.local_world + ndev - 1) / ndev;
    frac /= double(sharing);
  }
  if (k.ccache_frac >= 0.0) frac = k.ccache_frac;
  cap = std::min<int64_t>(cap, int64_t(double(total_b) * frac / double(slot_b)) - kMaxWS);
  int64_t min_cap = 256;
  if (k.ccache_slots_set) {
    cap = std::min<int64_t>(cap, k.ccache_slots);
    min_cap = 1;
  }
  if (cap >= min_cap && cap < int64_t(INT32_MAX) - kMaxWS) out->slab = ctx->ensure_rc_cache(size_t(cap + kMaxWS) * slot_b);
  if (!out->slab) {
    (void)hipGetLastError();  // a failed allocation is not sticky: the GEMV path runs
    return SVM_OK;
  }
  out->cap = int32_t(cap);
  out->ld = ld;
  return SVM_OK;
}

// The solve's workspace, in this order (the layout is part of what a fit's speed was measured on).
void layout_ws(Solve& S, bool warm, WsCarver& c) {
  DecompWs& w = S.w;
  const size_t nl1 = size_t(std::max<int64_t>(S.nloc, 1)), n = size_t(S.n), kq = size_t(S.kq), ld = size_t(S.R.ld);
  const size_t nr1 = size_t(std::max<int64_t>(S.rows(), 1)), ncol = size_t(S.cols());  // kernel rows / columns
  const bool f64 = S.f64, q8 = !f64, cache = S.cc.slab != nullptr, nzbuf = warm || S.shc.on, pack = S.pack_on;
  w.f = c.take<double>(nl1);
  w.own = c.take<CandRec>(size_t(S.Lr));
  w.all = c.take<CandRec>(size_t(S.sh.L));
  w.W = c.take<int32_t>(kMaxWS);
  w.Wf = c.take<double>(kMaxWS);
  w.Kw = c.take<double>(size_t(kMaxWS) * kLdw);
  w.coef = c.take<double>(kMaxWS);
  w.cols = c.take<int32_t>(kMaxWS);
  w.mcount = c.take<int32_t>(64);
  w.ctl = c.take<DecompCtl>(1);
  w.Qw = c.take<int8_t>(size_t(kMaxWS) * kq, q8);
  w.N0w = c.take<int32_t>(kMaxWS, q8);
  w.WNw = c.take<double>(kMaxWS, q8);
  w.part = c.take<double>(nr1 * kLdp, q8);
  w.Xw = c.take<double>(size_t(kMaxWS) * ld, f64);
  w.nw = c.take<double>(kMaxWS, f64);
  w.Xc = c.take<double>(size_t(kMaxWS) * ld, f64);
  w.nc = c.take<double>(kMaxWS, f64);
  w.Kc = c.take<double>(nr1 * kMaxWS, f64);
  w.cslot = c.take<int32_t>(ncol, cache);
  w.crd = c.take<int32_t>(kMaxWS, cache);
  w.cmid = c.take<int32_t>(kMaxWS, cache);
  w.cmsl = c.take<int32_t>(kMaxWS, cache);
  w.cst = c.take<int32_t>(16, cache);
  w.cmeta = c.take<int32_t>(size_t(S.cc.cap) * 3, cache && S.k.cache_evict);  // owner, last, ref per slot
  w.wid = c.take<int32_t>(kMaxWS + 16, q8);
  w.wcols = c.take<int32_t>(n, nzbuf);
  w.wcoef = c.take<double>(n, nzbuf);
  w.wcnt = c.take<int32_t>(size_t(S.nchunks + 1), nzbuf);
  w.shr = c.take<uint8_t>(nl1, S.shc.on);
  w.gAw = c.take<double>(kMaxWS);
  w.nAmat = c.take<double>(size_t(kMaxWS + 2) * kMaxWS, S.nwd.on != 0);
  w.act[0] = c.take<int32_t>(nl1 * 2, pack);
  w.act[1] = w.act[0] ? w.act[0] + nl1 : nullptr;
  w.boff[0] = c.take<int32_t>(size_t(S.NBr + 1) * 2, pack);
  w.boff[1] = w.boff[0] ? w.boff[0] + (S.NBr + 1) : nullptr;
  w.bcnt = c.take<int32_t>(size_t(S.NBr + 1), pack);
  w.pos_of = c.take<int32_t>(nl1, pack);
  w.nrows = c.take<int32_t>(16, pack);
  w.cdiag = c.take<int32_t>(kMaxWS, pack);
  w.mdiag = c.take<int32_t>(kMaxWS, pack);
  w.Qa = c.take<int8_t>(nl1 * kq, pack);
  w.N0a = c.take<int32_t>(nl1, pack);
  w.WNa = c.take<double>(nl1, pack);
  w.sgn = c.take<int32_t>(n, S.mode.own_signs());
  w.fcols = c.take<int32_t>(kMaxWS, S.mode.twin());
  w.fcoef = c.take<double>(kMaxWS, S.mode.twin());
  w.fcount = c.take<int32_t>(64, S.mode.twin());
}

// What the solve is asked to run with (decomp_mode.h); the class weights' range check comes with the boxes.
int mode_features(const DecompOpts& o, const svm_params& p, DecompFeatures* f) {
  double cp = 0.0, cn = 0.0;
  if (const int rc = svm_class_boxes(&p, &cp, &cn)) return rc;
  const bool classify = o.mode.kind == DecompModeKind::classify;
  *f = decomp_features(p, o.world, o.warm, classify ? cp != cn : cp != p.C || cn != p.C);
  return SVM_OK;
}

// The checks, the shape and this GPU's slice of it, the knobs and what follows from them.
int setup_solve(Solve& S, DeviceCtx* ctx, const DecompRows& R, const int32_t* y, double* alpha, int64_t n,
                const svm_params& p, int qws, const DecompOpts& o) {
  const int world = o.world, rank = o.rank;
  const int64_t nrow = n;  // the kernel rows; n below counts the points the solve selects among
  DecompFeatures ft;  // everything the mode does not cover is refused here, before any device work
  int rc = mode_features(o, p, &ft);
  if (rc || (rc = decomp_mode_check("decomposition SMO", o.mode, y, ft, nrow, DecompBackend::device))) return rc;
  n = o.mode.points(nrow);
  svm_params p1 = p;  // the solve's parameters (one-class mode: the box is 1 whatever p.C says)
  int64_t oc_full = 0;
  double oc_frac = 0.0;
  if (o.mode.kind == DecompModeKind::oneclass) {
    if ((rc = svm_oneclass_start(o.mode.oneclass_nu, n, &oc_full, &oc_frac))) return rc;
    p1.C = 1.0;
    p1.weight_pos = p1.weight_neg = 0.0;
  }
  if (world < 1 || rank < 0 || rank >= world || (world > 1 && !o.allgather)) {
    set_error("decomposition SMO: bad world / rank / exchange");
    return SVM_ERR_ARG;
  }
  const bool f64 = R.fp64();
  if (f64 ? (R.ld % 16 != 0 || !R.nrm) : (!R.Q || !R.P)) {
    set_error("decomposition SMO: bad row source");
    return SVM_ERR_ARG;
  }
  svm_decomp_trace* tr = o.trace;
  if (tr && (world != 1 || tr->cap < 0 || (tr->n != 0 && tr->n != n))) {
    set_error("decomposition SMO: a trace needs one GPU and snapshots of n = %lld", (long long)n);
    return SVM_ERR_ARG;
  }
  const DecompShape sh = decomp_shape(n, qws, world);
  if (!sh.ok) {
    set_error("decomposition SMO: n = %lld is outside the solver's shapes (2 <= n < 2^31 - 1, %lld candidates <= %d, "
              "world <= 64)", (long long)n, (long long)sh.L, kMaxWS);
    return SVM_ERR_ARG;
  }
  if ((rc = read_knobs(sh, &S.k))) return rc;
  if ((rc = svm_class_boxes(&p1, &S.Cp, &S.Cn))) return rc;
  S.ctx = ctx;
  S.s = ctx->stream;
  S.R = R;
  S.f64 = f64;
  S.kq = f64 ? 0 : R.P->kq;
  S.y = y;  // a mode with its own signs: those, in the workspace (alloc_solve)
  S.alpha = alpha;
  S.mode = o.mode;
  S.nrow = nrow;
  S.oc_full = oc_full;
  S.oc_frac = oc_frac;
  S.y_in = y;
  S.n = n;
  S.p = p1;
  S.sh = sh;
  S.world = world;
  S.rank = rank;
  S.NBr = sh.NB / world;
  const int64_t b0 = rank * S.NBr;
  S.lo = std::min<int64_t>(n, b0 * sh.per);
  S.nloc = std::min<int64_t>(n, (b0 + S.NBr) * sh.per) - S.lo;
  S.Lr = 2 * S.NBr * sh.T;  // this GPU's candidate records (I_high picks, then I_low)
  S.nchunks = (n + kMaxWS - 1) / kMaxWS;
  S.wide_select = sh.per > int64_t(kSelNT) * kSelE || sh.T > 64 || S.k.wide_select;
  S.kww_narrow = !f64 && !S.k.kww_sym && S.kq <= 1536;
  S.shc = shrink_cfg(p);
  S.pack_on = S.shc.on && !f64 && S.nloc > 0 && S.k.pack;
  const NewtonCfg nwc = newton_cfg(p);
  S.nwd = NwDev{nwc.on ? 1 : 0, nwc.every, nwc.per_solve, nwc.repeat, nwc.max_free, 0, nwc.frac};
  S.inner = InnerVariant{S.k.inner_nt, S.k.prof, S.k.wss2, S.k.dp, S.k.j2s, nwc.on, S.Cp != S.Cn};
  if (S.inner.weighted && !ws_inner_weighted_built(S.inner)) {
    set_error("decomposition SMO: the weighted inner solve is not built for SVM355_DECOMP_NT=%d SVM355_DECOMP_WSS=%d "
              "SVM355_DECOMP_PROF=%d (built: NT=256 with WSS=1, 2 or 3, PROF=0)",
              S.k.inner_nt, S.k.j2s ? 4 : S.k.dp ? 3 : S.k.wss2 ? 2 : 1, S.k.prof ? 1 : 0);
    return SVM_ERR_ARG;
  }
  S.allgather = &o.allgather;
  S.tr = tr;
  return SVM_OK;
}

// Sizing and allocating the cache and the workspace is one step per process: thread ranks sharing a
// GPU (the loopback rehearsal) would otherwise read the same free memory, each take half of it, and
// leave a later rank without room for its workspace.
int alloc_solve(Solve& S, bool warm) {
  static std::mutex alloc_mu;
  std::lock_guard<std::mutex> alloc_lock(alloc_mu);
  int rc = size_col_cache(S, warm, &S.cc);
  if (rc) return rc;
  if ((rc = carve_ws(S.ctx, [&](WsCarver& c) { layout_ws(S, warm, c); }))) return rc;
  if (S.mode.own_signs()) S.y = S.w.sgn;
  if ((rc = S.ctx->ensure_pinned(sizeof(DecompHost) * 2 + 2 * sizeof(DecompCtl) + 64))) return rc;
  char* pin = static_cast<char*>(S.ctx->pinned);
  S.hs = reinterpret_cast<DecompHost*>(pin);
  S.ctl_h = reinterpret_cast<DecompCtl*>(pin + sizeof(DecompHost) * 2);
  S.nz_h = reinterpret_cast<int64_t*>(pin + sizeof(DecompHost) * 2 + 2 * sizeof(DecompCtl));
  SVMD_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&S.ctl_pub), S.ctl_h, 0));  // as the device addresses it
  return SVM_OK;
}

// f += K(this GPU's rows, cols[0:*cnt]) coef: the exact-integer GEMV (column-half partials summed in
// order) or, for FP64 rows, the moved columns' rows gathered, their block on FP64 MFMA and a row sum
// tiled: also launch the tiled column store for updates of more than 64 misses (it exits at once
// otherwise, but a launch over every row tile costs ~5-8 us); off after the first outer iterations,
// where the narrow store takes any count itself (only the cold start misses hundreds of columns)
// Packed rows (a shrunk solve, pk >= 0): the row operand is the packed copy (Qa, N0a, WNa) of the active
// rows, pk_bound of them by the host's bound (the device count nrows gates the sums), the unit
// diagonal from the columns' packed positions (the inner solve's cdiag), and the sums go to f[act[k]].
int f_update(const Solve& S, const PackState& ps, const int32_t* cl, const double* cf, const int32_t* cnt,
             bool tiled = true) {
  const DecompWs& w = S.w;
  const DecompRows& R = S.R;
  hipStream_t s = S.s;
  // twin mode: cl / cf / cnt are the folded list (rows, one entry each), the kernel work runs over the nrow
  // rows exactly as a classification of them would, and the sums' TWIN instantiations add each row's sum to
  // both of its points
  const bool twin = S.mode.twin();
  const int64_t lo = S.lo, nloc = S.rows();
  if (nloc <= 0) return SVM_OK;
  if (S.f64) {
    hipLaunchKernelGGL(ws_gather_f64_kernel, dim3(unsigned(kMaxWS)), dim3(64), 0, s, R.X, R.nrm, R.ld, cl, cnt,
                       nullptr, w.Xc, w.nc);
    SVMD_LAUNCH_CHECK();
    const int rc = launch_rbf_block_dev(s, R.X + lo * R.ld, R.nrm + lo, nloc, R.ld, w.Xc, w.nc, kMaxWS, R.ld, R.ld,
                                        S.p.gamma, w.Kc, kMaxWS, false, nullptr, cnt, cl, lo);
    if (rc) return rc;
    hipLaunchKernelGGL(twin ? ws_rowsum_f64_kernel<true> : ws_rowsum_f64_kernel<false>, dim3(unsigned((nloc + 3) / 4)),
                       dim3(256), 0, s, w.Kc, int64_t(kMaxWS), cf, cnt, w.f, nloc);
    SVMD_LAUNCH_CHECK();
    return SVM_OK;
  }
  const QuantPlan& P = *R.P;
  const bool packed = ps.pk >= 0;
  const int8_t* Qr = packed ? w.Qa : R.Q + lo * int64_t(P.kq);
  const int32_t* N0r = packed ? w.N0a : R.N0 + lo;
  const double* WNr = packed ? w.WNa : R.WN + lo;
  const int64_t nr = packed ? ps.pk_bound : nloc, roff = packed ? 0 : lo;
  const int32_t* pa = packed ? w.act[ps.pk] : nullptr;
  const int32_t* pn = packed ? w.nrows : nullptr;
  if (nr <= 0) return SVM_OK;
  if (S.cc.slab) {  // plan the slots, compute and store the missing columns, sum every column from the cache
    hipLaunchKernelGGL(ws_cache_plan_kernel, dim3(1), dim3(kMaxWS), 0, s, cl, cnt, w.cslot, S.cc.cap, w.cst, w.crd,
                       w.cmid, w.cmsl, w.cmeta, packed ? w.cdiag : nullptr, w.mdiag);
    SVMD_LAUNCH_CHECK();
    const int rc = launch_igram_colstore(s, Qr, N0r, WNr, R.stw, nr, roff, R.Q, R.N0, R.WN, w.cmid, w.cmsl, w.cst + 1,
                                         kMaxWS, P, S.p.gamma, S.cc.slab, S.cc.ld, w.cst + 2, tiled,
                                         packed ? w.mdiag : nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL((twin ? ws_cache_fsum_kernel<2, true> : ws_cache_fsum_kernel<2, false>),
                       dim3(unsigned((nr + 511) / 512)), dim3(256), 0, s, S.cc.slab, S.cc.ld, w.crd, cf, cnt, w.f, nr, pa,
                       pn);
    SVMD_LAUNCH_CHECK();
    return SVM_OK;
  }
  const int rc = launch_igram_gemv(s, Qr, N0r, WNr, R.stw, nr, roff, R.Q, R.N0, R.WN, cl, cf, cnt, kMaxWS, P, S.p.gamma,
                                   w.part, kLdp, packed ? w.cdiag : nullptr);
  if (rc) return rc;
  hipLaunchKernelGGL(twin ? ws_fsum_count_kernel<true> : ws_fsum_count_kernel<false>, dim3(unsigned((nr + 255) / 256)),
                     dim3(256), 0, s, w.part, kLdp, cnt, w.f, nr, pa, pn);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int cache_reset(const Solve& S) {  // no point has a slot, the first free slot is 0
  if (!S.cc.slab) return SVM_OK;
  const DecompWs& w = S.w;
  SVMD_CHECK(hipMemsetAsync(w.cslot, 0xFF, size_t(S.cols()) * 4, S.s));
  SVMD_CHECK(hipMemsetAsync(w.cst, 0, 64, S.s));
  if (w.cmeta) {  // owners and stamps -1, CLOCK bits clear
    SVMD_CHECK(hipMemsetAsync(w.cmeta, 0xFF, size_t(S.cc.cap) * 8, S.s));
    SVMD_CHECK(hipMemsetAsync(w.cmeta + 2 * int64_t(S.cc.cap), 0, size_t(S.cc.cap) * 4, S.s));
  }
  return SVM_OK;
}

// f += K(:, nz) (alpha y)_nz: the nonzero alphas compacted (ascending ids), then the GEMV in chunks of
// kMaxWS columns, each summed into f in order (svm_decomp_train_gram does the same): a warm start, and
// the recomputation of f when a shrunk solve unshrinks.  The one host read: how many chunks.
int nz_update(const Solve& S, const PackState& ps, int64_t* nz_out) {
  const DecompWs& w = S.w;
  hipStream_t s = S.s;
  *S.nz_h = -1;
  hipLaunchKernelGGL(ws_nz_compact_kernel, dim3(1), dim3(1024), 0, s, S.alpha, S.y, S.n, w.wcols, w.wcoef,
                     w.wcnt + S.nchunks, S.nz_h);
  SVMD_LAUNCH_CHECK();
  SVMD_CHECK(hipStreamSynchronize(s));
  const int64_t nz = *S.nz_h;
  if (nz < 0 || nz > S.n) {
    set_error("decomposition SMO: the nonzero-alpha compaction returned no count");
    return SVM_ERR_INTERNAL;
  }
  const int nch = int((nz + kMaxWS - 1) / kMaxWS);
  if (nch > 0) {
    hipLaunchKernelGGL(ws_chunk_counts_kernel, dim3(unsigned((nch + 255) / 256)), dim3(256), 0, s, w.wcnt + S.nchunks,
                       w.wcnt, nch);
    SVMD_LAUNCH_CHECK();
  }
  for (int c = 0; c < nch; ++c) {
    const int rc = f_update(S, ps, w.wcols + int64_t(c) * kMaxWS, w.wcoef + int64_t(c) * kMaxWS, w.wcnt + c);
    if (rc) return rc;
  }
  if (nz_out) *nz_out = nz;
  return SVM_OK;
}

// The start of a solve on the stream: the control block running with its counters 0, a fresh cache,
// alpha (cold start) and f = -y, and a warm start's f (*warm_cols = its columns).  One-class mode: its own
// alpha, f = 0, and always the chunked start (*warm_cols = the start's columns).
int start_solve(const Solve& S, const PackState& ps, bool warm, int64_t* warm_cols) {
  const DecompWs& w = S.w;
  hipStream_t s = S.s;
  std::memset(S.hs, 0, sizeof(DecompHost));
  SVMD_CHECK(hipMemsetAsync(w.ctl, 0, sizeof(DecompCtl), s));  // stop = SVM_STOP_RUNNING, counters 0
  if (S.f64) SVMD_CHECK(hipMemsetAsync(w.Xw, 0, size_t(kMaxWS) * S.R.ld * 8, s));  // rows beyond m stay finite
  if (S.kww_narrow) {
    static const std::vector<int32_t> ident = [] {
      std::vector<int32_t> v(kMaxWS + 1);
      for (int k = 0; k < kMaxWS; ++k) v[k] = k;
      v[kMaxWS] = kMaxWS;
      return v;
    }();
    SVMD_CHECK(hipMemcpyAsync(w.wid, ident.data(), ident.size() * 4, hipMemcpyHostToDevice, s));
  }
  int rc = cache_reset(S);  // a fresh cache per fit
  if (rc) return rc;
  if (w.shr) SVMD_CHECK(hipMemsetAsync(w.shr, 0, size_t(std::max<int64_t>(S.nloc, 1)), s));
  switch (S.mode.kind) {
    case DecompModeKind::twin:
      hipLaunchKernelGGL(ws_twin_init_kernel, dim3(unsigned((S.nrow + 255) / 256)), dim3(256), 0, s, S.mode.twin_z,
                         S.mode.twin_eps, S.nrow, w.sgn, S.alpha, w.f, w.ctl);
      break;
    case DecompModeKind::oneclass:
      hipLaunchKernelGGL(ws_oneclass_init_kernel, dim3(unsigned((S.n + 255) / 256)), dim3(256), 0, s, S.oc_full,
                         S.oc_frac, S.n, w.sgn, S.alpha, w.f, w.ctl);
      break;
    case DecompModeKind::heldout:
      hipLaunchKernelGGL(ws_heldout_init_kernel, dim3(unsigned((S.n + 255) / 256)), dim3(256), 0, s, S.y_in,
                         S.mode.heldout, S.n, w.sgn, S.alpha, w.f, w.ctl);
      break;
    case DecompModeKind::classify:
      hipLaunchKernelGGL(ws_init_kernel, dim3(unsigned((S.n + 255) / 256)), dim3(256), 0, s, S.y, S.alpha, w.f, S.lo,
                         S.nloc, S.n, int(warm), w.ctl);
      break;
  }
  SVMD_LAUNCH_CHECK();
  if (S.mode.chunked_start(warm) && (rc = nz_update(S, ps, warm_cols))) return rc;
  return SVM_OK;
}

// repack: the active rows (not shrunk) into the other list buffer, their quantised rows copied, the
// column cache (whose rows are the packed ones) cleared
int repack(const Solve& S, PackState& ps) {
  const DecompWs& w = S.w;
  const DecompRows& R = S.R;
  const int nb = ps.pk < 0 ? 0 : ps.pk ^ 1;
  const int32_t* ca = ps.pk < 0 ? nullptr : w.act[ps.pk];
  const int32_t* cb = ps.pk < 0 ? nullptr : w.boff[ps.pk];
  hipLaunchKernelGGL(ws_pack_count_kernel, dim3(unsigned(S.NBr)), dim3(256), 0, S.s, ca, cb, S.sh.per, S.nloc, w.shr,
                     w.bcnt);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(ws_pack_write_kernel, dim3(unsigned(S.NBr)), dim3(256), 0, S.s, ca, cb, S.sh.per, S.nloc, w.shr,
                     w.bcnt, w.boff[nb], w.nrows, w.act[nb], w.pos_of, R.Q, R.N0, R.WN, S.lo, S.kq, w.Qa, w.N0a, w.WNa);
  SVMD_LAUNCH_CHECK();
  ps.pk = nb;
  ps.pk_bound = ps.seen_active;
  ++ps.repacks;
  return cache_reset(S);
}

// The wait for an event of the solver's stream: under the exchange's deadline / abort policy when the
// distributed solve has one, else here.
int wait_event(const Solve& S, hipEvent_t ev) {
  if (!(S.world > 1 && S.allgather->wait && S.allgather->wait(ev))) SVMD_CHECK(hipEventSynchronize(ev));
  return SVM_OK;
}

// The unshrink (decomp_shrink.h), when a readback shows kStopUnshrink: the queued batch ran as no-ops and
// `ev` (recorded after it) is waited for under the exchange's policy; then every row is active again, the
// rows are in place again (no packed list), the column cache is cleared, f is recomputed from alpha (the
// warm start's chunked update), and the outer loop resumes at the device's outer count.
int unshrink(const Solve& S, PackState& ps, const DecompCtl& seen, hipEvent_t ev) {
  const DecompWs& w = S.w;
  hipStream_t s = S.s;
  int rc = ev ? wait_event(S, ev) : SVM_OK;
  if (rc) return rc;
  hipLaunchKernelGGL(ws_unshrink_ctl_kernel, dim3(1), dim3(64), 0, s, w.ctl, S.nloc);
  SVMD_LAUNCH_CHECK();
  SVMD_CHECK(hipMemsetAsync(w.shr, 0, size_t(std::max<int64_t>(S.nloc, 1)), s));
  ps.pk = -1;
  ps.pk_bound = S.nloc;
  ps.seen_active = S.nloc;
  if ((rc = cache_reset(S))) return rc;
  hipLaunchKernelGGL(ws_init_kernel, dim3(unsigned((S.n + 255) / 256)), dim3(256), 0, s, S.y, S.alpha, w.f, S.lo, S.nloc,
                     S.n, 1, w.ctl);
  SVMD_LAUNCH_CHECK();
  if ((rc = nz_update(S, ps, nullptr))) return rc;
  ps.o_dev = ps.origin = seen.outer;
  ++ps.unshrinks;
  if (S.k.shrink_log) {
    SVMD_CHECK(hipStreamSynchronize(s));
    fprintf(stderr, "decomp: rank %d unshrink at outer %lld (%.3f ms)\n", S.rank, (long long)seen.outer, ms_since(S.t0));
  }
  return SVM_OK;
}

// solo timing (DecompSolo): the two device segments of an outer iteration under the shared mutex,
// each timed alone and waited for before the mutex is released
struct SoloTimer {
  DecompSolo* solo;
  hipStream_t s;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::unique_lock<std::mutex> lk;
  ~SoloTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int init() {
    if (solo)
      for (auto& e : ev) SVMD_CHECK(hipEventCreate(&e));
    return SVM_OK;
  }
  int begin(int k) {
    if (!solo) return SVM_OK;
    lk = std::unique_lock<std::mutex>(*solo->mu);
    SVMD_CHECK(hipEventRecord(ev[2 * k], s));
    return SVM_OK;
  }
  int end(int k) {
    if (!solo) return SVM_OK;
    SVMD_CHECK(hipEventRecord(ev[2 * k + 1], s));
    SVMD_CHECK(hipEventSynchronize(ev[2 * k + 1]));
    float ms = 0.0f;
    SVMD_CHECK(hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
    (k == 0 ? solo->sel_ms : solo->rest_ms).push_back(double(ms));
    lk.unlock();
    return SVM_OK;
  }
};

// K(W, W) of the working set the build left: its rows gathered, then the exact-integer Gram over the full
// capacity (the narrow column store, else the triangular launch) or the FP64-MFMA block.
int enqueue_kww(const Solve& S) {
  const DecompWs& w = S.w;
  const DecompRows& R = S.R;
  hipStream_t s = S.s;
  int32_t* gate = &w.ctl->stop;
  // twin mode: a point's row is its id mod nrow, and two twins in W get the diagonal's 1 between them
  auto twin_diag = [&]() -> int {
    if (!S.mode.twin()) return SVM_OK;
    hipLaunchKernelGGL(ws_twin_kww_kernel, dim3(1), dim3(kMaxWS), 0, s, w.W, w.ctl, S.nrow, w.Kw, kLdw);
    SVMD_LAUNCH_CHECK();
    return SVM_OK;
  };
  if (S.f64) {
    if (S.mode.twin())
      hipLaunchKernelGGL(ws_gather_f64_twin_kernel, dim3(unsigned(kMaxWS)), dim3(64), 0, s, R.X, R.nrm, R.ld, w.W,
                         &w.ctl->m, gate, w.Xw, w.nw, S.nrow);
    else
      hipLaunchKernelGGL(ws_gather_f64_kernel, dim3(unsigned(kMaxWS)), dim3(64), 0, s, R.X, R.nrm, R.ld, w.W, &w.ctl->m,
                         gate, w.Xw, w.nw);
    SVMD_LAUNCH_CHECK();
    // K(W, W) on FP64 MFMA, columns bounded by m, unit diagonal; skipped once stopped
    const int rc = launch_rbf_block_dev(s, w.Xw, w.nw, kMaxWS, R.ld, w.Xw, w.nw, kMaxWS, R.ld, R.ld, S.p.gamma, w.Kw,
                                        kLdw, true, gate, &w.ctl->m, nullptr, 0);
    return rc ? rc : twin_diag();
  }
  const QuantPlan& P = *R.P;
  if (S.mode.twin())
    hipLaunchKernelGGL(ws_gather_twin_kernel, dim3(unsigned(kMaxWS)), dim3(64), 0, s, R.Q, R.N0, R.WN, P.kq, w.W, w.ctl,
                       w.Qw, w.N0w, w.WNw, S.nrow);
  else
    hipLaunchKernelGGL(ws_gather_kernel, dim3(unsigned(kMaxWS)), dim3(64), 0, s, R.Q, R.N0, R.WN, P.kq, w.W, w.ctl,
                       w.Qw, w.N0w, w.WNw);
  SVMD_LAUNCH_CHECK();
  // K(W, W) over the full capacity (rows beyond m are never read); skipped once stopped
  bool ww = false;
  int rc = SVM_OK;
  if (S.kww_narrow && (rc = launch_igram_ww(s, w.Qw, w.N0w, w.WNw, R.stw, kMaxWS, w.wid, w.wid + kMaxWS, P, S.p.gamma,
                                            w.Kw, kLdw, gate, &ww)))
    return rc;
  if (!ww)
    rc = launch_igram_sym(s, w.Qw, w.N0w, w.WNw, const_cast<double*>(R.stw), kMaxWS, P, S.p.gamma, w.Kw, kLdw, false,
                          gate);
  return rc ? rc : twin_diag();
}

// One outer iteration on the stream, the `index`-th enqueued: (repack,) select, all-gather, build, gather,
// K(W, W), inner solve, f update, shrink pass.  Every kernel reads the device control block, so after the
// stop these are no-op launches.  pub: where the last kernel to change the control block publishes it.
int enqueue_outer(const Solve& S, PackState& ps, SoloTimer& solo, int64_t index, bool first_of_batch, DecompCtl* pub) {
  const DecompWs& w = S.w;
  const svm_params& p = S.p;
  hipStream_t s = S.s;
  const int64_t NBr = S.NBr, lo = S.lo, nloc = S.nloc;
  const int T = S.sh.T;
  int rc;
  if (S.world > 1 && S.k.fail_rank == S.rank && index == S.k.fail_outer) {
    set_error("injected failure of rank %d at outer iteration %lld", S.rank, (long long)S.k.fail_outer);
    return SVM_ERR_INTERNAL;
  }
  if ((rc = solo.begin(0))) return rc;
  // repack once the active rows the host last read are at most repack_frac of the packed ones
  if (S.pack_on && NBr > 0 && first_of_batch && ps.seen_active < ps.pk_bound &&
      double(ps.seen_active) <= S.k.repack_frac * double(ps.pk_bound))
    if ((rc = repack(S, ps))) return rc;
  const bool packed = ps.pk >= 0;
  const int32_t* act = packed ? w.act[ps.pk] : nullptr;
  if (NBr > 0)
    hipLaunchKernelGGL(S.wide_select ? ws_select_wide_kernel : ws_select_kernel, dim3(unsigned(NBr)), dim3(kSelNT), 0, s,
                       w.f, S.alpha, S.y, lo, nloc, S.sh.per, T, S.Cp, S.Cn, p.eps, w.own, w.own + NBr * T, w.ctl, act,
                       packed ? w.boff[ps.pk] : nullptr, w.shr);
  SVMD_LAUNCH_CHECK();
  if ((rc = solo.end(0))) return rc;
  CandRec* all = S.world > 1 ? w.all : w.own;
  if (S.world > 1) S.allgather->gather(w.own, int64_t(S.Lr * sizeof(CandRec)), all);  // stream-ordered
  if ((rc = solo.begin(1))) return rc;
  hipLaunchKernelGGL(ws_build_kernel, dim3(1), dim3(kMaxWS), 0, s, all, int(S.sh.L), int(S.Lr), int(NBr * T), int(T),
                     p.tau, S.k.tau_frac, int64_t(p.max_iter), w.W, w.Wf, w.ctl, w.mcount, pub);
  SVMD_LAUNCH_CHECK();
  if ((rc = enqueue_kww(S))) return rc;
  if ((rc = launch_ws_inner(s, S.inner,
                            InnerArgs{w.Kw, kLdw, w.W, w.ctl, S.y, S.alpha, w.Wf, S.Cp, p.eps, w.cols, w.coef, w.mcount,
                                      S.hs, pub, packed ? w.pos_of : nullptr, lo, nloc, packed ? w.cdiag : nullptr,
                                      w.gAw, w.Wf, w.nAmat, S.nwd, S.Cn})))
    return rc;
  SVMD_LAUNCH_CHECK();
  if (S.mode.twin()) {  // the moved points folded to one entry per kernel row
    hipLaunchKernelGGL(ws_twin_fold_kernel, dim3(1), dim3(kMaxWS), 0, s, w.cols, w.coef, w.mcount, S.nrow, w.fcols,
                       w.fcoef, w.fcount);
    SVMD_LAUNCH_CHECK();
    rc = f_update(S, ps, w.fcols, w.fcoef, w.fcount, index < 4);
  } else {
    rc = f_update(S, ps, w.cols, w.coef, w.mcount, index < 4);
  }
  if (rc) return rc;
  ++ps.o_dev;  // this outer iteration's count once it has run
  if (S.shc.pass_after(ps.o_dev, ps.origin) && nloc > 0) {  // the shrink pass, with this outer iteration's bounds
    const int64_t np = packed ? ps.pk_bound : nloc;
    hipLaunchKernelGGL(ws_shrink_pass_kernel, dim3(unsigned((np + 255) / 256)), dim3(256), 0, s, w.f, S.alpha, S.y, lo,
                       nloc, act, w.nrows, w.shr, p.C, p.eps, S.shc.margin, w.ctl);
    SVMD_LAUNCH_CHECK();
  }
  return solo.end(1);
}

// The trace's record of the outer iteration the control block `c` was read back after (one GPU).
int record_trace(const Solve& S, const DecompCtl& c) {
  svm_decomp_trace* tr = S.tr;
  const DecompWs& w = S.w;
  const int64_t n = S.n;
  if (tr->count >= tr->cap) return SVM_OK;
  const int64_t oi = tr->count++;
  const int m = c.m;
  int32_t mv = 0;
  SVMD_CHECK(hipMemcpy(&mv, w.mcount, 4, hipMemcpyDeviceToHost));
  if (tr->m) tr->m[oi] = m;
  // the first `cnt` of a device array into the record's kMaxWS entries, the rest `fill`
  auto padded = [&](auto* dst, const auto* src, int cnt, auto fill) -> int {
    if (!dst) return SVM_OK;
    SVMD_CHECK(hipMemcpy(dst + oi * kMaxWS, src, size_t(cnt) * sizeof(*dst), hipMemcpyDeviceToHost));
    std::fill(dst + oi * kMaxWS + cnt, dst + (oi + 1) * kMaxWS, fill);
    return SVM_OK;
  };
  if (tr->moved) tr->moved[oi] = mv;
  if (padded(tr->W, w.W, m, -1) || padded(tr->cols, w.cols, mv, -1) || padded(tr->coef, w.coef, mv, 0.0))
    return SVM_ERR_DEVICE;
  if (tr->inner) tr->inner[oi] = c.last_inner_it;
  if (tr->bounds) {
    tr->bounds[2 * oi] = c.b_high;
    tr->bounds[2 * oi + 1] = c.b_low;
  }
  if (tr->n == n && tr->alpha) SVMD_CHECK(hipMemcpy(tr->alpha + oi * n, S.alpha, size_t(n) * 8, hipMemcpyDeviceToHost));
  if (tr->n == n && tr->f) {
    SVMD_CHECK(hipMemcpy(tr->f + oi * n, w.f, size_t(n) * 8, hipMemcpyDeviceToHost));
    if (w.shr) {  // shrunk rows: NaN (their f is not part of the trajectory; the oracle's trace agrees)
      std::vector<uint8_t> sh_h(static_cast<size_t>(n));
      SVMD_CHECK(hipMemcpy(sh_h.data(), w.shr, size_t(n), hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < n; ++i)
        if (sh_h[size_t(i)]) tr->f[oi * n + i] = __builtin_nan("");
    }
  }
  return SVM_OK;
}

// The stopped solve's result, statistics (see run_decomp) and, from the PROF build, its phase totals.
int finish_solve(const Solve& S, const PackState& ps, const DecompCtl& fin, int64_t warm_cols, svm_result* r,
                 int64_t* stats) {
  if (fin.stop == kStopInternal) {
    set_error("decomposition SMO: working set outside [2, %d] points", kMaxWS);
    return SVM_ERR_INTERNAL;
  }
  const DecompHost* hs = S.hs;
  if (S.k.prof && fin.inner_total > 0) {
    const double it = double(fin.inner_total);
    fprintf(stderr, "decomp prof (clock64 ticks / inner iteration): select %.0f  publish+barrier %.0f  merge %.0f  "
            "row loads %.0f  update %.0f  (%lld iterations; inner kernels %.3f ms wall = %lld clock64 ticks)\n",
            hs->prof[0] / it, hs->prof[1] / it, hs->prof[2] / it,
            (hs->prof[3] + hs->prof[8] + hs->prof[9] + hs->prof[10] + hs->prof[11]) / it, hs->prof[4] / it,
            (long long)fin.inner_total, hs->prof[7] / 1e5, (long long)hs->prof[6]);
    if (S.k.wss2)
      fprintf(stderr, "decomp prof second-order j (inside row loads): row i %.0f  gains + wave reduction %.0f  "
              "publish + barrier %.0f  fold %.0f  row j %.0f\n", hs->prof[8] / it, hs->prof[9] / it,
              hs->prof[10] / it, hs->prof[11] / it, hs->prof[3] / it);
  }
  if (stats) {
    stats[0] = fin.outer;
    stats[1] = fin.inner_total;
    stats[2] = S.sh.L;  // the working-set capacity actually used (see decomp_shape)
    stats[3] = int64_t(ms_since(S.t0) * 1000.0);
    stats[4] = fin.changed_total;
    stats[5] = S.k.inner_nt;
    stats[6] = S.f64 ? 1 : 0;
    stats[7] = warm_cols;
    stats[8] = ps.unshrinks;
    stats[9] = fin.passes;
    stats[10] = ps.min_active;
    stats[11] = ps.repacks;
    stats[12] = fin.newton_steps;
  }
  if (r) {
    r->iterations = fin.inner_total + 1;
    r->b_high = fin.b_high;
    r->b_low = fin.b_low;
    r->b = (fin.b_high + fin.b_low) / 2;
    r->stop_reason = fin.stop;
    r->reserved = 0;
    r->n_sv = -1;
    r->seconds = ms_since(S.t0) / 1e3;
  }
  return SVM_OK;
}

}  // namespace

// Decomposition solve on quantised rows (Q, N0, WN: all n rows; the plan's step weights in stw on the
// device) or on FP64 rows (DecompRows).  alpha: n doubles (cold start: zeroed here).  q: working-set size
// (<= 1024).
// Distributed (world > 1): this GPU owns the blocks [rank NB / world, (rank + 1) NB / world) of the
// selection's global block partition, keeps f for their points only, and exchanges its candidate
// records once per outer iteration through `allgather`; every GPU then builds the same working set and
// runs the same inner solve on the same inputs (alpha is replicated and updated identically), and
// updates f for its own points.  With world dividing 8 the trajectory is the one-GPU trajectory.
// stats (kDecompStats = SVM_DECOMP_STATS int64, 13 written): outer iterations, inner iterations, working-set
// capacity, solve microseconds, columns of the f updates (points moved, summed over the outer iterations),
// inner workgroup size, kernel-value path (0 exact-integer int8 MFMA, 1 FP64 MFMA), warm-start columns,
// unshrinks, shrink passes, the fewest active rows, repacks, Newton polish steps.
int run_decomp(DeviceCtx* ctx, const DecompRows& R, const int32_t* y, double* alpha, int64_t n, const svm_params& p,
               int qws, svm_result* r, int64_t* stats, const DecompOpts& o) {
  Solve S;
  S.t0 = std::chrono::steady_clock::now();
  int rc = setup_solve(S, ctx, R, y, alpha, n, p, qws, o);
  if (rc) return rc;
  if ((rc = alloc_solve(S, S.mode.chunked_start(o.warm)))) return rc;  // sized by the start's columns
  hipStream_t s = S.s;
  svm_decomp_trace* tr = S.tr;
  PackState ps(S.nloc);
  int64_t warm_cols = 0;
  if ((rc = start_solve(S, ps, o.warm, &warm_cols))) return rc;
  if (tr) tr->count = 0;
  // Outer iterations are enqueued `batch` at a time (SVM355_DECOMP_BATCH, default 1): every kernel reads
  // the device control block, so after the stop the rest are no-op launches.  Each batch's last kernel
  // publishes the control block to the host and an event follows it; the host waits for batch k's event
  // only after it has enqueued batch k + 1, so the GPU always has the next batch queued (no idle host
  // round trip).  The trace reads every outer iteration back itself.
  const int batch = tr ? 1 : S.k.batch;
  const int64_t max_batches = p.max_iter / std::max(1, batch) + 64;  // a stop comes well before: never spin
  SoloTimer solo{(S.world > 1 && !tr) ? o.solo : nullptr, s};
  if ((rc = solo.init())) return rc;
  const DecompCtl* fin = nullptr;  // the readback that saw the stop
  bool queued = false;             // a batch is in flight whose readback the host has not checked
  for (int64_t bt = 0;; ++bt) {
    DecompCtl* pub = tr ? nullptr : S.ctl_pub + (bt & 1);  // the trace path copies the block itself
    for (int bi = 0; bi < batch; ++bi)
      if ((rc = enqueue_outer(S, ps, solo, bt * batch + bi, bi == 0, pub))) return rc;
    const DecompCtl* seen = S.ctl_h;
    hipEvent_t drain = nullptr;  // what an unshrink waits for first: the batch queued behind the one read
    if (tr) {  // trace: every outer iteration is read back before the next is enqueued
      SVMD_CHECK(hipMemcpyAsync(S.ctl_h, S.w.ctl, sizeof(DecompCtl), hipMemcpyDeviceToHost, s));
      SVMD_CHECK(hipStreamSynchronize(s));
    } else {
      SVMD_CHECK(hipEventRecord(ctx->ev_ctl[bt & 1], s));  // the batch's kernels published into ctl_h[bt & 1]
      if (!queued) {  // keep one batch queued ahead of the wait
        queued = true;
        continue;
      }
      const int64_t pb = bt - 1;
      const auto tw = std::chrono::steady_clock::now();
      if ((rc = wait_event(S, ctx->ev_ctl[pb & 1]))) return rc;
      if (o.host_wait_ms) *o.host_wait_ms += ms_since(tw);
      seen = S.ctl_h + (pb & 1);
      drain = ctx->ev_ctl[bt & 1];
    }
    if (seen->stop == kStopUnshrink) {  // batch bt ran as no-ops: drain it, unshrink, restart the pipeline
      const DecompCtl at = *seen;
      if ((rc = unshrink(S, ps, at, drain))) return rc;
      queued = false;
      continue;
    }
    if (seen->stop != SVM_STOP_RUNNING) {
      fin = seen;  // batch bt (queued) runs as no-ops; the state is final
      break;
    }
    ps.seen_active = seen->n_active;
    ps.min_active = std::min(ps.min_active, ps.seen_active);
    if (tr) {
      if ((rc = record_trace(S, *seen))) return rc;
    } else if (S.k.shrink_log) {
      fprintf(stderr, "decomp: rank %d outer %lld gap %.6g active %lld packed %lld (%.3f ms)\n", S.rank,
              (long long)seen->outer, seen->b_low - seen->b_high, (long long)ps.seen_active,
              (long long)(ps.pk >= 0 ? ps.pk_bound : S.nloc), ms_since(S.t0));
    }
    if (bt >= max_batches) {
      set_error("decomposition SMO: no stop after %lld outer iterations", (long long)seen->outer);
      return SVM_ERR_INTERNAL;
    }
  }
  if (S.mode.kind == DecompModeKind::heldout) {  // behind the queued no-op batch: the control block and f are final
    hipLaunchKernelGGL(ws_heldout_dec_kernel, dim3(unsigned((S.n + 255) / 256)), dim3(256), 0, s, S.w.f, S.mode.heldout,
                       S.n, S.w.ctl, S.mode.heldout_out);
    SVMD_LAUNCH_CHECK();
  }
  return finish_solve(S, ps, *fin, warm_cols, r, stats);
}

// ---- the fit entries ------------------------------------------------------------------------------------
namespace {

// The solve after quantisation: step weights to the device, the decomposition, the SV count.
int decomp_solve(DeviceCtx* ctx, const DecompRows& R, const int32_t* y_d, double* alpha_d, int64_t n,
                 const svm_params& p, int q, svm_result* r, int64_t* stats, const DecompOpts& o) {
  {
    TraceRange ts("svm355:decomp");
    const int rc = run_decomp(ctx, R, y_d, alpha_d, n, p, q > 0 ? q : 1024, r, stats, o);
    if (rc) return rc;
  }
  if (r) {  // twin mode: the points with a_k or a*_k above the tolerance (never both of a row at a solution)
    int64_t c = 0;
    const int rc = count_sv(ctx, alpha_d, o.mode.points(n), 1, p.sv_tol, &c);
    if (rc) return rc;
    r->n_sv = c;
  }
  return SVM_OK;
}

// The context's grow-only buffer holds the quantised rows (the solver's workspace is ctx->ws):
// Q (n x kq), N0, WN, the step weights and the quantiser's column tables (aux_bytes).
struct QuantBufs {
  int8_t* Q = nullptr;
  int32_t* N0 = nullptr;
  double *WN = nullptr, *stw = nullptr;
  void* aux = nullptr;
  DecompRows rows(const QuantPlan& P) const {  // as a solve's row source
    DecompRows R;
    R.Q = Q;
    R.N0 = N0;
    R.WN = WN;
    R.stw = stw;
    R.P = &P;
    return R;
  }
};
int decomp_quant_buffers(DeviceCtx* ctx, int64_t n, const QuantPlan& P, size_t aux_bytes, QuantBufs* b) {
  auto layout = [&](WsCarver& c) {
    b->Q = c.take<int8_t>(size_t(n) * P.kq);
    b->N0 = c.take<int32_t>(size_t(n));
    b->WN = c.take<double>(size_t(n));
    b->stw = c.take<double>(P.step_w.size());
    b->aux = c.take<char>(aux_bytes);
  };
  WsCarver size{nullptr};
  layout(size);
  const int rc = ctx->ensure_gram_bytes(size.off);
  if (rc) return rc;
  WsCarver c{reinterpret_cast<char*>(ctx->gram)};
  layout(c);
  return SVM_OK;
}

// The quantised rows' solve: the step weights to the device, then the decomposition.
int decomp_after_quant(DeviceCtx* ctx, const QuantBufs& b, const QuantPlan& P, const int32_t* y_d, double* alpha_d,
                       int64_t n, const svm_params& p, int q, svm_result* r, int64_t* stats, const DecompOpts& o) {
  SVMD_CHECK(hipMemcpyAsync(b.stw, P.step_w.data(), P.step_w.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  return decomp_solve(ctx, b.rows(P), y_d, alpha_d, n, p, q, r, stats, o);
}

}  // namespace

// The same solve from scaled FP64 rows (X_d: n x ld, the reference's host format, already min-max
// scaled on the device with mn_h / mx_h): quantize_rows produces the same Q, N0, WN as the uint8
// path, so the trajectory and the model are the uint8 path's.  Rows whose statistics admit no
// exact-integer plan (real-valued data; SVM355_DECOMP_F64=1 forces it) are solved on the FP64 rows
// themselves, every kernel value on FP64 MFMA (gram_mfma.hip) -- gpu_svm_main3.cu:119-147's RBF on
// arbitrary doubles.
int decomp_fit_rows(DeviceCtx* ctx, const double* X_d, int64_t n, int64_t ld, int64_t d, const double* mn_h,
                    const double* mx_h, const int32_t* y_d, double* alpha_d, const svm_params& p, int q, svm_result* r,
                    int64_t* stats, bool* used, double* prep_ms, const DecompOpts& o) {
  const auto t0 = std::chrono::steady_clock::now();
  *used = false;
  if (!decomp_shape(o.mode.points(n), q, o.world).ok) return SVM_OK;  // beyond the solver's shapes: the caller's fallback
  const char* fe = getenv("SVM355_DECOMP_F64");
  const bool force_f64 = fe && atoi(fe) == 1;
  QuantPlan P;
  if (!force_f64 && mn_h && mx_h && plan_quant(mn_h, mx_h, d, &P) && P.kq <= 32 * 128) {
    QuantBufs b;
    int rc = decomp_quant_buffers(ctx, n, P, quantize_aux_bytes(P), &b);
    if (rc) return rc;
    bool ok = false;
    {
      TraceRange tr("svm355:quantise");
      rc = quantize_rows(ctx->stream, X_d, n, ld, P, b.aux, b.Q, b.N0, b.WN, &ok);
      if (rc) return rc;
    }
    if (ok) {
      if (prep_ms) *prep_ms = ms_since(t0);
      rc = decomp_after_quant(ctx, b, P, y_d, alpha_d, n, p, q, r, stats, o);
      if (rc) return rc;
      *used = true;
      return SVM_OK;
    }
  }
  if (ld % 16 != 0 || ld < d) return SVM_OK;  // the FP64 block kernel's k-steps
  // The FP64-row solve keeps the moved columns' block K(rows, <= 1024 columns) per f update: n x 1024
  // doubles of workspace (8 GB at 1M rows).  When that does not fit 80 % of what the device has free
  // (plus the context's current workspace, which it would replace), nothing runs (*used = false) and
  // the caller takes the pairwise solver (SVC(solver="auto")).
  {
    size_t free_b = 0, total_b = 0;
    SVMD_CHECK(hipMemGetInfo(&free_b, &total_b));
    const double need = double(n) / double(std::max(1, o.world)) * double(kMaxWS) * 8.0 +
                        double(size_t(kMaxWS) * ld * 16);  // this GPU's rows (distributed: ~n / world)
    if (need > 0.8 * double(free_b + ctx->ws_bytes)) return SVM_OK;
  }
  // FP64 rows: their squared norms in the context's grow-only buffer, then the solve
  int rc = ctx->ensure_gram_bytes(size_t(n) * 8);
  if (rc) return rc;
  auto* nrm = reinterpret_cast<double*>(ctx->gram);
  rc = launch_scale_norms(ctx->stream, const_cast<double*>(X_d), n, d, ld, nullptr, nullptr, nrm);
  if (rc) return rc;
  if (prep_ms) *prep_ms = ms_since(t0);
  DecompRows R;
  R.X = X_d;
  R.nrm = nrm;
  R.ld = ld;
  rc = decomp_solve(ctx, R, y_d, alpha_d, n, p, q, r, stats, o);
  if (rc) return rc;
  *used = true;
  return SVM_OK;
}

int decomp_fit_u8(DeviceCtx* ctx, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h, const double* mx_h,
                  const int32_t* y_d, double* alpha_d, const svm_params& p, int q, svm_result* r, int64_t* stats,
                  bool* used, double* prep_ms, const DecompOpts& o) {
  const auto t0 = std::chrono::steady_clock::now();
  *used = false;
  // outside the solver's shapes (n < 2 or n >= 2^31 - 1, decomp_shape): nothing runs, the caller takes
  // the pairwise solver (SVC(solver="auto"))
  if (!decomp_shape(o.mode.points(n), q, o.world).ok) return SVM_OK;
  QuantPlan P;
  if (!plan_quant(mn_h, mx_h, d, &P) || P.kq > 32 * 128) return SVM_OK;  // igram's LDS table bound
  QuantBufs b;
  int rc = decomp_quant_buffers(ctx, n, P, quantize_u8_aux_bytes(P), &b);
  if (rc) return rc;
  bool ok = false;
  {
    TraceRange tr("svm355:quantise");
    rc = quantize_u8_rows(ctx->stream, Xu_d, n, d, mn_h, mx_h, P, b.aux, b.Q, b.N0, b.WN, &ok);
    if (rc) return rc;
  }
  if (!ok) return SVM_OK;
  if (prep_ms) *prep_ms = ms_since(t0);
  rc = decomp_after_quant(ctx, b, P, y_d, alpha_d, n, p, q, r, stats, o);
  if (rc) return rc;
  *used = true;
  return SVM_OK;
}

namespace {

// The C entries' one body after their argument checks: uint8 rows (X_d n x d) or min-max scaled FP64 rows
// (X_d n x ld), the parameters or the defaults, the fit between the context's stream joins, the timing.
// What the mode refuses is SVM_ERR_ARG under the entry's name (`who`) before the context's stream is joined:
// nothing is enqueued.  (setup_solve makes the same call for the solves that do not come through here.)
int train_decomp(DeviceCtx* ctx, const char* who, const void* X_d, bool is_u8, int64_t n, int64_t ld, int64_t d, const double* mn_h,
                 const double* mx_h, const int32_t* y_d, double* alpha_d, const svm_params* pp, int32_t q,
                 const DecompOpts& o, svm_result* r, svmd_timing* timing, int64_t* stats, int32_t* used_out) {
  const svm_params p = params_or_default(pp);
  DecompFeatures ft;
  int rc = mode_features(o, p, &ft);
  if (rc || (rc = decomp_mode_check(who, o.mode, y_d, ft, n, DecompBackend::device))) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  if ((rc = ctx->begin())) return rc;
  bool used = false;
  double prep = 0.0;
  rc = is_u8 ? decomp_fit_u8(ctx, static_cast<const uint8_t*>(X_d), n, d, mn_h, mx_h, y_d, alpha_d, p, q, r, stats,
                             &used, &prep, o)
             : decomp_fit_rows(ctx, static_cast<const double*>(X_d), n, ld, d, mn_h, mx_h, y_d, alpha_d, p, q, r,
                               stats, &used, &prep, o);
  if (rc) return rc;
  if (used && timing) {
    timing->gram_ms = prep;  // quantisation only: no Gram is stored
    timing->total_ms = ms_since(t0);
    timing->smo_ms = timing->total_ms - prep;
  }
  if (used_out) *used_out = used ? 1 : 0;
  return ctx->end();
}

}  // namespace

}  // namespace svm355

using namespace svm355;

// ---- the C ABI ------------------------------------------------------------------------------------------
extern "C" {

// Decomposition SMO straight from uint8 pixel rows (exact-integer kernel values, no stored Gram).
// *used = 0 and nothing done when the rows' statistics do not admit the integer plan.  stats
// (optional, SVM_DECOMP_STATS int64): see run_decomp.
SVM_API int svmd_train_decomp_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h,
                                 const double* mx_h, const int32_t* y_d, double* alpha_d, const svm_params* pp,
                                 int32_t q, svm_result* r, svmd_timing* timing, int64_t* stats, int32_t* used_out) {
  SVMD_CTX(h);
  if (used_out) *used_out = 0;
  if (!Xu_d || n < 2 || d <= 0 || !mn_h || !mx_h || !y_d || !alpha_d) {
    set_error("svmd_train_decomp_u8: bad arguments");
    return SVM_ERR_ARG;
  }
  return train_decomp(ctx, "svmd_train_decomp_u8", Xu_d, true, n, 0, d, mn_h, mx_h, y_d, alpha_d, pp, q, {}, r, timing, stats, used_out);
}

// The same solve from min-max scaled FP64 rows on the device (X_d: n x ld; mn_h / mx_h the training
// statistics they were scaled with): quantised into the same integers as the uint8 path, so the
// trajectory and the model are identical.  *used = 0 when the values admit no exact-integer plan.
SVM_API int svmd_train_decomp_rows(void* h, const double* X_d, int64_t n, int64_t ld, int64_t d, const double* mn_h,
                                   const double* mx_h, const int32_t* y_d, double* alpha_d, const svm_params* pp,
                                   int32_t q, svm_result* r, svmd_timing* timing, int64_t* stats, int32_t* used_out) {
  SVMD_CTX(h);
  if (used_out) *used_out = 0;
  if (!X_d || n < 2 || d <= 0 || ld < d || !mn_h || !mx_h || !y_d || !alpha_d) {
    set_error("svmd_train_decomp_rows: bad arguments");
    return SVM_ERR_ARG;
  }
  return train_decomp(ctx, "svmd_train_decomp_rows", X_d, false, n, ld, d, mn_h, mx_h, y_d, alpha_d, pp, q, {}, r, timing, stats, used_out);
}

// The general entries' one body: the arguments they all take checked (own_ok: the entry's own pointers), then the
// fit in the entry's mode.  *used = 0 and nothing done without an exact-integer plan.
static int train_decomp_entry(const char* who, void* h, const void* X_d, int32_t is_u8, int64_t n, int64_t ld,
                              int64_t d, const double* mn_h, const double* mx_h, bool own_ok, const int32_t* y_d,
                              double* alpha_d, const svm_params* pp, int32_t q, DecompOpts o, svm_result* r,
                              svmd_timing* timing, int64_t* stats, int32_t* used_out, svm_decomp_trace* trace) {
  SVMD_CTX(h);
  if (used_out) *used_out = 0;
  if (!X_d || n < 2 || d <= 0 || (!is_u8 && ld < d) || !mn_h || !mx_h || !alpha_d || !own_ok) {
    set_error("%s: bad arguments", who);
    return SVM_ERR_ARG;
  }
  o.trace = trace;
  return train_decomp(ctx, who, X_d, is_u8 != 0, n, ld, d, mn_h, mx_h, y_d, alpha_d, pp, q, o, r, timing, stats,
                      used_out);
}

// The general entry: uint8 rows (is_u8, X_d n x d) or min-max scaled FP64 rows (X_d n x ld), cold or
// warm start (alpha_d holds the start), an optional per-outer-iteration trace (tests: one
// synchronisation per outer iteration).
SVM_API int svmd_train_decomp(void* h, const void* X_d, int32_t is_u8, int64_t n, int64_t ld, int64_t d,
                              const double* mn_h, const double* mx_h, const int32_t* y_d, double* alpha_d,
                              const svm_params* pp, int32_t q, int32_t warm, svm_result* r, svmd_timing* timing,
                              int64_t* stats, int32_t* used_out, svm_decomp_trace* trace) {
  DecompOpts o;
  o.warm = warm != 0;
  return train_decomp_entry("svmd_train_decomp", h, X_d, is_u8, n, ld, d, mn_h, mx_h, y_d != nullptr, y_d, alpha_d, pp,
                            q, o, r, timing, stats, used_out, trace);
}

// The regression (epsilon-SVR) form of svmd_train_decomp: twin mode (decomp_mode.h) over the n rows and the n
// targets z_d (device FP64).  alpha_d: 2n doubles, out -- a (first n), then a* (last n); the model is beta =
// a - a*, a prediction sum_k beta_k K(x_k, x) - r->b.  r->n_sv counts the points of either half above sv_tol.
// A trace's W / cols / coef hold virtual ids (k and k + n) and its snapshots are 2n long (trace->n = 2n).  Cold
// start, one GPU; shrinking, the Newton polish and class weights in *pp are SVM_ERR_ARG, as is 2n > 2^31 - 1.
SVM_API int svmd_train_decomp_svr(void* h, const void* X_d, int32_t is_u8, int64_t n, int64_t ld, int64_t d,
                                  const double* mn_h, const double* mx_h, const double* z_d, double epsilon,
                                  double* alpha_d, const svm_params* pp, int32_t q, svm_result* r, svmd_timing* timing,
                                  int64_t* stats, int32_t* used_out, svm_decomp_trace* trace) {
  DecompOpts o;
  o.mode.kind = DecompModeKind::twin;
  o.mode.twin_z = z_d;
  o.mode.twin_eps = epsilon;
  return train_decomp_entry("svmd_train_decomp_svr", h, X_d, is_u8, n, ld, d, mn_h, mx_h, z_d != nullptr, nullptr,
                            alpha_d, pp, q, o, r, timing, stats, used_out, trace);
}

// The one-class form of svmd_train_decomp (LIBSVM's -s 2; svm355.h has the problem): one-class mode
// (decomp_mode.h) over the n rows.  alpha_d: n doubles, out; r->b is rho, and a decision value is sum_k alpha_k
// K(x_k, x) - rho.  The same row paths and *used contract as svmd_train_decomp_svr.  pp->C is not read (the box
// is 1).  stats[7]: the start's columns.  One GPU; shrinking, the Newton polish and class weights in *pp are
// SVM_ERR_ARG, as is nu outside (0, 1).
SVM_API int svmd_train_decomp_oneclass(void* h, const void* X_d, int32_t is_u8, int64_t n, int64_t ld, int64_t d,
                                       const double* mn_h, const double* mx_h, double nu, double* alpha_d,
                                       const svm_params* pp, int32_t q, svm_result* r, svmd_timing* timing,
                                       int64_t* stats, int32_t* used_out, svm_decomp_trace* trace) {
  DecompOpts o;
  o.mode.kind = DecompModeKind::oneclass;
  o.mode.oneclass_nu = nu;
  return train_decomp_entry("svmd_train_decomp_oneclass", h, X_d, is_u8, n, ld, d, mn_h, mx_h, true, nullptr, alpha_d,
                            pp, q, o, r, timing, stats, used_out, trace);
}

// The held-out form of svmd_train_decomp (svm355_device.h): held-out mode (decomp_mode.h) over the n rows.
SVM_API int svmd_train_decomp_heldout(void* h, const void* X_d, int32_t is_u8, int64_t n, int64_t ld, int64_t d,
                                      const double* mn_h, const double* mx_h, const int32_t* y_d,
                                      const uint8_t* heldout_d, double* alpha_d, double* dec_out_d,
                                      const svm_params* pp, int32_t q, svm_result* r, svmd_timing* timing,
                                      int64_t* stats, int32_t* used_out, svm_decomp_trace* trace) {
  DecompOpts o;
  o.mode.kind = DecompModeKind::heldout;
  o.mode.heldout = heldout_d;
  o.mode.heldout_out = dec_out_d;
  return train_decomp_entry("svmd_train_decomp_heldout", h, X_d, is_u8, n, ld, d, mn_h, mx_h,
                            y_d && heldout_d && dec_out_d, y_d, alpha_d, pp, q, o, r, timing, stats, used_out, trace);
}

// The decomposition solver's f update alone (tests): the uint8 rows quantised as a solve would, then
// f_out[i] = sum_k coef[k] K(lo + i, cols[k]) over k < m for the rows [lo, lo + nloc) -- the solver's own
// f_update from f = 0 with the device-side count m, on the GEMV (its partial halves summed in order) or,
// with SVM355_GEMV_VIA_CACHE set, on a fresh column cache of m persistent slots (every column a miss: the
// narrow store up to 64 columns, the tiled one beyond; then the reader).  cols / coef / f_out are host
// arrays; m <= 1024.  *used = 0 without an exact plan.
// Twin mode (twin: svmd_decomp_twin_step_u8): lo = 0 and nloc = n, cols_h holds virtual ids in [0, 2n), f_out
// is 2n long and holds the start on entry; the list is folded on the device (ws_twin_fold_kernel) and the
// update adds every row's sum to both of its points.
static int gemv_probe_u8(DeviceCtx* ctx, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h,
                         const double* mx_h, double gamma, int64_t lo, int64_t nloc, const int32_t* cols_h,
                         const double* coef_h, int32_t m, double* f_out, int32_t* used_out, bool twin) {
  const char* who = twin ? "svmd_decomp_twin_step_u8" : "svmd_decomp_gemv_u8";
  if (used_out) *used_out = 0;
  if (!Xu_d || n < 1 || d <= 0 || lo < 0 || nloc < 1 || lo + nloc > n || m < 1 || m > kMaxWS || !cols_h || !coef_h ||
      !f_out || (twin && (lo != 0 || nloc != n || 2 * n > int64_t(INT32_MAX)))) {
    set_error("%s: bad arguments", who);
    return SVM_ERR_ARG;
  }
  for (int k = 0; k < m; ++k)
    if (cols_h[k] < 0 || cols_h[k] >= (twin ? 2 * n : n)) {
      set_error("%s: column %d out of range", who, cols_h[k]);
      return SVM_ERR_ARG;
    }
  if (twin)  // a point is listed once (the inner solve's moved list): the fold pairs k with k + n only
    for (int k = 0; k < m; ++k)
      for (int q = 0; q < k; ++q)
        if (cols_h[q] == cols_h[k]) {
          set_error("%s: point %d listed twice", who, cols_h[k]);
          return SVM_ERR_ARG;
        }
  int rc = ctx->begin();
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  QuantPlan P;
  if (!plan_quant(mn_h, mx_h, d, &P) || P.kq > 32 * 128) return ctx->end();
  QuantBufs b;
  rc = decomp_quant_buffers(ctx, n, P, quantize_u8_aux_bytes(P), &b);
  if (rc) return rc;
  bool ok = false;
  rc = quantize_u8_rows(s, Xu_d, n, d, mn_h, mx_h, P, b.aux, b.Q, b.N0, b.WN, &ok);
  if (rc) return rc;
  if (!ok) return ctx->end();
  SVMD_CHECK(hipMemcpyAsync(b.stw, P.step_w.data(), P.step_w.size() * 8, hipMemcpyHostToDevice, s));
  Solve S;  // what f_update reads of a solve: the rows, the slice, gamma, the cache and the update's buffers
  S.ctx = ctx;
  S.s = s;
  S.R = b.rows(P);
  S.kq = P.kq;
  S.n = twin ? 2 * n : n;
  S.lo = lo;
  S.nloc = twin ? 2 * n : nloc;
  S.mode.kind = twin ? DecompModeKind::twin : DecompModeKind::classify;
  S.nrow = n;
  S.p.gamma = gamma;
  const char* vc = getenv("SVM355_GEMV_VIA_CACHE");
  const bool via_cache = vc && atoi(vc) != 0;
  if (via_cache) {
    S.cc.cap = m;
    S.cc.ld = (nloc + 3) & ~int64_t(3);
    S.cc.slab = ctx->ensure_rc_cache(size_t(m + kMaxWS) * S.cc.ld * 8);
    if (!S.cc.slab) {
      set_error("%s: no memory for the column cache", who);
      return SVM_ERR_DEVICE;
    }
  }
  DecompWs& w = S.w;
  rc = carve_ws(ctx, [&](WsCarver& c) {
    w.cols = c.take<int32_t>(kMaxWS);
    w.coef = c.take<double>(kMaxWS);
    w.mcount = c.take<int32_t>(64);
    w.f = c.take<double>(size_t(S.nloc));
    w.part = c.take<double>(size_t(nloc) * kLdp, !via_cache);
    w.cslot = c.take<int32_t>(size_t(n), via_cache);
    w.crd = c.take<int32_t>(kMaxWS, via_cache);
    w.cmid = c.take<int32_t>(kMaxWS, via_cache);
    w.cmsl = c.take<int32_t>(kMaxWS, via_cache);
    w.cst = c.take<int32_t>(64, via_cache);
    w.fcols = c.take<int32_t>(kMaxWS, twin);
    w.fcoef = c.take<double>(kMaxWS, twin);
    w.fcount = c.take<int32_t>(64, twin);
  });
  if (rc) return rc;
  SVMD_CHECK(hipMemcpyAsync(w.cols, cols_h, size_t(m) * 4, hipMemcpyHostToDevice, s));
  SVMD_CHECK(hipMemcpyAsync(w.coef, coef_h, size_t(m) * 8, hipMemcpyHostToDevice, s));
  SVMD_CHECK(hipMemcpyAsync(w.mcount, &m, 4, hipMemcpyHostToDevice, s));
  if (twin)
    SVMD_CHECK(hipMemcpyAsync(w.f, f_out, size_t(S.nloc) * 8, hipMemcpyHostToDevice, s));
  else
    SVMD_CHECK(hipMemsetAsync(w.f, 0, size_t(nloc) * 8, s));
  if ((rc = cache_reset(S))) return rc;
  if (twin) {
    hipLaunchKernelGGL(ws_twin_fold_kernel, dim3(1), dim3(kMaxWS), 0, s, w.cols, w.coef, w.mcount, n, w.fcols, w.fcoef,
                       w.fcount);
    SVMD_LAUNCH_CHECK();
    rc = f_update(S, PackState(nloc), w.fcols, w.fcoef, w.fcount);
  } else {
    rc = f_update(S, PackState(nloc), w.cols, w.coef, w.mcount);
  }
  if (rc) return rc;
  SVMD_CHECK(hipMemcpyAsync(f_out, w.f, size_t(S.nloc) * 8, hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipStreamSynchronize(s));
  if (used_out) *used_out = 1;
  return ctx->end();
}

SVM_API int svmd_decomp_gemv_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h,
                                const double* mx_h, double gamma, int64_t lo, int64_t nloc, const int32_t* cols_h,
                                const double* coef_h, int32_t m, double* f_out, int32_t* used_out) {
  SVMD_CTX(h);
  return gemv_probe_u8(ctx, Xu_d, n, d, mn_h, mx_h, gamma, lo, nloc, cols_h, coef_h, m, f_out, used_out, false);
}

// The twin mode's fold and f update alone (tests): cols_h / coef_h = a moved list of m <= 1024 distinct virtual
// ids in [0, 2n) (k: a_k, k + n: a*_k), f_io = the 2n points' f (host, in and out).  The list is folded on the
// device to one entry per kernel row and f_io[k] and f_io[k + n] both take row k's sum, computed once over the
// n rows by the solver's own f_update (the GEMV, or the column cache with SVM355_GEMV_VIA_CACHE).
SVM_API int svmd_decomp_twin_step_u8(void* h, const uint8_t* Xu_d, int64_t n, int64_t d, const double* mn_h,
                                     const double* mx_h, double gamma, const int32_t* cols_h, const double* coef_h,
                                     int32_t m, double* f_io, int32_t* used_out) {
  SVMD_CTX(h);
  return gemv_probe_u8(ctx, Xu_d, n, d, mn_h, mx_h, gamma, 0, n, cols_h, coef_h, m, f_io, used_out, true);
}

// One Newton polish step (decomp_newton.h) on the device for a host working set (tests / timing): Kw_h
// (m x m), y_h, a_h / f_h by position (overwritten with the result); *code = 0 / 1 / 2; prof (optional, 8
// int64): wall-clock stamps of the phases (free set, K_FF, factorisation, back substitution, step, f) of
// the last of `reps` runs (each from the same inputs), ticks at 100 MHz, then |F| (prof[6]; the stamps are
// zeroed before every run, so a refused step leaves |F| = 0); ms_out: the mean time per step.  threads: the
// workgroup's size, 64 / 128 / 256 / 512 (the inner solve's shapes); max_free above kNewtonMaxFree is capped.
SVM_API int svmd_decomp_newton_probe_nt(void* h, const double* Kw_h, const int32_t* y_h, int32_t m, double* a_h,
                                        double* f_h, double C, double eps, int32_t max_free, int32_t reps,
                                        int32_t threads, int32_t* code, int64_t* prof_h, double* ms_out) {
  SVMD_CTX(h);
  if (!Kw_h || !y_h || !a_h || !f_h || !code || m < 1 || m > kMaxWS || reps < 1 || !ws_newton_probe_built(threads)) {
    set_error("svmd_decomp_newton_probe: bad arguments (1 <= m <= %d, threads 64 / 128 / 256 / 512)", kMaxWS);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  double *Kw = nullptr, *ad = nullptr, *fd = nullptr, *a0 = nullptr, *f0 = nullptr, *Ad = nullptr;
  int32_t *yd = nullptr, *cd = nullptr;
  int64_t* pd = nullptr;
  rc = carve_ws(ctx, [&](WsCarver& c) {
    Kw = c.take<double>(size_t(kMaxWS) * kMaxWS);
    yd = c.take<int32_t>(kMaxWS);
    ad = c.take<double>(kMaxWS);
    fd = c.take<double>(kMaxWS);
    a0 = c.take<double>(kMaxWS);
    f0 = c.take<double>(kMaxWS);
    cd = c.take<int32_t>(64);
    pd = c.take<int64_t>(32);
    Ad = c.take<double>(size_t(kMaxWS + 2) * kMaxWS);
  });
  if (rc) return rc;
  SVMD_CHECK(hipMemcpy2DAsync(Kw, kMaxWS * 8, Kw_h, size_t(m) * 8, size_t(m) * 8, size_t(m), hipMemcpyHostToDevice, s));
  SVMD_CHECK(hipMemcpyAsync(yd, y_h, size_t(m) * 4, hipMemcpyHostToDevice, s));
  SVMD_CHECK(hipMemcpyAsync(a0, a_h, size_t(m) * 8, hipMemcpyHostToDevice, s));
  SVMD_CHECK(hipMemcpyAsync(f0, f_h, size_t(m) * 8, hipMemcpyHostToDevice, s));
  hipEvent_t e0, e1;
  SVMD_CHECK(hipEventCreate(&e0));
  SVMD_CHECK(hipEventCreate(&e1));
  float tot = 0.0f;
  for (int r = 0; r < reps; ++r) {
    SVMD_CHECK(hipMemcpyAsync(ad, a0, size_t(m) * 8, hipMemcpyDeviceToDevice, s));
    SVMD_CHECK(hipMemcpyAsync(fd, f0, size_t(m) * 8, hipMemcpyDeviceToDevice, s));
    SVMD_CHECK(hipMemsetAsync(pd, 0, 32 * sizeof(int64_t), s));
    SVMD_CHECK(hipEventRecord(e0, s));
    if ((rc = launch_ws_newton_probe(s, threads, m, Kw, int64_t(kMaxWS), yd, ad, fd, Ad, C, eps, max_free, cd, pd)))
      return rc;
    SVMD_LAUNCH_CHECK();
    SVMD_CHECK(hipEventRecord(e1, s));
    SVMD_CHECK(hipEventSynchronize(e1));
    float ms = 0.0f;
    SVMD_CHECK(hipEventElapsedTime(&ms, e0, e1));
    tot += ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  SVMD_CHECK(hipMemcpyAsync(a_h, ad, size_t(m) * 8, hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipMemcpyAsync(f_h, fd, size_t(m) * 8, hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipMemcpyAsync(code, cd, 4, hipMemcpyDeviceToHost, s));
  if (prof_h) SVMD_CHECK(hipMemcpyAsync(prof_h, pd, 16 * 8, hipMemcpyDeviceToHost, s));
  SVMD_CHECK(hipStreamSynchronize(s));
  if (ms_out) *ms_out = double(tot) / reps;
  return ctx->end();
}

// The probe in a 256-thread workgroup (the inner solve's default shape).
SVM_API int svmd_decomp_newton_probe(void* h, const double* Kw_h, const int32_t* y_h, int32_t m, double* a_h,
                                     double* f_h, double C, double eps, int32_t max_free, int32_t reps, int32_t* code,
                                     int64_t* prof_h, double* ms_out) {
  return svmd_decomp_newton_probe_nt(h, Kw_h, y_h, m, a_h, f_h, C, eps, max_free, reps, 256, code, prof_h, ms_out);
}

}  // extern "C"

SVMD_TU_WARM(decomp)
