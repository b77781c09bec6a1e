// The modes of the working-set decomposition solver and what each refuses: one descriptor and one table that
// the device driver (hip/decomp.hip) and its CPU oracle (core/decomp_cpu.cpp) share.  Host-only C++ with no
// HIP headers.  A mode is one kind, so two modes cannot be combined; a new mode is one row of the table here
// and one arm of the switches over `kind` in the two solvers.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include "decomp_newton.h"
#include "decomp_shrink.h"
#include "kfun.h"
#include "svm355.h"

namespace svm355 {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

enum class DecompModeKind { classify, twin, oneclass, heldout, nu_classify, nu_twin };
enum class DecompBackend { device, cpu_oracle };

// What a solve is of, beyond the classifier's n labelled points.  n rows go in as always.
//   * twin (epsilon-SVR): twin_z = the n targets (on the device for the device solver), twin_eps = the tube's
//     half width.  The solve runs over 2n virtual points that share the n kernel rows -- point k is a_k with
//     sign +1, point k + n its twin a*_k with sign -1, both on row k -- from f_k = eps - z_k, f_{k+n} = -eps -
//     z_k.  It reads no y (it keeps the signs itself), and alpha holds 2n values: a, then a*.
//   * oneclass (LIBSVM's -s 2; svm355.h has the problem): 0 < oneclass_nu < 1.  Every sign is +1, the box is 1
//     (p.C is not read), there is no linear term, and the solve starts from LIBSVM's feasible alpha
//     (svm_oneclass_start) with f = K[:, nz] alpha_nz summed by the chunked start.  It reads no y, and alpha
//     holds n values (out).
//   * heldout (svm355.h): heldout = uint8[n], 1 = point i is out of the fit.  The solve keeps its own signs (0
//     on the held-out points: never selected, alpha exactly 0, f collecting every update) and does not read the
//     caller's y after the start.  heldout_out = n doubles, out: on the device f_i - b for the held-out points
//     after the last outer iteration and 0.0 for the others; on the oracle the final f of every point, optional.
//     The training part must hold both classes (the caller checks).
//   * nu_classify (LIBSVM's -s 1, nu-SVC) and nu_twin (-s 4, nu-SVR; svm355.h has both problems): 0 < nu <= 1.  Two
//     equalities (y'a = 0 and e'a = const), so a step moves a pair of points of one sign, the stop test is the larger
//     of the two per-class gaps, and two multipliers come out: nu_out (2 doubles, host, out) = {r, rho}.  nu_classify
//     reads the caller's y for its start (each class walked in ascending index, a_i = min(1, what is left of nu n /
//     2); box 1, p.C is not read; f = K[:, nz] (a y)_nz by the chunked start) and keeps signs of its own; at the end
//     alpha is divided by r.  nu_twin is twin's layout with twin_z the targets: a_k = a*_k = min(C, what is left of
//     C nu n / 2), f_k = f_{k+n} = -z_k.  The kernels of these two modes are decomp_nu.hip's.
struct DecompMode {
  DecompModeKind kind = DecompModeKind::classify;
  const double* twin_z = nullptr;
  double twin_eps = 0.0;
  double oneclass_nu = 0.0;
  double nu = 0.0;
  int64_t nu_npos = -1;  // nu_classify on the device: how many labels are +1 (the caller counts its host labels)
  double* nu_out = nullptr;
  const uint8_t* heldout = nullptr;
  double* heldout_out = nullptr;
  // sample weights (classify and twin only): one weight >= 0 per kernel row, on the device for the device solver.
  // Row k's box is (C w_class(y_k)) w_k -- the class box of svm_class_boxes times the weight, in that order -- and in
  // twin mode both points of row k have it.  A weight of 0 freezes the point at alpha = 0 (it is on neither side
  // of any selection) while its f still collects every update.  The device's kernels are decomp_box.hip's.
  const double* sample_w = nullptr;
  bool boxed() const { return sample_w != nullptr; }
  bool twin() const { return kind == DecompModeKind::twin || kind == DecompModeKind::nu_twin; }
  // the same-sign-pair modes: four candidate lists, two gaps, decomp_nu.hip's select / build / inner kernels
  bool nu_pairs() const { return kind == DecompModeKind::nu_classify || kind == DecompModeKind::nu_twin; }
  // the solve keeps its own signs (its y is not the caller's)
  bool own_signs() const { return kind != DecompModeKind::classify; }
  // the start sums f over the nonzero alphas in chunks, as a warm start does (sized as one)
  bool chunked_start(bool warm) const {
    return warm || kind == DecompModeKind::oneclass || kind == DecompModeKind::nu_classify;
  }
  // the points the solve selects among, over nrow kernel rows
  int64_t points(int64_t nrow) const { return twin() ? 2 * nrow : nrow; }
};

// What a solve is asked to run with.  weighted: the classifier's two boxes differ (equal weights only scale
// C); for the other kinds, any class weight is set.
struct DecompFeatures {
  bool distributed = false, warm = false, shrinking = false, newton = false, weighted = false;
  bool boxed = false;  // sample weights: a box per point (DecompMode::sample_w)
};
inline DecompFeatures decomp_features(const svm_params& p, int world, bool warm, bool weighted, bool boxed = false) {
  return {world != 1, warm, shrink_cfg(p).on, newton_cfg(p).on, weighted, boxed};
}

// What each kind refuses, per backend {device, CPU oracle}: distributed, warm, shrinking, newton, weighted.
// The classifier's row holds only on top of class weights -- what is unweighted refuses them, it never solves
// another problem in silence -- and is where the backends differ: the oracle runs weighted ranks, the device's
// distributed solve does not.  One-class mode: shrinking's unshrink rebuilds f from -y (the oracle's entry
// clears the weights, so its `weighted` is never set).  Held-out mode: shrinking's unshrink rebuilds f from
// the nonzero alphas, the polish is untested on label 0; class weights are allowed.  The nu modes: their kernels
// have one pair per iteration and one box, no shrink pass, no polish, and their start is their own.
constexpr DecompFeatures kDecompRefuses[6][2] = {
    /* classify */ {{true, false, true, true, false}, {false, false, true, true, false}},
    /* twin     */ {{true, true, true, true, true}, {true, true, true, true, true}},
    /* oneclass */ {{true, true, true, true, true}, {true, true, true, true, true}},
    /* heldout  */ {{true, true, true, true, false}, {true, true, true, true, false}},
    /* nu-SVC   */ {{true, true, true, true, true}, {true, true, true, true, true}},
    /* nu-SVR   */ {{true, true, true, true, true}, {true, true, true, true, true}},
};

// The dot-product kernels (svm_params.kernel != 0: linear, polynomial, sigmoid; kfun.h, hip/decomp_kfun.hip): the
// kinds that run with one (the classifier, class weights included, and the regression (twin) solve) and what such a
// solve refuses whatever its kind, on both backends: one GPU, a cold start, no shrinking, no polish.
constexpr bool kDecompKfunKinds[6] = {true, true, false, false, false, false};
constexpr DecompFeatures kDecompKfunRefuses = {true, true, true, true, false};

// A dot-product kernel's own arguments and everything such a solve does not cover (csr: sparse rows, which only the
// linear kernel takes: hip/csr_linear.hip): SVM_ERR_ARG with `who` as the message's prefix, before the caller does
// any work.  SVM_OK at once for the RBF.  The additive distance kernels (kernel 4, 5: laplacian, chi2;
// hip/decomp_dist.hip) run with the same kinds and refuse the same things, in the same sentences; so does a
// precomputed kernel (kernel 6: hip/decomp_gram.hip), which reads no gamma.
inline int decomp_kfun_check(const char* who, const svm_params& p, DecompModeKind kind, const DecompFeatures& f,
                             bool csr) {
  if (p.kernel == kKernelRbf) return SVM_OK;
  static const char* const name[] = {"rbf", "linear", "poly", "sigmoid", "laplacian", "chi2", "precomputed"};
  if (!kfun_params_ok(p) || (p.kernel != kKernelPrecomputed && (!(p.gamma > 0.0) || !std::isfinite(p.gamma)))) {
    set_error("%s: kernel must be 0 (rbf), 1 (linear), 2 (poly, 1 <= degree <= %d) or 3 (sigmoid) with a finite "
              "coef0, 4 (laplacian) or 5 (chi2), and gamma > 0, or 6 (precomputed: the caller's Gram) (kernel = %d, "
              "degree = %d, coef0 = %g, gamma = %g)", who, kMaxDegree, p.kernel, p.degree, p.coef0, p.gamma);
    return SVM_ERR_ARG;
  }
  const DecompFeatures& r = kDecompKfunRefuses;
  const char* what = !kDecompKfunKinds[int(kind)] ? "this mode (the classifier and the regression (twin) solve only)"
                     : csr && p.kernel != kKernelLinear ? "sparse (CSR) rows"
                     : f.distributed && r.distributed ? "the distributed solve (world > 1)"
                     : f.warm && r.warm               ? "a warm start"
                     : f.shrinking && r.shrinking     ? "shrinking"
                     : f.newton && r.newton           ? "the Newton polish (SVM355_DECOMP_NEWTON)"
                                                      : nullptr;
  if (!what) return SVM_OK;
  set_error("%s: the %s kernel does not support %s", who, name[p.kernel], what);
  return SVM_ERR_ARG;
}

// Sample weights (a box per point; hip/decomp_box.hip): the kinds that run with them (the classifier, class weights
// included, and the regression (twin) solve) and what such a solve refuses whatever its kind, on both backends: one
// GPU, a cold start, no shrinking, no polish -- and the RBF kernel on dense uint8 or FP64 rows only.
constexpr bool kDecompBoxKinds[6] = {true, true, false, false, false, false};
constexpr DecompFeatures kDecompBoxRefuses = {true, true, true, true, false};

// Everything a solve with sample weights does not cover (csr / f32 / f16: the row source): SVM_ERR_ARG with `who` as the
// message's prefix, before the caller does any work.  SVM_OK at once without weights.
inline int decomp_box_check(const char* who, const svm_params& p, DecompModeKind kind, const DecompFeatures& f, bool csr,
                            bool f32, bool f16 = false) {
  if (!f.boxed) return SVM_OK;
  const DecompFeatures& r = kDecompBoxRefuses;
  const char* what = !kDecompBoxKinds[int(kind)] ? "this mode (the classifier and the regression (twin) solve only)"
                     : p.kernel != kKernelRbf     ? "a dot-product kernel (the RBF only)"
                     : csr                        ? "sparse (CSR) rows"
                     : f32                        ? "float32 rows"
                     : f16                        ? "float16 rows"
                     : f.distributed && r.distributed ? "the distributed solve (world > 1)"
                     : f.warm && r.warm               ? "a warm start"
                     : f.shrinking && r.shrinking     ? "shrinking"
                     : f.newton && r.newton           ? "the Newton polish (SVM355_DECOMP_NEWTON)"
                                                      : nullptr;
  if (!what) return SVM_OK;
  set_error("%s: sample weights do not support %s", who, what);
  return SVM_ERR_ARG;
}

// The nu modes' selection: NB blocks of at most kNuBlockPoints points give Tc picks to each of four lists, and the
// 4 NB Tc candidates must fit one working set (SVM_DECOMP_MAX_WS): at most 256 blocks, 1,048,576 points.
constexpr int64_t kNuBlockPoints = 4096;
constexpr int64_t kNuMaxPoints = int64_t(SVM_DECOMP_MAX_WS) / 4 * kNuBlockPoints;
// LIBSVM's start walk (solve_nu_svc, solve_nu_svr) over `cap` points in ascending index: a_i = min(box, what is
// left of `total`), in its own arithmetic (repeated subtraction).  The first `full` points get the box, point
// `full` (if any) gets `frac` < box, the rest 0 -- the two numbers the device's start kernels take.
inline void nu_start_walk(double total, double box, int64_t cap, int64_t* full, double* frac) {
  double left = total;
  int64_t k = 0;
  while (k < cap && left >= box) {
    left -= box;
    ++k;
  }
  *full = k;
  *frac = k < cap ? left : 0.0;
}
// nu-SVC's feasibility: nu n / 2 of alpha per class, at most 1 per point.  Counts the caller's host labels.
inline bool nu_svc_feasible(double nu, int64_t n, int64_t n_pos, int64_t n_neg) {
  return nu * double(n) / 2.0 <= double(n_pos < n_neg ? n_pos : n_neg);
}

// The first feature the kind refuses, in this fixed order, or nullptr.
inline const char* decomp_mode_refuses(DecompModeKind kind, const DecompFeatures& f, DecompBackend backend) {
  const DecompFeatures& r = kDecompRefuses[int(kind)][int(backend)];
  if (kind == DecompModeKind::classify && !f.weighted) return nullptr;
  return f.distributed && r.distributed ? "the distributed solve (world > 1)"
         : f.warm && r.warm             ? "a warm start"
         : f.shrinking && r.shrinking   ? "shrinking"
         : f.newton && r.newton         ? "the Newton polish (SVM355_DECOMP_NEWTON)"
         : f.weighted && r.weighted     ? "class weights"
                                        : nullptr;
}

// Everything a mode does not cover, and its own arguments (y: the caller's labels, nrow: the kernel rows):
// SVM_ERR_ARG with `who` as the message's prefix, before the caller does any work.
inline int decomp_mode_check(const char* who, const DecompMode& m, const int32_t* y, const DecompFeatures& f,
                             int64_t nrow, DecompBackend backend) {
  static const char* const solve[] = {nullptr, "regression (twin)", "one-class", "held-out", "nu-SVC", "nu-SVR"};
  if (const char* what = decomp_mode_refuses(m.kind, f, backend)) {
    if (m.kind == DecompModeKind::classify)
      set_error("%s: class weights are not supported with %s", who, what);
    else
      set_error("%s: the %s solve does not support %s", who, solve[int(m.kind)], what);
    return SVM_ERR_ARG;
  }
  int64_t full;
  double frac;
  switch (m.kind) {
    case DecompModeKind::classify: break;
    case DecompModeKind::twin:
      if (!m.twin_z || !(m.twin_eps >= 0.0) || !std::isfinite(m.twin_eps) || nrow < 2 || 2 * nrow > int64_t(INT32_MAX)) {
        set_error("%s: the regression (twin) solve needs targets, a finite epsilon >= 0 and 2 <= n with 2 n <= 2^31 - 1 "
                  "(epsilon = %g, n = %lld)", who, m.twin_eps, (long long)nrow);
        return SVM_ERR_ARG;
      }
      break;
    case DecompModeKind::oneclass: return svm_oneclass_start(m.oneclass_nu, nrow, &full, &frac);
    case DecompModeKind::heldout:
      if (!m.heldout || !y || (backend == DecompBackend::device && !m.heldout_out)) {
        set_error("%s: the held-out solve needs labels, a mask and a buffer for the held-out decisions", who);
        return SVM_ERR_ARG;
      }
      break;
    case DecompModeKind::nu_classify:
    case DecompModeKind::nu_twin: {
      const bool tw = m.kind == DecompModeKind::nu_twin;
      if (!(m.nu > 0.0 && m.nu <= 1.0)) {
        set_error("%s: nu must be in (0, 1], got %g", who, m.nu);
        return SVM_ERR_ARG;
      }
      if (nrow < 2 || m.points(nrow) > kNuMaxPoints) {
        set_error("%s: the %s solve takes 2 <= n and at most %lld points (%lld here): its four candidate lists of "
                  "every 4096-point block must fit one working set", who, solve[int(m.kind)], (long long)kNuMaxPoints,
                  (long long)m.points(nrow));
        return SVM_ERR_ARG;
      }
      if (tw ? !m.twin_z : !y) {
        set_error("%s: the %s solve needs %s", who, solve[int(m.kind)], tw ? "targets" : "labels");
        return SVM_ERR_ARG;
      }
      if (!tw) {  // the oracle's labels are the host's; the device's entry brings the count of its +1 labels
        int64_t np = m.nu_npos;
        if (backend == DecompBackend::cpu_oracle) {
          np = 0;
          for (int64_t i = 0; i < nrow; ++i) np += y[i] == 1 ? 1 : 0;
        }
        if (np < 0 || np > nrow || !nu_svc_feasible(m.nu, nrow, np, nrow - np)) {
          set_error("%s: specified nu is infeasible (nu = %g, %lld points of class +1 and %lld of class -1: nu n / 2 "
                    "must not exceed the smaller class)", who, m.nu, (long long)np, (long long)(nrow - np));
          return SVM_ERR_ARG;
        }
      }
      break;
    }
  }
  return SVM_OK;
}

}  // namespace svm355
