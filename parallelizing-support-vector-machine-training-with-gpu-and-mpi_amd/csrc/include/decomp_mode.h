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
#include "svm355.h"

namespace svm355 {

void set_error(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

enum class DecompModeKind { classify, twin, oneclass, heldout };
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
struct DecompMode {
  DecompModeKind kind = DecompModeKind::classify;
  const double* twin_z = nullptr;
  double twin_eps = 0.0;
  double oneclass_nu = 0.0;
  const uint8_t* heldout = nullptr;
  double* heldout_out = nullptr;
  bool twin() const { return kind == DecompModeKind::twin; }
  // the solve keeps its own signs (its y is not the caller's)
  bool own_signs() const { return kind != DecompModeKind::classify; }
  // the start sums f over the nonzero alphas in chunks, as a warm start does (sized as one)
  bool chunked_start(bool warm) const { return warm || kind == DecompModeKind::oneclass; }
  // the points the solve selects among, over nrow kernel rows
  int64_t points(int64_t nrow) const { return twin() ? 2 * nrow : nrow; }
};

// What a solve is asked to run with.  weighted: the classifier's two boxes differ (equal weights only scale
// C); for the other kinds, any class weight is set.
struct DecompFeatures {
  bool distributed = false, warm = false, shrinking = false, newton = false, weighted = false;
};
inline DecompFeatures decomp_features(const svm_params& p, int world, bool warm, bool weighted) {
  return {world != 1, warm, shrink_cfg(p).on, newton_cfg(p).on, weighted};
}

// What each kind refuses, per backend {device, CPU oracle}: distributed, warm, shrinking, newton, weighted.
// The classifier's row holds only on top of class weights -- what is unweighted refuses them, it never solves
// another problem in silence -- and is where the backends differ: the oracle runs weighted ranks, the device's
// distributed solve does not.  One-class mode: shrinking's unshrink rebuilds f from -y (the oracle's entry
// clears the weights, so its `weighted` is never set).  Held-out mode: shrinking's unshrink rebuilds f from
// the nonzero alphas, the polish is untested on label 0; class weights are allowed.
constexpr DecompFeatures kDecompRefuses[4][2] = {
    /* classify */ {{true, false, true, true, false}, {false, false, true, true, false}},
    /* twin     */ {{true, true, true, true, true}, {true, true, true, true, true}},
    /* oneclass */ {{true, true, true, true, true}, {true, true, true, true, true}},
    /* heldout  */ {{true, true, true, true, false}, {true, true, true, true, false}},
};

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
  static const char* const solve[] = {nullptr, "regression (twin)", "one-class", "held-out"};
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
  }
  return SVM_OK;
}

}  // namespace svm355
