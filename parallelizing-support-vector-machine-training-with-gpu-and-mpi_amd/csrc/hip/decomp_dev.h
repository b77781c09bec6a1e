// Working-set decomposition SMO: what the device code and the host driver share -- the control blocks
// the kernels of an outer iteration read and advance (device ABI: the CPU oracle mirrors them), the
// solver's capacities, and the launchers of the inner solve (decomp_inner.hip) the driver (decomp.hip)
// calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "svm355.h"

namespace svm355 {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct DecompHost {  // pinned: the PROF build's phase totals (the loop state is DecompCtl, on the device)
  int64_t prof[12];  // clock64 ticks per phase summed over iterations; [6] kernel clock64, [7] wall ticks;
                     // [8..11] the second-order j phase split (row i, gains + wave reduction, publish +
                     // barrier, fold)
};

// The outer loop's state on the device: the kernels of an outer iteration read and advance it, so the
// host enqueues several outer iterations between synchronisations (a stopped solve turns the rest of
// the batch into no-op launches).  stop = SVM_STOP_RUNNING (0) while running; kStopInternal: the working
// set came out outside [2, kMaxWS] (a bug).
struct DecompCtl {
  int32_t stop, m;
  double b_high, b_low;      // of the last working-set build
  double tau_in;             // the next inner solve's stop tolerance
  int64_t max_inner;         // and its iteration cap
  int64_t outer, inner_total, changed_total, last_inner_it;
  int32_t last_inner_reason;
  int32_t shrunk;            // a shrink pass has run since the start or the last unshrink
  int64_t n_active;          // this GPU's points not shrunk
  int64_t passes;            // shrink passes run
  int32_t last_m, pad2;      // the last inner solve's working-set size (the Newton polish's arming)
  int64_t newton_steps;      // Newton polish steps applied (decomp_newton.h)
};

// The Newton polish's knobs on the device (NewtonCfg).
struct NwDev {
  int32_t on, every, per_solve, repeat, max_free, pad;
  double frac;
};
constexpr int32_t kStopInternal = -100;

// The control block's host copy, written by the kernel that last changes it in an outer iteration (the
// inner solve, or the build when it stops the solve) with plain vector stores into pinned host memory:
// visible to the host once the batch's event has completed, with no copy in the stream.
__device__ __forceinline__ void publish_ctl(const DecompCtl& c, DecompCtl* __restrict__ pub) {
  if (pub) *pub = c;
}

constexpr int kSelNT = 256, kSelE = 16;  // per-block selection: up to 4096 points per block
constexpr int kMaxWS = 1024;             // working-set capacity (one 1024-thread inner workgroup)

// A working-set candidate: global point id (-1 = none) and its f.  Candidates carry f because in the
// distributed solve a GPU holds f only for its own points (every GPU holds alpha and y for all).
struct CandRec {
  double f;
  int32_t id, pad;
};

}  // namespace

// Which ws_inner_kernel instantiation an inner solve runs: nt threads (64 / 128 / 256 / 512 with
// 1024 / nt points each; 65: one wave x 6 points), the profiling build, second-order j (wss2), the second
// pair per iteration (dp), its j by second-order gain (j2s), the Newton polish compiled in (newton), per-class
// boxes (weighted: class weights that differ; built for some shapes and rules only, ws_inner_weighted_built).
struct InnerVariant {
  int nt = 256;
  bool prof = false, wss2 = true, dp = true, j2s = false, newton = false, weighted = false;
};

// ws_inner_kernel's arguments, in its parameter order.  (The control blocks above are file-local types, as
// the kernels' signatures have them; this header is their one definition in both translation units.)
struct InnerArgs {
  const double* Kw;
  int64_t ldw;
  const int32_t* W;
  DecompCtl* ctl;
  const int32_t* y;
  double* alpha;
  const double* Wf;
  double C, eps;  // C: the box of the y = +1 rows (every row's without class weights)
  int32_t* cols;
  double* coef;
  int32_t* mcount;
  DecompHost* hs;
  DecompCtl* pub;
  const int32_t* pos_of;
  int64_t lo, nloc;
  int32_t* cdiag;
  double *gAw, *gFw, *nAmat;
  NwDev nw;
  double Cn;  // the box of the y = -1 rows (read by the weighted variants only)
};

// Whether the weighted inner solve is built for v's workgroup shape and selection rule: 256 threads x 4
// points with SVM355_DECOMP_WSS = 1, 2 or 3, no profiling build, no Newton polish.
bool ws_inner_weighted_built(const InnerVariant& v);
// One inner solve on stream s (one workgroup; the caller checks the launch).  SVM_ERR_ARG, with nothing
// launched, for a weighted variant that is not built -- never the unweighted kernel in its place.
int launch_ws_inner(hipStream_t s, const InnerVariant& v, const InnerArgs& a);
// ws_newton_probe_kernel (one workgroup of nt threads): one Newton step on a given working set.  Built for
// nt = 64, 128, 256 and 512, the inner solve's shapes (ws_newton_probe_built); SVM_ERR_ARG, with nothing
// launched, for any other nt.
bool ws_newton_probe_built(int nt);
int launch_ws_newton_probe(hipStream_t s, int nt, int m, const double* Kw, int64_t ldw, const int32_t* y, double* gA,
                           double* gF, double* Amat, double C, double eps, int max_free, int32_t* code_out, int64_t* prof);

}  // namespace svm355
