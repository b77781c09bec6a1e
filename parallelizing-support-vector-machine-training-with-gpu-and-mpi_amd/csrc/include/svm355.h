// svm355 — C ABI of the native runtime (CPU core + HIP/gfx950 device library).
//
// Everything the Python package and the native CLIs call goes through this header.
// The CPU core (libsvm355_core.so) implements the reference semantics exactly and
// doubles as the correctness oracle; the device library (libsvm355_hip.so) implements
// the same contract on MI355X with hand-written CDNA4 kernels.
//
// Reference parity map (files under /root/reference/code):
//   svm_csv_load        <- read_CSV                 main3.cpp:13-54, gpu_svm_main4.cu:16-59 (row limit)
//   svm_minmax/scale    <- find_min_max/scale_features main3.cpp:57-89
//   svm_rbf             <- kernel                   main3.cpp:92-104 (gamma made a parameter)
//   svm_smo_train       <- SMO_train                main3.cpp:162-294, warm start mpi_svm_main3.cpp:155-290
//   svm_decision        <- predict loop             main3.cpp:391-402
//   svm_model_save      <- commented model dump     mpi_svm_main3.cpp:754-770
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVM_API __attribute__((visibility("default")))

enum svm_status {
  SVM_OK = 0,
  SVM_ERR_IO = 1,
  SVM_ERR_ARG = 2,
  SVM_ERR_EMPTY = 3,
  SVM_ERR_DEVICE = 4,
  SVM_ERR_INTERNAL = 5,
  SVM_ERR_OOM = 6,
};

// Why an SMO solve ended. Codes match the reference's stderr messages.
enum svm_stop {
  SVM_STOP_RUNNING = 0,
  SVM_STOP_CONVERGED = 1,     // b_low <= b_high + 2*tau
  SVM_STOP_NO_CANDIDATE = 2,  // "i_high or i_low not found; iteration stops"
  SVM_STOP_INFEASIBLE = 3,    // "warning: infeasible U and V; iteration stops"
  SVM_STOP_NONPOS_ETA = 4,    // "warning: non positive eta; iteration stops": the pairwise solvers only (smo.hip,
                              // persist.h, rowcache.hip, smo_cpu.cpp: the reference's stop); the decomposition
                              // solver and its oracle floor eta at eps instead and never report it
  SVM_STOP_MAX_ITER = 5,      // "Too many iterations; stopping"
};

typedef struct svm_params {
  double C;          // box constraint, reference default 10
  double gamma;      // RBF width, reference default 0.00125
  double tau;        // stop when b_low <= b_high + 2*tau, default 1e-5
  double eps;        // set-membership / eta floor, default 1e-12
  double sv_tol;     // alpha > sv_tol is a support vector, default 1e-8
  int64_t max_iter;  // default 100000 (num_iter starts at 1)
  int32_t n_threads; // CPU worker threads (1 = the serial reference baseline)
  int32_t verbose;
  int32_t wss;       // working-set selection: 0 / 1 = first order (reference), 2 = second-order j
  int32_t shrink;    // decomposition solver shrinking: 0 = default (off), -1 = off, k > 0 = every k outer
                     // iterations (decomp_shrink.h)
  double weight_pos; // class weights: row i's box is [0, C * weight_pos] where y_i = +1 and
  double weight_neg; //   [0, C * weight_neg] where y_i = -1 (LIBSVM's -wi); 0 reads as 1 (a zero-filled
                     //   struct from an older caller), negative or non-finite values are SVM_ERR_ARG
} svm_params;

typedef struct svm_result {
  int64_t iterations;  // the reference's printed num_iter (updates + 1)
  double b;            // (b_high + b_low) / 2
  double b_high;
  double b_low;
  int32_t stop_reason; // enum svm_stop
  int32_t reserved;
  int64_t n_sv;        // alpha > sv_tol
  double seconds;      // solver wall time
} svm_result;

SVM_API const char* svm_last_error(void);
SVM_API void svm_default_params(svm_params* p);
SVM_API const char* svm_stop_message(int32_t reason);
// The two classes' box constraints C * weight_pos / C * weight_neg of p (a weight of 0 reads as 1);
// SVM_ERR_ARG for a negative or non-finite weight.  Equal weights of 1 give C itself, bit for bit.
SVM_API int svm_class_boxes(const svm_params* p, double* c_pos, double* c_neg);

// ---------------------------------------------------------------- data I/O (L0)
// Loads a CSV with a header row; the last column is the integer label.
// limit < 0 reads every line; otherwise at most `limit` data lines are consumed
// (skipped short lines count toward the limit, as gpu_svm_main4.cu:34-38).
// y = +1 where label == positive_label, else -1 (main3.cpp:49-52 with positive_label=1).
SVM_API void* svm_csv_load(const char* path, int64_t limit, int32_t positive_label, int32_t n_threads);
SVM_API int svm_dataset_dims(void* h, int64_t* n, int64_t* d);
SVM_API int svm_dataset_copy(void* h, double* X, int32_t* y, int32_t* raw_labels);
SVM_API void svm_dataset_free(void* h);
SVM_API int svm_csv_write(const char* path, const double* X, const int32_t* labels, int64_t n, int64_t d);

// Deterministic MNIST-shaped generator: 28x28 (d=784) integer pixels 0..255, labels 0..9.
// Writes global samples [offset, offset + n); sample i depends only on (seed, i).
SVM_API int svm_synth_mnist(uint64_t seed, int64_t offset, int64_t n, double* X, int32_t* labels,
                            int32_t n_threads);

// ---------------------------------------------------------------- preprocessing (L1)
SVM_API int svm_minmax(const double* X, int64_t n, int64_t d, double* mn, double* mx);
SVM_API int svm_scale(double* X, int64_t n, int64_t d, const double* mn, const double* mx);

// ---------------------------------------------------------------- kernel (L2)
SVM_API double svm_rbf(const double* a, const double* b, int64_t d, double gamma);
SVM_API int svm_rbf_matrix(const double* A, int64_t m, const double* B, int64_t n, int64_t d,
                           double gamma, double* K, int32_t n_threads);

// ---------------------------------------------------------------- SMO (L3)
// alpha: in/out length n. warm=0: alpha reset to 0 and f = -y (main3.cpp:165-172).
// warm=1: f_i = sum_{alpha_j != 0} alpha_j y_j K_ij - y_i (mpi_svm_main3.cpp:169-186).
// trace (optional, may be NULL): receives (i_high, i_low) for each update, up to trace_cap pairs.
SVM_API int svm_smo_train(const double* X, const int32_t* y, int64_t n, int64_t d, double* alpha,
                          int32_t warm, const svm_params* p, svm_result* r, int64_t* trace,
                          int64_t trace_cap);
// Same solver on a precomputed kernel matrix K (n x n, row stride ldk).
SVM_API int svm_smo_train_gram(const double* K, int64_t ldk, const int32_t* y, int64_t n,
                               double* alpha, int32_t warm, const svm_params* p, svm_result* r,
                               int64_t* trace, int64_t trace_cap);

// ---------------------------------------------------------------- working-set decomposition (L3)
// Per-outer-iteration record of a working-set decomposition solve: the device solver's test trace
// (svmd_train_decomp with a trace) and its CPU oracle's (svm_decomp_train_gram).  Caller-allocated
// arrays for `cap` outer iterations; the stopping build is not recorded.
#define SVM_DECOMP_MAX_WS 1024
// int64 entries of a decomposition solve's stats array: outer / inner iterations, working-set capacity,
// solve us, moved columns, inner threads, kernel-value path, warm columns, unshrinks, shrink passes,
// the least active rows seen, repacks, Newton steps (decomp_shrink.h / decomp_newton.h), the oracle's chain
// iterations and its first-pair updates with eta floored at eps (0 from the device, which does not count), 1 reserved
#define SVM_DECOMP_STATS 16
typedef struct svm_decomp_trace {
  int64_t cap;     // capacity in outer iterations
  int64_t count;   // out: outer iterations recorded
  int64_t n;       // length of the alpha / f snapshots (0 = none)
  int32_t* m;      // cap: working-set size
  int32_t* W;      // cap x SVM_DECOMP_MAX_WS: the working set, ascending ids
  int32_t* moved;  // cap: points whose alpha changed in the inner solve
  int32_t* cols;   // cap x SVM_DECOMP_MAX_WS: their ids, ascending
  double* coef;    // cap x SVM_DECOMP_MAX_WS: (alpha_new - alpha_old) y
  int64_t* inner;  // cap: inner iterations (pair updates)
  double* bounds;  // cap x 2: b_high, b_low of the build
  double* alpha;   // cap x n or NULL: alpha after the outer iteration
  double* f;       // cap x n or NULL: f after the outer iteration's update
} svm_decomp_trace;

// CPU oracle of the device decomposition solver (csrc/hip/decomp.hip) on a precomputed kernel matrix
// K (n x n, row stride ldk; the device's own kernel values for a bit-for-bit comparison): the same
// block selection, working-set build and stop test, the inner solve's arithmetic and tie rules, and
// the f update in the device GEMV's summation order.  q: working-set size (<= 1024); tau_frac: inner
// stop fraction (device default 0.1); inner_wss: 3 = second-order second index plus a second pair per
// iteration (device default), 4 = the same with the second pair's j by the second-order gain of
// row i2 (SVM355_DECOMP_WSS=4), 2 = second order alone, 1 = first order.  warm = 1: alpha holds the start and f = K (alpha y) - y over its nonzero entries in
// chunks of 1024 columns (the device's warm start).  stats (8 int64, may be NULL) as the device's:
// outer, inner iterations, working-set capacity, microseconds, moved columns, 0, 0, warm-start columns.
SVM_API int svm_decomp_train_gram(const double* K, int64_t ldk, const int32_t* y, int64_t n, double* alpha,
                                  int32_t warm, const svm_params* p, int32_t q, double tau_frac, int32_t inner_wss,
                                  svm_result* r, int64_t* stats, svm_decomp_trace* trace);

// The same on a cold start with the f update's summation order chosen (tests): f64_rows = 1 sums as the device's
// FP64-row path does (real-valued rows: one wave per row, lane-strided terms, a 64-lane butterfly), 0 as the GEMV.
SVM_API int svm_decomp_train_gram_rows(const double* K, int64_t ldk, const int32_t* y, int64_t n, double* alpha,
                                       const svm_params* p, int32_t q, double tau_frac, int32_t inner_wss,
                                       int32_t f64_rows, svm_result* r, int64_t* stats, svm_decomp_trace* trace);

// The device f-update GEMV's arithmetic alone: f[i] += sum_{k < cnt} coef[k] K(i, cols[k]) for the n
// rows of K, in the device's summation order (bit-for-bit tests of the GEMV kernel).
SVM_API int svm_decomp_gemv_ref(const double* K, int64_t ldk, int64_t n, const int32_t* cols, const double* coef,
                                int64_t cnt, double* f);

// The FP64 MFMA Gram kernel's workgroup -> output-tile maps (csrc/hip/tile_map.h, the functions the kernel
// calls) for the CPU tests: tm[k], tn[k] = the tile of workgroup id0 + k, k < count.  kind 0: the rectangular
// launch of tiles_m x tiles_n workgroups; kind 1: the triangular launch of tiles_m (tiles_m + 1) / 2.
SVM_API int svm_tile_map_ref(int32_t kind, int64_t id0, int64_t count, int64_t tiles_m, int64_t tiles_n, int64_t* tm,
                             int64_t* tn);

// ---------------------------------------------------------------- epsilon-SVR (L3)
// epsilon-SVR is the same box-constrained problem over 2n variables in pairs ("twins") that share a kernel
// row: variable k is a_k with sign +1, variable k + n is a*_k with sign -1, Q_ij = s_i s_j K(i mod n, j mod n),
// and the start is f_k = epsilon - z_k, f_{k+n} = -epsilon - z_k.  alpha (2n, out): a, then a*.  The model is
// beta = a - a*; a prediction is sum_k beta_k K(x_k, x) - b.  Cold start only; class weights are refused.
// The pairwise oracle (small n: it solves on duplicated rows).
SVM_API int svm_smo_train_svr(const double* X, const double* z, int64_t n, int64_t d, double epsilon, double* alpha,
                              const svm_params* p, svm_result* r);
// The decomposition oracle's twin mode on the n x n kernel matrix K (the device's own kernel values for a
// bit-for-bit comparison with svmd_train_decomp_svr): selection and the working set over the 2n virtual
// points, kernel rows by id mod n, the moved list folded to one entry per row, every row's sum added to both
// twins' f.  The trace's W / cols / coef hold virtual ids, its snapshots 2n values (trace->n = 2n).
// f64_rows: 0 = the f update sums in the exact-integer GEMV's order (svm_decomp_gemv_ref), 1 = in the FP64-row
// path's (real-valued rows: one wave per row, lane-strided terms, a 64-lane butterfly).
SVM_API int svm_decomp_train_gram_svr(const double* K, int64_t ldk, const double* z, int64_t n, double epsilon,
                                      double* alpha, const svm_params* p, int32_t q, double tau_frac,
                                      int32_t inner_wss, int32_t f64_rows, svm_result* r, int64_t* stats,
                                      svm_decomp_trace* trace);
// The twin mode's moved-column fold alone (tests): cnt <= 1024 virtual ids in [0, 2n) with their coefficients
// become one entry per kernel row, at the position of the row's first occurrence; where both twins are listed
// the coefficient is coef_k + coef_{k+n}.  out_cols / out_coef: room for cnt entries; *out_cnt: entries written.
SVM_API int svm_decomp_twin_fold(const int32_t* cols, const double* coef, int32_t cnt, int64_t n, int32_t* out_cols,
                                 double* out_coef, int32_t* out_cnt);

// ---------------------------------------------------------------- one-class SVM (L3)
// LIBSVM's -s 2: minimise 1/2 a' K a over 0 <= a_i <= 1 with sum a_i = nu n, 0 < nu < 1.  It is the classifier's
// dual with every sign +1, box 1 and no linear term: f_i = sum_j a_j K_ij (no -y_i), I_high = {a_i < 1 - eps},
// I_low = {a_i > eps}, the stop test b_low <= b_high + 2 tau, rho = b = (b_high + b_low) / 2, and the decision
// value of x is sum_k a_k K(x_k, x) - rho.  The equality is carried by LIBSVM's feasible start: a_i = 1 for
// i < full = floor(nu n), a_full = frac = nu n - full (if full < n), 0 beyond; f starts as K[:, nz] a_nz over
// the start's nonzero ids in ascending order.  p->C and the class weights are not read.
// The start's two numbers (SVM_ERR_ARG unless 0 < nu < 1 and n >= 2).
SVM_API int svm_oneclass_start(double nu, int64_t n, int64_t* full, double* frac);
// The pairwise oracle from that start.  alpha (n, out); r->b is rho.
SVM_API int svm_smo_train_oneclass(const double* X, int64_t n, int64_t d, double nu, double* alpha,
                                   const svm_params* p, svm_result* r);
// The decomposition oracle's one-class mode on the n x n kernel matrix K (the device's own kernel values for a
// bit-for-bit comparison with svmd_train_decomp_oneclass): the start's f is summed in chunks of 1024 columns, each
// in the f update's order (f64_rows: 0 = the exact-integer GEMV's, 1 = the FP64-row path's); everything after the
// start is the classifier's solve with y = +1 and C = 1.  stats[7]: the start's columns.  Shrinking and the
// Newton polish are SVM_ERR_ARG.
SVM_API int svm_decomp_train_gram_oneclass(const double* K, int64_t ldk, int64_t n, double nu, double* alpha,
                                           const svm_params* p, int32_t q, double tau_frac, int32_t inner_wss,
                                           int32_t f64_rows, svm_result* r, int64_t* stats, svm_decomp_trace* trace);

// ---------------------------------------------------------------- held-out points and Platt scaling (L3)
// The held-out form of svm_decomp_train_gram_rows (cold start): heldout[i] != 0 takes point i out of the fit.  In
// THIS entry (and the device's svmd_train_decomp_heldout) only, such a point runs with label 0, which means "held
// out, never selected": it is in neither I_high nor I_low of any selection, so its alpha stays exactly 0, while
// its f starts from -0 and receives every f update.  At the end f_i = sum_j alpha_j y_j K_ij, and f_i - r->b is
// the decision value of a model that never saw point i.  f_out (n, optional): the final f of every point.  The
// training part must hold both classes (the caller checks).  One rank; a warm start, shrinking and the Newton
// polish are SVM_ERR_ARG; class weights are allowed.
SVM_API int svm_decomp_train_gram_heldout(const double* K, int64_t ldk, const int32_t* y, const uint8_t* heldout,
                                          int64_t n, double* alpha, const svm_params* p, int32_t q, double tau_frac,
                                          int32_t inner_wss, int32_t f64_rows, svm_result* r, int64_t* stats,
                                          double* f_out, svm_decomp_trace* trace);

// Platt scaling: P(y = +1 | f) = 1 / (1 + exp(A f + B)) fitted to (decision value, label) pairs by Lin, Lin and
// Weng's Newton method with backtracking, as LIBSVM's -b 1: targets (N+ + 1) / (N+ + 2) and 1 / (N- + 2), start
// A = 0, B = log((N- + 1) / (N+ + 1)), at most 100 iterations, stop when both gradient components are below 1e-5,
// Hessian ridge 1e-12, sufficient decrease 1e-4, step floor 1e-10.
enum svm_platt_status {
  SVM_PLATT_CONVERGED = 0,    // both gradient components below 1e-5
  SVM_PLATT_MAX_ITER = 1,     // 100 Newton iterations without that
  SVM_PLATT_LINE_SEARCH = 2,  // no step down to 1e-10 decreased the objective enough
  SVM_PLATT_DEGENERATE = 3,   // one class only, or all decision values equal: nothing to fit, (A, B) = the start
};
typedef struct svm_platt {
  double A, B;
  int32_t iterations, status;
} svm_platt;
// The host fit, every sum in ascending order.  y: labels, > 0 is the positive class; use: optional n bytes,
// nonzero = the pair counts (null: all of them).
SVM_API int svm_platt_fit(const double* dec, const int32_t* y, const uint8_t* use, int64_t n, svm_platt* out);
// Pairwise coupling: class probabilities from the P = k (k - 1) / 2 one-vs-one pair decisions of each of m rows
// (dec, m x ldd, LIBSVM's pair order (0,1), (0,2), ..., (k-2,k-1); 2 <= k <= 64), Wu, Lin and Weng's second
// method as in LIBSVM.  For the pair p = (a, b): z = dec A[p] + B[p], r_ab = 1 / (1 + e^z) in its overflow-safe
// form, clamped to [1e-7, 1 - 1e-7], r_ba = 1 - r_ab; A = B = null: dec holds r_ab (clamped all the same).  p
// starts at 1 / k and is swept at most max(100, k) times, until every |(Qp)_t - p'Qp| < 0.005 / k
// (core/ovo_couple.cpp has the order of every sum).  k = 2: [r_01, r_10], no sweep.  proba (m x ldp), label
// (optional: first index of the largest) and iters (optional: sweeps taken; the cap means not converged).  A row
// with a NaN decision comes out NaN with iters = the cap.
SVM_API int svm_ovo_couple(const double* dec, int64_t ldd, int64_t m, int64_t k, const double* A, const double* B,
                           double* proba, int64_t ldp, int32_t* label, int32_t* iters, int32_t n_threads);

// ---------------------------------------------------------------- evaluation (L4)
// out[i] = sum_k alphas[k]*ys[k]*K(Xq_i, Xs_k) - b, summed in SV order from -b (main3.cpp:391-402).
SVM_API int svm_decision(const double* Xs, const int32_t* ys, const double* alphas, int64_t nsv,
                         const double* Xq, int64_t m, int64_t d, double gamma, double b,
                         double* out, int32_t n_threads);
// Indices with alpha > tol, ascending; returns the count (out may be NULL to count only).
SVM_API int64_t svm_sv_indices(const double* alpha, int64_t n, double tol, int64_t* out);

// ---------------------------------------------------------------- model files (C31)
// Writes final_sv_ids.txt, final_sv_labels.txt, final_sv_alphas.txt, final_b.txt into dir.
SVM_API int svm_model_save(const char* dir, const int64_t* ids, const int32_t* labels,
                           const double* alphas, int64_t nsv, double b);

// ---------------------------------------------------------------- Cascade SVM (L5)
// One native driver (csrc/cascade) for the classical tree (mpi_svm_main3.cpp) and the modified
// two-layer star (mpi_svm_main2.cpp) cascades; see cascade.h for the round semantics.
typedef struct svm_cascade_cfg {
  int32_t tree;            // 0 = star (modified two-layer), 1 = tree (classical, P a power of 2)
  int32_t max_rounds;      // 50 (mpi_svm_main3.cpp:544)
  svm_params params;
  int32_t log;             // rank 0 prints the reference's [rank 0] lines
  int32_t resume;          // start from <checkpoint_dir>/cascade_state.bin if present
  const char* checkpoint_dir;  // NULL or "" = no per-round checkpoint
  double comm_timeout_s;   // deadline of one blocking exchange (<= 0: 600 s)
  int32_t fail_rank;       // fault injection: this rank fails at the start of fail_round (-1 = off):
  int32_t fail_round;      //   it throws, or with fail_stall_s > 0 it stops responding for that long
  double fail_stall_s;     //   (the others then hit comm_timeout_s)
  int32_t solver;          // every local / merge solve: 0 = the pairwise first-order SMO (the reference's
                           //   trajectory, default), 1 = the warm-started working-set decomposition
                           //   (device backend: decomp.hip; CPU backend: its oracle on the set's kernel
                           //   matrix), 2 = per solve: the decomposition for cold or small sets
                           //   (<= SVM_CASCADE_DECOMP_WARM_ROWS rows), the pairwise SMO for large warm ones
  int32_t reserved;
} svm_cascade_cfg;

#define SVM_CASCADE_SOLVE_COLS 14
#define SVM_CASCADE_DECOMP_WARM_ROWS 4096
// Result of a cascade fit (allocated by the library, release with svm_cascade_free).
typedef struct svm_cascade_out {
  int32_t world, rank, rounds, converged;
  double b;
  double train_ms;         // max over the ranks this call drove (after the data distribution)
  int64_t d, n_sv;
  int64_t* ids;            // n_sv global sample ids of the final SVs (rank 0's SV order)
  int32_t* y;              // n_sv labels
  double* alpha;           // n_sv alphas
  double* sv_rows;         // n_sv x d scaled rows
  double* mn;              // d: global column min / max the rows were scaled with
  double* mx;
  int64_t n_hist;          // rounds recorded on rank 0
  int64_t* sv_history;     // n_hist global SV counts
  double* round_ms;        // n_hist round wall times (rank 0)
  int64_t n_merged;
  int64_t* merged_history; // star: rank 0's merged set sizes
  int64_t n_solves;
  double* solves;          // n_solves x SVM_CASCADE_SOLVE_COLS: rank, round, layer (star 0 local /
                           //   -1 merge, tree step), rows, SMO iterations, ms, b, stop reason, of ms
                           //   the kernel matrix, skipped (warm start already optimal), row cache
                           //   (solved on kernel rows computed on demand: the Gram did not fit),
                           //   solo ms (device time alone, serial-solve rehearsals; < 0 otherwise),
                           //   solver (0 pairwise SMO, 1 decomposition), decomposition outer iterations (0 pairwise)
  int64_t n_ranks;
  double* rank_train_ms;   // train_ms of each rank this call drove
  char transport[16];
  char backend[16];
  // Lowest driven rank's wall time per driver phase (cascade.h CascadePhase): upload, scale, bcast,
  // assemble, solve, select, gather, sendrecv, checkpoint, final, setup.
  double phase_ms[11];
} svm_cascade_out;

SVM_API void svm_cascade_default_cfg(svm_cascade_cfg* c);
// world thread-ranks in this process on the CPU oracle backend, loopback transport; rows X (n x d,
// float64) are partitioned into contiguous chunks of ceil(n / world) with global ids.
// Returns NULL on failure (svm_last_error(); a failed rank makes every rank leave its exchange).
SVM_API svm_cascade_out* svm_cascade_fit_cpu(const double* X, const int32_t* y, int64_t n, int64_t d,
                                             int32_t world, const svm_cascade_cfg* cfg);
SVM_API void svm_cascade_free(svm_cascade_out* o);

// One cascade rank per process on the CPU oracle backend, exchanging through caller-supplied
// collectives (e.g. a torch.distributed gloo group: svm355.parallel.hostcomm) -- the CPU twin of
// the per-process RCCL rank, svmd_cascade_rank_fit.  Buffers are host memory; every callback
// returns 0 on success.  gather's recv is NULL on non-root ranks (root: world * bytes, rank order).
typedef struct svm_host_comm {
  void* ctx;
  int32_t rank, world;
  int (*bcast)(void* ctx, void* buf, int64_t bytes, int32_t root);
  int (*allgather)(void* ctx, const void* send, int64_t bytes, void* recv);  // recv: world * bytes
  int (*allreduce_f64)(void* ctx, double* buf, int64_t n, int32_t op);       // op 0 = min, 1 = max
  int (*gather)(void* ctx, const void* send, int64_t bytes, void* recv, int32_t root);
  int (*send)(void* ctx, const void* buf, int64_t bytes, int32_t peer);
  int (*recv)(void* ctx, void* buf, int64_t bytes, int32_t peer);
  int (*barrier)(void* ctx);
} svm_host_comm;
// This process's rank trains on its partition (n_part x d float64 host rows, labels, global ids).
SVM_API svm_cascade_out* svm_cascade_rank_fit_cpu(const svm_host_comm* comm, const double* X, const int32_t* y,
                                                  const int64_t* ids, int64_t n_part, int64_t d, int64_t n_total,
                                                  const svm_cascade_cfg* cfg);

// The distributed form of svm_decomp_train_gram (decomp.hip's world > 1 solve on the CPU oracle): this
// process's rank owns 1/world of the selection blocks and of f, and the ranks all-gather their
// candidate records once per outer iteration through `comm`; every rank passes the whole K and gets the
// whole alpha (a replica).  For world dividing 8 the trajectory is svm_decomp_train_gram's bit for bit.
// Fault injection: SVM355_DECOMP_FAIL_RANK / SVM355_DECOMP_FAIL_OUTER (that rank fails at that outer
// iteration; its peers leave their exchange with an error).
SVM_API int svm_decomp_rank_train_gram(const svm_host_comm* comm, const double* K, int64_t ldk, const int32_t* y,
                                       int64_t n, double* alpha, int32_t warm, const svm_params* p, int32_t q,
                                       double tau_frac, int32_t inner_wss, svm_result* r, int64_t* stats);
// The same over `world` thread-ranks of this process (strict loopback transport); alpha, r and stats
// are rank 0's, and every rank's alpha replica must equal it.
SVM_API int svm_decomp_group_train_gram(int32_t world, const double* K, int64_t ldk, const int32_t* y, int64_t n,
                                        double* alpha, int32_t warm, const svm_params* p, int32_t q, double tau_frac,
                                        int32_t inner_wss, svm_result* r, int64_t* stats, double comm_timeout_s);

// Crash evidence (opt-in; Python: SVM355_CRASH_MAPS=<path>, "{pid}" replaced by the process id): on
// SIGSEGV / SIGBUS / SIGILL / SIGFPE / SIGABRT append the signal, faulting address, PC, a raw backtrace
// and /proc/self/maps to `path` (async-signal-safe calls only), then chain to the previous handler.
SVM_API int svm_crash_handler_install(const char* path);

// Transport exerciser (tests): world CPU-backend thread-ranks over a loopback group (strict = RCCL
// rules: matched collectives, rendezvous sends, deadlock detection) run `script` (exercise.cpp) with
// checked payloads.  SVM_OK, or an error naming the ranks / op within timeout_s.
SVM_API int svm_loopback_exercise(int32_t world, const char* script, int32_t strict, double timeout_s,
                                  double* elapsed_s);
// The preflight op list the device groups run on their RCCL communicators (needs cap bytes; returns
// the size needed when cap is too small, else 0).
SVM_API int svm_preflight_script(int32_t world, int64_t bulk_bytes, char* out, int64_t cap);

#ifdef __cplusplus
}
#endif
