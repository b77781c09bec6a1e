// The linear kernel K(x, z) = x . z on sparse (CSR) rows (csr_linear.hip).  For this kernel the f update factors,
//   f_i += sum_j coef_j x_i . x_j  =  x_i . dw,   dw = X_moved' coef,
// into one weight-vector delta of dpad doubles (a reduce over the transposed panel csr_rbf.h's scatter fills) and
// one CSR x vector product: one 8-byte gather per stored value instead of ceil(cnt / 64) panel runs of 512 bytes.
// The same weight vector makes the decision function of CSR queries one sparse dot product per row.  All launchers
// enqueue on `s`; every sum has a fixed order, so every run gives the same bits.
#pragma once
#include "csr_rbf.h"

namespace svm355 {

// K[i * ldk + j] = a_i . p_j: CsrBlock's rows (arow0 / rowlist / rowcount / twin_nrow), panel rows (ncap / ncount)
// and gate as launch_csr_rbf's store; no norms, no exp and no unit diagonal (pid, sym, gamma, coef and f are not
// read).  A row's stored indices ascend, products are not contracted and an absent feature adds an exact zero, so
// K(R, R) of the rows R that fill the panel equals its transpose bit for bit, and a row met twice (two twins) gets
// its own |x|^2.
int launch_csr_dot_block(hipStream_t s, const CsrRows& A, const CsrPanel& P, const CsrBlock& b);

// w[c] = sum_{j < cnt} coef[j] PT[c * ldp + j] for the nrows feature rows of the panel, cnt = min(ncap, *count)
// (count null: ncap; ncap <= kCsrPanelCols <= ldp).  One wave per feature row: lane l sums its columns l, l + 64,
// ... in ascending order, then the wave_sum butterfly.  accumulate: w[c] += the sum (and cnt = 0 writes nothing);
// else cnt = 0 writes zeros.
int launch_csr_panel_reduce(hipStream_t s, const double* PT, int64_t ldp, int64_t nrows, const double* coef, int ncap,
                            const int32_t* count, bool accumulate, double* w);

// f[i] += a_{arow0 + i} . v for i < m (v: A.d doubles); twin: the same sum is also added to f[i + m].  One wave per
// CSR row: the lanes stride the row's stored values and gather v[index], then the wave_sum butterfly.  count
// (device, optional): *count <= 0 makes the launch a no-op, so f keeps its bits.
int launch_csr_matvec(hipStream_t s, const CsrRows& A, int64_t arow0, int64_t m, const double* v, bool twin,
                      const int32_t* count, double* f);

// w[0 : lds] = sum_k coef[k] Xs[k * lds + :] over a model's nsv dense padded support vectors: chunks of
// kCsrPanelCols rows transposed into PT (lds x ldp doubles, ldp >= kCsrPanelCols), then the accumulating reduce,
// chunk by chunk in order.  nsv = 0: zeros.
int launch_linear_weight_vector(hipStream_t s, const double* Xs, const double* coef, int64_t nsv, int64_t lds,
                                double* PT, int64_t ldp, double* w);

}  // namespace svm355
