// Sparse (CSR) rows against a dense transposed panel: RBF kernel values without densifying the rows
// (csr_rbf.hip).  The decomposition solver's third row source (decomp.hip), the sparse queries' decision
// function and the C entries of svm355_device.h share these launchers; all enqueue on `s`.
#pragma once
#include "ctx.h"

namespace svm355 {

constexpr int kCsrPanelCols = 1024;  // panel rows ("columns" of a kernel block): one working set, or one chunk of SVs

// n CSR rows of d features on the device: indptr (n + 1, int64), indices (int32, sorted and unique within a row,
// all in [0, d): the host checks them before upload), values, and the rows' squared norms.
struct CsrRows {
  const int64_t* indptr = nullptr;
  const int32_t* indices = nullptr;
  const double* values = nullptr;
  const double* nrm = nullptr;
  int64_t n = 0, d = 0;
};

// The panel: PT[c * ldp + j] = feature c of panel row j (FP64, at least d x ldp doubles, ldp >= the panel
// rows), nrm[j] = panel row j's squared norm.  prev / prev_cnt (the scatter's bookkeeping, on the device): the
// CSR rows whose nonzeros the panel holds now, so the next scatter clears exactly those.
struct CsrPanel {
  double* PT = nullptr;
  int64_t ldp = 0;
  double* nrm = nullptr;
  int32_t* prev = nullptr;
  int32_t* prev_cnt = nullptr;
};

enum class CsrEpilogue { store, sum, sum_twin };

// One block K(CSR rows, panel rows).  Rows: A's rows arow0 + i for i < m, or with `rowlist` the rows
// rowlist[i] (mod twin_nrow when that is > 0) for i < min(m, *rowcount).  Panel rows: j < min(ncap, *ncount)
// (ncount null: ncap).  gate: *gate != 0 -> no-op.  pid: panel row j is training row pid[j]; the CSR row whose
// id (row_off + i, or the listed row) equals it gets exactly 1.  sym: K[i][i] = 1 by position.
//   store:     K[i * ldk + j] = exp(-gamma max(0, |a_i|^2 + |p_j|^2 - 2 a_i . p_j))
//   sum:       f[i] += sum_j coef[j] K_ij, the lane's own columns ascending, then the wave butterfly
//   sum_twin:  the same sum added to f[i] and f[i + m]
struct CsrBlock {
  int64_t arow0 = 0, m = 0, row_off = 0;
  const int32_t* rowlist = nullptr;
  const int32_t* rowcount = nullptr;
  int64_t twin_nrow = 0;
  int ncap = 0;
  const int32_t* ncount = nullptr;
  const int32_t* gate = nullptr;
  const int32_t* pid = nullptr;
  double gamma = 0.0;
  double* K = nullptr;
  int64_t ldk = 0;
  bool sym = false;
  const double* coef = nullptr;
  double* f = nullptr;
};
int launch_csr_rbf(hipStream_t s, CsrEpilogue e, const CsrRows& A, const CsrPanel& P, const CsrBlock& b);

// The panel's previous rows' nonzeros set to zero (a re-walk of them: never a whole-panel memset), then the
// rows ids[0 : *cnt] (<= kCsrPanelCols; id mod twin_nrow when that is > 0) written into panel positions
// 0 .. *cnt - 1 with their norms, and remembered as the previous rows.  gate: *gate != 0 -> both are no-ops.
int launch_csr_panel_scatter(hipStream_t s, const CsrRows& A, const int32_t* ids, const int32_t* cnt,
                             const int32_t* gate, int64_t twin_nrow, const CsrPanel& P);

// PT[c * ldp + j] = Xs[(j0 + j) * lds + c] for j < cnt, c < lds: the panel of a chunk of dense rows (a model's
// support vectors), through an LDS tile transpose.  nothing is cleared: every entry of the cnt columns is written.
int launch_csr_panel_from_dense(hipStream_t s, const double* Xs, int64_t lds, int64_t cnt, double* PT, int64_t ldp);

}  // namespace svm355
