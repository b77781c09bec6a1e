// Float32 training rows: RBF kernel values K = exp(-gamma max(0, |a|^2 + |b|^2 - 2 a.b)) whose dot product a.b
// runs on FP32 MFMA and whose every later step (norms, distance, exp, the sums into f) is FP64.  The rows stay
// float32 in HBM (half the FP64 rows' bytes), no rows x 1024 kernel block is written, and CDNA4 issues FP32 MFMA
// at twice the FP64 rate.  The driver (decomp.hip) reads its kernel values here when DecompRows::X32 is set; the
// exact-integer, FP64 and CSR row sources are not touched.
//
// ---- rbf32_block_kernel<EPI> ------------------------------------------------------------------------------
// It is kfun_block_kernel's layout (decomp_kfun.hip) moved to FP32 operands and v_mfma_f32_32x32x2_f32.
// Split.  A workgroup of 4 waves owns 128 A rows; wave w owns rows 32 w .. 32 w + 31 of them for the WHOLE column
// range, so no sum ever crosses a wave.  Columns are walked in tiles of 64 (2 MFMA blocks of 32 per wave, 32
// accumulator registers): the store epilogue takes the one tile blockIdx.y names, the sum epilogues walk the
// tiles 0, 1, ... in ascending order up to the device-side count *ncount.
// Data movement.  Lane (lr = lane & 31, lh = lane >> 5) supplies the MFMA's A operand for row lr of its wave.  Per
// k stage of 16 floats it loads A[row][k0 + 4 lh .. + 3] and A[row][k0 + 8 + 4 lh .. + 3], two 16-byte loads
// straight from global memory into registers, prefetched one stage ahead; the A tile never goes through LDS and
// needs no barrier (it is re-read per column tile: 128 rows x d floats per workgroup, L2 traffic).  The B tile
// (64 columns x 16 floats, shared by the four waves) is staged through LDS, one 16-byte piece per thread, rows
// padded to 20 floats (80 bytes: 16-byte aligned pieces, and a 32-lane column walk that spreads over the banks),
// register-prefetched one stage ahead.  k-permutation: in half h (0, 1) at sub-step s (0..3) the MFMA's k slot lh
// is k = k0 + 8 h + 4 lh + s for BOTH operands, so one 16-byte load (global for A, ds_read_b128 for B) feeds four
// MFMAs.
// Accumulation order of one output element (invariant 1): stages k0 ascending, halves h, sub-steps s, the MFMA's
// two k slots in the hardware's fixed order.  It depends on k alone -- not on the tile's position, and the
// products commute -- so a.b and b.a are the same bits and a launch with A = B stores a matrix symmetric to the
// bit (|a|^2 + |b|^2 commutes too), with no mirror step.
// The epilogue is FP64: dist = nA[i] + nB[j] - 2 double(acc), floored at 0, exp(-gamma dist); the pair whose ids
// name one training row (Rbf32Block: ida / row_off against idb, modulo twin_nrow) gets exactly 1.0 -- rbf_gram_kernel's
// colid rule, by id, so two twin ids on one row both get it and K(W, W) needs no diagonal pass.  The sum
// epilogues evaluate the same expression (invariant 2: their kernel values are the store epilogue's bits; the
// file is compiled with contraction off like every other).
// Summation order of the sum epilogues.  A lane holds 16 FP64 row partials (the accumulator rows 8 (r / 4) + 4 lh
// + r % 4) across all column tiles.  For row i, lane lr starts from 0.0 and adds coef[c] * K_ic for the columns
// c = lr, lr + 32, lr + 64, ... < count in ascending order (product rounded, then the add); a column >= count adds
// +0.0.  The 32 lanes of a half-wave are then folded by the xor butterfly 16, 8, 4, 2, 1 (v = v + v[l ^ off]) and
// lane lr == 0 of each half adds the result to f[i] (and f[i + m] in the twin form).  No atomics, no order that
// depends on timing: two runs give the same bits.  A count of 0 and a non-zero gate return before any write.
// (v_mfma_f32_16x16x4_f32 with kfun's 64-row split was the alternative; neither was timed against the other --
// profiles/f32_rows.md says what was measured.)
//
// ---- around it ------------------------------------------------------------------------------------------------
// ws_gather_f32_kernel (listed rows and their norms into the 1024-row B panel), the float32 prep kernels (column
// min / max in one streaming pass; scaling x' = float((double(x) - mn) / range) -- subtract and divide in FP64, one
// rounding -- fused with the FP64 norms of the rounded values), and the widen-and-gather of listed rows into the
// padded FP64 rows every model keeps.
#include "rows_f32.h"

#include "rows_minmax.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRbM = 128, kRbN = 64, kRbK = 16, kRbLS = 20;

__device__ __forceinline__ int64_t fold_id(int64_t id, int64_t twin_nrow) {
  return (twin_nrow > 0 && id >= twin_nrow) ? id - twin_nrow : id;
}

template <int EPI>  // Rbf32Epilogue
__global__ __launch_bounds__(256) void rbf32_block_kernel(Rbf32Block a) {
  if (a.gate && *a.gate != 0) return;
  int64_t n = a.ncap;
  if (a.ncount) n = min(n, int64_t(*a.ncount));
  if (n <= 0) return;
  constexpr bool STORE = EPI == int(Rbf32Epilogue::store);
  const int64_t tiles = (n + kRbN - 1) / kRbN;
  const int64_t ct0 = STORE ? int64_t(blockIdx.y) : 0, ct1 = STORE ? ct0 + 1 : tiles;
  if (ct0 >= tiles) return;
  __shared__ __attribute__((aligned(16))) float Bs[kRbN * kRbLS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 31, lh = lane >> 5;
  const int64_t bm = int64_t(blockIdx.x) * kRbM;
  const int64_t arow = bm + 32 * w + lr;
  const bool aok = arow < a.m;
  const float* ap = a.A + (aok ? arow * a.lda : 0) + 4 * lh;
  const int srow = t >> 2, scol = (t & 3) * 4;  // B staging: thread t copies 4 floats of tile row t / 4
  const float4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const double neg_gamma = -a.gamma;
  // this lane's 16 accumulator rows (C / D layout of the f32 32x32x2 MFMA: column = lane & 31, row = 8 (r / 4) +
  // 4 (lane >> 5) + r % 4): their norms and training-row ids, once
  double na[16], part[16];
  int64_t ia[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gi = bm + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
    const bool iok = gi < a.m;
    na[r] = iok ? a.nA[gi] : 0.0;
    ia[r] = !iok ? -2 : fold_id(a.ida ? int64_t(a.ida[gi]) : a.row_off + gi, a.twin_nrow);
    part[r] = 0.0;
  }
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t bn = ct * kRbN;
    const bool bok = bn + srow < n;
    const float* bp = a.B + (bok ? (bn + srow) * a.ldb : 0) + scol;
    float4 ra0, ra1, rb;
#define RBF32_GLOAD(k0)                                                    \
  do {                                                                     \
    ra0 = aok ? *reinterpret_cast<const float4*>(ap + (k0)) : z4;          \
    ra1 = aok ? *reinterpret_cast<const float4*>(ap + (k0) + 8) : z4;      \
    rb = bok ? *reinterpret_cast<const float4*>(bp + (k0)) : z4;           \
  } while (0)
    RBF32_GLOAD(0);
    f32x16 acc[2];
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nj][r] = 0.0f;
    for (int64_t k0 = 0; k0 < a.kdim; k0 += kRbK) {
      __syncthreads();  // the previous stage (or tile) fully consumed
      *reinterpret_cast<float4*>(&Bs[srow * kRbLS + scol]) = rb;
      __syncthreads();
      const float4 x0 = ra0, x1 = ra1;
      if (k0 + kRbK < a.kdim) RBF32_GLOAD(k0 + kRbK);  // overlaps the MFMAs below
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const float* p = &Bs[(nj * 32 + lr) * kRbLS + 4 * lh];
        const float4 y0 = *reinterpret_cast<const float4*>(p);
        const float4 y1 = *reinterpret_cast<const float4*>(p + 8);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, y0.x, acc[nj], 0, 0, 0);  // half 0, sub-steps 0..3
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y0.y, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, y0.z, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, y0.w, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, y1.x, acc[nj], 0, 0, 0);  // half 1
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y1.y, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, y1.z, acc[nj], 0, 0, 0);
        acc[nj] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, y1.w, acc[nj], 0, 0, 0);
      }
    }
#undef RBF32_GLOAD
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int64_t gj = bn + nj * 32 + lr;
      const bool jok = gj < n;
      const double nbj = jok ? a.nB[gj] : 0.0;
      const double cj = (!STORE && jok) ? a.coef[gj] : 0.0;
      const int64_t idj = (jok && a.idb) ? fold_id(int64_t(a.idb[gj]), a.twin_nrow) : -1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double dist = na[r] + nbj - 2.0 * double(acc[nj][r]);
        dist = dist > 0.0 ? dist : 0.0;
        double kv = exp(neg_gamma * dist);
        if (idj == ia[r]) kv = 1.0;  // (-1 never meets -2 or an id)
        if (STORE) {
          const int64_t gi = bm + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
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
    for (int r = 0; r < 16; ++r) {
      double v = part[r];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
      const int64_t gi = bm + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
      if (lr == 0 && gi < a.m) {
        a.f[gi] += v;
        if (EPI == int(Rbf32Epilogue::sum_twin)) a.f[gi + a.m] += v;
      }
    }
  }
}

// One workgroup (64 threads) per listed row; see launch_ws_gather_f32.
__global__ __launch_bounds__(64) void ws_gather_f32_kernel(const float* __restrict__ X, const double* __restrict__ nrm,
                                                           int64_t ld, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ gate, int64_t twin_nrow,
                                                           float* __restrict__ Xo, double* __restrict__ no) {
  const int k = blockIdx.x;
  if ((gate && *gate != 0) || k >= *count) return;
  const int64_t src = fold_id(ids[k], twin_nrow);
  const float4* s = reinterpret_cast<const float4*>(X + src * ld);
  float4* d = reinterpret_cast<float4*>(Xo + int64_t(k) * ld);
  for (int64_t c = threadIdx.x; c < ld / 4; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) no[k] = nrm[src];
}

// ---- prep: the column min / max pass is rows_minmax.h's, on float.
// One wave per row: x' = float((double(x) - mn) / range) in place (range < 1e-12 divides by 1), the padding up to
// ld zeroed, and sqn = the FP64 sum of the rounded values' squares in scale_norm_kernel's order (lane-strided,
// then the wave butterfly), so the norms are row_norms' of the widened rows bit for bit.  mn == nullptr: norms only.
__global__ __launch_bounds__(256) void f32_scale_norm_kernel(float* __restrict__ X, int64_t n, int64_t d, int64_t ld,
                                                             const double* __restrict__ mn,
                                                             const double* __restrict__ mx, double* __restrict__ sqn) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  float* xr = X + row * ld;
  double acc = 0.0;
  for (int64_t c = lane; c < d; c += 64) {
    float x = xr[c];
    if (mn) {
      double range = mx[c] - mn[c];
      if (range < 1e-12) range = 1.0;
      x = float((double(x) - mn[c]) / range);
      xr[c] = x;
    }
    const double v = double(x);
    acc += v * v;
  }
  if (mn)
    for (int64_t c = d + lane; c < ld; c += 64) xr[c] = 0.0f;
  acc = wave_sum(acc);
  if (lane == 0) sqn[row] = acc;
}

// One wave per output row: Xs[r] = double(X[ids[r]]) (ld values, the zero padding with them), ns[r] = nrm[ids[r]].
__global__ __launch_bounds__(256) void f32_rows_dense_kernel(const float* __restrict__ X, const double* __restrict__ nrm,
                                                             int64_t ld, const int64_t* __restrict__ ids, int64_t k,
                                                             double* __restrict__ Xs, double* __restrict__ ns) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= k) return;
  const int64_t src = ids[row];
  const float* xr = X + src * ld;
  double* o = Xs + row * ld;
  for (int64_t c = lane; c < ld; c += 64) o[c] = double(xr[c]);
  if (lane == 0) ns[row] = nrm[src];
}

unsigned wave_rows_grid(int64_t rows) { return unsigned((rows + 3) / 4); }

bool rows_ok(const void* X, int64_t ld, int64_t d) {
  return X && d >= 1 && ld >= d && ld % kRbK == 0 && !(reinterpret_cast<uintptr_t>(X) & 15);
}

}  // namespace

int launch_rbf32_block(hipStream_t s, Rbf32Epilogue epi, const Rbf32Block& b) {
  if (b.m <= 0 || b.ncap <= 0) return SVM_OK;
  const bool store = epi == Rbf32Epilogue::store;
  if (!b.A || !b.B || !b.nA || !b.nB || b.kdim < kRbK || b.kdim % kRbK || b.lda < b.kdim || b.ldb < b.kdim ||
      (b.lda % 4) || (b.ldb % 4) || (reinterpret_cast<uintptr_t>(b.A) & 15) || (reinterpret_cast<uintptr_t>(b.B) & 15) ||
      (store ? (!b.K || b.ldk < b.ncap) : (!b.coef || !b.f)) || b.twin_nrow < 0 || !(b.gamma > 0.0)) {
    set_error("rbf32 block: rows and norms, kdim a multiple of %d, lda / ldb multiples of 4 and >= kdim, A / B 16-byte "
              "aligned, gamma > 0, ldk >= ncap (store) or coef and f (sum)", kRbK);
    return SVM_ERR_ARG;
  }
  const int64_t tiles_m = (b.m + kRbM - 1) / kRbM, tiles_n = (b.ncap + kRbN - 1) / kRbN;
  if (tiles_m > 0x7FFFFFFF || tiles_n > 65535) {
    set_error("rbf32 block: problem too large for one launch");
    return SVM_ERR_ARG;
  }
  switch (epi) {
    case Rbf32Epilogue::store:
      hipLaunchKernelGGL(rbf32_block_kernel<int(Rbf32Epilogue::store)>, dim3(unsigned(tiles_m), unsigned(tiles_n)),
                         dim3(256), 0, s, b);
      break;
    case Rbf32Epilogue::sum:
      hipLaunchKernelGGL(rbf32_block_kernel<int(Rbf32Epilogue::sum)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
    case Rbf32Epilogue::sum_twin:
      hipLaunchKernelGGL(rbf32_block_kernel<int(Rbf32Epilogue::sum_twin)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
  }
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_ws_gather_f32(hipStream_t s, const float* X, const double* nrm, int64_t ld, const int32_t* ids,
                         const int32_t* count, const int32_t* gate, int64_t twin_nrow, int cap, float* Xo, double* no) {
  if (cap <= 0) return SVM_OK;
  if (!X || !nrm || !ids || !count || !Xo || !no || ld % 4) {
    set_error("gather f32: bad arguments");
    return SVM_ERR_ARG;
  }
  hipLaunchKernelGGL(ws_gather_f32_kernel, dim3(unsigned(cap)), dim3(64), 0, s, X, nrm, ld, ids, count, gate, twin_nrow,
                     Xo, no);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace svm355

using namespace svm355;

extern "C" {

// Host float32 rows (n x d, contiguous) -> device rows (n x ld floats, zero padded).
SVM_API int svmd_upload_rows_f32(void* h, const float* X_host, int64_t n, int64_t d, float* X_d, int64_t ld) {
  SVMD_CTX(h);
  if (ld < d || n < 0 || d < 1 || (n > 0 && (!X_host || !X_d))) {
    set_error("svmd_upload_rows_f32: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (n > 0) {
    if (ld == d) {
      SVMD_CHECK(hipMemcpyAsync(X_d, X_host, size_t(n * d) * 4, hipMemcpyHostToDevice, ctx->stream));
    } else {
      SVMD_CHECK(hipMemsetAsync(X_d, 0, size_t(n * ld) * 4, ctx->stream));
      SVMD_CHECK(hipMemcpy2DAsync(X_d, size_t(ld) * 4, X_host, size_t(d) * 4, size_t(d) * 4, size_t(n),
                                  hipMemcpyHostToDevice, ctx->stream));
    }
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));  // the host buffer may be released on return
  }
  return ctx->end();
}

// Column min / max of the float32 values into mn_d / mx_d (d doubles each), then the rows scaled in place by
// x' = float((double(x) - mn) / (mx - mn)) (a range below 1e-12 divides by 1) and sqn_d[i] = the FP64 sum of row
// i's rounded squares.
SVM_API int svmd_preprocess_f32(void* h, float* X_d, int64_t n, int64_t d, int64_t ld, double* mn_d, double* mx_d,
                                double* sqn_d) {
  SVMD_CTX(h);
  if (n <= 0 || !rows_ok(X_d, ld, d) || !mn_d || !mx_d || !sqn_d) {
    set_error("svmd_preprocess_f32: bad arguments (ld a multiple of %d)", kRbK);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if ((rc = launch_rows_minmax(ctx, X_d, n, d, ld, mn_d, mx_d))) return rc;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(f32_scale_norm_kernel, dim3(wave_rows_grid(n)), dim3(256), 0, s, X_d, n, d, ld, mn_d, mx_d, sqn_d);
  SVMD_LAUNCH_CHECK();
  return ctx->end();
}

// The kernel block alone on caller-supplied device rows (tests): A (m x lda floats) against B (nb <= 1024 x ldb),
// kdim floats per row; the rows' FP64 norms are computed here.  ida_d (optional, m ids) / row_off, idb_d (optional,
// nb ids) and twin_nrow: Rbf32Block's id rule.  epi 0: K_d (m x ldk) = the block.  epi 1 / 2: f_d[i] += sum_j
// coef_d[j] K_ij (2: also f_d[i + m]).  count >= 0: a device-side column count of that value (count < 0: none, all
// nb columns); gate: the value of the device-side stop gate (non-zero: the launch is a no-op).
SVM_API int svmd_rbf_block_f32(void* h, const float* A_d, int64_t m, int64_t lda, const float* B_d, int64_t nb,
                               int64_t ldb, int64_t kdim, const int32_t* ida_d, int64_t row_off, const int32_t* idb_d,
                               int64_t twin_nrow, double gamma, int32_t epi, int32_t count, int32_t gate, double* K_d,
                               int64_t ldk, const double* coef_d, double* f_d) {
  SVMD_CTX(h);
  if (epi < 0 || epi > 2 || m < 1 || nb < 1 || nb > 1024 || kdim < 1 || !rows_ok(A_d, lda, kdim) ||
      !rows_ok(B_d, ldb, kdim)) {
    set_error("svmd_rbf_block_f32: bad arguments (epi 0..2, m >= 1, 1 <= nb <= 1024, padded 16-byte aligned rows)");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  int32_t* dev = nullptr;  // {gate, count}
  double *nA = nullptr, *nB = nullptr;
  if ((rc = carve_ws(ctx, [&](WsCarver& c) {
         dev = c.take<int32_t>(16);
         nA = c.take<double>(size_t(m));
         nB = c.take<double>(size_t(nb));
       })))
    return rc;
  hipStream_t s = ctx->stream;
  const int32_t host[2] = {gate, count};
  SVMD_CHECK(hipMemcpyAsync(dev, host, 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(f32_scale_norm_kernel, dim3(wave_rows_grid(m)), dim3(256), 0, s, const_cast<float*>(A_d), m, kdim,
                     lda, nullptr, nullptr, nA);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(f32_scale_norm_kernel, dim3(wave_rows_grid(nb)), dim3(256), 0, s, const_cast<float*>(B_d), nb,
                     kdim, ldb, nullptr, nullptr, nB);
  SVMD_LAUNCH_CHECK();
  Rbf32Block b;
  b.A = A_d;
  b.nA = nA;
  b.m = m;
  b.lda = lda;
  b.B = B_d;
  b.nB = nB;
  b.ncap = nb;
  b.ldb = ldb;
  b.kdim = kdim;
  b.gate = dev;
  b.ncount = count >= 0 ? dev + 1 : nullptr;
  b.ida = ida_d;
  b.row_off = row_off;
  b.idb = idb_d;
  b.twin_nrow = twin_nrow;
  b.gamma = gamma;
  b.K = K_d;
  b.ldk = ldk;
  b.coef = coef_d;
  b.f = f_d;
  if ((rc = launch_rbf32_block(s, Rbf32Epilogue(epi), b))) return rc;
  SVMD_CHECK(hipStreamSynchronize(s));
  return ctx->end();
}

// Xs_d (k x ld doubles, written whole) = the float32 rows ids_d[0 : k] widened, ns_d[k] their norms: the support
// vectors of a fit on float32 rows as every model's dense padded FP64 rows.
SVM_API int svmd_rows_f32_dense(void* h, const float* X_d, const double* nrm_d, int64_t n, int64_t ld,
                                const int64_t* ids_d, int64_t k, double* Xs_d, double* ns_d) {
  SVMD_CTX(h);
  if (k <= 0) return SVM_OK;
  if (!X_d || !nrm_d || n < 1 || ld < 1 || !ids_d || !Xs_d || !ns_d) {
    set_error("svmd_rows_f32_dense: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  hipLaunchKernelGGL(f32_rows_dense_kernel, dim3(wave_rows_grid(k)), dim3(256), 0, ctx->stream, X_d, nrm_d, ld, ids_d, k,
                     Xs_d, ns_d);
  SVMD_LAUNCH_CHECK();
  return ctx->end();
}

}  // extern "C"
