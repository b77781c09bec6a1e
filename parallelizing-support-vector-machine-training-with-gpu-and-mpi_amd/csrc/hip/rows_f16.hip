// Float16 training rows: RBF kernel values K = exp(-gamma max(0, |a|^2 + |b|^2 - 2 a.b)) whose dot product a.b runs
// on v_mfma_f32_32x32x16_f16 -- float16 operands, whose products are exact in float32 (11 + 11 significand bits), and
// float32 accumulation -- and whose every later step (norms, distance, exp, the sums into f) is FP64.  The rows stay
// float16 in HBM (a quarter of the FP64 rows' bytes) and no rows x 1024 kernel block is written.  The driver
// (decomp.hip) reads its kernel values here when DecompRows::X16 is set; the other row sources are not touched.
//
// ---- rbf16_block_kernel<EPI> ------------------------------------------------------------------------------
// Split.  A workgroup of 4 waves owns 128 A rows; wave w owns rows 32 w .. 32 w + 31 of them for the WHOLE column
// range, so no sum ever crosses a wave.  Columns are walked in tiles of 64 (2 MFMA blocks of 32 per wave, 32
// accumulator registers): the store epilogue takes the one tile blockIdx.y names, the sum epilogues walk the tiles
// 0, 1, ... in ascending order up to the device-side count *ncount.
// k stage.  One MFMA consumes 16 halves of k; a stage is 64 halves (128 bytes of a row), four MFMAs per column
// block, eight per wave between two barriers.  The float32 kernel's stage (16 floats, sixteen 32x32x2 MFMAs) would
// be one single MFMA here: the dot product is 8x cheaper per instruction, so the stage is made 4x longer in k and
// the B tile is double-buffered in LDS, which leaves ONE barrier per stage instead of two.
// Data movement.  Lane (lr = lane & 31, lh = lane >> 5) supplies the MFMA's A operand for row lr of its wave: in
// sub-step s (0..3) of a stage the 8 consecutive halves A[row][k0 + 16 s + 8 lh .. + 7], one 16-byte load straight
// from global memory into registers, the four of a stage prefetched one stage ahead; the A tile never goes through
// LDS (it is re-read per column tile: 128 rows x d halves per workgroup, L2 traffic, half the float32 kernel's
// bytes).  The B tile (64 columns x 64 halves, shared by the four waves) is staged through LDS, two 16-byte pieces
// per thread, register-prefetched one stage ahead; its rows are padded to 72 halves (144 bytes = 36 banks), so the
// 16 lanes one ds_read_b128 pass serves start at banks 0, 36, 8, 44, ... -- all 64 banks once, no conflict.  Stage g
// (counted across column tiles) writes buffer g & 1, passes the barrier and reads it; the write of stage g + 1 goes
// to the other buffer, which every wave finished reading before it arrived at barrier g.
// Accumulation order of one output element (invariant 1): stages k0 ascending, sub-steps s ascending, the MFMA's
// 16 k slots in the hardware's fixed order.  Both operands carry k = k0 + 16 s + 8 lh + i in slot (lh, i), so the
// order depends on k alone -- not on the tile's position, and the exact products commute -- so a.b and b.a are the
// same bits and a launch with A = B stores a matrix symmetric to the bit (|a|^2 + |b|^2 commutes too), with no
// mirror step and no diagonal pass.
// The epilogue is FP64: dist = nA[i] + nB[j] - 2 double(acc), floored at 0, exp(-gamma dist); the pair whose ids name
// one training row (Rbf16Block: ida / row_off against idb, modulo twin_nrow) gets exactly 1.0.  The sum epilogues
// evaluate the same expression (invariant 2: their kernel values are the store epilogue's bits; the file is compiled
// with contraction off like every other).  With the MFMA work of a tile cut 8x, the 32 FP64 exp of a lane per tile
// are the larger part of a tile's issue slots at d = 784 (profiles/f16_rows.md); they run on the vector ALU while
// another wave of the SIMD issues MFMAs, which is why the register budget below is held to two waves per SIMD.
// Summation order of the sum epilogues: rbf32_block_kernel's.  A lane holds 16 FP64 row partials (the accumulator
// rows 8 (r / 4) + 4 lh + r % 4) across all column tiles.  For row i, lane lr starts from 0.0 and adds
// coef[c] * K_ic for the columns c = lr, lr + 32, lr + 64, ... < count in ascending order (product rounded, then the
// add); a column >= count adds +0.0.  The 32 lanes of a half-wave are then folded by the xor butterfly 16, 8, 4, 2, 1
// (v = v + v[l ^ off]) and lane lr == 0 of each half adds the result to f[i] (and f[i + m] in the twin form).  No
// atomics, no order that depends on timing: two runs give the same bits.  A count of 0 and a non-zero gate return
// before any write.
//
// ---- around it ------------------------------------------------------------------------------------------------
// ws_gather_f16_kernel (listed rows and their norms into the 1024-row B panel), the scaling kernel (x' =
// float16(float32((double(x) - mn) / range)): subtract and divide in FP64, then the two roundings two hardware
// converts give, from float32 staging rows into a float16 buffer or in place on float16 rows, fused with the FP64
// norms of the rounded values; the column bounds are rows_minmax.h's pass on the uploaded element type), and the
// widen-and-gather of listed rows into the padded FP64 rows every model keeps.
#include "rows_f16.h"

#include "rows_minmax.h"
#include "svm355_device.h"

namespace svm355 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kHbM = 128, kHbN = 64, kHbK = kF16RowQuantum, kHbLS = 72;
static_assert(kHbK == 64 && kHbN * (kHbK / 8) == 2 * 256, "B staging: two 16-byte pieces per thread");

__device__ __forceinline__ int32_t fold_id(int64_t id, int64_t twin_nrow) {
  return int32_t((twin_nrow > 0 && id >= twin_nrow) ? id - twin_nrow : id);
}

template <int EPI>  // Rbf16Epilogue
__global__ __launch_bounds__(256, 2) void rbf16_block_kernel(Rbf16Block a) {
  if (a.gate && *a.gate != 0) return;
  int64_t n = a.ncap;
  if (a.ncount) n = min(n, int64_t(*a.ncount));
  if (n <= 0) return;
  constexpr bool STORE = EPI == int(Rbf16Epilogue::store);
  const int64_t tiles = (n + kHbN - 1) / kHbN;
  const int64_t ct0 = STORE ? int64_t(blockIdx.y) : 0, ct1 = STORE ? ct0 + 1 : tiles;
  if (ct0 >= tiles) return;
  __shared__ __attribute__((aligned(16))) half_t Bs[2][kHbN * kHbLS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, lr = lane & 31, lh = lane >> 5;
  const int64_t bm = int64_t(blockIdx.x) * kHbM;
  const int64_t arow = bm + 32 * w + lr;
  const bool aok = arow < a.m;
  const half_t* ap = a.A + (aok ? arow * a.lda : 0) + 8 * lh;
  const int srow = t >> 3, scol = (t & 7) * 8;  // B staging: thread t copies 8 halves of tile rows t / 8 and 32 + t / 8
  f16x8 z8;
#pragma unroll
  for (int i = 0; i < 8; ++i) z8[i] = half_t(0.0f);
  const double neg_gamma = -a.gamma;
  // this lane's 16 accumulator rows (C / D layout of the 32x32 MFMAs: column = lane & 31, row = 8 (r / 4) +
  // 4 (lane >> 5) + r % 4): their training-row ids, once (-2: no such row; ids are int32 by the solver's shapes)
  int32_t ia[16];
  double part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t gi = bm + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
    ia[r] = gi >= a.m ? -2 : fold_id(a.ida ? int64_t(a.ida[gi]) : a.row_off + gi, a.twin_nrow);
    part[r] = 0.0;
  }
  int par = 0;  // the LDS buffer of the next stage, alternating across stages and column tiles
  for (int64_t ct = ct0; ct < ct1; ++ct) {
    const int64_t bn = ct * kHbN;
    const bool bok0 = bn + srow < n, bok1 = bn + 32 + srow < n;
    const half_t* bp0 = a.B + (bok0 ? (bn + srow) * a.ldb : 0) + scol;
    const half_t* bp1 = a.B + (bok1 ? (bn + 32 + srow) * a.ldb : 0) + scol;
    f16x8 ra[4], rb0, rb1;
#define RBF16_GLOAD(k0)                                                                   \
  do {                                                                                    \
    _Pragma("unroll") for (int s = 0; s < 4; ++s)                                         \
      ra[s] = aok ? *reinterpret_cast<const f16x8*>(ap + (k0) + 16 * s) : z8;             \
    rb0 = bok0 ? *reinterpret_cast<const f16x8*>(bp0 + (k0)) : z8;                        \
    rb1 = bok1 ? *reinterpret_cast<const f16x8*>(bp1 + (k0)) : z8;                        \
  } while (0)
    RBF16_GLOAD(0);
    f32x16 acc[2];
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nj][r] = 0.0f;
    for (int64_t k0 = 0; k0 < a.kdim; k0 += kHbK) {
      half_t* bs = Bs[par];
      par ^= 1;
      *reinterpret_cast<f16x8*>(&bs[srow * kHbLS + scol]) = rb0;
      *reinterpret_cast<f16x8*>(&bs[(32 + srow) * kHbLS + scol]) = rb1;
      __syncthreads();  // the one barrier of a stage: the other buffer is free once every wave is here
      f16x8 x[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) x[s] = ra[s];
      if (k0 + kHbK < a.kdim) RBF16_GLOAD(k0 + kHbK);  // overlaps the MFMAs below
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const half_t* p = &bs[(nj * 32 + lr) * kHbLS + 8 * lh];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const f16x8 y = *reinterpret_cast<const f16x8*>(p + 16 * s);
          acc[nj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x[s], y, acc[nj], 0, 0, 0);
        }
      }
    }
#undef RBF16_GLOAD
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) {
      const int64_t gj = bn + nj * 32 + lr;
      const bool jok = gj < n;
      const double nbj = jok ? a.nB[gj] : 0.0;
      const double cj = (!STORE && jok) ? a.coef[gj] : 0.0;
      const int32_t idj = (jok && a.idb) ? fold_id(int64_t(a.idb[gj]), a.twin_nrow) : -1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t gi = bm + 32 * w + 8 * (r >> 2) + 4 * lh + (r & 3);
        const double nai = gi < a.m ? a.nA[gi] : 0.0;  // re-read per tile (L1): 32 registers not held across the k loop
        double dist = nai + nbj - 2.0 * double(acc[nj][r]);
        dist = dist > 0.0 ? dist : 0.0;
        double kv = exp(neg_gamma * dist);
        if (idj == ia[r]) kv = 1.0;  // (-1 never meets -2 or an id)
        if (STORE) {
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
        if (EPI == int(Rbf16Epilogue::sum_twin)) a.f[gi + a.m] += v;
      }
    }
  }
}

// One workgroup (64 threads) per listed row; see launch_ws_gather_f16.
__global__ __launch_bounds__(64) void ws_gather_f16_kernel(const half_t* __restrict__ X, const double* __restrict__ nrm,
                                                           int64_t ld, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ gate, int64_t twin_nrow,
                                                           half_t* __restrict__ Xo, double* __restrict__ no) {
  const int k = blockIdx.x;
  if ((gate && *gate != 0) || k >= *count) return;
  const int64_t src = fold_id(ids[k], twin_nrow);
  const f16x8* s = reinterpret_cast<const f16x8*>(X + src * ld);
  f16x8* d = reinterpret_cast<f16x8*>(Xo + int64_t(k) * ld);
  for (int64_t c = threadIdx.x; c < ld / 8; c += 64) d[c] = s[c];
  if (threadIdx.x == 0) no[k] = nrm[src];
}

// One wave per row: Y[row] = float16(float((double(X[row]) - mn) / range)) (range < 1e-12 divides by 1; FP64 subtract
// and divide, then the two converts, each to nearest-even; a float16 subnormal result is kept as it is -- the MFMA
// reads subnormal operands as they are, tests/test_gpu_f16_block_kernel.py), Y's padding up to ldy zeroed, and sqn =
// the FP64 sum of the rounded values' squares in scale_norm_kernel's order (lane-strided, then the wave butterfly),
// so the norms are row_norms' of the widened rows bit for bit.  Src float: staging rows into a separate buffer;
// Src half_t: in place (X == Y).  mn == nullptr: norms of Y only, nothing written to Y.
template <typename Src>
__global__ __launch_bounds__(256) void f16_scale_norm_kernel(const Src* X, int64_t ldx, half_t* Y, int64_t ldy,
                                                             int64_t n, int64_t d, const double* __restrict__ mn,
                                                             const double* __restrict__ mx, double* __restrict__ sqn) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  half_t* yr = Y + row * ldy;
  double acc = 0.0;
  for (int64_t c = lane; c < d; c += 64) {
    half_t h;
    if (mn) {
      double range = mx[c] - mn[c];
      if (range < 1e-12) range = 1.0;
      h = half_t(float((double(X[row * ldx + c]) - mn[c]) / range));
      yr[c] = h;
    } else {
      h = yr[c];
    }
    const double v = double(h);
    acc += v * v;
  }
  if (mn)
    for (int64_t c = d + lane; c < ldy; c += 64) yr[c] = half_t(0.0f);
  acc = wave_sum(acc);
  if (lane == 0) sqn[row] = acc;
}

// One wave per output row: Xs[r] = double(X[ids[r]]) (the first ldo <= ld values, the zero padding with them),
// ns[r] = nrm[ids[r]].
__global__ __launch_bounds__(256) void f16_rows_dense_kernel(const half_t* __restrict__ X, const double* __restrict__ nrm,
                                                             int64_t ld, const int64_t* __restrict__ ids, int64_t k,
                                                             double* __restrict__ Xs, int64_t ldo,
                                                             double* __restrict__ ns) {
  const int lane = threadIdx.x & 63;
  const int64_t row = int64_t(blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (row >= k) return;
  const int64_t src = ids[row];
  const half_t* xr = X + src * ld;
  double* o = Xs + row * ldo;
  for (int64_t c = lane; c < ldo; c += 64) o[c] = double(xr[c]);
  if (lane == 0) ns[row] = nrm[src];
}

unsigned wave_rows_grid(int64_t rows) { return unsigned((rows + 3) / 4); }

bool rows_ok(const void* X, int64_t ld, int64_t d) {
  return X && d >= 1 && ld >= d && ld % kHbK == 0 && !(reinterpret_cast<uintptr_t>(X) & 15);
}

}  // namespace

int launch_rbf16_block(hipStream_t s, Rbf16Epilogue epi, const Rbf16Block& b) {
  if (b.m <= 0 || b.ncap <= 0) return SVM_OK;
  const bool store = epi == Rbf16Epilogue::store;
  if (!b.A || !b.B || !b.nA || !b.nB || b.kdim < kHbK || b.kdim % kHbK || b.lda < b.kdim || b.ldb < b.kdim ||
      (b.lda % 8) || (b.ldb % 8) || (reinterpret_cast<uintptr_t>(b.A) & 15) || (reinterpret_cast<uintptr_t>(b.B) & 15) ||
      (store ? (!b.K || b.ldk < b.ncap) : (!b.coef || !b.f)) || b.twin_nrow < 0 || !(b.gamma > 0.0)) {
    set_error("rbf16 block: rows and norms, kdim a multiple of %d, lda / ldb multiples of 8 and >= kdim, A / B 16-byte "
              "aligned, gamma > 0, ldk >= ncap (store) or coef and f (sum)", kHbK);
    return SVM_ERR_ARG;
  }
  const int64_t tiles_m = (b.m + kHbM - 1) / kHbM, tiles_n = (b.ncap + kHbN - 1) / kHbN;
  if (tiles_m > 0x7FFFFFFF || tiles_n > 65535) {
    set_error("rbf16 block: problem too large for one launch");
    return SVM_ERR_ARG;
  }
  switch (epi) {
    case Rbf16Epilogue::store:
      hipLaunchKernelGGL(rbf16_block_kernel<int(Rbf16Epilogue::store)>, dim3(unsigned(tiles_m), unsigned(tiles_n)),
                         dim3(256), 0, s, b);
      break;
    case Rbf16Epilogue::sum:
      hipLaunchKernelGGL(rbf16_block_kernel<int(Rbf16Epilogue::sum)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
    case Rbf16Epilogue::sum_twin:
      hipLaunchKernelGGL(rbf16_block_kernel<int(Rbf16Epilogue::sum_twin)>, dim3(unsigned(tiles_m)), dim3(256), 0, s, b);
      break;
  }
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

int launch_ws_gather_f16(hipStream_t s, const half_t* X, const double* nrm, int64_t ld, const int32_t* ids,
                         const int32_t* count, const int32_t* gate, int64_t twin_nrow, int cap, half_t* Xo, double* no) {
  if (cap <= 0) return SVM_OK;
  if (!X || !nrm || !ids || !count || !Xo || !no || ld % 8) {
    set_error("gather f16: bad arguments");
    return SVM_ERR_ARG;
  }
  hipLaunchKernelGGL(ws_gather_f16_kernel, dim3(unsigned(cap)), dim3(64), 0, s, X, nrm, ld, ids, count, gate, twin_nrow,
                     Xo, no);
  SVMD_LAUNCH_CHECK();
  return SVM_OK;
}

}  // namespace svm355

using namespace svm355;

extern "C" {

// Host float16 rows (n x d, contiguous, 2 bytes per value over PCIe) -> device rows (n x ld halves, zero padded).
SVM_API int svmd_upload_rows_f16(void* h, const void* X_host, int64_t n, int64_t d, void* X_d, int64_t ld) {
  SVMD_CTX(h);
  if (ld < d || n < 0 || d < 1 || (n > 0 && (!X_host || !X_d))) {
    set_error("svmd_upload_rows_f16: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  if (n > 0) {
    if (ld == d) {
      SVMD_CHECK(hipMemcpyAsync(X_d, X_host, size_t(n * d) * 2, hipMemcpyHostToDevice, ctx->stream));
    } else {
      SVMD_CHECK(hipMemsetAsync(X_d, 0, size_t(n * ld) * 2, ctx->stream));
      SVMD_CHECK(hipMemcpy2DAsync(X_d, size_t(ld) * 2, X_host, size_t(d) * 2, size_t(d) * 2, size_t(n),
                                  hipMemcpyHostToDevice, ctx->stream));
    }
    SVMD_CHECK(hipStreamSynchronize(ctx->stream));  // the host buffer may be released on return
  }
  return ctx->end();
}

// Column min / max of the uploaded values into mn_d / mx_d (d doubles each), then X_d (n x ld halves) = the rows
// scaled by x' = float16(float((double(x) - mn) / (mx - mn))) (a range below 1e-12 divides by 1) and sqn_d[i] = the
// FP64 sum of row i's rounded squares.  src_d null: the uploaded values are X_d's own float16 ones, scaled in place.
// Otherwise src_d holds them as float32 staging rows (n x ld_src floats), which are left as they are.
SVM_API int svmd_preprocess_f16(void* h, const float* src_d, int64_t ld_src, void* X_d, int64_t n, int64_t d,
                                int64_t ld, double* mn_d, double* mx_d, double* sqn_d) {
  SVMD_CTX(h);
  if (n <= 0 || !rows_ok(X_d, ld, d) || (src_d && ld_src < d) || !mn_d || !mx_d || !sqn_d) {
    set_error("svmd_preprocess_f16: bad arguments (ld a multiple of %d)", kHbK);
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  half_t* X = static_cast<half_t*>(X_d);
  hipStream_t s = ctx->stream;
  if (src_d) {
    if ((rc = launch_rows_minmax(ctx, src_d, n, d, ld_src, mn_d, mx_d))) return rc;
    hipLaunchKernelGGL(f16_scale_norm_kernel<float>, dim3(wave_rows_grid(n)), dim3(256), 0, s, src_d, ld_src, X, ld, n, d,
                       mn_d, mx_d, sqn_d);
  } else {
    if ((rc = launch_rows_minmax(ctx, static_cast<const half_t*>(X), n, d, ld, mn_d, mx_d))) return rc;
    hipLaunchKernelGGL(f16_scale_norm_kernel<half_t>, dim3(wave_rows_grid(n)), dim3(256), 0, s,
                       static_cast<const half_t*>(X), ld, X, ld, n, d, mn_d, mx_d, sqn_d);
  }
  SVMD_LAUNCH_CHECK();
  return ctx->end();
}

// The kernel block alone on caller-supplied device rows (tests): A (m x lda halves) against B (nb <= 1024 x ldb),
// kdim halves per row; the rows' FP64 norms are computed here.  Ids, epi, count and gate as svmd_rbf_block_f32.
SVM_API int svmd_rbf_block_f16(void* h, const void* A_d, int64_t m, int64_t lda, const void* B_d, int64_t nb,
                               int64_t ldb, int64_t kdim, const int32_t* ida_d, int64_t row_off, const int32_t* idb_d,
                               int64_t twin_nrow, double gamma, int32_t epi, int32_t count, int32_t gate, double* K_d,
                               int64_t ldk, const double* coef_d, double* f_d) {
  SVMD_CTX(h);
  if (epi < 0 || epi > 2 || m < 1 || nb < 1 || nb > 1024 || kdim < 1 || !rows_ok(A_d, lda, kdim) ||
      !rows_ok(B_d, ldb, kdim)) {
    set_error("svmd_rbf_block_f16: bad arguments (epi 0..2, m >= 1, 1 <= nb <= 1024, padded 16-byte aligned rows)");
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
  half_t* A = static_cast<half_t*>(const_cast<void*>(A_d));  // norms only: nothing is written through these
  half_t* B = static_cast<half_t*>(const_cast<void*>(B_d));
  hipLaunchKernelGGL(f16_scale_norm_kernel<half_t>, dim3(wave_rows_grid(m)), dim3(256), 0, s, A, lda, A, lda, m, kdim,
                     nullptr, nullptr, nA);
  SVMD_LAUNCH_CHECK();
  hipLaunchKernelGGL(f16_scale_norm_kernel<half_t>, dim3(wave_rows_grid(nb)), dim3(256), 0, s, B, ldb, B, ldb, nb, kdim,
                     nullptr, nullptr, nB);
  SVMD_LAUNCH_CHECK();
  Rbf16Block b;
  b.A = A;
  b.nA = nA;
  b.m = m;
  b.lda = lda;
  b.B = B;
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
  if ((rc = launch_rbf16_block(s, Rbf16Epilogue(epi), b))) return rc;
  SVMD_CHECK(hipStreamSynchronize(s));
  return ctx->end();
}

// Xs_d (k x ldo doubles, written whole; d <= ldo <= ld) = the float16 rows ids_d[0 : k] widened, ns_d[k] their norms:
// the support vectors of a fit on float16 rows as every model's dense padded FP64 rows.
SVM_API int svmd_rows_f16_dense(void* h, const void* X_d, const double* nrm_d, int64_t n, int64_t ld,
                                const int64_t* ids_d, int64_t k, double* Xs_d, int64_t ldo, double* ns_d) {
  SVMD_CTX(h);
  if (k <= 0) return SVM_OK;
  if (!X_d || !nrm_d || n < 1 || ld < 1 || ldo < 1 || ldo > ld || !ids_d || !Xs_d || !ns_d) {
    set_error("svmd_rows_f16_dense: bad arguments");
    return SVM_ERR_ARG;
  }
  int rc = ctx->begin();
  if (rc) return rc;
  hipLaunchKernelGGL(f16_rows_dense_kernel, dim3(wave_rows_grid(k)), dim3(256), 0, ctx->stream,
                     static_cast<const half_t*>(X_d), nrm_d, ld, ids_d, k, Xs_d, ldo, ns_d);
  SVMD_LAUNCH_CHECK();
  return ctx->end();
}

}  // extern "C"
