// A precomputed kernel (svm_params.kernel = 6) on the device: the launchers of decomp_gram.hip that the
// decomposition solver's driver (decomp.hip) calls.  The row source is the caller's n x n Gram itself: nothing is
// computed, the f update streams moved rows of K and K(W, W) is a gather.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace svm355 {

// The Gram as every launcher takes it: n x n doubles, row stride ld >= n with ld even and K 16-byte aligned (a
// thread's two adjacent columns are one 16-byte load; the last column of an odd n is an 8-byte load, so nothing
// beyond a row's n entries is read).  K must be symmetric to the bit: row j is read where the mathematics says
// column j.
struct GramRows {
  const double* K = nullptr;
  int64_t n = 0, ld = 0;
};

// f[i] += sum_{k < *cnt} coef[k] K[cols[k] ld + lo + i] for i in [0, nloc), and with `twin` the same sum into
// f[i + nloc] too.  cols / coef: at most 1,024 entries; cnt and gate (optional) on the device.  *cnt = 0 or *gate != 0
// writes nothing.  The order is rowsum_update_kfun's (decomp_cpu.cpp): sixteen strided chains, the 8 4 2 1 tree.
int launch_gram_rowsum(hipStream_t s, const GramRows& G, int64_t lo, int64_t nloc, const int32_t* cols,
                       const double* coef, const int32_t* cnt, const int32_t* gate, bool twin, double* f);

// Kw[a ldw + b] = K[(W[a] mod n) ld + (W[b] mod n)] for a, b < min(*m, mcap), mcap <= min(1024, ldw); W's ids are
// points (twin mode: a row's two points are ids r and r + n), so both twins of a row get the row's values, its
// diagonal included.
int launch_gram_kww(hipStream_t s, const GramRows& G, const int32_t* W, const int32_t* m, int mcap,
                    const int32_t* gate, double* Kw, int64_t ldw);

// *bad (device, 64 bits) = the smallest row-major index i n + j at which K is not finite or K[i, j] and K[j, i]
// differ in their bits, or UINT64_MAX.  The launcher sets *bad first.
int launch_gram_check(hipStream_t s, const GramRows& G, unsigned long long* bad);

// dec[q] = sum_{s < nsv} coef[s] Kq[q ldq + sv[s]] - b for the m query rows of ncol entries (one wave each; lane l
// sums s = l, l + 64, ... ascending from 0.0, then the 64-lane butterfly 32 .. 1).  nsv = 0 writes -b.
int launch_gram_decision(hipStream_t s, const double* Kq, int64_t m, int64_t ncol, int64_t ldq, const int32_t* sv,
                         const double* coef, int64_t nsv, double b, double* dec);

}  // namespace svm355
