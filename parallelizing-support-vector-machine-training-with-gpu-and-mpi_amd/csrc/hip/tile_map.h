// Workgroup -> output-tile maps shared by the MFMA Gram kernels (gfx950, 8 XCDs).  Pure integer
// arithmetic (plus one sqrt), so the header also compiles as plain C++: the core library exports the
// maps through svm_tile_map_ref and tests/test_tile_map_cpu.py checks them exhaustively on the CPU.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SVM355_HD __host__ __device__ __forceinline__
#else
#define SVM355_HD inline
#endif

#include <cmath>
#include <cstdint>

namespace svm355 {

// Bijective remap: workgroups dispatched to the same XCD (orig % 8 under the round-robin dispatch
// of CDNA4) get a contiguous range of logical tile ids, so neighbouring tiles share an L2.  Speed
// only: correctness never depends on placement.
SVM355_HD int64_t xcd_remap(int64_t orig, int64_t nwg) {
  const int64_t q = nwg / 8, r = nwg % 8, xcd = orig % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + orig / 8;
}

// Band height (in tile rows) of the rectangular map as the FP64 Gram kernel uses it.
constexpr int64_t GROUP_M = 8;

// Rectangular tile enumeration in bands of group_m tile rows: inside a band the ids walk down a
// column of the band first (gsz row tiles, the last band may hold fewer than group_m), then move to
// the next column, so consecutive ids share the B column-panel and a band shares its A row-panels.
SVM355_HD void band_tile(int64_t id, int64_t tiles_m, int64_t tiles_n, int64_t group_m, int64_t& tm,
                         int64_t& tn) {
  const int64_t band = group_m * tiles_n;
  const int64_t first_m = (id / band) * group_m;
  const int64_t gsz = tiles_m - first_m < group_m ? tiles_m - first_m : group_m;
  tm = first_m + (id % band) % gsz;
  tn = (id % band) / gsz;
}

// Upper-triangle tile enumeration: id -> (tm, tn) with tn >= tm, row-major (row tm holds T - tm
// tiles starting at offset(tm) = tm*T - tm*(tm-1)/2).
SVM355_HD void tri_tile(int64_t id, int64_t T, int64_t& tm, int64_t& tn) {
  const double b = double(2 * T + 1);
  int64_t r = int64_t((b - sqrt(b * b - 8.0 * double(id))) * 0.5);
  auto off = [T](int64_t x) { return x * T - x * (x - 1) / 2; };
  while (r > 0 && off(r) > id) --r;
  while (off(r + 1) <= id) ++r;
  tm = r;
  tn = r + (id - off(r));
}

}  // namespace svm355
