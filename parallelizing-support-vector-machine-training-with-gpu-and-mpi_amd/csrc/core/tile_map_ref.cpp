// The MFMA Gram kernels' workgroup -> tile maps (csrc/hip/tile_map.h) for the CPU tests: the very functions
// rbf_gram_kernel calls, compiled for the host.
#include "tile_map.h"

#include "internal.h"

using namespace svm355;

// tm[k], tn[k] = the output tile of workgroup id0 + k, k < count, exactly as rbf_gram_kernel derives it from
// blockIdx.x.  kind 0: the rectangular launch of tiles_m x tiles_n workgroups (xcd_remap, then the GROUP_M
// band map).  kind 1: the triangular launch of tiles_m (tiles_m + 1) / 2 workgroups (xcd_remap, then tri_tile;
// tiles_n is ignored).
extern "C" SVM_API int svm_tile_map_ref(int32_t kind, int64_t id0, int64_t count, int64_t tiles_m, int64_t tiles_n,
                                        int64_t* tm, int64_t* tn) {
  const int64_t nwg = kind == 1 ? tiles_m * (tiles_m + 1) / 2 : tiles_m * tiles_n;
  if ((kind != 0 && kind != 1) || tiles_m <= 0 || (kind == 0 && tiles_n <= 0) || id0 < 0 || count < 0 ||
      id0 + count > nwg || !tm || !tn) {
    set_error("svm_tile_map_ref: bad arguments");
    return SVM_ERR_ARG;
  }
  for (int64_t k = 0; k < count; ++k) {
    const int64_t id = xcd_remap(id0 + k, nwg);
    if (kind == 1)
      tri_tile(id, tiles_m, tm[k], tn[k]);
    else
      band_tile(id, tiles_m, tiles_n, GROUP_M, tm[k], tn[k]);
  }
  return SVM_OK;
}
