// The pairwise SMO drivers' shape rule (smo_plan.h) for the CPU tests: the plans the device library would
// make for a problem under the current environment.
#include "smo_plan.h"

#include "internal.h"

using namespace svm355;

// smo[0..8] = resident Gram: path (0 single, 1 persistent, 2 graph), NT, E, G, XCD-local; then the
// device-wide re-plan of the XCD fallback: found, NT, E, G.  rc[0..5] = row cache with ncu compute units,
// exact-integer rows or not, kq quantised columns and nslots cache rows: applicable, E, G, records per
// lane, directory slots, LDS bytes.
extern "C" SVM_API int svm_smo_plan(int64_t n, int32_t wss, int32_t ncu, int32_t int_rows, int32_t kq, int64_t nslots,
                                    int64_t* smo, int64_t* rc) {
  if (!smo || !rc) {
    set_error("svm_smo_plan: bad arguments");
    return SVM_ERR_ARG;
  }
  const SmoKnobs k = read_smo_knobs();
  const SmoPlan pl = plan_smo(n, wss, k);
  SmoPlan dw = pl;
  const bool dw_ok = replan_smo_device_wide(n, k, &dw);
  const int64_t s[9] = {pl.path, pl.NT, pl.E, pl.G, pl.xlocal, dw_ok, dw_ok ? dw.NT : 0, dw_ok ? dw.E : 0, dw_ok ? dw.G : 0};
  std::copy(s, s + 9, smo);
  const RcPlan rp = plan_rc(n, ncu, int_rows != 0, kq, wss, nslots, k);
  const int64_t q[6] = {rp.ok, rp.E, rp.G, rp.rpl, rp.nd, int64_t(rp.lds)};
  std::copy(q, q + 6, rc);
  return SVM_OK;
}
