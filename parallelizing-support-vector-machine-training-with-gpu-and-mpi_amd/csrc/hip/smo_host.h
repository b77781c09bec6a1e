// Host pieces the pairwise SMO drivers share (smo.hip: resident Gram, rowcache.hip: row cache): the pinned
// state slots, the replay loop of a captured chunk of iterations, and the result block.  `State` is SmoState
// or KcState: both carry num_iter, b_high, b_low and stop.
#pragma once
#include <algorithm>
#include <chrono>

#include "ctx.h"

namespace svm355 {

// The context's pinned buffer holds three states during a solve.
constexpr int kHstPoll = 0;   // [0], [1]: the stop flags the replay loop polls, by chunk parity
constexpr int kHstFinal = 2;  // the state after the solve
constexpr int kHstSlots = 3;

struct EventPair {
  hipEvent_t ev[2] = {nullptr, nullptr};
  int create() {
    SVMD_CHECK(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    SVMD_CHECK(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    return SVM_OK;
  }
  ~EventPair() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
};

// Replay `exec` (one chunk of SMO iterations on state *st) with two chunks in flight, polling the stop flag
// of the older one, for at most max_replays chunks; then drain the stream and read the final state into
// hst[kHstFinal].  hst: kHstSlots pinned states.
template <class State>
int replay_until_stop(hipStream_t s, hipGraphExec_t exec, const State* st, State* hst, int64_t max_replays,
                      const char* who) {
  EventPair ev;
  int rc = ev.create();
  if (rc) return rc;
  hst[kHstPoll].stop = hst[kHstPoll + 1].stop = 0;
  auto enqueue = [&](int slot) {
    hipError_t e = hipGraphLaunch(exec, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&hst[kHstPoll + slot], st, sizeof(State), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(ev.ev[slot], s);
    return e;
  };
  hipError_t e = enqueue(0);
  for (int64_t rep = 0; e == hipSuccess; ++rep) {
    if (rep + 1 < max_replays) e = enqueue(int((rep + 1) & 1));
    if (e != hipSuccess) break;
    e = hipEventSynchronize(ev.ev[rep & 1]);
    if (e != hipSuccess || hst[kHstPoll + (rep & 1)].stop || rep + 1 >= max_replays) break;
  }
  const hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  if (e == hipSuccess) e = hipMemcpy(&hst[kHstFinal], st, sizeof(State), hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    set_error("%s: %s", who, hipGetErrorString(e));
    return SVM_ERR_DEVICE;
  }
  return SVM_OK;
}

// Fill *r (and the host trace) from the final state of a solve that started at t0.
template <class State>
int finish_smo(const State& fin, svm_result* r, int64_t* trace, const int64_t* dtrace, int64_t tcap,
               std::chrono::steady_clock::time_point t0, const char* who = "svmd_smo") {
  if (!fin.stop) {
    set_error("%s: solver did not stop within its budget", who);
    return SVM_ERR_INTERNAL;
  }
  if (tcap) {
    const int64_t nt = std::min<int64_t>(fin.num_iter - 1, tcap);
    if (nt > 0) SVMD_CHECK(hipMemcpy(trace, dtrace, size_t(nt) * 16, hipMemcpyDeviceToHost));
  }
  if (r) {
    r->iterations = fin.num_iter;
    r->b_high = fin.b_high;
    r->b_low = fin.b_low;
    r->b = (fin.b_high + fin.b_low) / 2;
    r->stop_reason = fin.stop;
    r->reserved = 0;
    r->n_sv = -1;  // filled by the caller (needs alpha on the host or a device count)
    r->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  return SVM_OK;
}

}  // namespace svm355
