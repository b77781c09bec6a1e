// The RCCL side of the device cascade: RcclTransport (declared in cascade_dev.h), the RCCL runtime's identity
// and the preflight switch, and the three C entries that only talk to RCCL.  No device code: every
// collective is an RCCL call on the backend's stream.
#include <chrono>
#include <cstring>
#include <thread>

#include "cascade_dev.h"

namespace svm355 {

#define NCCLT(expr)                                                                                 \
  do {                                                                                              \
    const ncclResult_t r_ = (expr);                                                                 \
    if (r_ != ncclSuccess) throw TransportError(std::string(#expr) + ": " + RC().GetErrorString(r_)); \
  } while (0)
#define HIPT(expr)                                                                                    \
  do {                                                                                                \
    const hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) throw TransportError(std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

RcclTransport::RcclTransport(ncclComm_t comm, int device, hipStream_t stream, WaitPolicy wp)
    : comm_(comm), device_(device), stream_(stream), wp_(std::move(wp)) {
  HIPT(hipSetDevice(device_));
  NCCLT(RC().CommUserRank(comm_, &rank_));
  NCCLT(RC().CommCount(comm_, &world_));
  HIPT(hipMalloc(&scratch_, size_t(64 + world_) * 8));
  HIPT(hipHostMalloc(&pinned_, size_t(64 + world_) * 8, hipHostMallocDefault));
}
RcclTransport::~RcclTransport() {
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(stream_);
  if (scratch_) (void)hipFree(scratch_);
  if (pinned_) (void)hipHostFree(pinned_);
}
int64_t RcclTransport::bcast_i64(int64_t v, int root) {
  static const bool prof = [] {
    const char* e = getenv("SVM355_CASCADE_PROFILE");
    return e && atoi(e) >= 3;
  }();
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t q0 = prof ? hipStreamQuery(stream_) : hipSuccess;
  pinned_[0] = v;
  HIPT(hipMemcpyAsync(scratch_, pinned_, 8, hipMemcpyHostToDevice, stream_));
  const auto t1 = std::chrono::steady_clock::now();
  NCCLT(RC().Broadcast(scratch_, scratch_, 1, ncclInt64, root, comm_, stream_));
  const auto t2 = std::chrono::steady_clock::now();
  HIPT(hipMemcpyAsync(pinned_ + 1, scratch_, 8, hipMemcpyDeviceToHost, stream_));
  wait("ncclBroadcast(i64)");
  if (prof) {
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    fprintf(stderr, "[rccl bcast_i64] stream idle at entry %d | h2d enqueue %.3f | bcast enqueue %.3f | rest %.3f ms\n",
            int(q0 == hipSuccess), ms(t0, t1), ms(t1, t2), ms(t2, std::chrono::steady_clock::now()));
  }
  return pinned_[1];
}
std::vector<int64_t> RcclTransport::allgather_i64(int64_t v) {
  pinned_[0] = v;
  HIPT(hipMemcpyAsync(scratch_, pinned_, 8, hipMemcpyHostToDevice, stream_));
  NCCLT(RC().AllGather(scratch_, scratch_ + 1, 1, ncclInt64, comm_, stream_));
  HIPT(hipMemcpyAsync(pinned_ + 1, scratch_ + 1, size_t(world_) * 8, hipMemcpyDeviceToHost, stream_));
  wait("ncclAllGather(i64)");
  return std::vector<int64_t>(pinned_ + 1, pinned_ + 1 + world_);
}
void RcclTransport::allreduce_min(double* buf, int64_t n) {
  NCCLT(RC().AllReduce(buf, buf, size_t(n), ncclFloat64, ncclMin, comm_, stream_));
  wait("ncclAllReduce(min)");
}
void RcclTransport::allreduce_max(double* buf, int64_t n) {
  NCCLT(RC().AllReduce(buf, buf, size_t(n), ncclFloat64, ncclMax, comm_, stream_));
  wait("ncclAllReduce(max)");
}
void RcclTransport::bcast(void* buf, int64_t bytes, int root) {
  if (bytes <= 0) return;
  NCCLT(RC().Broadcast(buf, buf, size_t(bytes), ncclUint8, root, comm_, stream_));
  wait("ncclBroadcast");
}
void RcclTransport::gather(const void* send, int64_t bytes, void* recv, int root) {
  if (bytes <= 0) return;
  NCCLT(RC().Gather(send, recv, size_t(bytes), ncclUint8, root, comm_, stream_));
  wait("ncclGather");
}
void RcclTransport::allgather(const void* send, int64_t bytes, void* recv) {
  if (bytes <= 0) return;
  NCCLT(RC().AllGather(send, recv, size_t(bytes), ncclUint8, comm_, stream_));
  wait("ncclAllGather");
}
void RcclTransport::allgather_async(const void* send, int64_t bytes, void* recv) {
  if (bytes > 0) NCCLT(RC().AllGather(send, recv, size_t(bytes), ncclUint8, comm_, stream_));
}
void RcclTransport::send_i64(int64_t v, int peer) {
  pinned_[2] = v;
  HIPT(hipMemcpyAsync(scratch_ + 2, pinned_ + 2, 8, hipMemcpyHostToDevice, stream_));
  NCCLT(RC().Send(scratch_ + 2, 1, ncclInt64, peer, comm_, stream_));
  wait("ncclSend(i64)");
}
int64_t RcclTransport::recv_i64(int peer) {
  NCCLT(RC().Recv(scratch_ + 3, 1, ncclInt64, peer, comm_, stream_));
  HIPT(hipMemcpyAsync(pinned_ + 3, scratch_ + 3, 8, hipMemcpyDeviceToHost, stream_));
  wait("ncclRecv(i64)");
  return pinned_[3];
}
void RcclTransport::send(const void* buf, int64_t bytes, int peer) {
  if (bytes <= 0) return;
  NCCLT(RC().Send(buf, size_t(bytes), ncclUint8, peer, comm_, stream_));
  wait("ncclSend");
}
void RcclTransport::recv(void* buf, int64_t bytes, int peer) {
  if (bytes <= 0) return;
  NCCLT(RC().Recv(buf, size_t(bytes), ncclUint8, peer, comm_, stream_));
  wait("ncclRecv");
}
void RcclTransport::barrier() {
  NCCLT(RC().AllReduce(scratch_ + 4, scratch_ + 4, 1, ncclInt64, ncclSum, comm_, stream_));
  wait("ncclAllReduce(barrier)");
}
void RcclTransport::abort() {
  if (aborted_ || !comm_) return;
  aborted_ = true;
  (void)RC().CommAbort(comm_);  // frees the communicator; in-flight kernels are torn down
}
void RcclTransport::wait(const char* what, hipEvent_t event) {
  const auto t0 = std::chrono::steady_clock::now();
  for (int spin = 0;; ++spin) {
    const hipError_t e = event ? hipEventQuery(event) : hipStreamQuery(stream_);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) throw TransportError(std::string(what) + ": " + hipGetErrorString(e));
    ncclResult_t ae = ncclSuccess;
    if (RC().CommGetAsyncError(comm_, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress)
      throw TransportError(std::string(what) + ": " + RC().GetErrorString(ae));
    wp_.check(t0, what);
    if (spin < 2000)
      std::this_thread::yield();
    else
      std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

const RcclInfo& rccl_info() {
  static const RcclInfo info = [] {
    RcclInfo r;
    const RcclApi& a = rccl();
    if (!a.ok() || a.GetVersion(&r.runtime) != ncclSuccess) r.runtime = 0;
    r.path = a.ok() ? a.path : a.error;
    return r;
  }();
  return info;
}
void require_rccl_runtime() {
  const RcclInfo& i = rccl_info();
  if (i.runtime / 10000 != NCCL_MAJOR || i.runtime < kMinRcclCode)
    throw CascadeError("RCCL runtime " + std::to_string(i.runtime) + " (" + i.path + ") is not usable: need major " +
                       std::to_string(NCCL_MAJOR) + " and at least " + std::to_string(kMinRcclCode) +
                       " (built against " + std::to_string(i.header) + ")");
}
bool preflight_enabled() {
  const char* e = getenv("SVM355_RCCL_PREFLIGHT");
  return !(e && atoi(e) == 0);
}

}  // namespace svm355

using namespace svm355;

extern "C" {

SVM_API int svmd_rccl_info(int32_t* header_code, int32_t* runtime_code, char* path, int64_t cap) {
  const RcclInfo& i = rccl_info();
  if (header_code) *header_code = i.header;
  if (runtime_code) *runtime_code = i.runtime;
  if (path && cap > 0) {
    std::strncpy(path, i.path.c_str(), size_t(cap) - 1);
    path[cap - 1] = 0;
  }
  return SVM_OK;
}

SVM_API int svmd_nccl_unique_id(uint8_t* out, int64_t cap) {
  if (!out || cap < int64_t(sizeof(ncclUniqueId))) {
    set_error("svmd_nccl_unique_id: need %zu bytes", sizeof(ncclUniqueId));
    return SVM_ERR_ARG;
  }
  try {  // RC() throws when RCCL cannot be loaded: never across the C ABI
    ncclUniqueId id;
    const ncclResult_t rc = RC().GetUniqueId(&id);
    if (rc != ncclSuccess) {
      set_error("ncclGetUniqueId: %s", RC().GetErrorString(rc));
      return SVM_ERR_DEVICE;
    }
    std::memcpy(out, &id, sizeof(id));
    return SVM_OK;
  } catch (const std::exception& e) {
    set_error("svmd_nccl_unique_id: %s", e.what());
    return SVM_ERR_DEVICE;
  }
}

SVM_API int64_t svmd_nccl_unique_id_bytes(void) { return int64_t(sizeof(ncclUniqueId)); }

}  // extern "C"
