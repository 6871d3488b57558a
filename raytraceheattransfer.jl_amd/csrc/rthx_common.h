// rthx_common.h -- host-side helpers shared by the C-ABI translation units:
// exported-symbol macro, thread-local error message, HIP error mapping and the
// return-on-error macros, the check of a caller's host CSR with its message
// recorded, grow-only device / pinned host buffers, a pair of
// timing events, and the opening of a device with the library's stream on it.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <utility>

#include "../../include/rthx.h"
#include "rthx_csr_host.h"

#define RTHX_EXPORT extern "C" __attribute__((visibility("default")))

namespace rthx {

extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);

// The device lookup tables (rthx_domain2d.h kTableDoubles: cos/sin of 2 pi j/256
// and the free-path log table), rthx_domain2d_build.cpp.
void fill_tables(double* t);

inline int hip_fail(hipError_t e, const char* what) {
  return fail(RTHX_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, what)                              \
  do {                                                   \
    hipError_t _e = (expr);                              \
    if (_e != hipSuccess) return rthx::hip_fail(_e, what); \
  } while (0)

// Returns the rc of a call that has already recorded its message (fail).
#define RTHX_TRY(expr)              \
  do {                              \
    int _rc = (expr);               \
    if (_rc != RTHX_OK) return _rc; \
  } while (0)

// The check of a caller's host CSR (rthx::csr::check, rthx_csr_host.h) with
// its refusal recorded by fail.
template <class Visit = csr::NoVisit>
int check_host_csr(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows, int64_t n_cols,
                   bool below_2g, bool ascending, Visit* visitor = nullptr) {
  std::string msg;
  const int rc = csr::check(row_ptr, cols, vals, n_rows, n_cols, below_2g, ascending, msg, visitor);
  return rc ? fail(rc, msg) : RTHX_OK;
}

// Device buffer with grow-only capacity.
// Tuning and test knobs from the environment (RTHX_NO_AXIS, RTHX_FORCE_HASH,
// RTHX_LB_WAIT_US, ...: the tests' and A/B tools' switches) are honoured only
// when RTHX_DEV_KNOBS=1 was set when the library first looked (read once, at
// the first knob): a user's environment cannot change the kernel path.
// knob(name) is getenv(name) then, else nullptr.
bool knobs_enabled();
const char* knob(const char* name);

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // fresh (optional): set when this call allocated (the contents are then
  // undefined -- a grown buffer can come back at its old address)
  hipError_t reserve(size_t bytes, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    if (bytes <= cap && p) return hipSuccess;
    if (fresh) *fresh = true;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Restores the calling thread's current device on scope exit (entry points
// that switch devices on behalf of a caller who keeps its own, e.g. torch).
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Pinned host buffer with grow-only capacity (fast D2H copies).
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  // fresh (optional): set when this call allocated (the contents are then
  // undefined -- a grown buffer can come back at its old address)
  hipError_t reserve(size_t bytes, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    if (bytes <= cap && p) return hipSuccess;
    if (fresh) *fresh = true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 4096 ? 4096 : bytes;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

inline double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// The library's stream on `device`: one non-blocking stream per device for
// the whole process, created on first use and never destroyed.  Creating a
// stream creates a hardware queue (~0.1 s on MI355X), so domains, scenes,
// smoothing results and solves share it instead of creating their own.
hipError_t device_stream(int device, hipStream_t* out);
// A second such stream per device for device-to-device copies out of a
// finished result (rthx_result_copy_csr_device), so that the next trace on
// the device stream does not queue behind them.
hipError_t copy_stream(int device, hipStream_t* out);
// Makes `device` the calling thread's current device: RTHX_EDEVICE without a
// visible device, RTHX_EINVAL for an ordinal out of range.  stream (optional)
// receives device_stream(device).
int open_device(int device, hipStream_t* stream);

// Two events around a stretch of a stream and the device time between them.
struct EventPair {
  hipEvent_t e[2] = {nullptr, nullptr};
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipError_t create() {
    const hipError_t err = hipEventCreate(&e[0]);
    return err != hipSuccess ? err : hipEventCreate(&e[1]);
  }
  hipError_t start(hipStream_t s) { return hipEventRecord(e[0], s); }
  hipError_t stop(hipStream_t s) { return hipEventRecord(e[1], s); }
  // (the stop event has completed: the caller synchronised the stream or the event)
  hipError_t elapsed(float* ms) { return hipEventElapsedTime(ms, e[0], e[1]); }
};

}  // namespace rthx
