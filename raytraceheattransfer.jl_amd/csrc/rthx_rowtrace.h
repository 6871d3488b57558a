// rthx_rowtrace.h -- the host sequence of the tracers that count every row
// into a dense array of N counters (rthx_trace_exchange_3d,
// rthx_gasbox_trace): what their handles hold on the device, the checks of
// rthx_trace_args, the row range and row split, and the two halves around the
// tracer's own launch (rthx_rowtrace.cpp).
#pragma once

#include "rthx_domain.h"
#include "rthx_kernels.h"

namespace rthx {

// The device side every such handle has: its device, the device's shared
// stream, three events (trace start, trace end, pack end) and the sampling
// tables (fill_tables).  open: on the current device (open_device).
struct RowDevice {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  DevBuf tables;
  int open(int device);
  ~RowDevice();
};

// One trace call between row_trace_plan and row_trace_finish.
struct RowTrace {
  double t0;  // now_ms() on entry
  const rthx_trace_args* a;
  rthx_result* res;
  const RowDevice* dev = nullptr;
  int64_t N = 0, R = 0, n_rows = 0, split = 1;
  TallyParams T{};  // (row_trace_begin)
};

// The checks of `a` alone (no handle, no HIP call): one grey bin, no ray
// recording, rays_per_emitter and the emitter range.  tracer: "3D", "gas-box".
int check_row_args(const rthx_trace_args* a, const char* tracer);
// Binds the result to the handle's device (`handle`: "scene", "box" in the
// messages; an unread async 2D trace on the result is absorbed) and plans the
// rows of N emitters: n_rows, and the split that gives about split_target
// workgroups (0: the default) of at least 1024 rays.  The caller may then set
// split.
int row_trace_plan(RowTrace& rt, const RowDevice& dev, const char* handle, int64_t N, int64_t split_target);
// Resets the result, reserves and zeroes its staging buffers, fills rt.T and
// records ev[0]: the caller launches on dev.stream next (when n_rows > 0).
int row_trace_begin(RowTrace& rt);
// Records ev[1], packs the dense rows into the CSR (finish_staged) and
// completes the result and its info.
int row_trace_finish(RowTrace& rt);

}  // namespace rthx
