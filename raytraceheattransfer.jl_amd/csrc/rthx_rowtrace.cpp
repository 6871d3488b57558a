// rthx_rowtrace.cpp -- the dense-row tracers' shared host sequence
// (rthx_rowtrace.h) and the staged rows' way into the final CSR
// (finish_staged, which the staged 2D path of rthx_api.cpp calls too).
#define RTHX_HOST_ONLY_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "rthx_rowtrace.h"

namespace rthx {

constexpr int64_t kSplitTargetBlocks = 16384;  // workgroups per launch (RTHX_T3_SPLIT_TARGET; 4096 / 8192 / 32768: slower at config 4)
constexpr int64_t kSplitMinRays = 1024;

void reset_result(rthx_result* res, int device, int64_t N, int64_t R, int64_t n_rows, int64_t begin, int64_t stride,
                  int64_t split) {
  for (rthx_result* q : res->parts) delete q;
  res->parts.clear();
  res->interleaved = false;
  res->valid = false;
  res->host_row_off = false;
  res->host_rec = false;
  res->rec_g.clear();
  res->device = device;
  res->N = N;
  res->R = R;
  res->n_rows = n_rows;
  res->begin = begin;
  res->stride = stride;
  res->split = split;
  res->info = rthx_result_info{};
  res->info.n_emitters = N;
  res->info.rows_traced = n_rows;
  res->info.rays_per_emitter = R;
  res->info.rays_traced = n_rows * R;
  res->info.n_devices = 1;
}

// Staged rows -> final CSR, after the trace launch on `st`: merge split rows
// into the staging slots, scan the per-row nnz (row_off, totals), read the
// totals back, size cols / counts to nnz and pack the slots.  totals[0..3] =
// nnz, lost rays, max lost per row, look-back stalls (0 here).
int finish_staged(rthx_result* res, const TallyParams& T, int merge, hipStream_t st, hipEvent_t ev_end,
                  int64_t totals[4]) {
  if (T.n_rows > 0) {
    if (merge == kMergeDense) HIP_TRY(launch_compact(T, st), "row_compact_kernel launch");
    if (merge == kMergeParts) HIP_TRY(launch_part_merge(T, st), "part_merge_kernel launch");
    HIP_TRY(launch_scan(T.row_nnz, T.row_tallied, T.n_rows, T.R, res->row_off.as<int64_t>(),
                        res->totals.as<int64_t>(), st),
            "row_scan_kernel launch");
  } else {
    HIP_TRY(hipMemsetAsync(res->row_off.p, 0, 8, st), "hipMemset");
  }
  HIP_TRY(hipMemcpyAsync(totals, res->totals.p, 32, hipMemcpyDeviceToHost, st), "hipMemcpy totals");
  HIP_TRY(hipStreamSynchronize(st), "row scan");
  const size_t nnz = (size_t)std::max<int64_t>(totals[0], 1);
  HIP_TRY(res->cols.reserve(nnz * 4), "hipMalloc cols");
  HIP_TRY(res->cnt.reserve(nnz * 4), "hipMalloc cnt");
  if (T.n_rows > 0)
    HIP_TRY(launch_pack(T.stage_cols, T.stage_cnt, T.row_cap, res->row_off.as<int64_t>(), T.n_rows,
                        res->cols.as<uint32_t>(), res->cnt.as<uint32_t>(), st),
            "csr_pack_kernel launch");
  HIP_TRY(hipEventRecord(ev_end, st), "hipEventRecord");
  HIP_TRY(hipStreamSynchronize(st), "CSR pack");
  return RTHX_OK;
}

int RowDevice::open(int dev) {
  device = dev;
  if (device_stream(dev, &stream) != hipSuccess) return fail(RTHX_EDEVICE, "hipStreamCreate");
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(RTHX_EDEVICE, "hipEventCreate");
  std::vector<double> t(kTableDoubles);
  fill_tables(t.data());
  if (tables.reserve(t.size() * 8) != hipSuccess ||
      hipMemcpy(tables.p, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(RTHX_ENOMEM, "uploading the sampling tables");
  return RTHX_OK;
}

RowDevice::~RowDevice() {
  (void)hipSetDevice(device);
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  // (stream: the device's shared stream, device_stream)
}

int check_row_args(const rthx_trace_args* a, const char* tracer) {
  const std::string name = std::string("the ") + tracer + " tracer";
  if (a->bin != 0) return fail(RTHX_EINVAL, name + " has one (grey) bin");
  if (a->n_record != 0) return fail(RTHX_EINVAL, "ray recording is not supported by " + name);
  if (a->rays_per_emitter < 0 || a->rays_per_emitter > 0xFFFFFFFFll)
    return fail(RTHX_ERANGE, "rays_per_emitter must be in [0, 2^32)");
  if (a->emitter_stride < 1 || a->emitter_begin < 0) return fail(RTHX_EINVAL, "bad emitter range");
  return RTHX_OK;
}

int row_trace_plan(RowTrace& rt, const RowDevice& dev, const char* handle, int64_t N, int64_t split_target) {
  const rthx_trace_args* a = rt.a;
  rthx_result* res = rt.res;
  if (a->device != dev.device) return fail(RTHX_EINVAL, std::string("args.device differs from the ") + handle + "'s device");
  HIP_TRY(hipSetDevice(dev.device), "hipSetDevice");
  if (res->device >= 0 && res->device != dev.device) return fail(RTHX_EINVAL, "result bound to another device");
  // (an unread async 2D trace on this result: counted and finished before its buffers go)
  RTHX_TRY(absorb_superseded(res));
  res->device = dev.device;
  rt.dev = &dev;
  rt.N = N;
  rt.R = a->rays_per_emitter;
  const int64_t end = std::min<int64_t>(a->emitter_end, N);
  rt.n_rows = end > a->emitter_begin ? (end - a->emitter_begin + a->emitter_stride - 1) / a->emitter_stride : 0;
  rt.split = 1;
  if (split_target <= 0) split_target = kSplitTargetBlocks;
  if (rt.n_rows > 0 && rt.R >= 2 * kSplitMinRays)
    rt.split = std::max<int64_t>(1, std::min<int64_t>((split_target + rt.n_rows - 1) / rt.n_rows, rt.R / kSplitMinRays));
  return RTHX_OK;
}

int row_trace_begin(RowTrace& rt) {
  rthx_result* res = rt.res;
  const int64_t N = rt.N, R = rt.R, n_rows = rt.n_rows;
  if (n_rows * rt.split >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "too many rows in one call");
  const int64_t row_cap = std::max<int64_t>(1, std::min<int64_t>(N, R));
  reset_result(res, rt.dev->device, N, R, n_rows, rt.a->emitter_begin, rt.a->emitter_stride, rt.split);
  res->lb_status.release();
  res->lb_totals.release();
  res->lb_epoch = 0;
  HIP_TRY(res->stage_cols.reserve((size_t)n_rows * row_cap * 4), "hipMalloc stage_cols");
  HIP_TRY(res->stage_cnt.reserve((size_t)n_rows * row_cap * 4), "hipMalloc stage_cnt");
  HIP_TRY(res->row_nnz.reserve((size_t)n_rows * 4), "hipMalloc row_nnz");
  HIP_TRY(res->row_tallied.reserve((size_t)n_rows * 4), "hipMalloc row_tallied");
  HIP_TRY(res->row_off.reserve((size_t)(n_rows + 1) * 8), "hipMalloc row_off");
  HIP_TRY(res->totals.reserve(4 * 8), "hipMalloc totals");
  HIP_TRY(res->dense.reserve((size_t)n_rows * N * 4), "hipMalloc dense rows");

  TallyParams& T = rt.T;
  T = TallyParams{};
  T.n_emitters = N;
  T.n_rows = n_rows;
  T.row_cap = row_cap;
  T.split = (int32_t)rt.split;
  T.stage_cols = res->stage_cols.as<uint32_t>();
  T.stage_cnt = res->stage_cnt.as<uint32_t>();
  T.row_nnz = res->row_nnz.as<uint32_t>();
  T.row_tallied = res->row_tallied.as<uint32_t>();
  T.dense = res->dense.as<uint32_t>();
  T.R = R;
  hipStream_t st = rt.dev->stream;
  HIP_TRY(hipMemsetAsync(res->totals.p, 0, 32, st), "hipMemset totals");
  if (n_rows > 0) {
    HIP_TRY(hipMemsetAsync(T.dense, 0, (size_t)n_rows * N * 4, st), "hipMemset dense rows");
    HIP_TRY(hipMemsetAsync(T.row_tallied, 0, (size_t)n_rows * 4, st), "hipMemset row_tallied");
  }
  HIP_TRY(hipEventRecord(rt.dev->ev[0], st), "hipEventRecord");
  return RTHX_OK;
}

int row_trace_finish(RowTrace& rt) {
  rthx_result* res = rt.res;
  const RowDevice& dev = *rt.dev;
  HIP_TRY(hipEventRecord(dev.ev[1], dev.stream), "hipEventRecord");
  int64_t totals[4] = {0, 0, 0, 0};
  RTHX_TRY(finish_staged(res, rt.T, kMergeDense, dev.stream, dev.ev[2], totals));
  float ms_trace = 0.f, ms_pack = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_trace, dev.ev[0], dev.ev[1]), "hipEventElapsedTime");
  HIP_TRY(hipEventElapsedTime(&ms_pack, dev.ev[1], dev.ev[2]), "hipEventElapsedTime");
  if (!(rt.a->flags & RTHX_FLAG_DEVICE_ONLY)) {
    res->h_row_off.resize(rt.n_rows + 1);
    HIP_TRY(hipMemcpy(res->h_row_off.data(), res->row_off.p, (rt.n_rows + 1) * 8, hipMemcpyDeviceToHost),
            "hipMemcpy row_off");
    res->host_row_off = true;
  }
  take_superseded(res, 0);
  res->info.nnz = totals[0];
  res->info.lost_total = totals[1];
  res->info.lost_max_row = totals[2];
  res->info.trace_ms = ms_trace;
  res->info.pack_ms = ms_pack;
  res->valid = true;
  res->info.total_ms = now_ms() - rt.t0;
  return RTHX_OK;
}

}  // namespace rthx
