// rthx_gasbox.cpp -- the 3D gas-box exchange tracer's C ABI (include/rthx.h
// rthx_gasbox_*).  The box is six numbers and a lattice, so the
// handle holds no geometry on the device beyond the sampling tables; a trace
// plans its rows like rthx_trace_exchange_3d (row split, dense per-row counts,
// row_compact_kernel, row_scan_kernel, csr_pack_kernel) and fills the
// caller's rthx_result.  Every argument check runs before the first HIP call.
#define RTHX_HOST_ONLY_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_common.h"
#include "rthx_domain.h"
#include "rthx_gasbox.h"
#include "rthx_kernels.h"

using rthx::DevBuf;
using rthx::fail;
using rthx::now_ms;
namespace gb = rthx::gasbox;

struct rthx_gasbox {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  DevBuf tables;
  gb::Box B{};
  ~rthx_gasbox() {
    (void)hipSetDevice(device);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    // (stream: the device's shared stream, rthx::device_stream)
  }
};

namespace {

// (as rthx_trace_exchange_3d)
constexpr int64_t kSplitTargetBlocks = 16384;
constexpr int64_t kSplitMinRays = 1024;

int check_lattice(const int32_t n[3]) {
  if (!n) return fail(RTHX_EINVAL, "null lattice");
  for (int k = 0; k < 3; ++k)
    if (n[k] < 1) return fail(RTHX_EINVAL, "every n must be >= 1");
  return RTHX_OK;
}

}  // namespace

RTHX_EXPORT int rthx_gasbox_layout(const int32_t n[3], int64_t* n_surfaces, int64_t* n_volumes,
                                   int64_t face_offset[7]) {
  RTHX_TRY(check_lattice(n));
  int64_t ns, nv, off[7];
  if ((double)n[0] * (double)n[1] * (double)n[2] >= 1.0e18) return fail(RTHX_ERANGE, "the lattice has too many cells");
  gb::layout(n, &ns, &nv, off);
  if (n_surfaces) *n_surfaces = ns;
  if (n_volumes) *n_volumes = nv;
  if (face_offset) std::copy(off, off + 7, face_offset);
  return RTHX_OK;
}

RTHX_EXPORT int rthx_gasbox_create(const double lo[3], const double hi[3], const int32_t n[3], int32_t device,
                                   rthx_gasbox** out) {
  if (!out) return fail(RTHX_EINVAL, "null out");
  *out = nullptr;
  if (!lo || !hi) return fail(RTHX_EINVAL, "null box corner");
  RTHX_TRY(check_lattice(n));
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(RTHX_EINVAL, "non-finite box corner");
    if (!(hi[k] > lo[k])) return fail(RTHX_EINVAL, "hi must be above lo on every axis");
    if (!std::isfinite(hi[k] - lo[k])) return fail(RTHX_EINVAL, "box extent overflows");
  }
  gb::Box B{};
  if (!gb::make_box(lo, hi, n, &B)) return fail(RTHX_ERANGE, "N = Ns + Nv must be below 2^31");
  std::vector<double> tables(rthx::kTableDoubles);
  rthx::fill_tables(tables.data());

  RTHX_TRY(rthx::open_device(device, nullptr));
  rthx_gasbox* b = new (std::nothrow) rthx_gasbox();
  if (!b) return fail(RTHX_ENOMEM, "host allocation failed");
  b->device = device;
  b->B = B;
  auto bail = [&](int code) {
    delete b;
    return code;
  };
  if (rthx::device_stream(device, &b->stream) != hipSuccess) return bail(fail(RTHX_EDEVICE, "hipStreamCreate"));
  for (auto& e : b->ev)
    if (hipEventCreate(&e) != hipSuccess) return bail(fail(RTHX_EDEVICE, "hipEventCreate"));
  if (b->tables.reserve(tables.size() * 8) != hipSuccess ||
      hipMemcpy(b->tables.p, tables.data(), tables.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(RTHX_ENOMEM, "uploading the sampling tables"));
  *out = b;
  return RTHX_OK;
}

RTHX_EXPORT void rthx_gasbox_destroy(rthx_gasbox* box) { delete box; }

RTHX_EXPORT int rthx_gasbox_trace(rthx_gasbox* box, const rthx_trace_args* a, double beta, int64_t ray_begin,
                                  rthx_result* res) {
  const double t0 = now_ms();
  // (the checks of the arguments alone come first: they need no handle)
  if (!a) return fail(RTHX_EINVAL, "null args");
  if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(RTHX_EINVAL, "beta must be finite and >= 0");
  if (a->bin != 0) return fail(RTHX_EINVAL, "the gas-box tracer has one (grey) bin");
  if (a->n_record != 0) return fail(RTHX_EINVAL, "ray recording is not supported by the gas-box tracer");
  if (a->flags & ~(RTHX_FLAG_FAITHFUL_SAMPLING | RTHX_FLAG_DEVICE_ONLY))
    return fail(RTHX_EINVAL, "the gas-box tracer takes RTHX_FLAG_FAITHFUL_SAMPLING and RTHX_FLAG_DEVICE_ONLY only");
  if (a->rays_per_emitter < 0 || a->rays_per_emitter > 0xFFFFFFFFll)
    return fail(RTHX_ERANGE, "rays_per_emitter must be in [0, 2^32)");
  if (ray_begin < 0) return fail(RTHX_EINVAL, "ray_begin must be >= 0");
  if (ray_begin >= (int64_t(1) << 32) || ray_begin + a->rays_per_emitter >= (int64_t(1) << 32))
    return fail(RTHX_ERANGE, "ray_begin + rays_per_emitter must be below 2^32");
  if (a->emitter_stride < 1 || a->emitter_begin < 0) return fail(RTHX_EINVAL, "bad emitter range");
  if (!box || !res) return fail(RTHX_EINVAL, "null box or result");
  if (a->device != box->device) return fail(RTHX_EINVAL, "args.device differs from the box's device");
  HIP_TRY(hipSetDevice(box->device), "hipSetDevice");
  if (res->device >= 0 && res->device != box->device) return fail(RTHX_EINVAL, "result bound to another device");
  {  // (an unread async 2D trace on this result: counted and finished before its buffers go)
    const int rc0 = rthx::absorb_superseded(res);
    if (rc0) return rc0;
  }
  res->device = box->device;
  const int64_t N = box->B.n_elements, R = a->rays_per_emitter;
  const int64_t end = std::min<int64_t>(a->emitter_end, N);
  const int64_t n_rows = end > a->emitter_begin ? (end - a->emitter_begin + a->emitter_stride - 1) / a->emitter_stride : 0;
  // the row split of rthx_trace_exchange_3d (RTHX_GASBOX_SPLIT forces it)
  int64_t split = 1;
  if (n_rows > 0 && R >= 2 * kSplitMinRays)
    split = std::max<int64_t>(1, std::min<int64_t>((kSplitTargetBlocks + n_rows - 1) / n_rows, R / kSplitMinRays));
  if (const char* e = rthx::knob("RTHX_GASBOX_SPLIT"))
    split = std::max<int64_t>(1, std::min<int64_t>(std::atoll(e), std::max<int64_t>(R, 1)));
  if (n_rows * split >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "too many rows in one call");
  // Row tally: the LDS histogram (u16 counters when a part has fewer than
  // 65536 rays) when it fits and a part has at least as many rays as the row
  // has columns -- below that, clearing and flushing N counters costs more
  // than the part's rays added one by one -- else the dense row in global
  // memory.  RTHX_GASBOX_GHIST=1 forces the global form, =0 the histogram
  // wherever it fits.
  const int64_t part_rays = (R + split - 1) / split;
  int tally = part_rays < 65536 ? gb::kU16 : gb::kU32;
  const bool fits = gb::lds_bytes(tally, N) <= rthx::kMaxLdsBytes;
  const char* gh = rthx::knob("RTHX_GASBOX_GHIST");
  if (!fits || (gh && gh[0] == '1') || (!(gh && gh[0] == '0') && part_rays < N)) tally = gb::kGlobal;
  const int64_t row_cap = std::max<int64_t>(1, std::min<int64_t>(N, R));
  for (rthx_result* q : res->parts) delete q;
  res->parts.clear();
  res->interleaved = false;
  res->valid = false;
  res->host_row_off = false;
  res->host_rec = false;
  res->rec_g.clear();
  res->N = N;
  res->R = R;
  res->n_rows = n_rows;
  res->begin = a->emitter_begin;
  res->stride = a->emitter_stride;
  res->split = split;
  res->info = rthx_result_info{};
  res->info.n_emitters = N;
  res->info.rows_traced = n_rows;
  res->info.rays_per_emitter = R;
  res->info.rays_traced = n_rows * R;
  res->info.n_devices = 1;
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

  rthx::TallyParams T{};
  T.n_emitters = N;
  T.n_rows = n_rows;
  T.row_cap = row_cap;
  T.split = (int32_t)split;
  T.stage_cols = res->stage_cols.as<uint32_t>();
  T.stage_cnt = res->stage_cnt.as<uint32_t>();
  T.row_nnz = res->row_nnz.as<uint32_t>();
  T.row_tallied = res->row_tallied.as<uint32_t>();
  T.dense = res->dense.as<uint32_t>();
  T.R = R;
  hipStream_t st = box->stream;
  HIP_TRY(hipMemsetAsync(res->totals.p, 0, 32, st), "hipMemset totals");
  if (n_rows > 0) {
    HIP_TRY(hipMemsetAsync(T.dense, 0, (size_t)n_rows * N * 4, st), "hipMemset dense rows");
    HIP_TRY(hipMemsetAsync(T.row_tallied, 0, (size_t)n_rows * 4, st), "hipMemset row_tallied");
  }
  HIP_TRY(hipEventRecord(box->ev[0], st), "hipEventRecord");
  if (n_rows > 0) {
    gb::Launch L{};
    L.B = box->B;
    L.beta = beta;
    L.tables = box->tables.as<double>();
    L.R = R;
    L.ray_base = ray_begin;
    L.g_begin = a->emitter_begin;
    L.g_stride = a->emitter_stride;
    L.n_rows = n_rows;
    L.split = (int32_t)split;
    L.key0 = (uint32_t)a->seed;
    L.key1 = (uint32_t)(a->seed >> 32);
    L.dense = T.dense;
    L.row_tallied = T.row_tallied;
    L.faithful = (a->flags & RTHX_FLAG_FAITHFUL_SAMPLING) != 0;
    L.tally = tally;
    L.stream = st;
    HIP_TRY(gb::launch(L), "gasbox_trace_kernel launch");
  }
  HIP_TRY(hipEventRecord(box->ev[1], st), "hipEventRecord");
  int64_t totals[4] = {0, 0, 0, 0};
  {
    const int rc = rthx::finish_staged(res, T, rthx::kMergeDense, st, box->ev[2], totals);
    if (rc) return rc;
  }
  float ms_trace = 0.f, ms_pack = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_trace, box->ev[0], box->ev[1]), "hipEventElapsedTime");
  HIP_TRY(hipEventElapsedTime(&ms_pack, box->ev[1], box->ev[2]), "hipEventElapsedTime");
  if (!(a->flags & RTHX_FLAG_DEVICE_ONLY)) {
    res->h_row_off.resize(n_rows + 1);
    HIP_TRY(hipMemcpy(res->h_row_off.data(), res->row_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToHost),
            "hipMemcpy row_off");
    res->host_row_off = true;
  }
  rthx::take_superseded(res, 0);
  res->info.nnz = totals[0];
  res->info.lost_total = totals[1];
  res->info.lost_max_row = totals[2];
  res->info.trace_ms = ms_trace;
  res->info.pack_ms = ms_pack;
  res->valid = true;
  res->info.total_ms = now_ms() - t0;
  return RTHX_OK;
}
