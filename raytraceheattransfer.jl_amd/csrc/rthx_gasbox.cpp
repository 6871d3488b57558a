// rthx_gasbox.cpp -- the 3D gas-box exchange tracer's C ABI (include/rthx.h
// rthx_gasbox_*).  The box is six numbers and a lattice,
// so the handle holds no geometry on the device beyond the sampling tables
// (and the last per-voxel field traced, rthx_gasbox_trace_field); a trace is
// the dense-row sequence of rthx_rowtrace.h (row split, dense per-row counts,
// row_compact_kernel, row_scan_kernel, csr_pack_kernel) around its own launch
// and fills the caller's rthx_result.  Every argument check runs before the
// first HIP call.
#define RTHX_HOST_ONLY_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>

#include "../../include/rthx.h"
#include "rthx_common.h"
#include "rthx_gasbox.h"
#include "rthx_gasbox_walk.h"
#include "rthx_rowtrace.h"

using rthx::fail;
using rthx::now_ms;
namespace gb = rthx::gasbox;

struct rthx_gasbox {
  gb::Box B{};
  rthx::RowDevice dev;
  rthx::DevBuf beta_v;  // the field of the last rthx_gasbox_trace_field (grown, never shrunk)
};

namespace {

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

  RTHX_TRY(rthx::open_device(device, nullptr));
  rthx_gasbox* b = new (std::nothrow) rthx_gasbox();
  if (!b) return fail(RTHX_ENOMEM, "host allocation failed");
  b->B = B;
  if (const int rc = b->dev.open(device)) {
    delete b;
    return rc;
  }
  *out = b;
  return RTHX_OK;
}

RTHX_EXPORT void rthx_gasbox_destroy(rthx_gasbox* box) { delete box; }

namespace {

// Both traces.  beta_v == nullptr: the uniform medium `beta`; else the field
// beta_v[n_beta] (checked by the caller apart from its length, which needs
// the box).
int trace(rthx_gasbox* box, const rthx_trace_args* a, double beta, const double* beta_v, int64_t n_beta,
          int64_t ray_begin, rthx_result* res) {
  rthx::RowTrace rt{now_ms(), a, res};
  RTHX_TRY(rthx::check_row_args(a, "gas-box"));
  if (a->flags & ~(RTHX_FLAG_FAITHFUL_SAMPLING | RTHX_FLAG_DEVICE_ONLY))
    return fail(RTHX_EINVAL, "the gas-box tracer takes RTHX_FLAG_FAITHFUL_SAMPLING and RTHX_FLAG_DEVICE_ONLY only");
  if (ray_begin < 0) return fail(RTHX_EINVAL, "ray_begin must be >= 0");
  if (ray_begin >= (int64_t(1) << 32) || ray_begin + a->rays_per_emitter >= (int64_t(1) << 32))
    return fail(RTHX_ERANGE, "ray_begin + rays_per_emitter must be below 2^32");
  if (!box || !res) return fail(RTHX_EINVAL, "null box or result");
  const int64_t N = box->B.n_elements;
  if (beta_v && n_beta != N - box->B.n_surfaces) return fail(RTHX_EINVAL, "n_beta must be the box's Nv");
  RTHX_TRY(rthx::row_trace_plan(rt, box->dev, "box", N, 0));
  const int64_t R = rt.R;
  if (const char* e = rthx::knob("RTHX_GASBOX_SPLIT"))  // (forces the split)
    rt.split = std::max<int64_t>(1, std::min<int64_t>(std::atoll(e), std::max<int64_t>(R, 1)));
  // Row tally: the LDS histogram (u16 counters when a part has fewer than
  // 65536 rays) when it fits and a part has at least as many rays as the row
  // has columns -- below that, clearing and flushing N counters costs more
  // than the part's rays added one by one -- else the dense row in global
  // memory.  RTHX_GASBOX_GHIST=1 forces the global form, =0 the histogram
  // wherever it fits.
  const int64_t part_rays = (R + rt.split - 1) / rt.split;
  int tally = part_rays < 65536 ? gb::kU16 : gb::kU32;
  const bool fits = gb::lds_bytes(tally, N) <= rthx::kMaxLdsBytes;
  const char* gh = rthx::knob("RTHX_GASBOX_GHIST");
  if (!fits || (gh && gh[0] == '1') || (!(gh && gh[0] == '0') && part_rays < N)) tally = gb::kGlobal;
  const bool field = beta_v && rt.n_rows > 0;
  if (field) {
    // (on the handle's stream, ahead of the trace's start event: the call's time, not the kernel's)
    HIP_TRY(box->beta_v.reserve((size_t)n_beta * 8), "hipMalloc beta field");
    HIP_TRY(hipMemcpyAsync(box->beta_v.p, beta_v, (size_t)n_beta * 8, hipMemcpyHostToDevice, box->dev.stream),
            "hipMemcpy beta field");
  }
  const auto run = [&]() -> int {
    RTHX_TRY(rthx::row_trace_begin(rt));
    if (rt.n_rows > 0) {
      gb::Launch L{};
      L.B = box->B;
      L.beta = beta;
      L.tables = box->dev.tables.as<double>();
      L.R = R;
      L.ray_base = ray_begin;
      L.g_begin = a->emitter_begin;
      L.g_stride = a->emitter_stride;
      L.n_rows = rt.n_rows;
      L.split = (int32_t)rt.split;
      L.key0 = (uint32_t)a->seed;
      L.key1 = (uint32_t)(a->seed >> 32);
      L.dense = rt.T.dense;
      L.row_tallied = rt.T.row_tallied;
      L.faithful = (a->flags & RTHX_FLAG_FAITHFUL_SAMPLING) != 0;
      L.tally = tally;
      L.stream = box->dev.stream;
      if (field)
        HIP_TRY(gb::launch_field(gb::FieldLaunch{L, box->beta_v.as<double>()}), "gasbox_field_trace_kernel launch");
      else
        HIP_TRY(gb::launch(L), "gasbox_trace_kernel launch");
    }
    return rthx::row_trace_finish(rt);
  };
  const int rc = run();
  // (the copy may still be reading the caller's array when a later step failed)
  if (rc != RTHX_OK && field) (void)hipStreamSynchronize(box->dev.stream);
  return rc;
}

}  // namespace

RTHX_EXPORT int rthx_gasbox_trace(rthx_gasbox* box, const rthx_trace_args* a, double beta, int64_t ray_begin,
                                  rthx_result* res) {
  // (the checks of the arguments alone come first: they need no handle)
  if (!a) return fail(RTHX_EINVAL, "null args");
  if (!(beta >= 0.0) || !std::isfinite(beta)) return fail(RTHX_EINVAL, "beta must be finite and >= 0");
  return trace(box, a, beta, nullptr, 0, ray_begin, res);
}

RTHX_EXPORT int rthx_gasbox_trace_field(rthx_gasbox* box, const rthx_trace_args* a, const double* beta_v,
                                        int64_t n_beta, int64_t ray_begin, rthx_result* res) {
  if (!a) return fail(RTHX_EINVAL, "null args");
  if (!beta_v) return fail(RTHX_EINVAL, "null beta field");
  if (n_beta < 1 || n_beta >= (int64_t(1) << 31)) return fail(RTHX_EINVAL, "n_beta must be the box's Nv");
  for (int64_t v = 0; v < n_beta; ++v)
    if (!(beta_v[v] >= 0.0) || !std::isfinite(beta_v[v]))
      return fail(RTHX_EINVAL, "every beta of the field must be finite and >= 0");
  return trace(box, a, 0.0, beta_v, n_beta, ray_begin, res);
}
