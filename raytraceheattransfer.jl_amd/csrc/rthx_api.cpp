// rthx_api.cpp — the C ABI declared in include/rthx.h (host side, HIP runtime).
//
// Replaces the body of computeExchangeFactorsBin
// (src/RayTracing/RayTracing2D/ExchangeFactors2D/parallelRayTracing.jl:64-159):
// the domain is validated and uploaded once (rthx_domain_create), each traced
// bin is one rthx_trace_exchange call (trace -> scan -> CSR pack on one HIP
// stream), and the count matrix comes back as CSR for the host to turn into
// SparseMatrixCSC (V = c/R, row_normalize!).
// host-only translation unit: device pointers are plain pointers here
#define RTHX_HOST_ONLY_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_domain2d_build.h"
#include "rthx_kernels.h"

#include "rthx_common.h"
#include "rthx_domain.h"

using rthx::DevBuf;
using rthx::HostBuf;
using rthx::fail;
using rthx::hip_fail;
using rthx::now_ms;

namespace rthx {
thread_local std::string g_last_error;
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

namespace {
hipError_t lib_stream(int device, hipStream_t* out, int which) {
  static std::mutex mu;
  static std::vector<hipStream_t> all[2];
  std::vector<hipStream_t>& streams = all[which];
  std::lock_guard<std::mutex> lock(mu);
  if (device < 0) return hipErrorInvalidDevice;
  if ((size_t)device >= streams.size()) streams.resize(device + 1, nullptr);
  if (!streams[device]) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking);
    if (e != hipSuccess) {
      streams[device] = nullptr;
      return e;
    }
  }
  *out = streams[device];
  return hipSuccess;
}
}  // namespace

hipError_t device_stream(int device, hipStream_t* out) { return lib_stream(device, out, 0); }
hipError_t copy_stream(int device, hipStream_t* out) { return lib_stream(device, out, 1); }

int open_device(int device, hipStream_t* stream) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(RTHX_EDEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RTHX_EINVAL, "device ordinal out of range");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  if (stream) HIP_TRY(device_stream(device, stream), "hipStreamCreate");
  return RTHX_OK;
}
}  // namespace rthx

namespace rthx {
bool knobs_enabled() {
  static const bool on = [] {
    const char* e = getenv("RTHX_DEV_KNOBS");
    return e && e[0] == '1';
  }();
  return on;
}

const char* knob(const char* name) { return knobs_enabled() ? getenv(name) : nullptr; }
}  // namespace rthx

namespace {

// Integer tuning knob (rthx::knob), clamped to [lo, hi].
int64_t env_int(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
  const char* e = rthx::knob(name);
  if (!e || !*e) return dflt;
  return std::min<int64_t>(hi, std::max<int64_t>(lo, std::strtoll(e, nullptr, 10)));
}

bool env_flag(const char* name) {
  const char* e = rthx::knob(name);
  return e && e[0] == '1';
}

template <class T>
int upload(rthx_domain* d, const T* src, size_t n, const T** dst, const char* what) {
  if (n == 0) {
    *dst = nullptr;
    return RTHX_OK;
  }
  if (!src) return fail(RTHX_EINVAL, std::string("null descriptor array: ") + what);
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, n * sizeof(T));
  if (e != hipSuccess) return fail(RTHX_ENOMEM, std::string("hipMalloc failed for ") + what);
  d->allocs.push_back(p);
  e = hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
  if (e != hipSuccess) return hip_fail(e, what);
  *dst = static_cast<const T*>(p);
  return RTHX_OK;
}

// Row splitting.  A launch of fewer rows than half the chip's resident
// workgroup slots (CUs x workgroups per CU of the unsplit kernel, from the
// occupancy query) leaves CUs idle for the whole trace, so every row is
// split into floor(slots / rows) parts, all resident in one round.  A split
// part hands its histogram to the part of its row that finishes last
// (rthx_kernels.hip, a uint4 slab store and load per lane).  Larger launches
// stay unsplit: the emulated 8-rank C2 strong shard (1326 rows, 1024 slots)
// runs 0.145 ms unsplit against 0.173 / 0.208 / 0.254 ms split into 2 / 3 /
// 4 parts, and splitting only the last round of rows (the drain) into 2 or
// 4 parts measured slower at every W (profiles/round4/ab/tail_split_*.log).
// RTHX_SPLIT_TARGET=<workgroups> replaces the slot count and
// RTHX_SPLIT_BELOW=<rows> splits only launches of fewer rows (1: never).
constexpr int64_t kSplitMinRays = 2048;

}  // namespace

// Host evaluation of the device free-path log (tests/test_numerics.py); not
// part of include/rthx.h.
extern "C" __attribute__((visibility("default"))) int rthx_debug_neg_log(const double* u, int64_t n, double* out) {
  if ((!u || !out) && n > 0) return -1;
  std::vector<double> t(rthx::kTableDoubles);
  rthx::fill_tables(t.data());
  for (int64_t k = 0; k < n; ++k) out[k] = rthx::neg_log_tab(u[k], t.data() + rthx::kLogTableOffset);
  return 0;
}

// The same log taken from a 32-bit draw w (neg_log_u32, the trace kernels'
// free path): tests check it equals neg_log_tab(w 2^-32) bit for bit.
extern "C" __attribute__((visibility("default"))) int rthx_debug_neg_log_u32(const uint32_t* w, int64_t n,
                                                                             double* out) {
  if ((!w || !out) && n > 0) return -1;
  std::vector<double> t(rthx::kTableDoubles);
  rthx::fill_tables(t.data());
  for (int64_t k = 0; k < n; ++k) out[k] = rthx::neg_log_u32(w[k], t.data() + rthx::kLogTableOffset);
  return 0;
}

// Host evaluation of the box walls' candidacy test (wall_candidate,
// rthx_device.h) beside the two forms it stands for: form 0 the shipped
// predicate, 1 the product form |s| |d| > 0 of earlier versions, 2 the
// reference's quotient form |s| / |d| > 0, each with |d| >= 1e-10.
extern "C" __attribute__((visibility("default"))) int rthx_debug_wall_candidate(double s, double d, int32_t form) {
  const double as = std::fabs(s), ad = std::fabs(d);
  switch (form) {
    case 0: return rthx::wall_candidate(s, d) ? 1 : 0;
    case 1: return (ad >= 1e-10 && as * ad > 0.0) ? 1 : 0;
    case 2: return (as / ad > 0.0 && ad >= 1e-10) ? 1 : 0;
    default: return -1;
  }
}

// Host evaluation of the LAT ray's choice of the x wall in the coarse
// two-wall test (rthx_device.h): form 0 the deferred copy's x_wall_untied,
// bit 0 the choice and bit 1 its tie flag; form 1 the reference form with the
// tie order y_first, bit 0.  cx, cy: the cross products |sx||dy|, |sy||dx|.
extern "C" __attribute__((visibility("default"))) int rthx_debug_x_wall(int32_t vx, int32_t vy, int32_t y_first,
                                                                        double cx, double cy, int32_t form) {
  const bool bx = vx != 0, by = vy != 0, yf = y_first != 0;
  switch (form) {
    case 0: {
      bool tie = false;
      const bool xw = rthx::x_wall_untied(bx, by, cx, cy, tie);
      return (xw ? 1 : 0) | (tie ? 2 : 0);
    }
    case 1: return (bx & (!by | (yf & (cx < cy)) | (!yf & !(cy < cx)))) ? 1 : 0;
    default: return -1;
  }
}

// The theta draw's sine on the device (sin_theta_u32, rthx_device.h), for
// tests.  The sweep compares it with the earlier expression
// 2.0 * sqrt_unit(u (1 - u)) on the n words from w_begin (w_begin + n <= 2^32)
// and returns the number of words whose bits differ and the least of them
// (2^64 - 1 if none); rthx_debug_sin_theta returns the values for given words.
extern "C" __attribute__((visibility("default"))) int rthx_debug_sin_theta_sweep(int32_t device, uint32_t w_begin,
                                                                                 uint64_t n, uint64_t* n_diff,
                                                                                 uint64_t* first_diff) {
  if (!n_diff || !first_diff) return fail(RTHX_EINVAL, "null output");
  if ((uint64_t)w_begin + n > (1ull << 32)) return fail(RTHX_EINVAL, "word range past 2^32");
  hipStream_t stream = nullptr;
  RTHX_TRY(rthx::open_device(device, &stream));
  DevBuf buf;
  HIP_TRY(buf.reserve(2 * sizeof(unsigned long long)), "hipMalloc (sin theta sweep)");
  unsigned long long h[2] = {0ull, ~0ull};
  HIP_TRY(hipMemcpyAsync(buf.p, h, sizeof(h), hipMemcpyHostToDevice, stream), "hipMemcpy (sin theta sweep)");
  HIP_TRY(rthx::launch_sin_theta_sweep(w_begin, n, (unsigned long long*)buf.p, stream), "sin_theta_sweep_kernel");
  HIP_TRY(hipMemcpyAsync(h, buf.p, sizeof(h), hipMemcpyDeviceToHost, stream), "hipMemcpy (sin theta sweep)");
  HIP_TRY(hipStreamSynchronize(stream), "hipStreamSynchronize (sin theta sweep)");
  *n_diff = h[0];
  *first_diff = h[1];
  return RTHX_OK;
}

extern "C" __attribute__((visibility("default"))) int rthx_debug_sin_theta(int32_t device, const uint32_t* words,
                                                                           int64_t n, double* out) {
  if (n < 0 || ((!words || !out) && n > 0)) return fail(RTHX_EINVAL, "null or negative argument");
  if (n == 0) return RTHX_OK;
  hipStream_t stream = nullptr;
  RTHX_TRY(rthx::open_device(device, &stream));
  DevBuf dw, dout;
  HIP_TRY(dw.reserve((size_t)n * sizeof(uint32_t)), "hipMalloc (sin theta)");
  HIP_TRY(dout.reserve((size_t)n * sizeof(double)), "hipMalloc (sin theta)");
  HIP_TRY(hipMemcpyAsync(dw.p, words, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, stream), "hipMemcpy (sin theta)");
  HIP_TRY(rthx::launch_sin_theta((const uint32_t*)dw.p, n, (double*)dout.p, stream), "sin_theta_kernel");
  HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream), "hipMemcpy (sin theta)");
  HIP_TRY(hipStreamSynchronize(stream), "hipStreamSynchronize (sin theta)");
  return RTHX_OK;
}

RTHX_EXPORT int rthx_abi_version(void) { return RTHX_ABI_VERSION; }

RTHX_EXPORT const char* rthx_last_error(void) { return rthx::g_last_error.c_str(); }

RTHX_EXPORT int rthx_device_count(int32_t* count) {
  if (!count) return fail(RTHX_EINVAL, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  *count = n;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_device_synchronize(int32_t device) {
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "hipDeviceSynchronize");
  return RTHX_OK;
}

// The host work -- the descriptor's checks, the derived arrays, the grids, the
// tables and the choice and layout of the fast paths -- is build_domain2d
// (rthx_domain2d_build.h); here the knobs are read and the result is uploaded.
RTHX_EXPORT int rthx_domain_create(const rthx_domain_desc* desc, int32_t device, rthx_domain** out) {
  if (!out) return fail(RTHX_EINVAL, "null out");
  *out = nullptr;
  if (!desc) return fail(RTHX_EINVAL, "null descriptor");
  if (desc->abi_version != RTHX_ABI_VERSION) return fail(RTHX_EINVAL, "descriptor ABI version mismatch");
  const rthx_domain_desc& s = *desc;
  rthx::Domain2dOptions opt;
  opt.no_mlat = env_flag("RTHX_NO_MLAT");
  opt.no_lat = env_flag("RTHX_NO_LAT");
  // RTHX_LAT_GUESS_SCALE (tests): the first guess of the LAT cell scaled.  The
  // guess only seeds the exact search against xs / ys, so the counts are the
  // same for any scale; a scale off 1 sends most rays through the LAT ray's
  // fix-up block (rthx_device.h lat_ray_fixup).
  if (const char* gs = rthx::knob("RTHX_LAT_GUESS_SCALE")) opt.lat_guess_scale = std::strtod(gs, nullptr);
  rthx::Domain2dBuild B;
  std::string err;
  if (const int rc = rthx::build_domain2d(s, opt, B, err)) return fail(rc, err);

  RTHX_TRY(rthx::open_device(device, nullptr));  // (the stream: below, once the handle exists)
  std::unique_ptr<rthx_domain> d(new (std::nothrow) rthx_domain());
  if (!d) return fail(RTHX_ENOMEM, "host allocation failed");
  d->device = device;
  if (rthx::device_stream(device, &d->stream) != hipSuccess) return fail(RTHX_EDEVICE, "hipStreamCreate");
  for (auto& e : d->ev)
    if (hipEventCreate(&e) != hipSuccess) return fail(RTHX_EDEVICE, "hipEventCreate");

  rthx::DevDomain& D = d->D;
  const size_t nc = s.n_coarse, nf = s.n_fine;
  const std::vector<uint32_t> no_mirror(nc, 0u);  // (until rthx_domain_set_mirror_walls flags some)
  int rc = RTHX_OK;
  auto up = [&](const auto* src, size_t n, auto& dst, const char* what) {
    if (rc == RTHX_OK) rc = upload(d.get(), src, n, &dst, what);
  };
  auto up_blob = [&](const std::vector<unsigned char>& b, const uint4*& dst, const char* what) {
    up(reinterpret_cast<const uint4*>(b.data()), b.size() / 16, dst, what);
  };
  up(B.cpoly.data(), nc, D.c_poly, "D.c_poly");
  up(B.csolid.data(), nc, D.c_solid, "D.c_solid");
  up(no_mirror.data(), nc, D.c_mirror, "D.c_mirror");
  up(s.coarse_bbox, 4 * nc, D.c_bbox, "D.c_bbox");
  up(s.fine_offset, nc + 1, D.f_offset, "D.f_offset");
  up(s.fine_nv, nf, D.f_nv, "D.f_nv");
  up(B.fpoly.data(), nf, D.f_poly, "D.f_poly");
  up(s.fine_mid, 2 * nf, D.f_mid, "D.f_mid");
  up(B.trifrac.data(), nf, D.f_trifrac, "D.f_trifrac");
  up(s.fine_bbox, 4 * nf, D.f_bbox, "D.f_bbox");
  up(s.fine_surface, 4 * nf, D.f_surf, "D.f_surf");
  up(B.fcoarse.data(), nf, D.f_coarse, "D.f_coarse");
  up(B.fgrids.data(), nc, D.f_grid, "D.f_grid");
  up(reinterpret_cast<const rthx::DevCell*>(B.gcells.data()), B.gcells.size(), D.grid_cells, "D.grid_cells");
  up(B.glists.data(), B.glists.size(), D.grid_lists, "D.grid_lists");
  up(B.gitems.data(), B.gitems.size(), D.grid_items, "D.grid_items");
  up(s.beta, (size_t)s.n_bins * nf, D.beta, "D.beta");
  up(B.s_face.data(), B.s_face.size(), D.s_face, "D.s_face");
  up(B.s_wall.data(), B.s_wall.size(), D.s_wall, "D.s_wall");
  up(B.tables.data(), B.tables.size(), D.tables, "D.tables");
  // (what a fast path does not use is empty and stays a null pointer)
  up_blob(B.c_blob, D.c_blob, "D.c_blob");
  up(B.c_beta.data(), B.c_beta.size(), D.c_beta, "D.c_beta");
  up_blob(B.ml_blob, D.ml_blob, "D.ml_blob");
  up(B.ml_bbeta.data(), B.ml_bbeta.size(), D.ml_bbeta, "D.ml_bbeta");
  up_blob(B.lat_blob, D.lat_blob, "D.lat_blob");
  up(B.lat_map.data(), B.lat_map.size(), D.lat_map, "D.lat_map");
  D.n_coarse = s.n_coarse;
  D.n_fine = s.n_fine;
  D.n_surfaces = s.n_surfaces;
  D.n_bins = s.n_bins;
  D.c_grid = B.c_grid;
  D.cl = B.cl;
  D.ml = B.ml;
  D.lat = B.lat;
  up(&d->D, 1, d->d_dom, "domain record");
  if (rc) return rc;

  d->n_emitters = (int64_t)s.n_surfaces + s.n_fine;
  d->n_bins = s.n_bins;
  d->uniform_beta.assign(s.uniform_beta, s.uniform_beta + s.n_bins);
  d->beta_first = std::move(B.beta_first);
  d->single_convex = B.single_convex;
  d->axis_rect = B.axis_rect;
  d->ml_mixed = std::move(B.ml_mixed);
  d->d_mirror = const_cast<uint32_t*>(static_cast<const uint32_t*>(D.c_mirror));
  d->c_nv.assign(s.coarse_nv, s.coarse_nv + nc);
  d->c_xy.assign(s.coarse_xy, s.coarse_xy + 8 * nc);
  d->c_solid = std::move(B.csolid);
  *out = d.release();
  return RTHX_OK;
}

RTHX_EXPORT int rthx_domain_set_mirror_walls(rthx_domain* dom, const uint8_t* mirror) {
  if (!dom) return fail(RTHX_EINVAL, "null domain");
  std::vector<uint32_t> mask;
  int64_t n = 0;
  std::string err;
  if (const int rc = rthx::mirror_masks(dom->c_nv, dom->c_xy, dom->c_solid, mirror, mask, n, err)) return fail(rc, err);
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(dom->device), "hipSetDevice");
  // (stream order: after every trace enqueued on this domain; the masks are
  // in place when the call returns)
  HIP_TRY(hipMemcpyAsync(dom->d_mirror, mask.data(), mask.size() * sizeof(uint32_t), hipMemcpyHostToDevice, dom->stream),
          "hipMemcpy mirror masks");
  HIP_TRY(hipStreamSynchronize(dom->stream), "mirror masks");
  dom->n_mirror = n;
  return RTHX_OK;
}

// Whether the domain's LAT rows take the closed-enclosure copy of the LAT ray
// (lat_plain, rthx_device.h, on the host's copy of the domain record): 1 or
// 0, -1 for a domain without the lattice.  The launcher's own choice of the
// PLAINK instances (launch_of) and the tests' view of it; not part of
// include/rthx.h.
extern "C" __attribute__((visibility("default"))) int rthx_debug_lat_plain(const rthx_domain* dom) {
  if (!dom || dom->D.lat.bytes <= 0 || dom->c_solid.empty()) return -1;
  return rthx::lat_plain(dom->c_solid[0], dom->D.lat.identity) ? 1 : 0;
}

RTHX_EXPORT int rthx_domain_get_mirror_walls(const rthx_domain* dom, int64_t* n_mirror) {
  if (!dom || !n_mirror) return fail(RTHX_EINVAL, "null domain or output");
  *n_mirror = dom->n_mirror;
  return RTHX_OK;
}

RTHX_EXPORT void rthx_domain_destroy(rthx_domain* dom) {
  if (!dom) return;
  (void)hipSetDevice(dom->device);
  (void)hipStreamSynchronize(dom->stream);
  delete dom;
}

RTHX_EXPORT int rthx_result_create(rthx_result** out) {
  if (!out) return fail(RTHX_EINVAL, "null out");
  *out = new (std::nothrow) rthx_result();
  return *out ? RTHX_OK : fail(RTHX_ENOMEM, "host allocation failed");
}

RTHX_EXPORT void rthx_result_destroy(rthx_result* res) { delete res; }

namespace {

// Default bound on one look-back wait (100 MHz s_memrealtime ticks): a row
// waits for its predecessors' nnz, which are published within about one row
// time (~0.1-1 ms); a quarter second means the wait has gone wrong.
// RTHX_LB_WAIT_US overrides it (tests force the fallback with 0).
constexpr uint64_t kLookbackWaitTicks = 25'000'000;

uint64_t lookback_wait_ticks() {
  const char* e = rthx::knob("RTHX_LB_WAIT_US");
  if (e && *e) return (uint64_t)std::strtoull(e, nullptr, 10) * 100;  // 100 ticks per microsecond
  return kLookbackWaitTicks;
}

using rthx::TracePlan;  // (rthx_domain.h: a pending async trace keeps its plan)
static_assert(rthx::kTallyU16 == 1, "TracePlan::tally default");

// Hash tallies (large N): the largest table the trace kernel's LDS holds
// (keys + counts, 8 B per slot); a workgroup traces at most 3/4 as many rays.
constexpr int64_t kMaxHashCap = 16384;

// slots: resident workgroups of the unsplit launch (0: not known yet; rows
// are then split only where a row's rays need it).
int plan_trace(const rthx_domain* dom, const rthx_trace_args* a, TracePlan& p, int64_t slots = 0) {
  if (a->bin < 0 || a->bin >= dom->n_bins) return fail(RTHX_EINVAL, "bin out of range");
  if (a->rays_per_emitter < 0 || a->rays_per_emitter > 0xFFFFFFFFll)
    return fail(RTHX_ERANGE, "rays_per_emitter must be in [0, 2^32)");
  if (a->emitter_stride < 1 || a->emitter_begin < 0) return fail(RTHX_EINVAL, "bad emitter range");
  if (!std::isfinite(a->nudge)) return fail(RTHX_EINVAL, "non-finite nudge");
  if (a->n_record < 0 || (a->n_record > 0 && !a->record_ids)) return fail(RTHX_EINVAL, "bad record ids");
  // Mirror walls (rthx_domain_set_mirror_walls): the reflection lives in the
  // general multi-polygon walker only, so such a domain is planned as a
  // multi-polygon one without anything staged in LDS -- no lattice (LAT,
  // MLAT, walk_layers), no coarse mesh in LDS, no look-back -- and no
  // recording instance carries it.
  p.mirror = dom->n_mirror > 0;
  if (p.mirror && a->n_record > 0) return fail(RTHX_EINVAL, "ray recording is not supported on a domain with mirror walls");
  const bool single = dom->single_convex && !p.mirror;
  p.N = dom->n_emitters;
  p.R = a->rays_per_emitter;
  p.end = std::min<int64_t>(a->emitter_end, p.N);
  p.n_rows = p.end > a->emitter_begin ? (p.end - a->emitter_begin + a->emitter_stride - 1) / a->emitter_stride : 0;
  if (p.n_rows >= (1ll << 31)) return fail(RTHX_ERANGE, "too many rows in one call");
  const int64_t N = p.N, R = p.R;
  // Rows are split over several workgroups when there are too few rows to
  // fill the chip (or a row's rays would overflow the packed 16-bit LDS
  // counters of a large row); each workgroup then traces R/split rays.
  p.recording = a->n_record > 0 && a->record_bin == a->bin;
  p.split = 1;
  const int64_t target = env_int("RTHX_SPLIT_TARGET", slots, 0, 1 << 20);
  const int64_t split_below = env_int("RTHX_SPLIT_BELOW", 1 << 30, 1, 1 << 30);
  if (!p.recording && p.n_rows > 0 && p.n_rows < split_below && 2 * p.n_rows <= target && R >= 2 * kSplitMinRays)
    p.split = std::max<int64_t>(1, std::min<int64_t>(target / p.n_rows, R / kSplitMinRays));
  if (!p.recording && R >= 65536 && ((N + 1) / 2) * 4 + rthx::kStaticLdsBytes <= (int64_t)rthx::kMaxLdsBytes &&
      N * 4 + rthx::kStaticLdsBytes > (int64_t)rthx::kMaxLdsBytes)
    p.split = std::max<int64_t>(p.split, (R + 65534) / 65535);
  int64_t rays_per_block = p.split > 1 ? (R + p.split - 1) / p.split : R;
  p.tally = rays_per_block < 65536 ? rthx::kTallyU16 : rthx::kTallyU32;
  const int64_t words = p.tally == rthx::kTallyU16 ? (N + 1) / 2 : N;
  p.lds_bytes = (size_t)((words + 3) & ~int64_t(3)) * 4;  // (whole uint4s: the split rows' slab hand-off)
  p.row_cap = std::max<int64_t>(1, std::min<int64_t>(N, R));
  // Short rows over many emitters (C5 at 1e8 rays per band: R = 2426, N =
  // 41205): a hash table of the row's few distinct absorbers plus an N-bit
  // bitmap is less than half the packed histogram, so more workgroups fit a
  // CU and the per-row zeroing and compaction shrink: C5 12.97 -> 8.79 ms
  // per band.  Only unsplit rows (no part merge) of packed histograms.
  bool short_rows = false;
  if (p.tally == rthx::kTallyU16 && p.split == 1 && !env_flag("RTHX_NO_SHORT_HASH")) {
    int64_t h = 256;
    while (h * 75 < 100 * R) h *= 2;
    short_rows = h <= kMaxHashCap && 2 * (8 * h + 4 * ((N + 31) / 32)) <= (int64_t)p.lds_bytes;
  }
  if (p.lds_bytes + rthx::kStaticLdsBytes > rthx::kMaxLdsBytes || short_rows || env_flag("RTHX_FORCE_HASH")) {
    // Large N: the row is an LDS hash table (rthx_kernels.hip hash_tally)
    // filled at most to load_pct, so a workgroup traces at most 3/4 x
    // kMaxHashCap rays by default; longer rows are split, and their sorted
    // parts merged.
    p.tally = rthx::kTallyHash;
    const int64_t cap_max = env_int("RTHX_HASH_MAX", kMaxHashCap, 256, kMaxHashCap);
    const int64_t load_pct = env_int("RTHX_HASH_LOAD_PCT", 75, 10, 90);  // most slots a workgroup fills (A/B: tools/hash_ab.sh)
    const int64_t max_rays = cap_max * load_pct / 100;
    if (rays_per_block > max_rays) {  // (recorded rows too: the recorder indexes rays by (emitter, ray))
      p.split = (R + max_rays - 1) / max_rays;
      rays_per_block = (R + p.split - 1) / p.split;
    }
    p.hash_cap = 256;
    while (p.hash_cap * load_pct < 100 * rays_per_block) p.hash_cap *= 2;
    p.lds_bytes = (size_t)p.hash_cap * 8;
    // ascending output through an N-bit bitmap behind the table when it fits
    // (and leaves room for the single rectangle's lattice); else LDS sort
    const int64_t bm = (N + 31) / 32;
    const size_t lat = single ? (size_t)dom->D.lat.bytes + 16 : 0;
    if (p.lds_bytes + 4 * bm + lat + rthx::kStaticLdsBytes <= rthx::kMaxLdsBytes && !env_flag("RTHX_HASH_SORT")) {
      p.bm_words = bm;
      p.lds_bytes += 4 * (size_t)bm;
    }
    if (p.split > 1) {  // part lists at p * chunk
      p.row_cap = std::max<int64_t>(1, R);
      p.part_cap = (R + p.split - 1) / p.split;
      p.part_lists = true;
    }
  }
  // multi-polygon domains: the coarse mesh goes behind the histogram in LDS
  // when it fits (CLDS kernels, rthx_device.h segment_cl)
  p.cl_offset = (p.lds_bytes + 15) & ~(size_t)15;
  const bool axis = dom->axis_rect && !env_flag("RTHX_NO_AXIS");
  const bool no_clds = env_flag("RTHX_NO_CLDS");  // (tests: the global-memory multi-polygon kernels)
  if (!p.mirror && !dom->single_convex && axis && dom->D.ml.bytes > 0 && !no_clds &&
      p.cl_offset + (size_t)dom->D.ml.bytes + (size_t)rthx::kTraceThreads * rthx::kRaySlotBytes +
              rthx::kStaticLdsBytes <= rthx::kMaxLdsBytes) {
    p.clds = 2;  // multi-polygon lattice (MLAT kernels)
    p.lds_bytes = p.cl_offset + (size_t)dom->D.ml.bytes;
  } else if (!p.mirror && !dom->single_convex && dom->D.cl.bytes > 0 &&
             p.cl_offset + (size_t)dom->D.cl.bytes + rthx::kStaticLdsBytes <= rthx::kMaxLdsBytes && !no_clds) {
    p.clds = 1;
    p.lds_bytes = p.cl_offset + (size_t)dom->D.cl.bytes;
  }
  // single axis-aligned rectangles: the lattice behind the histogram (LAT kernels)
  if (single && dom->D.lat.bytes > 0 && !p.recording &&
      p.cl_offset + (size_t)dom->D.lat.bytes + rthx::kStaticLdsBytes <= rthx::kMaxLdsBytes) {
    p.clds = 1;
    p.lds_bytes = p.cl_offset + (size_t)dom->D.lat.bytes;
  }
  if (p.n_rows * p.split >= (1ll << 31)) return fail(RTHX_ERANGE, "too many workgroups in one call");
  p.uniform = dom->uniform_beta[a->bin] > -0.1;  // traceRay.jl:4
  return RTHX_OK;
}

// The kernel choice of a planned trace (launch_trace picks the variant and
// workgroup size from these); the caller adds the parameters and stream.
rthx::LaunchCfg launch_of(const rthx_domain* dom, const rthx_trace_args* a, const TracePlan& p) {
  rthx::LaunchCfg L{};
  L.D = dom->d_dom;
  L.lds_bytes = p.lds_bytes;
  L.uniform = p.uniform;
  L.tally = p.tally;
  L.threads = (int)env_int("RTHX_TRACE_THREADS", 0, 0, rthx::kMaxTraceThreads);
  L.faithful = (a->flags & RTHX_FLAG_FAITHFUL_SAMPLING) != 0;
  // (p.mirror, not the domain's present setting: a pending async trace that
  // is traced again keeps the kernels it was planned with)
  L.mirror = p.mirror;
  L.lat_plain = rthx_debug_lat_plain(dom) == 1;
  L.single = dom->single_convex && !p.mirror;
  L.clds = p.clds;
  L.axis = dom->axis_rect && !p.mirror && !env_flag("RTHX_NO_AXIS");
  L.T.split = (int32_t)p.split;
  L.T.n_rows = p.n_rows;
  L.rec.n = p.recording ? 1 : 0;
  return L;
}

// Plan of a trace with its rows split to the unsplit launch's resident
// workgroups (plan_trace): the occupancy of the unsplit plan's kernel, then
// the plan again with that slot count.
int plan_trace_split(const rthx_domain* dom, const rthx_trace_args* a, TracePlan& p) {
  int rc = plan_trace(dom, a, p);
  if (rc || p.split > 1 || p.recording || p.n_rows == 0 || p.R < 2 * kSplitMinRays) return rc;
  int64_t slots = 0;
  rthx::LaunchCfg L = launch_of(dom, a, p);
  L.slots = &slots;
  HIP_TRY(rthx::launch_trace(L), "trace kernel occupancy query");  // (a failed query is a real HIP error)
  if (slots <= 0) return RTHX_OK;  // (no resident slot reported: the plan without a slot split)
  return plan_trace(dom, a, p, slots);
}

// One launch sequence of a planned trace.  lookback: the trace kernel writes
// the final CSR itself (decoupled look-back over the rows); otherwise rows go
// to staging slots, then row_scan + csr_pack.  Fills totals (see
// finish_staged; totals[3] > 0: a look-back wait gave up).
int run_trace(rthx_domain* dom, const rthx_trace_args* a, const TracePlan& p, rthx_result* res, bool lookback,
              const rthx::RecordParams& rec, int64_t totals[rthx::kLbTotals], float* ms_trace, float* ms_pack,
              bool async = false, bool check_prev = false) {
  const int64_t n_rows = p.n_rows, N = p.N, R = p.R;
  hipStream_t st = dom->stream;
  HIP_TRY(res->row_nnz.reserve((size_t)n_rows * 4), "hipMalloc row_nnz");
  HIP_TRY(res->row_tallied.reserve((size_t)n_rows * 4), "hipMalloc row_tallied");
  HIP_TRY(res->row_off.reserve((size_t)(n_rows + 1) * 8), "hipMalloc row_off");
  HIP_TRY(res->totals.reserve(4 * 8), "hipMalloc totals");
  // Staging slots only when the rows are staged.  The direct CSR writes
  // cols / counts in place: sized from the nnz of the previous launch of the
  // same shape (N, rows, R) plus an eighth, or else from a guess (2048
  // entries per row); rows that would end past them write nothing and
  // flag an overflow, and the host then traces the launch again with the
  // exact size, which the look-back's prefix sums give (trace_exchange_one).
  // Never more than the worst case n_rows x min(N, R).
  if (lookback) {
    res->stage_cols.release();
    res->stage_cnt.release();
    const int64_t worst = n_rows * p.row_cap;
    const bool same = res->lb_hint_shape[0] == N && res->lb_hint_shape[1] == n_rows && res->lb_hint_shape[2] == R;
    // (a first launch of a shape reserves the worst case when it is at most
    // 256 Mi entries -- 2 GiB of columns and counts; C2: 100 M entries, 800
    // MB -- so it never re-traces; round 3's 2048 entries per row made the
    // first C2 launch overflow and trace twice, profiles/round4/overflow_cost.json.
    // The second launch shrinks the buffers to the measured nnz + 1/8.)
    const int64_t first_guess = worst <= (int64_t(1) << 28) ? worst : std::max<int64_t>(1 << 20, n_rows * std::min<int64_t>(p.row_cap, 4096));
    int64_t want = same && res->lb_nnz_hint > 0
                       ? res->lb_nnz_hint + res->lb_nnz_hint / 8 + 65536
                       : env_int("RTHX_CSR_CAP", first_guess, 1, worst);  // (tests force a small first guess)
    want = std::min<int64_t>(worst, want);
    want = std::max<int64_t>(want, 1);
    for (rthx::DevBuf* b : {&res->cols, &res->cnt}) {
      if (b->cap > 2 * (size_t)want * 4 + (64u << 20)) b->release();  // (a much larger earlier trace, or the worst-case first guess of this shape)
      HIP_TRY(b->reserve((size_t)want * 4), "hipMalloc direct CSR");
    }
    // fresh words or totals (or a wrapped epoch): zero them once, epoch 1
    const size_t lb_bytes = (size_t)n_rows * 8;
    if (!res->lb_status.p || lb_bytes > res->lb_status.cap || !res->lb_totals.p) res->lb_epoch = 0;
    HIP_TRY(res->lb_status.reserve(lb_bytes), "hipMalloc look-back words");
    HIP_TRY(res->lb_totals.reserve(2 * 8 * 8), "hipMalloc look-back totals");  // (2 sets of kLbTotals <= 8)
    HIP_TRY(res->h_totals.reserve(8 * 8), "hipHostMalloc totals");
  } else {
    res->lb_status.release();
    res->lb_totals.release();
    res->lb_epoch = 0;
    HIP_TRY(res->stage_cols.reserve((size_t)n_rows * p.row_cap * 4), "hipMalloc stage_cols");
    HIP_TRY(res->stage_cnt.reserve((size_t)n_rows * p.row_cap * 4), "hipMalloc stage_cnt");
  }
  // split rows: (hash part lists) the part merge's scratch [2][n_rows][row_cap]
  // followed by part_nnz [n_rows][split]; (histograms) one slab of the
  // histogram's words (rounded to uint4s) per part, [n_rows][split][words4],
  // the parts' tallied counts [n_rows][split] and the arrival counters
  // [n_rows] (zero between launches: zeroed when allocated)
  const int64_t hist_words4 = ((p.tally == rthx::kTallyU16 ? (N + 1) / 2 : N) + 3) & ~int64_t(3);
  const int64_t split_rows = n_rows;
  const size_t dense_bytes = p.part_lists ? (size_t)n_rows * p.row_cap * 8 + (size_t)n_rows * p.split * 4
                                          : (size_t)split_rows * p.split * (hist_words4 + 1) * 4;
  if (p.split > 1) HIP_TRY(res->dense.reserve(dense_bytes), "hipMalloc dense rows");
  else res->dense.release();
  if (p.split > 1 && !p.part_lists) {
    // (zeroed whenever reserve allocates: a grown buffer may come back at the
    // same address, so the pointer alone does not tell)
    bool fresh = false;
    HIP_TRY(res->arrive.reserve((size_t)split_rows * 4, &fresh), "hipMalloc arrival counters");
    if (fresh) HIP_TRY(hipMemsetAsync(res->arrive.p, 0, res->arrive.cap, st), "hipMemset arrivals");
  }

  rthx::TraceParams P{};
  P.R = R;
  P.ray_base = p.ray_base;
  P.g_begin = a->emitter_begin;
  P.g_stride = a->emitter_stride;
  P.eta = a->nudge;
  P.key0 = (uint32_t)a->seed;
  P.key1 = (uint32_t)(a->seed >> 32);
  P.bin = a->bin;
  P.mixed = p.clds == 2 && !dom->ml_mixed.empty() ? dom->ml_mixed[a->bin] : 1;
  P.beta_uniform = dom->beta_first[a->bin];
  P.inv_beta_uniform = P.beta_uniform > 0 ? 1.0 / P.beta_uniform : HUGE_VAL;

  rthx::TallyParams T{};
  T.n_emitters = N;
  T.n_rows = n_rows;
  T.row_cap = p.row_cap;
  T.split = (int32_t)p.split;
  T.cl_offset = p.clds ? (int32_t)p.cl_offset : 0;
  T.stage_cols = res->stage_cols.as<uint32_t>();
  T.stage_cnt = res->stage_cnt.as<uint32_t>();
  T.row_nnz = res->row_nnz.as<uint32_t>();
  T.row_tallied = res->row_tallied.as<uint32_t>();
  T.dense = p.split > 1 ? res->dense.as<uint32_t>() : nullptr;
  T.part_nnz = p.split > 1 && p.part_lists ? T.dense + 2 * (size_t)n_rows * p.row_cap : nullptr;
  T.row_arrive = p.split > 1 && !p.part_lists ? res->arrive.as<uint32_t>() : nullptr;
  T.part_tallied = T.row_arrive ? T.dense + (size_t)split_rows * p.split * hist_words4 : nullptr;
  T.part_cap = p.part_cap;
  T.hash_cap = (int32_t)p.hash_cap;
  int32_t shift = 32;
  for (int64_t c = p.hash_cap; c > 1; c >>= 1) --shift;
  T.hash_shift = shift;
  T.bm_words = p.bm_words;
  T.R = R;
  if (lookback) {
    T.lb_status = res->lb_status.as<unsigned long long>();
    T.lb_wait_ticks = lookback_wait_ticks();
    T.out_cols = res->cols.as<uint32_t>();
    T.out_cnt = res->cnt.as<uint32_t>();
    T.out_cap = (int64_t)(std::min(res->cols.cap, res->cnt.cap) / 4);
    T.row_off = res->row_off.as<int64_t>();
    // The words carry the launch's epoch and row 0 zeroes the other set of
    // totals for the next launch, so nothing is zeroed between launches but
    // at the first and after 65535 (the epoch's wrap).
    uint32_t e = res->lb_epoch;
    if (e == 0 || e >= rthx::kLbEpochMax) {
      HIP_TRY(hipMemsetAsync(T.lb_status, 0, res->lb_status.cap, st), "hipMemset look-back words");
      HIP_TRY(hipMemsetAsync(res->lb_totals.p, 0, 2 * 8 * 8, st), "hipMemset look-back totals");
      e = 0;
      check_prev = false;  // (trace_exchange_one absorbed a replaced launch on the host: lb_chain_ok)
    }
    T.check_prev = check_prev ? 1u : 0u;
    ++e;
    res->lb_epoch = 0;  // set again once the launch has completed
    T.lb_epoch = e;
    T.totals = res->lb_totals.as<unsigned long long>() + 8 * (e & 1);
    T.totals_next = res->lb_totals.as<unsigned long long>() + 8 * ((e + 1) & 1);
  } else {
    HIP_TRY(hipMemsetAsync(res->totals.p, 0, 32, st), "hipMemset totals");
  }
  if (p.split > 1 && p.part_lists && n_rows > 0)
    HIP_TRY(hipMemsetAsync(T.row_tallied, 0, (size_t)n_rows * 4, st), "hipMemset row_tallied");
  // (async: the result's own events, read when the result completes)
  hipEvent_t ev0 = async ? res->pend_ev[0] : dom->ev[0], ev1 = async ? res->pend_ev[1] : dom->ev[1];
  HIP_TRY(hipEventRecord(ev0, st), "hipEventRecord");
  if (n_rows > 0) {
    rthx::LaunchCfg L = launch_of(dom, a, p);
    L.P = P;
    L.T = T;
    L.rec = rec;
    L.stream = st;
    HIP_TRY(rthx::launch_trace(L), "trace_exchange_kernel launch");
  }
  HIP_TRY(hipEventRecord(ev1, st), "hipEventRecord");
  if (lookback && async) {  // (complete_pending reads the totals back)
    res->pend_totals = T.totals;
    res->lb_epoch = T.lb_epoch;
    return RTHX_OK;
  }
  if (lookback) {
    HIP_TRY(hipEventRecord(dom->ev[2], st), "hipEventRecord");
    // (a last-row hand-over of the totals into page-locked memory, counting
    // finished rows with one more atomic per row, measured 14 us slower per
    // launch than this copy: profiles/round2/hosttot_ab.txt)
    HIP_TRY(hipMemcpyAsync(res->h_totals.p, T.totals, 8 * rthx::kLbTotals, hipMemcpyDeviceToHost, st),
            "hipMemcpy totals");
    HIP_TRY(hipStreamSynchronize(st), "trace kernel");
    std::memcpy(totals, res->h_totals.p, 8 * rthx::kLbTotals);
    res->lb_epoch = T.lb_epoch;
  } else {
    const int merge = p.part_lists ? rthx::kMergeParts : rthx::kNoMerge;
    int rc = rthx::finish_staged(res, T, merge, st, dom->ev[2], totals);
    if (rc) return rc;
  }
  HIP_TRY(hipEventElapsedTime(ms_trace, dom->ev[0], dom->ev[1]), "hipEventElapsedTime");
  HIP_TRY(hipEventElapsedTime(ms_pack, dom->ev[1], dom->ev[2]), "hipEventElapsedTime");
  return RTHX_OK;
}

// The look-back words and totals of `res` serve a launch of n_rows without
// being zeroed first (run_trace's epoch test, reserve sizes).
bool lb_chain_ok(const rthx_result* res, int64_t n_rows) {
  return res->lb_status.p && (size_t)n_rows * 8 <= res->lb_status.cap && res->lb_totals.p && res->lb_epoch != 0 &&
         res->lb_epoch < rthx::kLbEpochMax;
}

int finish_trace(rthx_domain* dom, const rthx_trace_args* a, const TracePlan& p, rthx_result* res, bool lookback,
                 const rthx::RecordParams& rec, int64_t totals[rthx::kLbTotals], float ms_trace, float ms_pack,
                 double t0);

// The whole of one device's trace (validated arguments, any device state).
// ray_begin: the first ray id of every row (rthx_trace_exchange_rays); it
// travels in the plan, so a re-trace or a completed async launch keeps it.
int trace_exchange_one(rthx_domain* dom, const rthx_trace_args* a, rthx_result* res, int64_t ray_begin = 0) {
  const double t0 = now_ms();
  HIP_TRY(hipSetDevice(dom->device), "hipSetDevice");
  // An unread async trace on this result is replaced by this one (stream
  // order keeps its launch before this one).  The result reads as empty
  // until this trace is done, whatever happens below.
  const bool superseding = res->pending;
  res->valid = false;
  TracePlan p;
  p.ray_base = ray_begin;
  int rc = plan_trace_split(dom, a, p);
  if (rc) return rc;
  if (res->device >= 0 && res->device != dom->device) return fail(RTHX_EINVAL, "result bound to another device");
  const int64_t R = p.R, n_rows = p.n_rows;
  rthx::reset_result(res, dom->device, p.N, R, n_rows, a->emitter_begin, a->emitter_stride, p.split);

  // recorded emitters traced by this call (ascending, unique)
  if (p.recording) {
    for (int i = 0; i < a->n_record; ++i) {
      const int64_t g = a->record_ids[i];
      if (g >= a->emitter_begin && g < p.end && (g - a->emitter_begin) % a->emitter_stride == 0)
        res->rec_g.push_back(g);
    }
    std::sort(res->rec_g.begin(), res->rec_g.end());
    res->rec_g.erase(std::unique(res->rec_g.begin(), res->rec_g.end()), res->rec_g.end());
  }
  const size_t n_rec = res->rec_g.size();
  rthx::RecordParams rec{};
  if (n_rec > 0) {
    HIP_TRY(res->rec_ids.reserve(n_rec * 8), "hipMalloc rec_ids");
    HIP_TRY(res->rec_ok.reserve(n_rec * (size_t)R), "hipMalloc rec_ok");
    HIP_TRY(res->rec_orig.reserve(n_rec * (size_t)R * 16), "hipMalloc rec_orig");
    HIP_TRY(res->rec_end.reserve(n_rec * (size_t)R * 16), "hipMalloc rec_end");
    HIP_TRY(hipMemcpyAsync(res->rec_ids.p, res->rec_g.data(), n_rec * 8, hipMemcpyHostToDevice, dom->stream),
            "hipMemcpy rec ids");
    rec.n = (int32_t)n_rec;
    rec.ids = res->rec_ids.as<int64_t>();
    rec.ok = res->rec_ok.as<uint8_t>();
    rec.orig = res->rec_orig.as<double>();
    rec.end = res->rec_end.as<double>();
  }

  // Unsplit launches on single-polygon domains write rows straight into the
  // final CSR (decoupled look-back); RTHX_NO_LOOKBACK=1 keeps the staging +
  // scan + pack sequence.  Multi-polygon domains keep it too: their rows
  // finish at widely different times (rays cross different numbers of
  // layers), and a row waiting on a slower predecessor idles its CU slot
  // (C5 greenhouse: 15.2 -> 17.6 ms per band with the look-back).  The
  // recorder's kernels stage.
  const bool lookback = !p.part_lists && n_rows > 0 && dom->single_convex && !p.mirror && !p.recording &&
                        (uint64_t)n_rows * (uint64_t)p.row_cap <= rthx::kLbValMax && !env_flag("RTHX_NO_LOOKBACK");
  // The replaced launch's stall / overflow flags: read by this launch's row 0
  // when it uses the same look-back totals without zeroing them (run_trace),
  // else on the host now, before its buffers are reused.
  bool check_prev = false;
  if (superseding) {
    if (lookback && lb_chain_ok(res, n_rows)) {
      res->pending = false;
      res->sup_count += 1;
      check_prev = true;
    } else {
      rc = rthx::absorb_superseded(res);
      if (rc) return rc;
    }
  }
  int64_t totals[rthx::kLbTotals] = {0, 0, 0, 0, 0};
  float ms_trace = 0.f, ms_pack = 0.f;
  // RTHX_FLAG_ASYNC: enqueue only, when the direct CSR is sized from an
  // earlier launch of this shape (no overflow expected); the checks and the
  // info wait for the first read (complete_pending)
  const bool async = (a->flags & RTHX_FLAG_ASYNC) && lookback && n_rec == 0 && res->lb_nnz_hint > 0 &&
                     res->lb_hint_shape[0] == p.N && res->lb_hint_shape[1] == n_rows && res->lb_hint_shape[2] == R;
  if (async) {
    for (auto& e : res->pend_ev)
      if (!e) HIP_TRY(hipEventCreate(&e), "hipEventCreate");
    rc = run_trace(dom, a, p, res, true, rec, totals, &ms_trace, &ms_pack, true, check_prev);
    if (rc) return rc;
    res->pending = true;
    res->pend_plan = p;
    res->pend_dom = dom;
    res->pend_args = *a;
    res->pend_args.n_record = 0;
    res->pend_args.record_ids = nullptr;
    res->pend_t0 = t0;
    res->valid = true;
    return RTHX_OK;
  }
  rc = run_trace(dom, a, p, res, lookback, rec, totals, &ms_trace, &ms_pack, false, check_prev);
  if (rc) return rc;
  return finish_trace(dom, a, p, res, lookback, rec, totals, ms_trace, ms_pack, t0);
}

// The checks after a look-back or staged launch (overflow or stall: the same
// launch traced again), the size hint for the next launch, the info and the
// row offsets on the host.
int finish_trace(rthx_domain* dom, const rthx_trace_args* a, const TracePlan& p, rthx_result* res, bool lookback,
                 const rthx::RecordParams& rec, int64_t totals[rthx::kLbTotals], float ms_trace, float ms_pack,
                 double t0) {
  int rc = RTHX_OK;
  const int64_t R = p.R, n_rows = p.n_rows;
  const size_t n_rec = res->rec_g.size();
  const int64_t chained_faults = lookback ? totals[5] : 0;  // (replaced async launches, TallyParams::check_prev)
  if (lookback && totals[3] == 0 && totals[4] != 0) {
    // Rows outgrew the reserved direct CSR: the look-back's totals hold the
    // exact nnz, so the same launch -- same draws, same counts -- is traced
    // again into buffers of that size.
    res->info.lookback_fallbacks += 1;
    res->lb_nnz_hint = totals[0];
    res->lb_hint_shape[0] = p.N;
    res->lb_hint_shape[1] = n_rows;
    res->lb_hint_shape[2] = R;
    float ms2 = 0.f, mp2 = 0.f;
    rc = run_trace(dom, a, p, res, true, rec, totals, &ms2, &mp2);
    if (rc) return rc;
    ms_trace += ms2;
    ms_pack += mp2;
    if (totals[4] != 0) return fail(RTHX_ESTATE, "direct CSR overflow after resizing");
  }
  if (lookback && totals[3] != 0) {
    // A look-back wait gave up (a predecessor row did not publish its nnz in
    // time): the direct CSR may be misplaced, so the same launch -- same
    // draws, same counts -- is traced again on the staging path.
    res->info.lookback_fallbacks += 1;
    float ms2 = 0.f, mp2 = 0.f;
    rc = run_trace(dom, a, p, res, false, rec, totals, &ms2, &mp2);
    if (rc) return rc;
    ms_trace += ms2;
    ms_pack += mp2;
  }
  if (lookback) {
    res->lb_nnz_hint = totals[0];
    res->lb_hint_shape[0] = p.N;
    res->lb_hint_shape[1] = n_rows;
    res->lb_hint_shape[2] = R;
  }
  res->info.nnz = totals[0];
  res->info.lost_total = totals[1];
  res->info.lost_max_row = totals[2];
  res->info.trace_ms = ms_trace;
  res->info.pack_ms = ms_pack;
  rthx::take_superseded(res, chained_faults);

  if (!(a->flags & RTHX_FLAG_DEVICE_ONLY)) {
    res->h_row_off.resize(n_rows + 1);
    HIP_TRY(hipMemcpy(res->h_row_off.data(), res->row_off.p, (n_rows + 1) * 8, hipMemcpyDeviceToHost),
            "hipMemcpy row_off");
    res->host_row_off = true;
  }
  int64_t nrec = 0;
  if (n_rec > 0) {
    res->h_ok.resize(n_rec * (size_t)R);
    HIP_TRY(hipMemcpy(res->h_ok.data(), res->rec_ok.p, n_rec * (size_t)R, hipMemcpyDeviceToHost), "hipMemcpy rec");
    for (uint8_t v : res->h_ok) nrec += v;
  }
  res->info.n_recorded = nrec;
  res->valid = true;
  res->info.total_ms = now_ms() - t0;
  return RTHX_OK;
}

// A result traced with RTHX_FLAG_ASYNC, on its first read: its totals back
// from the device, then the same checks and info as a blocking trace
// (finish_trace: an overflowed or stalled launch is traced again here).
int complete_pending(rthx_result* res) {
  if (!res->pending) return RTHX_OK;
  res->pending = false;
  rthx_domain* dom = res->pend_dom;
  const rthx_trace_args* a = &res->pend_args;
  HIP_TRY(hipSetDevice(dom->device), "hipSetDevice");
  HIP_TRY(res->h_totals.reserve(8 * 8), "hipHostMalloc totals");
  HIP_TRY(hipMemcpyAsync(res->h_totals.p, res->pend_totals, 8 * rthx::kLbTotals, hipMemcpyDeviceToHost, dom->stream),
          "hipMemcpy totals");
  HIP_TRY(hipStreamSynchronize(dom->stream), "trace kernel");
  int64_t totals[rthx::kLbTotals];
  std::memcpy(totals, res->h_totals.p, 8 * rthx::kLbTotals);
  float ms_trace = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms_trace, res->pend_ev[0], res->pend_ev[1]), "hipEventElapsedTime");
  res->valid = false;
  // (the launched plan, not a new one: environment knobs or the occupancy
  // query must not change what finish_trace checks or re-traces)
  return finish_trace(dom, a, res->pend_plan, res, true, rthx::RecordParams{}, totals, ms_trace, 0.f, res->pend_t0);
}

// A result that can be read: traced, and a pending async trace completed.
int ready(const rthx_result* cres) {
  if (!cres) return fail(RTHX_EINVAL, "null result");
  if (!cres->valid) return fail(RTHX_ESTATE, "result holds no trace");
  rthx::DeviceGuard keep_device;
  return complete_pending(const_cast<rthx_result*>(cres));
}

int fetch_row_off(rthx_result* res) {
  if (res->host_row_off) return RTHX_OK;
  HIP_TRY(hipSetDevice(res->device), "hipSetDevice");
  res->h_row_off.resize(res->n_rows + 1);
  HIP_TRY(hipMemcpy(res->h_row_off.data(), res->row_off.p, (res->n_rows + 1) * 8, hipMemcpyDeviceToHost),
          "hipMemcpy row_off");
  res->host_row_off = true;
  return RTHX_OK;
}

int fetch_rays(rthx_result* res) {
  const size_t n_rec = res->rec_g.size(), R = (size_t)res->R;
  if (n_rec == 0 || res->host_rec) return RTHX_OK;
  HIP_TRY(hipSetDevice(res->device), "hipSetDevice");
  res->h_orig.resize(n_rec * R * 2);
  res->h_end.resize(n_rec * R * 2);
  HIP_TRY(hipMemcpy(res->h_orig.data(), res->rec_orig.p, n_rec * R * 16, hipMemcpyDeviceToHost), "hipMemcpy rec");
  HIP_TRY(hipMemcpy(res->h_end.data(), res->rec_end.p, n_rec * R * 16, hipMemcpyDeviceToHost), "hipMemcpy rec");
  res->host_rec = true;
  return RTHX_OK;
}

// Run f(d) for every device part on its own host thread; the first error
// (with its thread-local message) is returned on the calling thread.
template <class F>
int for_each_part(size_t n, F f) {
  std::vector<int> rc(n, RTHX_OK);
  std::vector<std::string> msg(n);
  std::vector<std::thread> th;
  th.reserve(n);
  for (size_t d = 0; d < n; ++d)
    th.emplace_back([&, d] {
      rc[d] = f(d);
      if (rc[d]) msg[d] = rthx::g_last_error;
    });
  for (auto& t : th) t.join();
  for (size_t d = 0; d < n; ++d)
    if (rc[d]) return fail(rc[d], msg[d]);
  return RTHX_OK;
}

}  // namespace

namespace rthx {
int result_ready(const rthx_result* res) { return ready(res); }

int absorb_superseded(rthx_result* res) {
  if (!res->pending) return RTHX_OK;
  res->pending = false;
  res->valid = false;
  rthx_domain* dom = res->pend_dom;
  HIP_TRY(hipSetDevice(dom->device), "hipSetDevice");
  HIP_TRY(res->h_totals.reserve(8 * 8), "hipHostMalloc totals");
  HIP_TRY(hipMemcpyAsync(res->h_totals.p, res->pend_totals, 8 * kLbTotals, hipMemcpyDeviceToHost, dom->stream),
          "hipMemcpy totals");
  HIP_TRY(hipStreamSynchronize(dom->stream), "replaced trace");
  const int64_t* t = static_cast<const int64_t*>(res->h_totals.p);
  res->sup_count += 1;
  res->sup_faults += (int32_t)(((t[3] | t[4]) != 0 ? 1 : 0) + t[5]);
  return RTHX_OK;
}

void take_superseded(rthx_result* res, int64_t chained_faults) {
  res->info.superseded = res->sup_count;
  res->info.superseded_faults = res->sup_faults + (int32_t)chained_faults;
  res->sup_count = res->sup_faults = 0;
}
}  // namespace rthx

RTHX_EXPORT int rthx_trace_exchange(rthx_domain* dom, const rthx_trace_args* a, rthx_result* res) {
  if (!dom || !a || !res) return fail(RTHX_EINVAL, "null argument");
  if (a->device != dom->device) return fail(RTHX_EINVAL, "args.device differs from the domain's device");
  return trace_exchange_one(dom, a, res);
}

RTHX_EXPORT int rthx_trace_exchange_rays(rthx_domain* dom, const rthx_trace_args* a, int64_t ray_begin,
                                         rthx_result* res) {
  // (the ray range first: it is checked whatever else the call was given)
  if (!a) return fail(RTHX_EINVAL, "null argument");
  if (ray_begin < 0) return fail(RTHX_EINVAL, "negative ray_begin");
  if (a->rays_per_emitter < 0 || a->rays_per_emitter > 0xFFFFFFFFll)
    return fail(RTHX_ERANGE, "rays_per_emitter must be in [0, 2^32)");
  if (ray_begin > 0xFFFFFFFFll || ray_begin + a->rays_per_emitter > 0xFFFFFFFFll)
    return fail(RTHX_ERANGE, "ray_begin + rays_per_emitter must be below 2^32");
  if (!dom || !res) return fail(RTHX_EINVAL, "null argument");
  if (a->device != dom->device) return fail(RTHX_EINVAL, "args.device differs from the domain's device");
  return trace_exchange_one(dom, a, res, ray_begin);
}

RTHX_EXPORT int rthx_result_get_info(const rthx_result* res, rthx_result_info* info) {
  if (!res || !info) return fail(RTHX_EINVAL, "null argument");
  if (int rc = ready(res)) return rc;
  *info = res->info;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_host_register(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(RTHX_EINVAL, "null or empty host range");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable), "hipHostRegister");
  return RTHX_OK;
}

RTHX_EXPORT int rthx_host_unregister(void* ptr) {
  if (!ptr) return fail(RTHX_EINVAL, "null pointer");
  HIP_TRY(hipHostUnregister(ptr), "hipHostUnregister");
  return RTHX_OK;
}

namespace {

// Global CSR row pointers over all N rows of a single-device result: rows
// g = begin + k * stride hold slot k, every other row is empty.
void expand_row_ptr(const rthx_result* res, int64_t* row_ptr) {
  row_ptr[0] = 0;
  int64_t k = 0;
  for (int64_t g = 0; g < res->N; ++g) {
    int64_t n = 0;
    if (k < res->n_rows && g == res->begin + k * res->stride) {
      n = res->h_row_off[k + 1] - res->h_row_off[k];
      ++k;
    }
    row_ptr[g + 1] = row_ptr[g] + n;
  }
}

// D2H of one single-device result's cols / counts / F values (nnz entries
// each) to the given host arrays (any may be null).  F values are formed on
// the device first (counts_to_F_kernel).
int copy_part_csr(rthx_result* res, int32_t* cols, uint32_t* counts, double* vals) {
  const size_t nnz = (size_t)res->info.nnz;
  if (nnz == 0) return RTHX_OK;
  HIP_TRY(hipSetDevice(res->device), "hipSetDevice");
  if (vals) {
    HIP_TRY(res->fvals.reserve(nnz * 8), "hipMalloc F values");
    HIP_TRY(rthx::launch_counts_to_F(res->row_off.as<int64_t>(), res->cnt.as<uint32_t>(), res->n_rows,
                                     res->fvals.as<double>(), nullptr),
            "counts_to_F_kernel launch");
    HIP_TRY(hipMemcpy(vals, res->fvals.p, nnz * 8, hipMemcpyDeviceToHost), "hipMemcpy F values");
  }
  if (cols) HIP_TRY(hipMemcpy(cols, res->cols.p, nnz * 4, hipMemcpyDeviceToHost), "hipMemcpy cols");
  if (counts) HIP_TRY(hipMemcpy(counts, res->cnt.p, nnz * 4, hipMemcpyDeviceToHost), "hipMemcpy counts");
  return RTHX_OK;
}

// rthx_result_copy_csr / rthx_result_copy_F: row pointers over all N rows,
// then per device its entries -- straight into place for contiguous row
// blocks, through pinned bounce buffers and a row scatter for interleaved ones.
int copy_result(rthx_result* res, int64_t* row_ptr, int32_t* cols, uint32_t* counts, double* vals) {
  if (res->parts.empty()) {
    int rc = copy_part_csr(res, cols, counts, vals);
    if (rc) return rc;
    if (row_ptr) {
      if ((rc = fetch_row_off(res))) return rc;
      expand_row_ptr(res, row_ptr);
    }
    return RTHX_OK;
  }
  const size_t nd = res->parts.size();
  int rc = for_each_part(nd, [&](size_t d) { return fetch_row_off(res->parts[d]); });
  if (rc) return rc;
  // global row pointers: part d's slot k is row g = begin_d + k * stride_d
  std::vector<int64_t> len(res->N, 0);
  for (rthx_result* q : res->parts)
    for (int64_t k = 0; k < q->n_rows; ++k) len[q->begin + k * q->stride] = q->h_row_off[k + 1] - q->h_row_off[k];
  std::vector<int64_t> rp_local;
  int64_t* rp = row_ptr;
  if (!rp) {
    rp_local.resize(res->N + 1);
    rp = rp_local.data();
  }
  rp[0] = 0;
  for (int64_t g = 0; g < res->N; ++g) rp[g + 1] = rp[g] + len[g];
  if (!cols && !counts && !vals) return RTHX_OK;
  if (!res->interleaved) {
    return for_each_part(nd, [&](size_t d) {
      rthx_result* q = res->parts[d];
      const int64_t off = q->n_rows > 0 ? rp[q->begin] : 0;
      return copy_part_csr(q, cols ? cols + off : nullptr, counts ? counts + off : nullptr, vals ? vals + off : nullptr);
    });
  }
  return for_each_part(nd, [&](size_t d) {
    rthx_result* q = res->parts[d];
    const size_t nnz = (size_t)q->info.nnz;
    if (nnz == 0) return (int)RTHX_OK;
    HIP_TRY(hipSetDevice(q->device), "hipSetDevice");
    int32_t* bc = nullptr;
    uint32_t* bn = nullptr;
    double* bv = nullptr;
    if (cols) {
      HIP_TRY(q->h_cols.reserve(nnz * 4), "hipHostMalloc cols");
      bc = static_cast<int32_t*>(q->h_cols.p);
    }
    if (counts) {
      HIP_TRY(q->h_cnt.reserve(nnz * 4), "hipHostMalloc counts");
      bn = static_cast<uint32_t*>(q->h_cnt.p);
    }
    if (vals) {
      HIP_TRY(q->h_vals.reserve(nnz * 8), "hipHostMalloc F values");
      bv = static_cast<double*>(q->h_vals.p);
    }
    int r2 = copy_part_csr(q, bc, bn, bv);
    if (r2) return r2;
    for (int64_t k = 0; k < q->n_rows; ++k) {
      const int64_t g = q->begin + k * q->stride, a0 = q->h_row_off[k], n = q->h_row_off[k + 1] - a0;
      if (cols) std::memcpy(cols + rp[g], bc + a0, n * 4);
      if (counts) std::memcpy(counts + rp[g], bn + a0, n * 4);
      if (vals) std::memcpy(vals + rp[g], bv + a0, n * 8);
    }
    return (int)RTHX_OK;
  });
}

}  // namespace

RTHX_EXPORT int rthx_result_copy_csr(const rthx_result* cres, int64_t* row_ptr, int32_t* cols, uint32_t* counts) {
  if (int rc = ready(cres)) return rc;
  return copy_result(const_cast<rthx_result*>(cres), row_ptr, cols, counts, nullptr);
}

RTHX_EXPORT int rthx_result_copy_F(const rthx_result* cres, int64_t* row_ptr, int32_t* cols, double* vals) {
  if (int rc = ready(cres)) return rc;
  return copy_result(const_cast<rthx_result*>(cres), row_ptr, cols, nullptr, vals);
}

namespace {
// Block `part` of a result (itself for a one-device trace).
int device_block(const rthx_result* cres, int32_t part, rthx_result** out, int32_t* n_parts) {
  if (int rc = ready(cres)) return rc;
  rthx_result* res = const_cast<rthx_result*>(cres);
  const int32_t np = res->parts.empty() ? 1 : (int32_t)res->parts.size();
  if (part < 0 || part >= np) return fail(RTHX_EINVAL, "part out of range");
  *out = res->parts.empty() ? res : res->parts[part];
  if (n_parts) *n_parts = np;
  return RTHX_OK;
}
}  // namespace

RTHX_EXPORT int rthx_result_get_device_csr(const rthx_result* cres, int32_t part, rthx_device_csr* out) {
  if (!out) return fail(RTHX_EINVAL, "null output");
  rthx_result* q = nullptr;
  int32_t np = 1;
  int rc = device_block(cres, part, &q, &np);
  if (rc) return rc;
  *out = rthx_device_csr{};
  out->device = q->device;
  out->n_parts = np;
  out->n_rows = q->n_rows;
  out->nnz = q->info.nnz;
  out->emitter_begin = q->begin;
  out->emitter_stride = q->stride;
  out->row_off = q->row_off.as<int64_t>();
  out->cols = q->cols.as<uint32_t>();
  out->counts = q->cnt.as<uint32_t>();
  return RTHX_OK;
}

RTHX_EXPORT int rthx_result_copy_csr_device(const rthx_result* cres, int32_t part, int64_t* row_off, uint32_t* cols,
                                            uint32_t* counts) {
  rthx_result* q = nullptr;
  int rc = device_block(cres, part, &q, nullptr);
  if (rc) return rc;
  rthx::DeviceGuard keep_device;  // (the caller's current device, e.g. torch's, is restored)
  HIP_TRY(hipSetDevice(q->device), "hipSetDevice");
  // (the library's copy stream: the trace is complete -- device_block waited
  // for it -- and the next trace, on the device stream, need not wait for this copy)
  hipStream_t st = nullptr;
  HIP_TRY(rthx::copy_stream(q->device, &st), "copy stream");
  const size_t nnz = (size_t)q->info.nnz;
  if (row_off && q->n_rows >= 0)
    HIP_TRY(hipMemcpyAsync(row_off, q->row_off.p, (size_t)(q->n_rows + 1) * 8, hipMemcpyDeviceToDevice, st),
            "hipMemcpy row_off D2D");
  if (cols && nnz) HIP_TRY(hipMemcpyAsync(cols, q->cols.p, nnz * 4, hipMemcpyDeviceToDevice, st), "hipMemcpy cols D2D");
  if (counts && nnz)
    HIP_TRY(hipMemcpyAsync(counts, q->cnt.p, nnz * 4, hipMemcpyDeviceToDevice, st), "hipMemcpy counts D2D");
  HIP_TRY(hipStreamSynchronize(st), "device CSR copy");
  return RTHX_OK;
}

RTHX_EXPORT int rthx_result_copy_rays(const rthx_result* cres, double* origins_xy, double* endpoints_xy,
                                      int64_t* emitter, int64_t cap, int64_t* n_out) {
  if (int rc = ready(cres)) return rc;
  rthx_result* res = const_cast<rthx_result*>(cres);
  // (emitter, part, index in part) of every recorded emitter, ascending emitter
  std::vector<rthx_result*> srcs = res->parts.empty() ? std::vector<rthx_result*>{res} : res->parts;
  std::vector<std::pair<int64_t, std::pair<size_t, size_t>>> order;
  for (size_t d = 0; d < srcs.size(); ++d) {
    int rc = fetch_rays(srcs[d]);
    if (rc) return rc;
    for (size_t i = 0; i < srcs[d]->rec_g.size(); ++i) order.push_back({srcs[d]->rec_g[i], {d, i}});
  }
  std::sort(order.begin(), order.end());
  const size_t R = (size_t)res->R;
  int64_t n = 0;
  for (const auto& o : order) {
    const rthx_result* q = srcs[o.second.first];
    const size_t i = o.second.second;
    for (size_t r = 0; r < R; ++r) {
      const size_t k = i * R + r;
      if (!q->h_ok[k]) continue;
      if (n >= cap) break;
      if (origins_xy) { origins_xy[2 * n] = q->h_orig[2 * k]; origins_xy[2 * n + 1] = q->h_orig[2 * k + 1]; }
      if (endpoints_xy) { endpoints_xy[2 * n] = q->h_end[2 * k]; endpoints_xy[2 * n + 1] = q->h_end[2 * k + 1]; }
      if (emitter) emitter[n] = o.first;
      ++n;
    }
  }
  if (n_out) *n_out = n;
  return RTHX_OK;
}

// ---------------------------------------------------------------------------
// Several devices
// ---------------------------------------------------------------------------
struct rthx_multi {
  std::vector<rthx_domain*> doms;
  ~rthx_multi() {
    for (rthx_domain* d : doms) rthx_domain_destroy(d);
  }
};

RTHX_EXPORT int rthx_multi_create(const rthx_domain_desc* desc, const int32_t* devices, int32_t n_devices,
                                  rthx_multi** out) {
  if (!out) return fail(RTHX_EINVAL, "null out");
  *out = nullptr;
  if (!devices || n_devices < 1) return fail(RTHX_EINVAL, "empty device list");
  // (a device may be listed more than once: its blocks then run one after
  // another on that device's one shared stream, rthx::device_stream -- a
  // correctness configuration for tests, not a way to overlap work)
  rthx_multi* m = new (std::nothrow) rthx_multi();
  if (!m) return fail(RTHX_ENOMEM, "host allocation failed");
  m->doms.assign(n_devices, nullptr);
  const int rc = for_each_part((size_t)n_devices, [&](size_t d) { return rthx_domain_create(desc, devices[d], &m->doms[d]); });
  if (rc) {
    delete m;
    return rc;
  }
  *out = m;
  return RTHX_OK;
}

RTHX_EXPORT void rthx_multi_destroy(rthx_multi* m) { delete m; }

RTHX_EXPORT int rthx_multi_trace_exchange(rthx_multi* m, const rthx_trace_args* a, rthx_result* res) {
  const double t0 = now_ms();
  if (!m || !a || !res) return fail(RTHX_EINVAL, "null argument");
  const size_t nd = m->doms.size();
  TracePlan p;
  int rc = plan_trace(m->doms[0], a, p);  // argument checks
  if (res->pending) {  // (an unread async single-device trace: counted and finished before its buffers go)
    rthx::DeviceGuard keep_device;
    const int rc2 = rthx::absorb_superseded(res);
    if (rc2) return rc2;
  }
  if (rc) return rc;
  // a result that held a single-device trace gives up its device buffers
  if (res->device >= 0) {
    (void)hipSetDevice(res->device);
    rthx::DevBuf* all[] = {&res->stage_cols, &res->stage_cnt, &res->row_nnz, &res->row_tallied, &res->row_off,
                           &res->totals,     &res->cols,      &res->cnt,     &res->dense,       &res->rec_ids,
                           &res->rec_ok,     &res->rec_orig,  &res->rec_end, &res->lb_status, &res->lb_totals, &res->arrive,
                           &res->acc_off,    &res->acc_cols,  &res->acc_cnt, &res->acc_len,   &res->acc_totals,
                           &res->acc_mark,   &res->acc_err};
    for (rthx::DevBuf* b : all) b->release();
    res->lb_epoch = 0;
    res->device = -1;
  }
  while (res->parts.size() < nd) res->parts.push_back(new rthx_result());
  while (res->parts.size() > nd) {
    delete res->parts.back();
    res->parts.pop_back();
  }
  for (size_t d = 0; d < nd; ++d)
    if (res->parts[d]->device >= 0 && res->parts[d]->device != m->doms[d]->device) {
      delete res->parts[d];
      res->parts[d] = new rthx_result();
    }
  // Row blocks: contiguous slots [n_rows d / nd, n_rows (d+1) / nd) on
  // single-polygon domains (every row costs about the same), interleaved
  // slots d, d + nd, ... on multi-polygon domains.
  const bool interleave = !m->doms[0]->single_convex;
  std::vector<rthx_trace_args> pa(nd, *a);
  for (size_t d = 0; d < nd; ++d) {
    pa[d].device = m->doms[d]->device;
    if (interleave) {
      pa[d].emitter_begin = a->emitter_begin + (int64_t)d * a->emitter_stride;
      pa[d].emitter_stride = a->emitter_stride * (int64_t)nd;
      pa[d].emitter_end = p.end;
    } else {
      const int64_t s0 = p.n_rows * (int64_t)d / (int64_t)nd, s1 = p.n_rows * (int64_t)(d + 1) / (int64_t)nd;
      pa[d].emitter_begin = a->emitter_begin + s0 * a->emitter_stride;
      pa[d].emitter_end = std::min<int64_t>(a->emitter_begin + s1 * a->emitter_stride, p.end);
      if (s1 <= s0) pa[d].emitter_end = pa[d].emitter_begin;
    }
  }
  res->valid = false;
  rc = for_each_part(nd, [&](size_t d) { return trace_exchange_one(m->doms[d], &pa[d], res->parts[d]); });
  if (rc) return rc;
  res->interleaved = interleave;
  res->N = p.N;
  res->R = p.R;
  res->n_rows = p.n_rows;
  res->begin = a->emitter_begin;
  res->stride = a->emitter_stride;
  res->split = 1;
  rthx_result_info& I = res->info;
  I = rthx_result_info{};
  I.n_emitters = p.N;
  I.rays_per_emitter = p.R;
  I.n_devices = (int32_t)nd;
  for (rthx_result* q : res->parts) {
    const rthx_result_info& J = q->info;
    I.rows_traced += J.rows_traced;
    I.rays_traced += J.rays_traced;
    I.nnz += J.nnz;
    I.lost_total += J.lost_total;
    I.lost_max_row = std::max(I.lost_max_row, J.lost_max_row);
    I.n_recorded += J.n_recorded;
    I.trace_ms = std::max(I.trace_ms, J.trace_ms);
    I.pack_ms = std::max(I.pack_ms, J.pack_ms);
    I.lookback_fallbacks += J.lookback_fallbacks;
    I.superseded += J.superseded;
    I.superseded_faults += J.superseded_faults;
  }
  I.superseded += res->sup_count;  // (a replaced single-device trace of this result)
  I.superseded_faults += res->sup_faults;
  res->sup_count = res->sup_faults = 0;
  res->valid = true;
  I.total_ms = now_ms() - t0;
  return RTHX_OK;
}
