// rthx_trace3d.cpp -- the 3D Monte Carlo exchange-factor tracer's C ABI
// (include/rthx.h rthx_scene3d_*, rthx_trace_exchange_3d; SURVEY.md §8(f4),
// BASELINE config 4).
//
// rthx_scene3d_create* reads the knobs, has build_scene3d
// (rthx_scene3d_build.h) validate the polygons and build the triangles, the
// BVH and the fast paths' tables on the host, and uploads the result.
// rthx_trace_exchange_3d traces R rays per emitter polygon into the
// caller's rthx_result exactly like the 2D split-row path: dense per-row
// counts, row_compact_kernel, row_scan_kernel, csr_pack_kernel (the sequence
// of rthx_rowtrace.h around its own launch).
#define RTHX_HOST_ONLY_TU 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_common.h"
#include "rthx_rowtrace.h"
#include "rthx_scene3d_build.h"
#include "rthx_trace3d.h"

using rthx::DevBuf;
using rthx::fail;
using rthx::now_ms;

struct rthx_scene3d {
  DevBuf polys, tris, nodes, scene, faces, lines, hull_tris, cvx_planes, cvx_start, cvx_items, mirror_n;
  rthx::DevScene3D S{};
  int64_t n_poly = 0;
  int64_t n_mirror = 0, n_mirror_tris = 0;  // symmetry planes (rthx_scene3d_create_mirrored) and their triangles
  int64_t n_hull_tris = 0, n_in_tris = 0;  // box hull: hull / interior triangles
  bool convex_interior = false;             // box hull: the interior is one convex set (Emit3::convex)
  int top_choice[32] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1,
                        -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};  // LDS node-cache size per kernel variant (launch_trace3d)
  int ghist_choice[4] = {-1, -1, -1, -1};  // per (faithful, pack16, N, R): global-histogram form chosen (1) or not (0)
  int64_t ghist_key[4] = {-1, -1, -1, -1};
  rthx::RowDevice dev;  // (last: destroyed first, so the buffers above are freed with its device current)
};

RTHX_EXPORT int rthx_scene3d_create(const double* xyz, const int32_t* nv, const double* normal, int64_t n,
                                    int32_t device, rthx_scene3d** out) {
  return rthx_scene3d_create_grouped(xyz, nv, normal, nullptr, n, device, out);
}

RTHX_EXPORT int rthx_scene3d_create_grouped(const double* xyz, const int32_t* nv, const double* normal,
                                            const int32_t* group, int64_t n, int32_t device, rthx_scene3d** out) {
  return rthx_scene3d_create_mirrored(xyz, nv, normal, group, n, nullptr, nullptr, 0, device, out);
}

RTHX_EXPORT int rthx_scene3d_create_mirrored(const double* xyz, const int32_t* nv, const double* normal,
                                             const int32_t* group, int64_t n, const double* mirror_xyz,
                                             const int32_t* mirror_nv, int64_t n_mirror, int32_t device,
                                             rthx_scene3d** out) {
  if (!out) return fail(RTHX_EINVAL, "null out");
  *out = nullptr;
  const double t_start = now_ms();
  rthx::Scene3dOptions opt;
  const char* e = rthx::knob("RTHX_T3_NO_HULL");
  opt.no_hull = e && e[0] == '1';
  e = rthx::knob("RTHX_T3_NO_CVX");
  opt.no_cvx = e && e[0] == '1';
  // (RTHX_T3_CVX_RES: 2 / 3 / 4 / 6 measured, profiles/round6/ab/cvx_res_arc.log)
  if ((e = rthx::knob("RTHX_T3_CVX_RES"))) opt.cvx_cells_per_tri = std::max(0.5, std::atof(e));
  if ((e = rthx::knob("RTHX_T3_CVX_ARC"))) opt.cvx_arc = std::max(1e-4, std::atof(e));
  rthx::Scene3dBuild B;
  std::string err;
  if (const int rc = rthx::build_scene3d(xyz, nv, normal, group, n, mirror_xyz, mirror_nv, n_mirror, opt, B, err))
    return fail(rc, err);

  const double t_bvh = now_ms();
  RTHX_TRY(rthx::open_device(device, nullptr));  // (the stream: below, once the handle exists)
  rthx_scene3d* s = new (std::nothrow) rthx_scene3d();
  if (!s) return fail(RTHX_ENOMEM, "host allocation failed");
  s->n_poly = B.n_poly;
  s->n_mirror = B.n_mirror;
  s->n_mirror_tris = B.n_mirror_tris;
  s->n_hull_tris = (int64_t)B.hull_tris.size();
  s->convex_interior = B.convex_interior;
  s->n_in_tris = B.n_in_tris;
  auto bail = [&](int code) {
    delete s;
    return code;
  };
  if (const int rc = s->dev.open(device)) return bail(rc);
  auto up = [&](DevBuf& b, const void* src, size_t bytes) {
    if (b.reserve(bytes) != hipSuccess) return false;
    return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(s->polys, B.polys.data(), B.polys.size() * sizeof(rthx::Emit3)) ||
      !up(s->tris, B.tris.data(), B.tris.size() * sizeof(rthx::Tri3)) ||
      !up(s->nodes, B.nodes.data(), B.nodes.size() * sizeof(rthx::Bvh2Node)))
    return bail(fail(RTHX_ENOMEM, "uploading the 3D scene"));
  if (B.hull && (!up(s->faces, B.faces.data(), B.faces.size() * sizeof(rthx::HullFace)) ||
                 !up(s->lines, B.lines.data(), B.lines.size() * sizeof(float)) ||
                 !up(s->hull_tris, B.hull_tris.data(), B.hull_tris.size() * sizeof(rthx::Tri3))))
    return bail(fail(RTHX_ENOMEM, "uploading the 3D scene's box hull"));
  if (B.cvx && (!up(s->cvx_planes, B.cvx_list_planes.data(), std::max<size_t>(B.cvx_list_planes.size(), 1) * sizeof(rthx::CvxPlane)) ||
                !up(s->cvx_start, B.cvx_start.data(), B.cvx_start.size() * 4) ||
                !up(s->cvx_items, B.cvx_items.data(), std::max<size_t>(B.cvx_items.size(), 1) * 4)))
    return bail(fail(RTHX_ENOMEM, "uploading the 3D scene's exit-direction map"));
  if (B.n_mirror > 0 && !up(s->mirror_n, B.mirror_n.data(), B.mirror_n.size() * 8))
    return bail(fail(RTHX_ENOMEM, "uploading the 3D scene's mirror normals"));
  s->S.n_poly = (int32_t)B.n_poly;
  s->S.n_tri = (int32_t)B.n_tri;
  s->S.n_nodes = (int32_t)B.nodes.size();
  s->S.stack = B.stack;
  s->S.polys = s->polys.as<rthx::Emit3>();
  s->S.tris = s->tris.as<rthx::Tri3>();
  s->S.nodes = s->nodes.as<rthx::Bvh2Node>();
  s->S.tables = s->dev.tables.as<double>();
  s->S.hull = B.hull ? 1 : 0;
  s->S.full_root = B.full_root;
  s->S.n_in_nodes = B.n_in_nodes;
  s->S.n_hull_lines = B.hull ? (int32_t)B.lines.size() : -1;
  for (int k = 0; k < 3; ++k) {
    s->S.box_lo[k] = B.box_lo[k];
    s->S.box_len[k] = B.box_len[k];
  }
  s->S.margin = B.margin;
  for (int k = 0; k < 4; ++k) s->S.ball[k] = B.ball[k];
  s->S.faces = B.hull ? s->faces.as<rthx::HullFace>() : nullptr;
  s->S.hull_lines = B.hull ? s->lines.as<float>() : nullptr;
  s->S.hull_tris = B.hull ? s->hull_tris.as<rthx::Tri3>() : nullptr;
  s->S.cvx = B.cvx ? 1 : 0;
  s->S.cvx_res = B.cvx_res;
  s->S.cvx_cos_arc = B.cvx_cos_arc;
  s->S.cvx_tpad = B.cvx_tpad;
  for (int k = 0; k < 3; ++k) s->S.cvx_c[k] = B.cvx_c[k];
  s->S.cvx_rin2 = B.cvx_rin2;
  s->S.cvx_rout2 = B.cvx_rout2;
  s->S.cvx_planes = B.cvx ? s->cvx_planes.as<rthx::CvxPlane>() : nullptr;
  s->S.cvx_start = B.cvx ? s->cvx_start.as<int32_t>() : nullptr;
  s->S.cvx_items = B.cvx ? s->cvx_items.as<int32_t>() : nullptr;
  s->S.n_real = (int32_t)B.n_poly;
  s->S.mirror_group0 = B.mirror_group0;
  s->S.mirror_n = B.n_mirror > 0 ? s->mirror_n.as<double>() : nullptr;
  if (!up(s->scene, &s->S, sizeof(s->S))) return bail(fail(RTHX_ENOMEM, "uploading the 3D scene"));
  if (rthx::knob("RTHX_VERBOSE"))
    std::fprintf(stderr, "rthx_scene3d_create: host geometry + BVH %.2f ms, device setup + upload %.2f ms\n",
                 t_bvh - t_start, now_ms() - t_bvh);
  *out = s;
  return RTHX_OK;
}

RTHX_EXPORT void rthx_scene3d_destroy(rthx_scene3d* s) { delete s; }

RTHX_EXPORT int rthx_scene3d_stats(const rthx_scene3d* sc, int64_t* n_tri, int64_t* n_nodes, int32_t* depth,
                                   int64_t* lds_bytes) {
  if (!sc) return fail(RTHX_EINVAL, "null scene");
  if (n_tri) *n_tri = sc->S.n_tri;
  if (n_nodes) *n_nodes = sc->S.n_nodes;
  if (depth) *depth = sc->S.stack;
  if (lds_bytes) *lds_bytes = (int64_t)(rthx::trace3d_dynamic_lds(sc->n_poly, sc->S.stack, sc->S.n_hull_lines) + rthx::kTrace3dStaticLds);
  return RTHX_OK;
}

RTHX_EXPORT int rthx_scene3d_hull(const rthx_scene3d* sc, int32_t* hull, int64_t* hull_tris, int64_t* interior_tris) {
  if (!sc) return fail(RTHX_EINVAL, "null scene");
  if (hull) *hull = sc->S.hull ? (sc->convex_interior ? 2 : 1) : sc->S.cvx ? 3 : 0;
  if (hull_tris) *hull_tris = sc->n_hull_tris;
  if (interior_tris) *interior_tris = sc->n_in_tris;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_scene3d_mirrors(const rthx_scene3d* sc, int64_t* n_mirror, int64_t* n_mirror_tris) {
  if (!sc) return fail(RTHX_EINVAL, "null scene");
  if (n_mirror) *n_mirror = sc->n_mirror;
  if (n_mirror_tris) *n_mirror_tris = sc->n_mirror_tris;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_trace_exchange_3d(rthx_scene3d* sc, const rthx_trace_args* a, rthx_result* res) {
  rthx::RowTrace rt{now_ms(), a, res};
  if (!sc || !a || !res) return fail(RTHX_EINVAL, "null argument");
  RTHX_TRY(rthx::check_row_args(a, "3D"));
  int64_t split_target = 0;  // (the driver's default)
  if (const char* e = rthx::knob("RTHX_T3_SPLIT_TARGET")) split_target = std::max<int64_t>(1, std::atoll(e));
  const int64_t N = sc->n_poly;
  RTHX_TRY(rthx::row_trace_plan(rt, sc->dev, "scene", N, split_target));
  const int64_t R = rt.R;
  const bool pack16 = (R + rt.split - 1) / rt.split < 65536;
  // A box hull's face records and lattice lines sit in LDS beside the row
  // histogram and the stacks; when they do not fit, the plain walk of the
  // whole scene's BVH (root full_root) traces the scene instead.
  bool use_hull = sc->S.hull != 0;
  size_t lds_bytes = rthx::trace3d_dynamic_lds(pack16 ? (N + 1) / 2 : N, sc->S.stack, use_hull ? sc->S.n_hull_lines : -1);
  if (use_hull && lds_bytes + rthx::kTrace3dStaticLds > rthx::kMaxLdsBytes) {
    use_hull = false;
    lds_bytes = rthx::trace3d_dynamic_lds(pack16 ? (N + 1) / 2 : N, sc->S.stack, -1);
  }
  if (lds_bytes + rthx::kTrace3dStaticLds > rthx::kMaxLdsBytes)
    return fail(RTHX_ERANGE, "N too large for the LDS row histogram and walk stacks of the 3D tracer");
  RTHX_TRY(rthx::row_trace_begin(rt));
  if (rt.n_rows > 0) {
    rthx::Trace3dLaunch L{};
    L.S = sc->scene.as<rthx::DevScene3D>();
    L.P.R = R;
    L.P.g_begin = a->emitter_begin;
    L.P.g_stride = a->emitter_stride;
    L.P.key0 = (uint32_t)a->seed;
    L.P.key1 = (uint32_t)(a->seed >> 32);
    L.T = rt.T;
    L.lds_bytes = lds_bytes;
    L.stream = sc->dev.stream;
    L.faithful = (a->flags & RTHX_FLAG_FAITHFUL_SAMPLING) != 0;
    L.pack16 = pack16;
    L.top_choice = sc->top_choice;
    L.hull = use_hull;
    L.cvx = sc->S.cvx != 0;
    L.mirror = sc->n_mirror > 0;  // (hull and cvx are then 0: rthx_scene3d_create_mirrored)
    // The global-histogram form when its LDS (the stacks alone) keeps more
    // workgroups resident than the LDS histogram's (RTHX_T3_GHIST=0/1 forces).
    const char* gh = rthx::knob("RTHX_T3_GHIST");
    if (gh && (gh[0] == '0' || gh[0] == '1')) {
      L.ghist = gh[0] == '1';
    } else {
      const int slot_k = (L.faithful ? 2 : 0) + (pack16 ? 1 : 0);
      const int64_t key = N * 2 + (pack16 ? 1 : 0);
      if (sc->ghist_key[slot_k] != key) {
        int wh = 0, wg = 0;
        HIP_TRY(rthx::trace3d_occupancy(L, lds_bytes, rthx::trace3d_dynamic_lds(0, sc->S.stack, use_hull ? sc->S.n_hull_lines : -1), &wh, &wg),
                "3D tracer occupancy");
        // (more than a quarter more workgroups: at config 4 L3 the GH form's
        // 6 against the histogram's 5 measured 4 % slower -- a returnless
        // global atomic per ray -- at L4 its 6 against 2 is 3 % faster)
        sc->ghist_choice[slot_k] = 4 * wg > 5 * wh ? 1 : 0;
        sc->ghist_key[slot_k] = key;
      }
      L.ghist = sc->ghist_choice[slot_k] == 1;
    }
    if (L.ghist) L.lds_bytes = rthx::trace3d_dynamic_lds(0, sc->S.stack, use_hull ? sc->S.n_hull_lines : -1);
    HIP_TRY(rthx::launch_trace3d(L), "trace_exchange_3d_kernel launch");
  }
  return rthx::row_trace_finish(rt);
}
