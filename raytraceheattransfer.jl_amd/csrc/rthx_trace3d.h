// rthx_trace3d.h -- device scene and launcher of the 3D Monte Carlo
// exchange-factor tracer (rthx_trace3d_kernels.hip, rthx_trace3d.cpp).  The
// records the scene holds, and their constants, are rthx_scene3d.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_kernels.h"
#include "rthx_scene3d.h"

namespace rthx {

struct DevScene3D {
  int32_t n_poly, n_tri, n_nodes;
  int32_t stack;  // walk stack entries a lane needs (inner-node depth of the BVHs)
  const Emit3 RTHX_GLOBAL* polys;
  const Tri3 RTHX_GLOBAL* tris;
  const Bvh2Node RTHX_GLOBAL* nodes;
  const double RTHX_GLOBAL* tables;  // kTableDoubles (cos/sin table for the azimuth)
  // nodes / tris hold one BVH -- the whole scene's, root 0 -- or, with a box
  // hull, two: the interior triangles' (root 0, its top first: the LDS cache)
  // and, from full_root on, the whole scene's (the fallback walk).
  int32_t hull;         // 1: box hull fast path (HullFace x 6)
  int32_t full_root;    // root node of the whole scene's BVH
  int32_t n_in_nodes;   // nodes of the interior BVH (0: no interior triangles)
  int32_t n_hull_lines; // lattice lines of all faces (staged in LDS behind the face records)
  double box_lo[3];     // box corner (hull coordinates are relative to it)
  double ball[4];       // box hull: a ball (centre, radius) around every interior triangle, padded
                        // (radius 0: no interior); a ray that misses it meets no interior triangle
  float box_len[3];     // box extents
  float margin;         // kHullMargin x the largest extent
  const HullFace RTHX_GLOBAL* faces;       // [6]
  const float RTHX_GLOBAL* hull_lines;     // lattice lines relative to the box corner
  const Tri3 RTHX_GLOBAL* hull_tris;       // [2 x cells], cell order, (v0 v1 v2), (v2 v3 v0)
  // convex enclosure seen from inside (CvxPlane): 1 = the fast path
  int32_t cvx;
  int32_t cvx_res;           // cube-map cells per face edge
  float cvx_cos_arc;         // cos(2 x the largest half-arc): the longest arc (between the cap's ends) taken
  float cvx_tpad;            // absolute window above t_min (1e-9 of the scene scale)
  double cvx_c[3];           // the vertices' centroid
  double cvx_rin2, cvx_rout2;  // squared inscribed (shrunk 1e-9) and circumscribed (grown 1e-9) radii
  const int32_t RTHX_GLOBAL* cvx_start;    // [6 res^2 + 1] list offsets per cell
  const CvxPlane RTHX_GLOBAL* cvx_planes;  // per list entry: its triangle's plane (inline)
  const int32_t RTHX_GLOBAL* cvx_items;    // per list entry: its triangle's index into `tris`
  // Specular symmetry planes (rthx_scene3d_create_mirrored),
  // appended so that no field above moves.  Polygons [0, n_real) absorb and
  // emit; a triangle whose poly is n_real + m belongs to mirror m, which is
  // the group mirror_group0 + m of its own and has the unit normal
  // mirror_n[3 m ..].  Without mirrors n_real == n_poly and mirror_n is null.
  int32_t n_real;
  int32_t mirror_group0;
  const double RTHX_GLOBAL* mirror_n;
};

constexpr uint32_t kTrace3dTag = 0x40000000u;  // Philox counter word 3 of the 3D tracer
// A ray still travelling after this many reflections off symmetry planes is
// lost (the 2D walk's segment cap: two facing mirrors with nothing between).
constexpr int kTrace3dMaxReflections = 10000;

#ifndef RTHX_T3_THREADS
#define RTHX_T3_THREADS 256
#endif
constexpr int kTrace3dThreads = RTHX_T3_THREADS;  // lanes per workgroup
// static LDS of the 3D kernel: emitter, counters, (at least) the 64-node
// cache and the fast-path kernels' deferred-walk rings (128 ray indices per wave)
constexpr size_t kTrace3dStaticLds = 512 + 64 * 64 + (size_t)(kTrace3dThreads / 64) * 128 * 4;
// dynamic LDS: the row histogram (`words` = N, or (N + 1) / 2 packed u16,
// padded to 64), then the stacks, then (box hull) the face records and lines
__host__ __device__ constexpr size_t trace3d_stack_offset(int64_t words) { return (size_t)((words + 63) & ~int64_t(63)); }
// (box hull: the face records and lattice lines follow the stacks)
__host__ __device__ constexpr size_t trace3d_dynamic_lds(int64_t words, int stack, int hull_lines = -1) {
  return 4 * (trace3d_stack_offset(words) + (size_t)stack * kTrace3dThreads +
              (hull_lines >= 0 ? (size_t)(kHullFaceWords + hull_lines) : 0));
}

struct Trace3dLaunch {
  const DevScene3D* S;
  TraceParams P;        // R, g_begin, g_stride, key (bin / beta unused)
  TallyParams T;        // split path: dense rows + row_tallied
  size_t lds_bytes;
  hipStream_t stream;
  bool faithful;
  bool pack16;  // < 65536 rays per workgroup: u16 row-histogram counters
  bool ghist;   // counts straight to the dense rows (no LDS histogram)
  bool hull;    // box hull fast path (DevScene3D::hull)
  bool cvx;     // convex-enclosure fast path (DevScene3D::cvx)
  bool mirror;  // the scene holds symmetry planes (DevScene3D::n_real < its polygons): MODE 0's MIRROR kernels
  int* top_choice;  // [mode * 8 + ghist * 4 + faithful * 2 + pack16] (mode 0 plain, 1 hull, 2 cvx, 3 mirror): LDS node-cache size (64 / 128), -1 = not chosen yet
};

hipError_t launch_trace3d(const Trace3dLaunch& L);
hipError_t trace3d_occupancy(const Trace3dLaunch& L, size_t lds_hist, size_t lds_gh, int* wg_hist, int* wg_gh);

}  // namespace rthx
