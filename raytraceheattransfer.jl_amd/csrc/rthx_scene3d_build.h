// rthx_scene3d_build.h -- the 3D tracer's host-side scene build
// (rthx_scene3d_build.cpp): polygons in, everything the device scene holds
// out.  No HIP, no environment, no global error state: the C ABI
// (rthx_trace3d.cpp) reads the knobs, calls build_scene3d and uploads the
// result; tests/scene3d_host_check.cpp calls it on the host and checks the
// result by brute force.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "rthx_scene3d.h"

namespace rthx {

#ifndef RTHX_T3_LEAF
#define RTHX_T3_LEAF 2
#endif
constexpr int kLeafTris = RTHX_T3_LEAF;  // triangles per BVH leaf (at most)
static_assert(kLeafTris >= 1 && kLeafTris < (1 << kLeafBits), "a leaf's count fits its reference");

// What the environment's knobs set (rthx_trace3d.cpp reads them).
struct Scene3dOptions {
  bool no_hull = false;          // RTHX_T3_NO_HULL=1: never the box hull
  bool no_cvx = false;           // RTHX_T3_NO_CVX=1: never the exit-direction map
  double cvx_cells_per_tri = 0;  // RTHX_T3_CVX_RES: cube-map cells per triangle edge (0: the default, 4)
  double cvx_arc = 0;            // RTHX_T3_CVX_ARC: the largest half-arc in radians (0: the scene's own)
};

// A triangle as the BVH build sees it: bounds, centroid, group.
struct BuildTri {
  double lo[3], hi[3], c[3];
  int group;
};

// Builds the two-child BVH over bt; `order` (bt.size() entries) receives the
// triangle permutation.  Binned SAH, or median splits on the longest centroid
// axis (`median`).  The root is always inner node 0 (a scene of <= kLeafTris
// triangles gets one leaf and one empty child).  Returns the inner-node depth.
int build_bvh2(std::vector<Bvh2Node>& nodes, std::vector<int>& order, const std::vector<BuildTri>& bt, double pad,
               bool median);

struct Scene3dBuild {
  std::vector<Emit3> polys;     // the real polygons
  std::vector<Tri3> tris;       // device order: the BVH's permutation (box hull: the interior's, then the whole scene's)
  std::vector<Bvh2Node> nodes;  // device order (box hull: the interior BVH, then from full_root the whole scene's)
  int64_t n_poly = 0, n_mirror = 0;
  int64_t n_tri = 0;            // triangles of the scene, mirrors' included (tris holds each twice with a box hull)
  int64_t n_mirror_tris = 0;
  int32_t mirror_group0 = 0;    // mirror m is group mirror_group0 + m
  std::vector<double> mirror_n; // [3 n_mirror] unit normals
  int stack = 0;                // inner-node depth of the deepest BVH
  double scale = 0.0;           // scene scale: the largest |coordinate| or extent
  double box_lo[3] = {0.0, 0.0, 0.0};
  float box_len[3] = {0.0f, 0.0f, 0.0f};
  // box hull
  bool hull = false;
  std::vector<HullFace> faces;  // [6], 2 axis + side
  std::vector<float> lines;
  std::vector<Tri3> hull_tris;  // [2 x cells], cell order
  std::vector<char> in_hull;    // per polygon: a hull cell
  int32_t full_root = 0, n_in_nodes = 0;
  int64_t n_in_tris = 0;
  bool convex_interior = false;
  float margin = 0.0f;
  double ball[4] = {0.0, 0.0, 0.0, 0.0};
  // convex enclosure: the cube map of exit directions
  bool cvx = false;
  int cvx_res = 0;
  double cvx_max_arc = 0.0;
  float cvx_cos_arc = 1.0f, cvx_tpad = 0.0f;
  double cvx_c[3] = {0.0, 0.0, 0.0};
  double cvx_rin2 = 0.0, cvx_rout2 = 0.0;
  std::vector<int32_t> cvx_start, cvx_items;
  std::vector<CvxPlane> cvx_list_planes;  // per list entry: the plane of tris[cvx_items[e]]
};

// Builds the scene of rthx_scene3d_create_mirrored's arrays (include/rthx.h).
// Returns RTHX_OK, or an RTHX_E* code with its message in `err` (`out` is then
// left empty).
int build_scene3d(const double* xyz, const int32_t* nv, const double* normal, const int32_t* group, int64_t n,
                  const double* mirror_xyz, const int32_t* mirror_nv, int64_t n_mirror, const Scene3dOptions& opt,
                  Scene3dBuild& out, std::string& err);

}  // namespace rthx
