// Stand-alone check of the 3D tracer's host-side scene build
// (csrc/rthx_scene3d_build.h build_scene3d, build_bvh2), compiled together
// with csrc/rthx_scene3d_build.cpp under -fsanitize=address,undefined by
// tests/test_scene3d_build_host.py and run as a program.
//
// The kernel's fast paths are correct only for what this build produces: fp32
// boxes that contain their triangles padded outward, a box hull whose cells
// are the polygons they claim, an exit-direction map whose lists hold every
// triangle a short cap can reach.  Each is checked here by brute force, on
// scenes generated in this file, each the smallest that reaches its path.
// Every error the builder can return is provoked once -- but for "BVH too
// deep for the traversal stack" (a median tree deeper than 32 needs 2^33
// triangles) and "too many triangles" (2^26 of them), which no test-sized
// scene reaches.  For every scene a 64-bit FNV-1a hash over the named fields
// of the result is printed; the pytest compares it with
// tests/golden/scene3d_build.json.  The cube map's lists pass through libm
// thresholds, so they are pinned by their contract, not by the hash.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_scene3d_build.h"

using namespace rthx;

static int fails = 0;
static const char* current = "";
#define EXPECT(cond, ...)                            \
  do {                                               \
    if (!(cond)) {                                   \
      if (fails < 30) {                              \
        std::printf("FAIL [%s] %s: ", current, #cond); \
        std::printf(__VA_ARGS__);                    \
        std::printf("\n");                           \
      }                                              \
      ++fails;                                       \
    }                                                \
  } while (0)

struct P3 {
  double x, y, z;
};
static P3 operator+(P3 a, P3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static P3 operator-(P3 a, P3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static P3 operator*(P3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dot(P3 a, P3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static P3 cross(P3 a, P3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(P3 a) { return std::sqrt(dot(a, a)); }
static P3 unit(P3 a) { return a * (1.0 / len(a)); }

// ---------------------------------------------------------------- scenes

struct Scene {
  std::string name;
  std::vector<double> xyz, nrm, mxyz;  // [n][4][3], [n][3], [m][4][3]
  std::vector<int32_t> nv, group, mnv;
  bool grouped = false;
  int64_t n() const { return (int64_t)nv.size(); }
  int64_t n_mirror() const { return (int64_t)mnv.size(); }
  void add(std::vector<P3> v, P3 normal, int32_t g) {
    nv.push_back((int32_t)v.size());
    v.resize(4, P3{0.0, 0.0, 0.0});
    for (const P3& p : v) xyz.insert(xyz.end(), {p.x, p.y, p.z});
    nrm.insert(nrm.end(), {normal.x, normal.y, normal.z});
    group.push_back(g);
  }
  void add_mirror(std::vector<P3> v) {
    mnv.push_back((int32_t)v.size());
    v.resize(4, P3{0.0, 0.0, 0.0});
    for (const P3& p : v) mxyz.insert(mxyz.end(), {p.x, p.y, p.z});
  }
  int build(Scene3dBuild& B, std::string& err, const Scene3dOptions& opt = Scene3dOptions{}) const {
    return build_scene3d(xyz.data(), nv.data(), nrm.data(), grouped ? group.data() : nullptr, n(),
                         mnv.empty() ? nullptr : mxyz.data(), mnv.empty() ? nullptr : mnv.data(), n_mirror(), opt, B,
                         err);
  }
};

static P3 axis_point(int k, double a, double u, double v) {
  double c[3];
  c[k] = a;
  c[(k + 1) % 3] = u;
  c[(k + 2) % 3] = v;
  return {c[0], c[1], c[2]};
}

// The six faces of the box [0, L]: face 2 k + side a lattice of cells[u] x
// cells[v] quads, rays leaving inward, one group per face (from group0 on).
static void add_box(Scene& s, const double L[3], const int cells[3], int32_t group0) {
  for (int k = 0; k < 3; ++k)
    for (int side = 0; side < 2; ++side) {
      const int u = (k + 1) % 3, v = (k + 2) % 3;
      P3 nn = axis_point(k, side ? -1.0 : 1.0, 0.0, 0.0);
      for (int j = 0; j < cells[v]; ++j)
        for (int i = 0; i < cells[u]; ++i) {
          const double u0 = L[u] * i / cells[u], u1 = L[u] * (i + 1) / cells[u];
          const double v0 = L[v] * j / cells[v], v1 = L[v] * (j + 1) / cells[v];
          const double a = side ? L[k] : 0.0;
          s.add({axis_point(k, a, u0, v0), axis_point(k, a, u1, v0), axis_point(k, a, u1, v1), axis_point(k, a, u0, v1)},
                nn, group0 + 2 * k + side);
        }
    }
}

// A tetrahedron about `c` of size r: rays leave outward (a body) or inward (an
// enclosure); every face a group of its own from group0 on.
static void add_tetra(Scene& s, P3 c, double r, bool outward, int32_t group0) {
  const P3 v[4] = {c + P3{r, r, r}, c + P3{r, -r, -r}, c + P3{-r, r, -r}, c + P3{-r, -r, r}};
  const int f[4][3] = {{0, 1, 2}, {0, 3, 1}, {0, 2, 3}, {1, 3, 2}};
  for (int k = 0; k < 4; ++k) {
    const P3 m = (v[f[k][0]] + v[f[k][1]] + v[f[k][2]]) * (1.0 / 3.0);
    s.add({v[f[k][0]], v[f[k][1]], v[f[k][2]]}, outward ? m - c : c - m, group0 + k);
  }
}

// The unit icosphere after one subdivision (80 triangles), rays leaving inward.
static void add_icosphere1(Scene& s) {
  const double t = (1.0 + std::sqrt(5.0)) / 2.0;
  std::vector<P3> v = {{-1, t, 0}, {1, t, 0}, {-1, -t, 0}, {1, -t, 0}, {0, -1, t}, {0, 1, t},
                       {0, -1, -t}, {0, 1, -t}, {t, 0, -1}, {t, 0, 1}, {-t, 0, -1}, {-t, 0, 1}};
  for (P3& p : v) p = unit(p);
  const int f[20][3] = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                        {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                        {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
  int32_t g = 0;
  for (int k = 0; k < 20; ++k) {
    const P3 a = v[f[k][0]], b = v[f[k][1]], c = v[f[k][2]];
    const P3 ab = unit(a + b), bc = unit(b + c), ca = unit(c + a);
    const P3 sub[4][3] = {{a, ab, ca}, {b, bc, ab}, {c, ca, bc}, {ab, bc, ca}};
    for (const auto& q : sub) s.add({q[0], q[1], q[2]}, (q[0] + q[1] + q[2]) * -1.0, g++);
  }
}

// x -> R x + o with the rational rotation (3,4,5) about z then (5,12,13) about x.
static Scene moved(const Scene& s, const char* name) {
  auto rot = [](double* p, bool offset) {
    const double x = 0.6 * p[0] - 0.8 * p[1], y = 0.8 * p[0] + 0.6 * p[1], z = p[2];
    const double y2 = (5.0 * y - 12.0 * z) / 13.0, z2 = (12.0 * y + 5.0 * z) / 13.0;
    p[0] = x + (offset ? 3.0 : 0.0);
    p[1] = y2 + (offset ? -2.0 : 0.0);
    p[2] = z2 + (offset ? 0.5 : 0.0);
  };
  Scene r = s;
  r.name = name;
  for (size_t i = 0; i < r.xyz.size(); i += 3) rot(&r.xyz[i], true);
  for (size_t i = 0; i < r.nrm.size(); i += 3) rot(&r.nrm[i], false);
  return r;
}

static Scene few_triangles(int count) {
  Scene s;
  s.name = count == 2 ? "two_triangles" : "three_triangles";
  for (int k = 0; k < count; ++k) {  // stacked, all facing up: no enclosure
    const double z = 0.5 * k;
    s.add({{0.1 * k, 0, z}, {1, 0, z}, {0, 1, z}}, {0, 0, 1}, k);
  }
  return s;
}

static Scene hull_scene(const char* name, const int cells[3], int tetras, bool split_face = false) {
  Scene s;
  s.name = name;
  s.grouped = true;
  const double L[3] = {1.0, 1.5, 0.75};
  add_box(s, L, cells, 0);
  if (split_face)  // (the second half of face 0's polygons)
    for (int p = cells[1] * cells[2] / 2; p < cells[1] * cells[2]; ++p) s.group[(size_t)p] = 6;
  if (tetras >= 1) add_tetra(s, {0.4, 0.6, 0.35}, 0.1, true, 6);
  if (tetras >= 2) add_tetra(s, {0.7, 1.1, 0.4}, 0.08, true, 10);
  return s;
}

static Scene octant_mirrored() {  // tests/mirror3d_scenes.py octant_cube
  Scene s;
  s.name = "octant_mirrors";
  for (int k = 0; k < 3; ++k)
    s.add({axis_point(k, 0, 0, 0), axis_point(k, 0, 0.5, 0), axis_point(k, 0, 0.5, 0.5), axis_point(k, 0, 0, 0.5)},
          axis_point(k, 1, 0, 0), k);
  for (int k = 0; k < 3; ++k)
    s.add_mirror({axis_point(k, 0.5, -0.25, -0.25), axis_point(k, 0.5, 1.25, -0.25), axis_point(k, 0.5, 1.25, 1.25),
                  axis_point(k, 0.5, -0.25, 1.25)});
  return s;
}

// ---------------------------------------------------------------- checks

static int32_t tri_group(const Scene3dBuild& B, const Tri3& T) {
  return T.poly < B.n_poly ? B.polys[(size_t)T.poly].group : (int32_t)(B.mirror_group0 + (T.poly - B.n_poly));
}

// The three input vertices of a built triangle (and that its record holds them).
static void tri_vertices(const Scene& s, const Scene3dBuild& B, const Tri3& T, double v[3][3]) {
  const bool mirror = T.poly >= B.n_poly;
  const int64_t p = mirror ? T.poly - B.n_poly : T.poly;
  const double* q = (mirror ? s.mxyz.data() : s.xyz.data()) + 12 * p;
  const int m = mirror ? s.mnv[(size_t)p] : s.nv[(size_t)p];
  const bool first = T.v0[0] == q[0] && T.v0[1] == q[1] && T.v0[2] == q[2];
  EXPECT(first || m == 4, "triangle %d of polygon %d", T.id, T.poly);
  const int c[3] = {first ? 0 : 2, first ? 1 : 3, first ? 2 : 0};
  for (int i = 0; i < 3; ++i)
    for (int d = 0; d < 3; ++d) v[i][d] = q[3 * c[i] + d];
  for (int d = 0; d < 3; ++d)
    EXPECT(T.v0[d] == v[0][d] && T.e1[d] == v[1][d] - v[0][d] && T.e2[d] == v[2][d] - v[0][d], "triangle %d", T.id);
}

// One tree: nodes [node0, node0 + n_nodes) with root node0, triangles
// [tri0, tri0 + n_tris).  Returns its inner-node depth.
static int check_tree(const std::vector<Bvh2Node>& nodes, int32_t node0, int32_t n_nodes, int64_t tri0, int64_t n_tris,
                      double pad, bool laid_out, const std::function<void(int64_t, double (*)[3])>& verts,
                      const std::function<int32_t(int64_t)>& group_of) {
  std::vector<int> covered((size_t)n_tris, 0), seen((size_t)n_nodes, 0);
  // triangles below a child reference, depth of inner nodes
  std::function<int(int32_t, std::vector<int64_t>&)> below = [&](int32_t ref, std::vector<int64_t>& out) -> int {
    if (ref < 0) {
      const int32_t r = ~ref, first = r >> kLeafBits, count = r & ((1 << kLeafBits) - 1);
      EXPECT(count <= kLeafTris, "leaf of %d", count);
      EXPECT(count == 0 || (first >= tri0 && first + count <= tri0 + n_tris), "leaf [%d, +%d)", first, count);
      for (int i = 0; i < count; ++i)
        if (first + i >= tri0 && first + i < tri0 + n_tris) {
          ++covered[(size_t)(first + i - tri0)];
          out.push_back(first + i);
        }
      return 0;
    }
    if (ref < node0 || ref >= node0 + n_nodes) {
      EXPECT(false, "child %d outside [%d, +%d)", ref, node0, n_nodes);
      return 0;
    }
    if (seen[(size_t)(ref - node0)]++) {
      EXPECT(false, "node %d reached twice", ref);
      return 0;
    }
    const Bvh2Node& nd = nodes[(size_t)ref];
    int depth = 0;
    for (int c = 0; c < 2; ++c) {
      std::vector<int64_t> sub;
      EXPECT(nd.child[c] < 0 || nd.child[c] > ref, "node %d child %d points back", ref, nd.child[c]);
      depth = std::max(depth, below(nd.child[c], sub));
      int32_t g = sub.empty() ? -1 : group_of(sub[0]);
      for (int64_t t : sub) {
        if (group_of(t) != g) g = -1;
        double v[3][3];
        verts(t, v);
        for (int i = 0; i < 3; ++i)
          for (int d = 0; d < 3; ++d)
            EXPECT((double)nd.lo[c][d] <= v[i][d] - pad && (double)nd.hi[c][d] >= v[i][d] + pad,
                   "node %d child %d: [%g, %g] against %.17g +- %g", ref, c, nd.lo[c][d], nd.hi[c][d], v[i][d], pad);
      }
      EXPECT(nd.group[c] == g, "node %d child %d: group %d, below it %d", ref, c, nd.group[c], g);
      out.insert(out.end(), sub.begin(), sub.end());
    }
    return depth + 1;
  };
  std::vector<int64_t> all;
  const int depth = below(node0, all);
  for (int64_t t = 0; t < n_tris; ++t) EXPECT(covered[(size_t)t] == 1, "triangle %lld under %d leaves", (long long)(tri0 + t), covered[(size_t)t]);
  for (int32_t k = 0; k < n_nodes; ++k) EXPECT(seen[(size_t)k] == 1, "node %d unreachable", node0 + k);
  if (laid_out) {  // the first min(n, kTopNodes) nodes are the breadth-first top
    std::vector<int32_t> bfs{node0};
    for (size_t h = 0; h < bfs.size() && (int)bfs.size() < kTopNodes + 2; ++h)
      for (int c = 0; c < 2; ++c)
        if (nodes[(size_t)bfs[h]].child[c] >= 0) bfs.push_back(nodes[(size_t)bfs[h]].child[c]);
    for (int k = 0; k < std::min<int>(n_nodes, kTopNodes) && k < (int)bfs.size(); ++k)
      EXPECT(bfs[(size_t)k] == node0 + k, "breadth-first node %d is %d", k, bfs[(size_t)k]);
  }
  return depth;
}

static void check_bvh(const Scene& s, const Scene3dBuild& B) {
  const double pad = kBoxPad * B.scale;
  auto verts = [&](int64_t t, double (*v)[3]) { tri_vertices(s, B, B.tris[(size_t)t], v); };
  auto group_of = [&](int64_t t) { return tri_group(B, B.tris[(size_t)t]); };
  const int64_t n_real_tris = B.n_tri - B.n_mirror_tris;
  EXPECT((int64_t)B.tris.size() == (B.hull ? B.n_in_tris + B.n_tri : B.n_tri), "%zu triangles", B.tris.size());
  EXPECT((int64_t)B.polys.size() == B.n_poly && B.n_poly == s.n() && B.n_mirror == s.n_mirror(), "counts");
  int depth = 0;
  const int64_t full_tri0 = B.hull ? B.n_in_tris : 0;
  if (B.hull) {
    EXPECT(B.full_root == B.n_in_nodes, "full_root %d, interior nodes %d", B.full_root, B.n_in_nodes);
    if (B.n_in_nodes > 0)
      depth = check_tree(B.nodes, 0, B.n_in_nodes, 0, B.n_in_tris, pad, true, verts, group_of);
    std::vector<int32_t> ids;
    for (int64_t t = 0; t < B.n_in_tris; ++t) {
      ids.push_back(B.tris[(size_t)t].id);
      EXPECT(!B.in_hull[(size_t)B.tris[(size_t)t].poly], "interior triangle %lld of a hull polygon", (long long)t);
    }
    std::sort(ids.begin(), ids.end());
    EXPECT(std::adjacent_find(ids.begin(), ids.end()) == ids.end(), "interior ids repeat");
  } else {
    EXPECT(B.full_root == 0 && B.n_in_nodes == (int32_t)B.nodes.size(), "full_root %d", B.full_root);
  }
  depth = std::max(depth, check_tree(B.nodes, B.full_root, (int32_t)B.nodes.size() - B.full_root, full_tri0, B.n_tri, pad,
                                     true, verts, group_of));
  EXPECT(depth == B.stack && B.stack <= kBvhStack, "measured depth %d, reported %d", depth, B.stack);
  std::vector<int> id_seen((size_t)B.n_tri, 0);
  for (int64_t t = 0; t < B.n_tri; ++t) {
    const Tri3& T = B.tris[(size_t)(full_tri0 + t)];
    if (T.id < 0 || T.id >= B.n_tri) {
      EXPECT(false, "id %d", T.id);
      continue;
    }
    ++id_seen[(size_t)T.id];
    EXPECT((T.poly >= B.n_poly) == (T.id >= n_real_tris), "triangle id %d of polygon %d", T.id, T.poly);
    EXPECT(T.poly >= 0 && T.poly < B.n_poly + B.n_mirror, "polygon %d", T.poly);
  }
  for (int64_t t = 0; t < B.n_tri; ++t) EXPECT(id_seen[(size_t)t] == 1, "id %lld held %d times", (long long)t, id_seen[(size_t)t]);
  EXPECT((int64_t)B.mirror_n.size() == 3 * B.n_mirror, "mirror normals");
  for (int64_t k = 0; k < B.n_poly; ++k) EXPECT(B.polys[(size_t)k].group < B.mirror_group0, "real group above the mirrors'");
}

static void check_hull(const Scene& s, const Scene3dBuild& B) {
  if (!B.hull) {
    EXPECT(B.faces.empty() && B.lines.empty() && B.hull_tris.empty() && !B.convex_interior, "hull data without a hull");
    for (const Emit3& E : B.polys) EXPECT(E.convex == 0, "convex flag without a hull");
    return;
  }
  EXPECT(B.faces.size() == 6 && B.lines.size() <= 4096 && B.in_hull.size() == (size_t)B.n_poly, "hull sizes");
  if (B.faces.size() != 6 || B.in_hull.size() != (size_t)B.n_poly) return;
  const double Lmax = std::max({B.box_len[0], B.box_len[1], B.box_len[2]});
  const double tol = 1e-6 * Lmax;  // (the lines are fp32)
  EXPECT(std::fabs(B.margin - kHullMargin * Lmax) <= 1e-6 * B.margin, "margin %g", B.margin);
  int64_t cells = 0;
  for (int f = 0; f < 6; ++f) {
    const HullFace& F = B.faces[(size_t)f];
    EXPECT(F.axis == (f >> 1) && F.side == (f & 1), "face %d is (%d, %d)", f, F.axis, F.side);
    const int k = f >> 1, u = (k + 1) % 3, v = (k + 2) % 3;
    EXPECT(F.cell0 == cells && F.nu >= 1 && F.nv >= 1, "face %d cells", f);
    EXPECT(F.lu >= 0 && F.lv == F.lu + F.nu + 1 && (size_t)(F.lv + F.nv + 1) <= B.lines.size(), "face %d lines", f);
    if (F.nu < 1 || F.nv < 1 || F.lu < 0 || (size_t)(F.lv + F.nv + 1) > B.lines.size()) return;
    const float* lu = &B.lines[(size_t)F.lu];
    const float* lv = &B.lines[(size_t)F.lv];
    EXPECT(lu[0] == 0.0f && lv[0] == 0.0f && lu[F.nu] == B.box_len[u] && lv[F.nv] == B.box_len[v], "face %d line ends", f);
    for (int i = 0; i < F.nu; ++i) EXPECT(lu[i] < lu[i + 1], "face %d u lines", f);
    for (int j = 0; j < F.nv; ++j) EXPECT(lv[j] < lv[j + 1], "face %d v lines", f);
    EXPECT(F.plane == (F.side ? B.box_len[k] : 0.0f), "face %d plane", f);
    for (int j = 0; j < F.nv; ++j)
      for (int i = 0; i < F.nu; ++i) {
        const size_t cell = (size_t)(F.cell0 + j * F.nu + i);
        if (2 * cell + 1 >= B.hull_tris.size()) {
          EXPECT(false, "cell %zu beyond hull_tris", cell);
          return;
        }
        const int32_t p = B.hull_tris[2 * cell].poly;
        EXPECT(B.hull_tris[2 * cell + 1].poly == p && p >= 0 && p < B.n_poly, "cell %zu polygons", cell);
        if (p < 0 || p >= B.n_poly) continue;
        EXPECT(B.in_hull[(size_t)p] && B.polys[(size_t)p].group == F.group && s.nv[(size_t)p] == 4, "cell %zu polygon %d", cell, p);
        double v0[3][3], v1[3][3];
        tri_vertices(s, B, B.hull_tris[2 * cell], v0);
        tri_vertices(s, B, B.hull_tris[2 * cell + 1], v1);
        for (int d = 0; d < 3; ++d)  // (v0 v1 v2), then (v2 v3 v0)
          EXPECT(v0[0][d] == s.xyz[(size_t)(12 * p + d)] && v1[0][d] == s.xyz[(size_t)(12 * p + 6 + d)] &&
                     v0[2][d] == v1[0][d] && v1[2][d] == v0[0][d],
                 "cell %zu halves", cell);
        double ulo = 1e300, uhi = -1e300, vlo = 1e300, vhi = -1e300;
        for (int c = 0; c < 4; ++c) {
          const double* q = &s.xyz[(size_t)(12 * p + 3 * c)];
          EXPECT(std::fabs(q[k] - B.box_lo[k] - F.plane) <= tol, "cell %zu off its plane", cell);
          ulo = std::min(ulo, q[u] - B.box_lo[u]);
          uhi = std::max(uhi, q[u] - B.box_lo[u]);
          vlo = std::min(vlo, q[v] - B.box_lo[v]);
          vhi = std::max(vhi, q[v] - B.box_lo[v]);
        }
        EXPECT(std::fabs(ulo - lu[i]) <= tol && std::fabs(uhi - lu[i + 1]) <= tol && std::fabs(vlo - lv[j]) <= tol &&
                   std::fabs(vhi - lv[j + 1]) <= tol,
               "cell %zu (%d, %d) of face %d is not polygon %d's quad", cell, i, j, f, p);
      }
    cells += (int64_t)F.nu * F.nv;
  }
  EXPECT((int64_t)B.hull_tris.size() == 2 * cells, "%zu hull triangles, %lld cells", B.hull_tris.size(), (long long)cells);
  int64_t n_hull_polys = 0, n_in = 0;
  for (int64_t p = 0; p < B.n_poly; ++p) n_hull_polys += B.in_hull[(size_t)p] ? 1 : 0;
  for (int64_t p = 0; p < B.n_poly; ++p)
    if (!B.in_hull[(size_t)p]) n_in += s.nv[(size_t)p] == 4 ? 2 : 1;
  EXPECT(n_hull_polys == cells && n_in == B.n_in_tris, "%lld hull polygons, %lld interior triangles", (long long)n_hull_polys, (long long)n_in);
  EXPECT((B.ball[3] > 0.0) == (n_in > 0), "ball radius %g", B.ball[3]);
  for (int64_t p = 0; p < B.n_poly; ++p) {
    EXPECT(B.polys[(size_t)p].convex == (B.convex_interior && !B.in_hull[(size_t)p] ? 1 : 0), "convex flag of polygon %lld", (long long)p);
    if (B.in_hull[(size_t)p]) continue;
    for (int c = 0; c < s.nv[(size_t)p]; ++c) {
      const double* q = &s.xyz[(size_t)(12 * p + 3 * c)];
      EXPECT(len(P3{q[0] - B.ball[0], q[1] - B.ball[1], q[2] - B.ball[2]}) <= B.ball[3], "vertex outside the ball");
    }
  }
}

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// The exit-direction map's contract (csrc/rthx_scene3d.h CvxPlane): a
// triangle is in the list of every cell holding a direction within the
// largest half-arc of its central projection.
static void check_cube_map(const Scene3dBuild& B) {
  if (!B.cvx) {
    EXPECT(B.cvx_res == 0 && B.cvx_start.empty() && B.cvx_items.empty() && B.cvx_list_planes.empty(), "map data without a map");
    return;
  }
  const int res = B.cvx_res;
  EXPECT(!B.hull && B.n_mirror == 0 && res >= 4 && res <= 96, "res %d", res);
  EXPECT(B.cvx_start.size() == (size_t)6 * res * res + 1 && B.cvx_start.front() == 0 &&
             B.cvx_start.back() == (int32_t)B.cvx_items.size() && B.cvx_list_planes.size() == B.cvx_items.size(),
         "list offsets");
  if (B.cvx_start.size() != (size_t)6 * res * res + 1 || B.cvx_start.back() != (int32_t)B.cvx_items.size()) return;
  EXPECT(B.cvx_max_arc >= 1e-4 && B.cvx_rin2 > 0.0 && B.cvx_rin2 < B.cvx_rout2, "arc %g", B.cvx_max_arc);
  for (size_t c = 0; c + 1 < B.cvx_start.size(); ++c) {
    EXPECT(B.cvx_start[c] <= B.cvx_start[c + 1], "start falls at cell %zu", c);
    std::vector<int32_t> l(B.cvx_items.begin() + B.cvx_start[c], B.cvx_items.begin() + B.cvx_start[c + 1]);
    std::sort(l.begin(), l.end());
    EXPECT(std::adjacent_find(l.begin(), l.end()) == l.end(), "cell %zu lists a triangle twice", c);
  }
  for (size_t e = 0; e < B.cvx_items.size(); ++e) {
    const int32_t t = B.cvx_items[e];
    if (t < 0 || t >= B.n_tri) {
      EXPECT(false, "item %d", t);
      return;
    }
    const Tri3& T = B.tris[(size_t)t];
    const Emit3& E = B.polys[(size_t)T.poly];
    const CvxPlane& pl = B.cvx_list_planes[e];
    EXPECT(pl.n[0] == E.n[0] && pl.n[1] == E.n[1] && pl.n[2] == E.n[2] &&
               pl.h == E.n[0] * T.v0[0] + E.n[1] * T.v0[1] + E.n[2] * T.v0[2],
           "entry %zu is not the plane of triangle %d", e, t);
  }
  Rng rng{20261021};
  const P3 c{B.cvx_c[0], B.cvx_c[1], B.cvx_c[2]};
  int64_t missing = 0, tested = 0;
  for (int64_t t = 0; t < B.n_tri; ++t) {
    const Tri3& T = B.tris[(size_t)t];
    const P3 a{T.v0[0], T.v0[1], T.v0[2]}, e1{T.e1[0], T.e1[1], T.e1[2]}, e2{T.e2[0], T.e2[1], T.e2[2]};
    std::vector<P3> pts = {a, a + e1, a + e2, a + e1 * 0.5, a + e2 * 0.5, a + (e1 + e2) * 0.5, a + (e1 + e2) * (1.0 / 3.0)};
    for (int k = 0; k < 64; ++k) {
      double u = rng.uniform(), v = rng.uniform();
      if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
      pts.push_back(a + e1 * u + e2 * v);
    }
    for (const P3& p : pts) {
      const P3 d = unit(p - c);
      const P3 w1 = unit(cross(d, std::fabs(d.x) < 0.6 ? P3{1, 0, 0} : P3{0, 1, 0})), w2 = cross(d, w1);
      for (int k = 0; k <= 16; ++k) {
        P3 x = d;
        if (k > 0) {
          const double arc = B.cvx_max_arc * rng.uniform(), phi = 6.283185307179586 * rng.uniform();
          x = d * std::cos(arc) + (w1 * std::cos(phi) + w2 * std::sin(phi)) * std::sin(arc);
        }
        const int cell = cvx_cell((float)x.x, (float)x.y, (float)x.z, res);
        const int32_t* b = &B.cvx_items[(size_t)B.cvx_start[(size_t)cell]];
        const int32_t* e = &B.cvx_items[(size_t)B.cvx_start[(size_t)cell + 1]];
        ++tested;
        if (std::find(b, e, (int32_t)t) == e) ++missing;
      }
    }
  }
  EXPECT(missing == 0, "%lld of %lld directions: the triangle is not in the cell's list", (long long)missing, (long long)tested);
}

// ---------------------------------------------------------------- fingerprint

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
  }
  void f64(double x) { bytes(&x, 8); }
  void f32(float x) { bytes(&x, 4); }
  void i64(int64_t x) { bytes(&x, 8); }
  template <class T, size_t N>
  void f64s(const T (&a)[N]) {
    for (size_t i = 0; i < N; ++i) f64(a[i]);
  }
  void tri(const Tri3& T) {
    f64s(T.v0), f64s(T.e1), f64s(T.e2);
    i64(T.poly), i64(T.id);
  }
};

// Everything but the cube map's lists and the scalars that pass through
// sin / cos / atan2 / asin (cvx_cos_arc).
static uint64_t fingerprint(const Scene3dBuild& B) {
  Fnv F;
  for (const Emit3& E : B.polys) {
    for (const auto& v : E.v) F.f64s(v);
    F.f64s(E.n), F.f64s(E.t1), F.f64s(E.t2);
    F.f64(E.tri_frac);
    F.i64(E.nv), F.i64(E.group), F.i64(E.glo), F.i64(E.ghi), F.i64(E.convex);
  }
  for (const Tri3& T : B.tris) F.tri(T);
  for (const Bvh2Node& N : B.nodes)
    for (int c = 0; c < 2; ++c) {
      for (int d = 0; d < 3; ++d) F.f32(N.lo[c][d]), F.f32(N.hi[c][d]);
      F.i64(N.child[c]), F.i64(N.group[c]);
    }
  for (const HullFace& H : B.faces) {
    for (int32_t x : {H.axis, H.side, H.group, H.nu, H.nv, H.lu, H.lv, H.cell0}) F.i64(x);
    F.f32(H.plane), F.f32(H.inv_du), F.f32(H.inv_dv);
  }
  for (float x : B.lines) F.f32(x);
  for (const Tri3& T : B.hull_tris) F.tri(T);
  for (double x : B.mirror_n) F.f64(x);
  for (int64_t x : {B.n_poly, B.n_mirror, B.n_tri, B.n_mirror_tris, (int64_t)B.mirror_group0, (int64_t)B.stack,
                    (int64_t)B.hull, (int64_t)B.full_root, (int64_t)B.n_in_nodes, B.n_in_tris,
                    (int64_t)B.convex_interior, (int64_t)B.cvx, (int64_t)B.cvx_res})
    F.i64(x);
  F.f64(B.scale);
  F.f64s(B.box_lo), F.f64s(B.ball), F.f64s(B.cvx_c);
  for (float x : B.box_len) F.f32(x);
  F.f32(B.margin), F.f32(B.cvx_tpad);
  F.f64(B.cvx_max_arc), F.f64(B.cvx_rin2), F.f64(B.cvx_rout2);
  return F.h;
}

// mode as rthx_scene3d_hull reports it: 0 plain, 1 hull, 2 hull with a convex interior, 3 exit-direction map
static void run_scene(const Scene& s, int mode, const Scene3dOptions& opt = Scene3dOptions{}) {
  current = s.name.c_str();
  Scene3dBuild B;
  std::string err;
  const int rc = s.build(B, err, opt);
  EXPECT(rc == RTHX_OK, "refused: %s", err.c_str());
  if (rc != RTHX_OK) return;
  const int got = B.hull ? (B.convex_interior ? 2 : 1) : B.cvx ? 3 : 0;
  EXPECT(got == mode, "mode %d, expected %d", got, mode);
  check_bvh(s, B);
  check_hull(s, B);
  check_cube_map(B);
  std::printf("scene %s hash %016llx mode %d tris %lld nodes %zu stack %d res %d items %zu\n", s.name.c_str(),
              (unsigned long long)fingerprint(B), got, (long long)B.n_tri, B.nodes.size(), B.stack, B.cvx_res,
              B.cvx_items.size());
}

// ---------------------------------------------------------------- BVH alone

// About 40 triangles sharing a corner, each `ratio` times the one before:
// binned SAH peels them off a few at a time.
static Scene nested_triangles(double ratio) {
  Scene s;
  s.name = "nested_triangles";
  double r = 1e-3;
  for (int k = 0; k < 40; ++k, r *= ratio) s.add({{0, 0, 0}, {r, 0, 0.1 * r}, {0, r, 0.2 * r}}, {0, 0, 1}, k);
  return s;
}

static void check_bvh2_forms() {
  const Scene s = nested_triangles(8.0);
  current = "build_bvh2";
  std::vector<BuildTri> bt;
  for (int64_t k = 0; k < s.n(); ++k) {
    BuildTri T{};
    for (int d = 0; d < 3; ++d) {
      const double x[3] = {s.xyz[(size_t)(12 * k + d)], s.xyz[(size_t)(12 * k + 3 + d)], s.xyz[(size_t)(12 * k + 6 + d)]};
      T.lo[d] = std::min({x[0], x[1], x[2]});
      T.hi[d] = std::max({x[0], x[1], x[2]});
      T.c[d] = (x[0] + x[1] + x[2]) / 3.0;
    }
    T.group = (int)k;
    bt.push_back(T);
  }
  const double pad = kBoxPad * s.xyz[(size_t)(12 * 39 + 3)];
  int depth[2];
  for (int median = 0; median < 2; ++median) {
    std::vector<Bvh2Node> nodes;
    std::vector<int> order(bt.size());
    depth[median] = build_bvh2(nodes, order, bt, pad, median != 0);
    std::vector<int> sorted = order;
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 0; i < sorted.size(); ++i) EXPECT(sorted[i] == (int)i, "order is no permutation");
    auto verts = [&](int64_t t, double (*v)[3]) {
      for (int i = 0; i < 3; ++i)
        for (int d = 0; d < 3; ++d) v[i][d] = s.xyz[(size_t)(12 * order[(size_t)t] + 3 * i + d)];
    };
    auto group_of = [&](int64_t t) { return (int32_t)order[(size_t)t]; };
    const int measured = check_tree(nodes, 0, (int32_t)nodes.size(), 0, (int64_t)bt.size(), pad, false, verts, group_of);
    EXPECT(measured == depth[median], "median %d: measured depth %d, returned %d", median, measured, depth[median]);
  }
  EXPECT(depth[1] == 5, "median depth %d of 40 triangles in leaves of <= 2", depth[1]);  // ceil(log2(40 / 2))
  std::printf("build_bvh2 nested_triangles: SAH depth %d, median depth %d\n", depth[0], depth[1]);
  Scene3dBuild B;
  std::string err;
  EXPECT(s.build(B, err) == RTHX_OK, "%s", err.c_str());
  if (depth[0] > kBvhStack) EXPECT(B.stack == depth[1], "fallback: stack %d, median depth %d", B.stack, depth[1]);
  else EXPECT(B.stack == depth[0], "stack %d, SAH depth %d", B.stack, depth[0]);
  run_scene(s, 0);
}

// ---------------------------------------------------------------- refusals

static void expect_refusal(const char* what, const Scene& s, int code, const char* text, int64_t n = -1,
                           int64_t n_mirror = -1, bool null_xyz = false, bool null_mirror = false) {
  current = what;
  Scene3dBuild B;
  B.n_poly = 77;  // (a refusal leaves an empty result)
  std::string err;
  const int rc = build_scene3d(null_xyz ? nullptr : s.xyz.data(), s.nv.data(), s.nrm.data(), s.grouped ? s.group.data() : nullptr,
                               n >= 0 ? n : s.n(), null_mirror ? nullptr : s.mxyz.data(), s.mnv.data(),
                               n_mirror != -1 ? n_mirror : s.n_mirror(), Scene3dOptions{}, B, err);
  EXPECT(rc == code && err == text, "rc %d \"%s\", expected %d \"%s\"", rc, err.c_str(), code, text);
  EXPECT(B.polys.empty() && B.tris.empty() && B.nodes.empty() && B.n_poly == 0 && B.n_tri == 0 && !B.hull && !B.cvx, "something was built");
}

static void check_refusals() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const Scene ok = octant_mirrored();
  Scene s;
  expect_refusal("mirror count", ok, RTHX_EINVAL, "mirror count must be >= 0", -1, -2);
  expect_refusal("null mirrors", ok, RTHX_EINVAL, "null mirror arrays with n_mirror > 0", -1, -1, false, true);
  expect_refusal("null xyz", ok, RTHX_EINVAL, "null argument or fewer than 2 polygons", -1, -1, true);
  expect_refusal("one polygon", ok, RTHX_EINVAL, "null argument or fewer than 2 polygons", 1, 0);
  expect_refusal("2^30 polygons", ok, RTHX_ERANGE, "too many polygons", int64_t(1) << 30, 0);
  s = ok, s.grouped = true, s.group[1] = -1;
  expect_refusal("negative group", s, RTHX_EINVAL, "group ids must be >= 0");
  s = ok, s.grouped = true, s.group = {0, 1, 0};
  expect_refusal("split group", s, RTHX_EINVAL, "a group's polygons must be contiguous");
  s = ok, s.nv[2] = 5;
  expect_refusal("pentagon", s, RTHX_EINVAL, "polygon with n not in {3,4}");
  s = ok, s.xyz[13] = nan;
  expect_refusal("nan vertex", s, RTHX_EINVAL, "non-finite vertex");
  s = ok;
  for (int d = 0; d < 3; ++d) s.xyz[(size_t)(3 + d)] = s.xyz[(size_t)d];  // v1 = v0
  expect_refusal("zero area", s, RTHX_EINVAL, "degenerate polygon (zero area)");
  s = ok, s.nrm[3] = s.nrm[4] = s.nrm[5] = 0.0;
  expect_refusal("zero normal", s, RTHX_EINVAL, "normal must be finite and non-zero");
  s = ok, s.xyz[9] += 0.1;  // v3 of the x = 0 quad off its plane
  expect_refusal("bent quad", s, RTHX_EINVAL, "quad vertices are not coplanar");
  s = ok, s.grouped = true, s.group = {0, 1, std::numeric_limits<int32_t>::max()};
  expect_refusal("group 2^31 - 1", s, RTHX_ERANGE, "group ids leave no room for the mirror groups");
  s = ok, s.mnv[1] = 0;
  expect_refusal("mirror of 0", s, RTHX_EINVAL, "mirror polygon with n not in {3,4}");
  s = ok, s.mxyz[30] = std::numeric_limits<double>::infinity();
  expect_refusal("inf mirror vertex", s, RTHX_EINVAL, "non-finite mirror vertex");
  s = ok;
  for (int d = 0; d < 3; ++d) s.mxyz[(size_t)(6 + d)] = s.mxyz[(size_t)d];  // v2 = v0
  expect_refusal("zero-area mirror", s, RTHX_EINVAL, "degenerate mirror polygon (zero area)");
  s = ok, s.mxyz[9] += 0.1;
  expect_refusal("bent mirror", s, RTHX_EINVAL, "mirror quad vertices are not coplanar");
}

int main() {
  const int c111[3] = {1, 1, 1}, c232[3] = {2, 3, 2};
  run_scene(few_triangles(2), 0);
  run_scene(few_triangles(3), 0);
  Scene cube;
  cube.name = "cube_inward";
  const double L1[3] = {1.0, 1.0, 1.0};
  add_box(cube, L1, c111, 0);
  run_scene(cube, 3);
  Scene tetra;
  tetra.name = "tetrahedron_inward";
  add_tetra(tetra, {0.1, 0.2, 0.3}, 1.0, false, 0);
  run_scene(tetra, 3);
  Scene ico;
  ico.name = "icosphere1_inward";
  add_icosphere1(ico);
  run_scene(ico, 3);
  run_scene(hull_scene("hull_1x1", c111, 0), 1);
  const Scene hull_tetra = hull_scene("hull_2x3x2_tetrahedron", c232, 1);
  run_scene(hull_tetra, 2);
  run_scene(hull_scene("hull_2x3x2_two_tetrahedra", c232, 2), 1);
  run_scene(hull_scene("hull_face_group_split", c232, 0, true), 3);  // (no hull; the empty box is still convex)
  Scene mixed = tetra;
  mixed.name = "tetrahedron_noncoplanar_group";
  mixed.grouped = true;
  mixed.group = {0, 0, 1, 2};
  run_scene(mixed, 0);
  run_scene(octant_mirrored(), 0);
  run_scene(moved(hull_tetra, "hull_2x3x2_tetrahedron_moved"), 0);
  run_scene(moved(cube, "cube_inward_moved"), 3);
  // the knobs' options: no hull (the convex interior makes it no enclosure), no map
  Scene3dOptions no_hull, no_cvx;
  no_hull.no_hull = true;
  no_cvx.no_cvx = true;
  Scene off = hull_tetra;
  off.name = "hull_2x3x2_tetrahedron_no_hull";
  run_scene(off, 0, no_hull);
  off = cube, off.name = "cube_inward_no_cvx";
  run_scene(off, 0, no_cvx);
  check_bvh2_forms();
  check_refusals();
  if (fails) {
    std::printf("scene3d check FAILED: %d\n", fails);
    return 1;
  }
  std::printf("scene3d check ok\n");
  return 0;
}
