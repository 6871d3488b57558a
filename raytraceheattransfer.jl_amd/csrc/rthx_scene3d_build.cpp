// rthx_scene3d_build.cpp -- the 3D tracer's host-side scene build
// (rthx_scene3d_build.h build_scene3d; the C ABI around it is rthx_trace3d.cpp).
//
// build_scene3d validates the polygons, orients each emission frame by the
// caller's normal, splits quads into two triangles (v0 v1 v2, v2 v3 v0 -- the
// same split the emission uses) and builds a two-child BVH (binned SAH, leaves
// of <= kLeafTris triangles, both children's bounds in each node as fp32
// padded outward by kBoxPad of the scene scale, so the device's fp32 slab
// tests never drop a hit the fp64 Moeller-Trumbore test would find).  It then
// detects the two fast paths' scenes: the box hull (HullFace) with its
// interior BVH, and the convex enclosure with its cube map of exit directions
// (CvxPlane).  Pure host code: no HIP, no environment, no global state;
// tests/scene3d_host_check.cpp checks what it produces by brute force.
#include "rthx_scene3d_build.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <numeric>
#include <unordered_map>

#include "../../include/rthx.h"

namespace rthx {
namespace {

int refuse(std::string& err, int code, const std::string& msg) {
  err = msg;
  return code;
}

struct V {
  double x, y, z;
};
V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double norm(V a) { return std::sqrt(dot(a, a)); }
V scale(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
V at(const double* p) { return {p[0], p[1], p[2]}; }
void put(double* p, V a) { p[0] = a.x, p[1] = a.y, p[2] = a.z; }
// Signed distance of q from polygon E's plane, positive on the emitting side.
double plane_dist(const Emit3& E, V q) { return dot(at(E.n), sub(q, at(E.v[0]))); }

#ifndef RTHX_T3_SAH_BINS
#define RTHX_T3_SAH_BINS 16
#endif

struct Box {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  void grow(const double* l, const double* h) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], l[k]);
      hi[k] = std::max(hi[k], h[k]);
    }
  }
  double area() const {
    const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
    return x < 0 ? 0.0 : 2.0 * (x * y + y * z + z * x);
  }
};

// fp32 bound below x - pad / above x + pad (rounded outward)
float down32(double x) {
  float f = (float)x;
  while ((double)f > x) f = std::nextafter(f, -HUGE_VALF);
  return f;
}
float up32(double x) {
  float f = (float)x;
  while ((double)f < x) f = std::nextafter(f, HUGE_VALF);
  return f;
}

int32_t leaf_ref(int first, int count) { return ~((first << kLeafBits) | count); }

// Binary BVH over triangle indices order[b, e): binned SAH (16 bins per axis
// over the centroid bounds; `median` forces median splits on the longest
// centroid axis).  Leaves hold <= kLeafTris triangles.  Returns the child
// reference of the range and its bounds; `depth` tracks the deepest inner
// node (stack bound of the walk).
struct Bvh2Builder {
  std::vector<Bvh2Node>& nodes;
  std::vector<int>& order;
  const std::vector<BuildTri>& bt;
  double pad;
  bool median;
  int depth = 0;

  void set_child(int idx, int slot, int32_t ref, const Box& bx, int group) {
    Bvh2Node& nd = nodes[idx];
    nd.child[slot] = ref;
    nd.group[slot] = group;
    for (int k = 0; k < 3; ++k) {
      nd.lo[slot][k] = down32(bx.lo[k] - pad);
      nd.hi[slot][k] = up32(bx.hi[k] + pad);
    }
  }

  // group of the range order[b, e): the common group of its triangles, or -1
  int range_group(int b, int e) const {
    const int g = b < e ? bt[order[b]].group : -1;
    for (int i = b + 1; i < e; ++i)
      if (bt[order[i]].group != g) return -1;
    return g;
  }

  int32_t build(int b, int e, int level, Box& out) {
    Box bx, cb;
    for (int i = b; i < e; ++i) {
      const BuildTri& t = bt[order[i]];
      bx.grow(t.lo, t.hi);
      cb.grow(t.c, t.c);
    }
    out = bx;
    if (e - b <= kLeafTris) return leaf_ref(b, e - b);
    depth = std::max(depth, level + 1);
    int axis = 0;
    for (int k = 1; k < 3; ++k)
      if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
    int mid = b + (e - b) / 2;
    bool done = false;
    if (!median) {
      constexpr int kBins = RTHX_T3_SAH_BINS;
      double best = 1e300;
      int best_axis = -1, best_bin = -1;
      for (int k = 0; k < 3; ++k) {
        const double ext = cb.hi[k] - cb.lo[k];
        if (!(ext > 0.0)) continue;
        Box bin_box[kBins];
        int bin_n[kBins] = {0};
        for (int i = b; i < e; ++i) {
          const BuildTri& t = bt[order[i]];
          int j = (int)((t.c[k] - cb.lo[k]) / ext * kBins);
          j = std::min(kBins - 1, std::max(0, j));
          bin_box[j].grow(t.lo, t.hi);
          ++bin_n[j];
        }
        Box left[kBins];
        int nl[kBins];
        Box acc;
        int n = 0;
        for (int j = 0; j < kBins; ++j) {
          acc.grow(bin_box[j].lo, bin_box[j].hi);
          n += bin_n[j];
          left[j] = acc;
          nl[j] = n;
        }
        Box racc;
        int nr = 0;
        for (int j = kBins - 1; j > 0; --j) {
          racc.grow(bin_box[j].lo, bin_box[j].hi);
          nr += bin_n[j];
          if (nl[j - 1] == 0 || nr == 0) continue;
          const double cost = left[j - 1].area() * nl[j - 1] + racc.area() * nr;
          if (cost < best) {
            best = cost;
            best_axis = k;
            best_bin = j;
          }
        }
      }
      if (best_axis >= 0) {
        const int k = best_axis;
        const double ext = cb.hi[k] - cb.lo[k];
        auto in_left = [&](int ti) {
          int j = (int)((bt[ti].c[k] - cb.lo[k]) / ext * kBins);
          j = std::min(kBins - 1, std::max(0, j));
          return j < best_bin;
        };
        // stable partition: deterministic order of equal keys
        mid = (int)(std::stable_partition(order.begin() + b, order.begin() + e, in_left) - order.begin());
        done = mid > b && mid < e;
      }
    }
    if (!done) {
      mid = b + (e - b) / 2;
      std::nth_element(order.begin() + b, order.begin() + mid, order.begin() + e, [&](int x, int y) {
        return bt[x].c[axis] < bt[y].c[axis] || (bt[x].c[axis] == bt[y].c[axis] && x < y);
      });
    }
    const int idx = (int)nodes.size();
    nodes.push_back(Bvh2Node{});
    Box lb, rb;
    const int32_t l = build(b, mid, level + 1, lb);
    const int32_t r = build(mid, e, level + 1, rb);
    set_child(idx, 0, l, lb, range_group(b, mid));
    set_child(idx, 1, r, rb, range_group(mid, e));
    return idx;
  }
};

}  // namespace

int build_bvh2(std::vector<Bvh2Node>& nodes, std::vector<int>& order, const std::vector<BuildTri>& bt, double pad,
               bool median) {
  nodes.clear();
  std::iota(order.begin(), order.end(), 0);
  Bvh2Builder B{nodes, order, bt, pad, median};
  const int n = (int)order.size();
  if (n <= kLeafTris) {
    nodes.push_back(Bvh2Node{});
    Box bx, empty;
    for (int i = 0; i < n; ++i) bx.grow(bt[i].lo, bt[i].hi);
    B.set_child(0, 0, leaf_ref(0, n), bx, B.range_group(0, n));
    B.set_child(0, 1, leaf_ref(0, 0), empty, -1);
    return 1;
  }
  Box root;
  B.build(0, n, 0, root);
  return B.depth;
}

namespace {

// Node layout: the top kTopNodes inner nodes in breadth-first order at the
// start of the array (the hottest nodes contiguous; the kernel may stage them
// in LDS), every subtree below them depth-first (a walk descending one path
// reads neighbouring records).  Child references are remapped; leaf
// references are unchanged.  The root stays node 0.
void layout_nodes(std::vector<Bvh2Node>& nodes) {
  const int n = (int)nodes.size();
  std::vector<int> order;
  order.reserve(n);
  std::vector<char> taken(n, 0);
  std::vector<int> frontier{0};
  taken[0] = 1;
  for (size_t h = 0; h < frontier.size() && (int)order.size() < kTopNodes; ++h) {
    const int i = frontier[h];
    order.push_back(i);
    for (int c = 0; c < 2; ++c) {
      const int ch = nodes[i].child[c];
      if (ch >= 0 && !taken[ch]) {
        taken[ch] = 1;
        frontier.push_back(ch);
      }
    }
  }
  std::vector<char> placed(n, 0);
  for (int i : order) placed[i] = 1;
  // depth-first below the breadth-first top, in frontier order
  std::vector<int> st;
  for (int f : frontier) {
    if (placed[f]) continue;
    st.push_back(f);
    while (!st.empty()) {
      const int i = st.back();
      st.pop_back();
      if (placed[i]) continue;
      placed[i] = 1;
      order.push_back(i);
      for (int c = 1; c >= 0; --c) {
        const int ch = nodes[i].child[c];
        if (ch >= 0 && !placed[ch]) st.push_back(ch);
      }
    }
  }
  std::vector<int> pos(n);
  for (int k = 0; k < n; ++k) pos[order[k]] = k;
  std::vector<Bvh2Node> out(n);
  for (int k = 0; k < n; ++k) {
    out[k] = nodes[order[k]];
    for (int c = 0; c < 2; ++c)
      if (out[k].child[c] >= 0) out[k].child[c] = pos[out[k].child[c]];
  }
  nodes.swap(out);
}

// Box hull (rthx_scene3d.h HullFace): six coplanar groups that are the six
// faces of the scene's bounding box, each a lattice of quads whose corners
// lie within 1e-12 of the box's extent of the lattice lines.  Faces are
// stored in the order 2 axis + side.
struct HullBuild {
  std::vector<HullFace> faces;
  std::vector<float> lines;
  std::vector<int64_t> cell_poly;  // polygon of every hull cell, in face / cell order
  std::vector<char> in_hull;       // per polygon
  double margin = 0.0;
};

// Sorted distinct values of v, those within tol of the previous one merged.
std::vector<double> cluster_lines(std::vector<double> v, double tol) {
  std::sort(v.begin(), v.end());
  std::vector<double> out;
  for (double x : v)
    if (out.empty() || x - out.back() > tol) out.push_back(x);
  return out;
}

// Index of x among the lines (within tol), or -1.
int64_t line_index(const std::vector<double>& L, double x, double tol) {
  const auto it = std::lower_bound(L.begin(), L.end(), x - tol);
  return (it != L.end() && std::fabs(*it - x) <= tol) ? (int64_t)(it - L.begin()) : -1;
}

bool detect_box_hull(const std::vector<Emit3>& P, int64_t n, const double* slo, const double* shi,
                     HullBuild& hb) {
  double L[3], Lmax = 0.0;
  for (int k = 0; k < 3; ++k) {
    L[k] = shi[k] - slo[k];
    if (!(L[k] > 0.0)) return false;
    Lmax = std::max(Lmax, L[k]);
  }
  const double tol = 1e-12 * Lmax;
  hb.margin = (double)kHullMargin * Lmax;
  int64_t run_b[6], run_e[6];
  for (int f = 0; f < 6; ++f) run_b[f] = run_e[f] = -1;
  // which box plane each group lies on (all its polygons quads)
  for (int64_t b = 0; b < n; b = P[b].ghi) {
    const int64_t e = P[b].ghi;
    int face = -1;
    for (int f = 0; f < 6 && face < 0; ++f) {
      const int k = f >> 1;
      const double plane = (f & 1) ? shi[k] : slo[k];
      bool on = true;
      for (int64_t p = b; p < e && on; ++p) {
        on = P[p].nv == 4;
        for (int i = 0; i < 4 && on; ++i) on = std::fabs(P[p].v[i][k] - plane) <= tol;
      }
      if (on) face = f;
    }
    if (face < 0) continue;  // an interior group
    if (run_b[face] >= 0) return false;  // (two groups on one face plane)
    run_b[face] = b;
    run_e[face] = e;
  }
  hb.faces.clear();
  hb.lines.clear();
  hb.cell_poly.clear();
  hb.in_hull.assign((size_t)n, 0);
  for (int f = 0; f < 6; ++f) {
    if (run_b[f] < 0) return false;
    const int k = f >> 1, u = (k + 1) % 3, v = (k + 2) % 3;
    std::vector<double> cu, cv;
    for (int64_t p = run_b[f]; p < run_e[f]; ++p)
      for (int i = 0; i < 4; ++i) {
        cu.push_back(P[p].v[i][u] - slo[u]);
        cv.push_back(P[p].v[i][v] - slo[v]);
      }
    const std::vector<double> lu = cluster_lines(cu, tol), lv = cluster_lines(cv, tol);
    const int64_t nu = (int64_t)lu.size() - 1, nv = (int64_t)lv.size() - 1;
    if (nu < 1 || nv < 1 || nu * nv != run_e[f] - run_b[f]) return false;
    if (std::fabs(lu.front()) > tol || std::fabs(lu.back() - L[u]) > tol || std::fabs(lv.front()) > tol ||
        std::fabs(lv.back() - L[v]) > tol)
      return false;  // (the face must cover the box face)
    for (int64_t i = 0; i < nu; ++i)
      if (lu[i + 1] - lu[i] < 8.0 * hb.margin) return false;  // (one neighbour cell covers the margin)
    for (int64_t j = 0; j < nv; ++j)
      if (lv[j + 1] - lv[j] < 8.0 * hb.margin) return false;
    std::vector<int64_t> cell((size_t)(nu * nv), -1);
    for (int64_t p = run_b[f]; p < run_e[f]; ++p) {
      int64_t iu[4], iv[4];
      for (int i = 0; i < 4; ++i) {
        iu[i] = line_index(lu, P[p].v[i][u] - slo[u], tol);
        iv[i] = line_index(lv, P[p].v[i][v] - slo[v], tol);
        if (iu[i] < 0 || iv[i] < 0) return false;
      }
      const int64_t i0 = *std::min_element(iu, iu + 4), j0 = *std::min_element(iv, iv + 4);
      int seen = 0;  // the four corners of cell (i0, j0), each once
      for (int i = 0; i < 4; ++i) {
        const int64_t di = iu[i] - i0, dj = iv[i] - j0;
        if (di < 0 || di > 1 || dj < 0 || dj > 1) return false;
        seen |= 1 << (di + 2 * dj);
      }
      if (seen != 15 || cell[(size_t)(j0 * nu + i0)] >= 0) return false;
      cell[(size_t)(j0 * nu + i0)] = p;
    }
    HullFace F{};
    F.axis = k;
    F.side = f & 1;
    F.group = P[run_b[f]].group;
    F.nu = (int32_t)nu;
    F.nv = (int32_t)nv;
    F.lu = (int32_t)hb.lines.size();
    for (double x : lu) hb.lines.push_back((float)x);
    F.lv = (int32_t)hb.lines.size();
    for (double x : lv) hb.lines.push_back((float)x);
    F.cell0 = (int32_t)hb.cell_poly.size();
    F.plane = (f & 1) ? (float)L[k] : 0.0f;
    F.inv_du = (float)((double)nu / L[u]);
    F.inv_dv = (float)((double)nv / L[v]);
    for (int64_t c : cell) {
      hb.cell_poly.push_back(c);
      hb.in_hull[(size_t)c] = 1;
    }
    hb.faces.push_back(F);
  }
  return hb.lines.size() <= 4096;  // (the kernel stages the lines in LDS: at most 16 KB)
}

// The distinct vertices of the polygons k with take(k), sorted.
template <class Take>
std::vector<V> unique_vertices(const std::vector<Emit3>& P, Take take) {
  std::vector<V> verts;
  for (size_t k = 0; k < P.size(); ++k)
    if (take(k))
      for (int i = 0; i < P[k].nv; ++i) verts.push_back(at(P[k].v[i]));
  std::sort(verts.begin(), verts.end(), [](const V& a, const V& b) {
    return a.x < b.x || (a.x == b.x && (a.y < b.y || (a.y == b.y && a.z < b.z)));
  });
  verts.erase(std::unique(verts.begin(), verts.end(),
                          [](const V& a, const V& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }),
              verts.end());
  return verts;
}

// The vertices' mean and the distance of the farthest from it.
void mean_and_reach(const std::vector<V>& verts, V& mean, double& reach) {
  mean = {0.0, 0.0, 0.0};
  for (const V& q : verts) mean = {mean.x + q.x, mean.y + q.y, mean.z + q.z};
  mean = scale(mean, 1.0 / (double)verts.size());
  reach = 0.0;
  for (const V& q : verts) reach = std::max(reach, norm(sub(q, mean)));
}

// Convex enclosure seen from inside (rthx_scene3d.h CvxPlane): every vertex
// on or in front of every polygon's emitting plane (within 1e-12 of the
// scene scale) and the vertices' centroid strictly inside.  Fills B's
// centroid, its inscribed / circumscribed radii (padded outward), the largest
// half-arc and the cube map's lists over the triangles of `tris`, each entry
// with its triangle's plane; false when the scene is not such an enclosure
// (the lists are then left empty).
double angle_between(V a, V b) {  // unit vectors; robust near 0 and pi
  return std::atan2(norm(cross(a, b)), dot(a, b));
}

// Angular distance from unit direction x to the spherical triangle with unit
// corners w[0..2] (0 inside): the nearest of its three great-circle arcs,
// or corner.
double sph_tri_dist(V x, const V w[3]) {
  const V n01 = cross(w[0], w[1]), n12 = cross(w[1], w[2]), n20 = cross(w[2], w[0]);
  const double s = dot(cross(sub(w[1], w[0]), sub(w[2], w[0])), w[0]) >= 0.0 ? 1.0 : -1.0;  // orientation
  if (s * dot(x, n01) >= 0.0 && s * dot(x, n12) >= 0.0 && s * dot(x, n20) >= 0.0) return 0.0;
  double best = 1e300;
  for (int e = 0; e < 3; ++e) {
    const V a = w[e], b = w[(e + 1) % 3];
    const V nn = cross(a, b);
    const double ln = norm(nn);
    best = std::min({best, angle_between(x, a), angle_between(x, b)});
    if (!(ln > 0.0)) continue;
    const V u = scale(nn, 1.0 / ln);
    const double xn = dot(x, u);
    V p = sub(x, scale(u, xn));
    const double lp = norm(p);
    if (!(lp > 0.0)) continue;
    p = scale(p, 1.0 / lp);
    // p within the arc a -> b
    if (dot(cross(a, p), u) >= 0.0 && dot(cross(p, b), u) >= 0.0) best = std::min(best, std::asin(std::min(1.0, std::fabs(xn))));
  }
  return best;
}

// The unit direction of cube-map face f at (u, v) in [-1, 1]^2 (the inverse
// of cvx_cell's mapping).
V cvx_dir(int f, double u, double v) {
  const double s = (f & 1) ? -1.0 : 1.0;
  V m = f < 2 ? V{s, u, v} : f < 4 ? V{v, s, u} : V{u, v, s};
  return scale(m, 1.0 / norm(m));
}

bool detect_convex_enclosure(const std::vector<Emit3>& P, const std::vector<Tri3>& tris, double scale_,
                             const Scene3dOptions& opt, Scene3dBuild& B) {
  const std::vector<V> verts = unique_vertices(P, [](size_t) { return true; });
  const double tol = 1e-12 * scale_;
  for (const Emit3& E : P)
    for (const V& q : verts)
      if (plane_dist(E, q) < -tol) return false;
  V c;
  double rout;
  mean_and_reach(verts, c, rout);
  double rin = 1e300;
  for (const Emit3& E : P) rin = std::min(rin, plane_dist(E, c));
  if (!(rin > 1e-6 * scale_)) return false;  // (the centroid must lie well inside)
  put(B.cvx_c, c);
  const double rin_pad = rin * (1.0 - 1e-9), rout_pad = rout * (1.0 + 1e-9) + 1e-12 * scale_;
  B.cvx_rin2 = rin_pad * rin_pad;
  B.cvx_rout2 = rout_pad * rout_pad;
  {
    const double q = rin / rout;
    B.cvx_max_arc = std::min(kCvxArcMax, std::max(kCvxArcMin, 0.25 * std::sqrt(std::max(0.0, 1.0 - q * q))));
    if (opt.cvx_arc > 0.0) B.cvx_max_arc = opt.cvx_arc;
    B.cvx_cos_arc = (float)std::cos(2.0 * B.cvx_max_arc);
  }
  // one plane per triangle (its polygon's emitting normal)
  std::vector<CvxPlane> planes(tris.size());
  std::vector<V> tcen(tris.size());
  std::vector<std::array<V, 3>> tw(tris.size());  // corner directions
  std::vector<double> tha(tris.size());
  for (size_t t = 0; t < tris.size(); ++t) {
    const Tri3& T = tris[t];
    const Emit3& E = P[(size_t)T.poly];
    CvxPlane& pl = planes[t];
    for (int k = 0; k < 3; ++k) pl.n[k] = E.n[k];
    pl.h = E.n[0] * T.v0[0] + E.n[1] * T.v0[1] + E.n[2] * T.v0[2];
    const V a{T.v0[0], T.v0[1], T.v0[2]};
    const V b{a.x + T.e1[0], a.y + T.e1[1], a.z + T.e1[2]}, d{a.x + T.e2[0], a.y + T.e2[1], a.z + T.e2[2]};
    V w[3] = {sub(a, c), sub(b, c), sub(d, c)};
    for (V& x : w) x = scale(x, 1.0 / norm(x));
    V m = {w[0].x + w[1].x + w[2].x, w[0].y + w[1].y + w[2].y, w[0].z + w[1].z + w[2].z};
    m = scale(m, 1.0 / norm(m));
    tcen[t] = m;
    tw[t][0] = w[0];
    tw[t][1] = w[1];
    tw[t][2] = w[2];
    // (the spherical triangle lies in the cap through its corners: a cap
    // under 90 degrees is convex on the sphere)
    tha[t] = std::max({angle_between(m, w[0]), angle_between(m, w[1]), angle_between(m, w[2])});
    if (!(tha[t] < 1.4)) return false;  // (a triangle too wide for the cone bound)
  }
  std::vector<double> tcos(tris.size()), tsin(tris.size());
  for (size_t t = 0; t < tris.size(); ++t) {
    tcos[t] = std::cos(tha[t]);
    tsin[t] = std::sin(tha[t]);
  }
  // cube-map resolution: cells about a quarter of a triangle across
  // (RTHX_T3_CVX_RES: cells per triangle edge; 2 / 3 / 4 / 6 measured,
  // profiles/round6/ab/cvx_res_arc.log)
  const double per_face = std::sqrt((double)tris.size() / 6.0);
  const double cells_per_tri = opt.cvx_cells_per_tri > 0.0 ? opt.cvx_cells_per_tri : 4.0;
  const int res = B.cvx_res = (int)std::min(96.0, std::max(4.0, std::ceil(cells_per_tri * per_face)));
  const size_t n_cells = (size_t)6 * res * res;
  B.cvx_start.assign(n_cells + 1, 0);
  for (int f = 0; f < 6; ++f)
    for (int j = 0; j < res; ++j)
      for (int i = 0; i < res; ++i) {
        const double u0 = -1.0 + 2.0 * i / res, u1 = -1.0 + 2.0 * (i + 1) / res;
        const double v0 = -1.0 + 2.0 * j / res, v1 = -1.0 + 2.0 * (j + 1) / res;
        const V cc = cvx_dir(f, 0.5 * (u0 + u1), 0.5 * (v0 + v1));
        const double ha = std::max({angle_between(cc, cvx_dir(f, u0, v0)), angle_between(cc, cvx_dir(f, u1, v0)),
                                    angle_between(cc, cvx_dir(f, u0, v1)), angle_between(cc, cvx_dir(f, u1, v1))});
        const size_t cell = ((size_t)f * res + j) * res + i;
        // angle(cc, tcen) <= a + tha  <=>  cc . tcen >= cos(a) cos(tha) - sin(a) sin(tha)
        // (a + tha < pi; the cosine falls on [0, pi])
        const double a = ha + B.cvx_max_arc + kCvxPad, ca = std::cos(a), sa = std::sin(a);
        std::vector<std::pair<double, int32_t>> in_cell;  // (distance from the cell's centre, triangle)
        // a triangle is listed when its spherical triangle comes within
        // a of the cell's centre (cones first, then the exact distance)
        for (size_t t = 0; t < tris.size(); ++t) {
          const double ct = dot(cc, tcen[t]);
          if (ct >= ca * tcos[t] - sa * tsin[t] - 1e-12 && sph_tri_dist(cc, tw[t].data()) <= a + 1e-9)
            in_cell.push_back({-ct, (int32_t)t});
        }
        std::sort(in_cell.begin(), in_cell.end());
        for (const auto& e : in_cell) {
          B.cvx_items.push_back(e.second);
          B.cvx_list_planes.push_back(planes[(size_t)e.second]);
        }
        B.cvx_start[cell + 1] = (int32_t)B.cvx_items.size();
      }
  return true;
}

// Does every group of more than one polygon lie in one plane -- each vertex
// of the group within tol of its first polygon's plane?  The exit-direction
// map applies no emitter-group skip (Walk::convex_exit): it relies on a
// ray's own plane never being an exit plane (n . d > 0 there), which covers
// the emitter's group only when the group is coplanar.
bool groups_coplanar(const std::vector<Emit3>& P, double tol) {
  const int64_t n = (int64_t)P.size();
  for (int64_t b = 0; b < n; b = P[(size_t)b].ghi) {
    const Emit3& E = P[(size_t)b];
    for (int64_t p = b + 1; p < E.ghi; ++p)
      for (int i = 0; i < P[(size_t)p].nv; ++i)
        if (!(std::fabs(plane_dist(E, at(P[(size_t)p].v[i]))) <= tol)) return false;
  }
  return true;
}

// Leaf references of `nodes` shifted by `tri_off` triangles and inner
// references by `node_off` nodes (a BVH appended behind another).
void shift_bvh(std::vector<Bvh2Node>& nodes, int32_t node_off, int32_t tri_off) {
  for (auto& nd : nodes)
    for (int c = 0; c < 2; ++c) {
      const int32_t r = nd.child[c];
      if (r >= 0) {
        nd.child[c] = r + node_off;
      } else {
        const int32_t ref = ~r;
        nd.child[c] = leaf_ref((ref >> kLeafBits) + tri_off, ref & ((1 << kLeafBits) - 1));
      }
    }
}

// Groups: each a contiguous run of polygon indices ([glo, ghi) per polygon;
// without `group` every polygon is a group of its own).
int group_runs(const int32_t* group, int64_t n, std::vector<int32_t>& glo, std::vector<int32_t>& ghi, std::string& err) {
  glo.resize((size_t)n);
  ghi.resize((size_t)n);
  std::unordered_map<int32_t, int64_t> seen;
  int64_t run = 0;
  for (int64_t k = 0; k < n; ++k) {
    if (group && group[k] < 0) return refuse(err, RTHX_EINVAL, "group ids must be >= 0");
    if (k > 0 && (!group || group[k] != group[k - 1])) run = k;
    const int32_t gk = group ? group[k] : (int32_t)k;
    auto it = seen.find(gk);
    if (it != seen.end() && it->second != run) return refuse(err, RTHX_EINVAL, "a group's polygons must be contiguous");
    seen[gk] = run;
    glo[k] = (int32_t)run;
  }
  for (int64_t k = n - 1; k >= 0; --k)
    ghi[k] = (k == n - 1 || glo[k + 1] != glo[k]) ? (int32_t)(k + 1) : ghi[k + 1];
  return RTHX_OK;
}

// The polygons read so far: their triangles in input order (Tri3::id), the
// same as the BVH build sees them, and the scene's bounds.
struct Ingest {
  std::vector<Tri3> tris;
  std::vector<BuildTri> bt;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
};

// Reads one polygon -- `m` vertices at p -- as polygon `poly` of group
// `group`: checks it, grows the scene's bounds and appends its one or two
// triangles (a quad: v0 v1 v2, then v2 v3 v0).  A real polygon has the
// caller's `normal` and fills its emission record E, its frame oriented by
// that normal; a mirror (`what` = "mirror ", named in its errors) has neither.
// `nn` receives the unit normal.
int ingest_polygon(const double* p, int m, const double* normal, int32_t poly, int32_t group, const char* what, Ingest& in,
                   Emit3* E, V& nn, std::string& err) {
  auto bad = [&](const char* before, const char* after) {
    return refuse(err, RTHX_EINVAL, std::string(before) + what + after);
  };
  if (m != 3 && m != 4) return bad("", "polygon with n not in {3,4}");
  for (int i = 0; i < 3 * m; ++i)
    if (!std::isfinite(p[i])) return bad("non-finite ", "vertex");
  V v[4];
  for (int i = 0; i < 4; ++i) {
    const int j = i < m ? i : m - 1;
    v[i] = at(p + 3 * j);
    for (int d = 0; d < 3; ++d) {
      in.lo[d] = std::min(in.lo[d], p[3 * j + d]);
      in.hi[d] = std::max(in.hi[d], p[3 * j + d]);
    }
  }
  const V ng = cross(sub(v[1], v[0]), sub(v[2], v[0]));
  const double a1 = norm(ng) / 2;
  const double a2 = m == 4 ? norm(cross(sub(v[3], v[2]), sub(v[0], v[2]))) / 2 : 0.0;
  if (!(a1 > 0.0) || (m == 4 && !(a2 > 0.0))) return bad("degenerate ", "polygon (zero area)");
  nn = scale(ng, 1.0 / norm(ng));
  if (normal) {
    const V un = at(normal);
    if (!(std::isfinite(un.x) && std::isfinite(un.y) && std::isfinite(un.z)) || norm(un) == 0.0)
      return refuse(err, RTHX_EINVAL, "normal must be finite and non-zero");
    if (dot(nn, un) < 0.0) nn = scale(nn, -1.0);
  }
  if (m == 4) {  // planarity within 1e-9 of the polygon size
    const double size = std::max(norm(sub(v[2], v[0])), norm(sub(v[3], v[1])));
    if (std::fabs(dot(nn, sub(v[3], v[0]))) > 1e-9 * size) return bad("", "quad vertices are not coplanar");
  }
  if (E) {
    const V e01 = sub(v[1], v[0]);
    const V t1 = scale(e01, 1.0 / norm(e01));
    const V t2 = cross(nn, t1);
    for (int i = 0; i < 4; ++i) put(E->v[i], v[i]);
    put(E->n, nn);
    put(E->t1, t1);
    put(E->t2, t2);
    E->tri_frac = m == 4 ? a1 / (a1 + a2) : 1.0;
    E->nv = m;
    E->group = group;
  }
  const int corners[2][3] = {{0, 1, 2}, {2, 3, 0}};
  for (int h = 0; h < (m == 4 ? 2 : 1); ++h) {
    const V a = v[corners[h][0]], b = v[corners[h][1]], c = v[corners[h][2]];
    Tri3 T{};
    put(T.v0, a);
    put(T.e1, sub(b, a));
    put(T.e2, sub(c, a));
    T.poly = poly;
    T.id = (int32_t)in.tris.size();
    in.tris.push_back(T);
    BuildTri B{};
    for (int d = 0; d < 3; ++d) {
      const double x[3] = {d == 0 ? a.x : d == 1 ? a.y : a.z, d == 0 ? b.x : d == 1 ? b.y : b.z,
                           d == 0 ? c.x : d == 1 ? c.y : c.z};
      B.lo[d] = std::min({x[0], x[1], x[2]});
      B.hi[d] = std::max({x[0], x[1], x[2]});
      B.c[d] = (x[0] + x[1] + x[2]) / 3.0;
    }
    B.group = group;
    in.bt.push_back(B);
  }
  return RTHX_OK;
}

// A BVH that fits the walk's stack, laid out for the device: binned SAH, or
// median splits when the SAH tree is deeper than kBvhStack.
struct Tree {
  std::vector<Bvh2Node> nodes;
  std::vector<int> order;  // order[i]: the triangle of bt at device position i
  int depth = 0;
};
int build_bvh_within_stack(const std::vector<BuildTri>& bt, double pad, Tree& T, std::string& err) {
  T.order.resize(bt.size());
  T.nodes.reserve(bt.size());
  T.depth = build_bvh2(T.nodes, T.order, bt, pad, false);
  if (T.depth > kBvhStack) T.depth = build_bvh2(T.nodes, T.order, bt, pad, true);
  if (T.depth > kBvhStack) return refuse(err, RTHX_ERANGE, "BVH too deep for the traversal stack");
  layout_nodes(T.nodes);
  return RTHX_OK;
}

// Is the interior one convex set, seen from the sides its rays leave?
// Every interior vertex must lie on or behind every interior polygon's
// emitting plane (within tol: 1e-12 of the scene scale).  Then a ray leaving
// an interior polygon away from its edges meets no interior triangle:
// the points it reaches are beyond that plane, and every other interior
// triangle is behind it but for the edges and vertices it shares
// (DESIGN.md §7e).
bool interior_is_convex(const std::vector<Emit3>& P, const std::vector<char>& in_hull, const std::vector<V>& verts,
                        double tol) {
  for (size_t k = 0; k < P.size(); ++k) {
    if (in_hull[k]) continue;
    for (const V& q : verts)
      if (plane_dist(P[k], q) > tol) return false;
  }
  return true;
}

// Box hull: the hull cells' triangles, and the interior triangles' BVH in
// front of the whole scene's (the interior BVH's top is what the kernel
// caches in LDS; the whole scene's, from full_root on, is the fallback walk).
// B holds the whole scene's tree on entry.
int add_box_hull(const Ingest& in, HullBuild& hb, Scene3dBuild& B, std::string& err) {
  std::vector<int64_t> tri0(B.polys.size() + 1, 0);  // first triangle of each polygon
  for (size_t k = 0; k < B.polys.size(); ++k) tri0[k + 1] = tri0[k] + (B.polys[k].nv == 4 ? 2 : 1);
  for (int64_t c : hb.cell_poly)
    for (int h = 0; h < 2; ++h) B.hull_tris.push_back(in.tris[(size_t)(tri0[(size_t)c] + h)]);
  // the interior: every triangle of a polygon that is no hull cell
  std::vector<BuildTri> bt_in;
  std::vector<Tri3> tris_in;
  for (size_t t = 0; t < in.tris.size(); ++t)
    if (!hb.in_hull[(size_t)in.tris[t].poly]) {
      bt_in.push_back(in.bt[t]);
      tris_in.push_back(in.tris[t]);
    }
  Tree I;
  std::vector<Tri3> all_tris;
  if (!bt_in.empty()) {
    if (const int rc = build_bvh_within_stack(bt_in, kBoxPad * B.scale, I, err)) return rc;
    B.stack = std::max(B.stack, I.depth);
    for (int i : I.order) all_tris.push_back(tris_in[(size_t)i]);
    const std::vector<V> verts = unique_vertices(B.polys, [&](size_t k) { return !hb.in_hull[k]; });
    B.convex_interior = interior_is_convex(B.polys, hb.in_hull, verts, 1e-12 * B.scale);
    if (B.convex_interior)
      for (size_t k = 0; k < B.polys.size(); ++k)
        if (!hb.in_hull[k]) B.polys[k].convex = 1;
    // the interior's bounding ball: centre the vertices' mean, radius the
    // farthest vertex, padded by 1e-9 relative plus 1e-12 of the scene
    // (every interior triangle lies within it: convex combinations)
    V cen;
    double r;
    mean_and_reach(verts, cen, r);
    put(B.ball, cen);
    B.ball[3] = r * (1.0 + 1e-9) + 1e-12 * B.scale;
  }
  B.n_in_tris = (int64_t)all_tris.size();
  B.n_in_nodes = B.full_root = (int32_t)I.nodes.size();
  shift_bvh(B.nodes, B.full_root, (int32_t)B.n_in_tris);
  I.nodes.insert(I.nodes.end(), B.nodes.begin(), B.nodes.end());
  B.nodes.swap(I.nodes);
  all_tris.insert(all_tris.end(), B.tris.begin(), B.tris.end());
  B.tris.swap(all_tris);
  B.faces.swap(hb.faces);
  B.lines.swap(hb.lines);
  B.in_hull.swap(hb.in_hull);
  return RTHX_OK;
}

// The real polygons, in their groups: emission records and triangles.
int ingest_real(const double* xyz, const int32_t* nv, const double* normal, const int32_t* group, int64_t n, Ingest& in,
                Scene3dBuild& B, std::string& err) {
  std::vector<int32_t> glo, ghi;
  if (const int rc = group_runs(group, n, glo, ghi, err)) return rc;
  V nn;
  B.n_poly = n;
  B.polys.resize((size_t)n);
  for (int64_t k = 0; k < n; ++k) {
    Emit3& E = B.polys[(size_t)k];
    if (const int rc = ingest_polygon(xyz + 12 * k, nv[k], normal + 3 * k, (int32_t)k, group ? group[k] : (int32_t)k, "",
                                      in, &E, nn, err))
      return rc;
    E.glo = glo[(size_t)k];
    E.ghi = ghi[(size_t)k];
  }
  return RTHX_OK;
}

// Symmetry planes: two-sided, no emission frame and no row; their triangles
// follow the real ones (the highest ids: a tie on t at a seam goes to the
// real polygon), polygon n + m, each a group of its own above every real
// group id.
int ingest_mirrors(const double* mirror_xyz, const int32_t* mirror_nv, int64_t n_mirror, Ingest& in, Scene3dBuild& B,
                   std::string& err) {
  int64_t group0 = 0;
  for (const Emit3& E : B.polys) group0 = std::max<int64_t>(group0, (int64_t)E.group + 1);
  if (group0 + n_mirror >= (int64_t(1) << 31)) return refuse(err, RTHX_ERANGE, "group ids leave no room for the mirror groups");
  B.mirror_group0 = (int32_t)group0;
  B.n_mirror = n_mirror;
  const size_t n_real_tris = in.tris.size();
  V nn;
  for (int64_t k = 0; k < n_mirror; ++k) {
    if (const int rc = ingest_polygon(mirror_xyz + 12 * k, mirror_nv[k], nullptr, (int32_t)(B.n_poly + k),
                                      (int32_t)(group0 + k), "mirror ", in, nullptr, nn, err))
      return rc;
    B.mirror_n.insert(B.mirror_n.end(), {nn.x, nn.y, nn.z});
  }
  B.n_tri = (int64_t)in.tris.size();
  B.n_mirror_tris = (int64_t)(in.tris.size() - n_real_tris);
  return RTHX_OK;
}

// The scene's box and its scale: the largest |coordinate| or extent.
void set_bounds(const Ingest& in, Scene3dBuild& B) {
  for (int k = 0; k < 3; ++k) {
    B.box_lo[k] = in.lo[k];
    B.box_len[k] = (float)(in.hi[k] - in.lo[k]);
    B.scale = std::max({B.scale, std::fabs(in.lo[k]), std::fabs(in.hi[k]), in.hi[k] - in.lo[k]});
  }
  B.cvx_tpad = (float)(1e-9 * B.scale);
}

// The whole scene's BVH (without a box hull: the only one) and its
// triangles in the tree's order.  fp32 box padding: covers the rounding of
// the fp32 slab test for any ray that stays within the scene scale
// (DESIGN.md §7e).
int build_whole_bvh(const Ingest& in, Scene3dBuild& B, std::string& err) {
  if (2 * in.tris.size() >= (size_t(1) << (30 - kLeafBits))) return refuse(err, RTHX_ERANGE, "too many triangles");
  Tree W;
  if (const int rc = build_bvh_within_stack(in.bt, kBoxPad * B.scale, W, err)) return rc;
  B.stack = W.depth;
  B.nodes.swap(W.nodes);
  for (int i : W.order) B.tris.push_back(in.tris[(size_t)i]);
  B.n_in_nodes = (int32_t)B.nodes.size();
  B.n_in_tris = B.n_tri;
  return RTHX_OK;
}

}  // namespace

int build_scene3d(const double* xyz, const int32_t* nv, const double* normal, const int32_t* group, int64_t n,
                  const double* mirror_xyz, const int32_t* mirror_nv, int64_t n_mirror, const Scene3dOptions& opt,
                  Scene3dBuild& out, std::string& err) {
  out = Scene3dBuild{};
  if (n_mirror < 0) return refuse(err, RTHX_EINVAL, "mirror count must be >= 0");
  if (n_mirror > 0 && (!mirror_xyz || !mirror_nv)) return refuse(err, RTHX_EINVAL, "null mirror arrays with n_mirror > 0");
  // (behind mirrors one polygon is an enclosure: it sees its own images)
  if (!xyz || !nv || !normal || n < (n_mirror > 0 ? 1 : 2))
    return refuse(err, RTHX_EINVAL, "null argument or fewer than 2 polygons");
  if (n >= (int64_t(1) << 30) || n_mirror >= (int64_t(1) << 30) || n + n_mirror >= (int64_t(1) << 30))
    return refuse(err, RTHX_ERANGE, "too many polygons");
  Scene3dBuild B;
  Ingest in;
  if (const int rc = ingest_real(xyz, nv, normal, group, n, in, B, err)) return rc;
  if (const int rc = ingest_mirrors(mirror_xyz, mirror_nv, n_mirror, in, B, err)) return rc;
  set_bounds(in, B);
  if (const int rc = build_whole_bvh(in, B, err)) return rc;
  // The fast paths.  (A scene with a mirror is traced by the plain walk: no
  // box hull, no exit-direction map -- DESIGN.md §7k.)
  HullBuild hb;
  B.hull = n_mirror == 0 && group && !opt.no_hull && detect_box_hull(B.polys, n, in.lo, in.hi, hb);
  B.margin = (float)hb.margin;  // (the kernel reads it only with a hull)
  if (B.hull)
    if (const int rc = add_box_hull(in, hb, B, err)) return rc;
  // Convex enclosure seen from inside (no box hull): the cube map of exit
  // directions (rthx_scene3d.h CvxPlane).  Not with a group that is not
  // coplanar (within the vertex test's 1e-12 of the scene scale): the map
  // would count rays that leave through their emitter's group, which the
  // walk loses.
  B.cvx = n_mirror == 0 && !B.hull && !opt.no_cvx && (!group || groups_coplanar(B.polys, 1e-12 * B.scale)) &&
          detect_convex_enclosure(B.polys, B.tris, B.scale, opt, B);
  out = std::move(B);
  return RTHX_OK;
}

}  // namespace rthx
