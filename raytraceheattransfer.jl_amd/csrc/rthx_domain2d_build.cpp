// rthx_domain2d_build.cpp -- the 2D tracer's host-side domain build
// (rthx_domain2d_build.h build_domain2d; the C ABI around it is rthx_api.cpp
// rthx_domain_create): the descriptor's checks, the derived per-polygon
// arrays, the point-location grids, the lookup tables, and the choice and LDS
// layout of the fast paths (CLDS, MLAT, LAT).  Plain C++, built without
// contraction, so trifrac rounds like the reference's expression.
#include "rthx_domain2d_build.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

namespace rthx {

static double double_of_bits(uint64_t b) {
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

void fill_tables(double* t) {
  for (int j = 0; j < kCosTable; ++j) {
    const long double a = 2.0L * 3.141592653589793238462643383279502884L * j / kCosTable;
    t[2 * j] = (double)cosl(a);
    t[2 * j + 1] = (double)sinl(a);
  }
  double* L = t + kLogTableOffset;
  for (int i = 0; i < kLogTable; ++i) {
    const double z0 = double_of_bits(kLogOff + ((uint64_t)i << 45));
    const double z1 = double_of_bits(kLogOff + ((uint64_t)(i + 1) << 45));
    const double invc = (double)(2.0L / ((long double)z0 + (long double)z1));
    const long double T = logl((long double)invc);
    const double hi = (double)T;
    L[4 * i] = invc;
    L[4 * i + 1] = hi;
    L[4 * i + 2] = (double)(T - (long double)hi);
    L[4 * i + 3] = 0.0;
  }
}

namespace {

int refuse(std::string& err, int code, const std::string& msg) {
  err = msg;
  return code;
}

int check_grid(const rthx_grid_desc& g, int32_t count, const char* what, std::string& err) {
  if (g.nx < 1 || g.ny < 1 || !g.cell_start || !(std::isfinite(g.inv_cell_size)) || g.inv_cell_size <= 0)
    return refuse(err, RTHX_EINVAL, std::string("invalid grid: ") + what);
  int64_t cells = (int64_t)g.nx * g.ny;
  if (cells > (1ll << 30)) return refuse(err, RTHX_ERANGE, std::string("grid too large: ") + what);
  if (g.cell_start[0] != 0) return refuse(err, RTHX_EINVAL, std::string("grid cell_start[0] != 0: ") + what);
  for (int64_t c = 0; c < cells; ++c)
    if (g.cell_start[c + 1] < g.cell_start[c])
      return refuse(err, RTHX_EINVAL, std::string("grid cell_start not monotone: ") + what);
  int64_t n_items = g.cell_start[cells];
  if (n_items > 0 && !g.cell_items) return refuse(err, RTHX_EINVAL, std::string("null grid items: ") + what);
  for (int64_t k = 0; k < n_items; ++k)
    if (g.cell_items[k] < 0 || g.cell_items[k] >= count)
      return refuse(err, RTHX_EINVAL, std::string("grid item out of range: ") + what);
  return RTHX_OK;
}

// The descriptor's checks; s_face / s_wall (the inverse of fine_surface) fall
// out of the check that every surface index is used once.
int validate_desc(const rthx_domain_desc& s, Domain2dBuild& B, std::string& err) {
  if (s.n_coarse < 1 || s.n_fine < 1 || s.n_surfaces < 0 || s.n_bins < 1)
    return refuse(err, RTHX_EINVAL, "empty or negative domain sizes");
  if ((int64_t)s.n_surfaces + s.n_fine >= (1ll << 31)) return refuse(err, RTHX_ERANGE, "too many elements");
  if (!s.coarse_nv || !s.coarse_xy || !s.coarse_normal || !s.coarse_solid || !s.coarse_bbox || !s.fine_offset ||
      !s.fine_nv || !s.fine_xy || !s.fine_normal || !s.fine_mid || !s.fine_volume || !s.fine_bbox ||
      !s.fine_surface || !s.fine_grid || !s.beta || !s.uniform_beta)
    return refuse(err, RTHX_EINVAL, "null descriptor array");
  for (int c = 0; c < s.n_coarse; ++c)
    if (s.coarse_nv[c] != 3 && s.coarse_nv[c] != 4) return refuse(err, RTHX_EINVAL, "coarse polygon with n not in {3,4}");
  if (s.fine_offset[0] != 0 || s.fine_offset[s.n_coarse] != s.n_fine)
    return refuse(err, RTHX_EINVAL, "fine_offset must run from 0 to n_fine");
  for (int c = 0; c < s.n_coarse; ++c)
    if (s.fine_offset[c + 1] <= s.fine_offset[c]) return refuse(err, RTHX_EINVAL, "coarse polygon without fine polygons");
  for (int f = 0; f < s.n_fine; ++f)
    if (s.fine_nv[f] != 3 && s.fine_nv[f] != 4) return refuse(err, RTHX_EINVAL, "fine polygon with n not in {3,4}");
  B.s_face.assign(s.n_surfaces, -1);
  B.s_wall.assign(s.n_surfaces, -1);
  for (int f = 0; f < s.n_fine; ++f)
    for (int w = 0; w < 4; ++w) {
      int32_t sidx = s.fine_surface[4 * (size_t)f + w];
      if (sidx < -1 || sidx >= s.n_surfaces || (sidx >= 0 && w >= s.fine_nv[f]))
        return refuse(err, RTHX_EINVAL, "fine_surface index out of range");
      if (sidx >= 0) {
        if (B.s_face[sidx] != -1) return refuse(err, RTHX_EINVAL, "surface index used twice");
        B.s_face[sidx] = f;
        B.s_wall[sidx] = w;
      }
    }
  for (int i = 0; i < s.n_surfaces; ++i)
    if (B.s_face[i] < 0) return refuse(err, RTHX_EINVAL, "surface index without a solid fine wall");
  for (int64_t k = 0; k < (int64_t)s.n_bins * s.n_fine; ++k)
    if (!std::isfinite(s.beta[k]) || s.beta[k] < 0) return refuse(err, RTHX_EINVAL, "non-finite or negative extinction");
  for (int64_t k = 0; k < 8ll * s.n_fine; ++k)
    if (!std::isfinite(s.fine_xy[k]) || !std::isfinite(s.fine_normal[k]))
      return refuse(err, RTHX_EINVAL, "non-finite fine geometry");
  if (const int rc = check_grid(s.coarse_grid, s.n_coarse, "coarse grid", err)) return rc;
  for (int c = 0; c < s.n_coarse; ++c)
    if (const int rc = check_grid(s.fine_grid[c], s.fine_offset[c + 1] - s.fine_offset[c], "fine grid", err)) return rc;
  return RTHX_OK;
}

// Polygon records padded to 4 slots (rthx_domain2d.h DevPoly): a triangle
// repeats vertex 2 and has a zero normal in slot 3.
std::vector<DevPoly> pad_polygons(const int32_t* nv, const double* xy, const double* nrm, size_t n) {
  std::vector<DevPoly> out(n);
  for (size_t p = 0; p < n; ++p) {
    DevPoly& q = out[p];
    for (int i = 0; i < 4; ++i) {
      const int v = i < nv[p] ? i : nv[p] - 1;
      q.x[i] = xy[8 * p + 2 * v];
      q.y[i] = xy[8 * p + 2 * v + 1];
      q.nx[i] = i < nv[p] ? nrm[8 * p + 2 * i] : 0.0;
      q.ny[i] = i < nv[p] ? nrm[8 * p + 2 * i + 1] : 0.0;
    }
  }
  return out;
}

// AXIS kernels (rthx_device.h dist_to_rect): v0 the min corner, CCW, wall
// normals exactly (0,-1), (1,0), (0,1), (-1,0) (calculateInwardNormal's
// orientation).
bool canonical_rect(int32_t nv, const DevPoly& q) {
  return nv == 4 && q.x[0] < q.x[1] && q.y[0] < q.y[2] && q.x[1] == q.x[2] && q.x[3] == q.x[0] &&
         q.y[1] == q.y[0] && q.y[3] == q.y[2] && q.nx[0] == 0.0 && q.ny[0] == -1.0 && q.nx[1] == 1.0 &&
         q.ny[1] == 0.0 && q.nx[2] == 0.0 && q.ny[2] == 1.0 && q.nx[3] == -1.0 && q.ny[3] == 0.0;
}

// What the kernels are chosen by and the per-polygon arrays derived from the
// descriptor's (needs cpoly / fpoly).
void classify(const rthx_domain_desc& s, Domain2dBuild& B) {
  const size_t nc = s.n_coarse, nf = s.n_fine;
  B.csolid.assign(nc, 0u);
  for (size_t c = 0; c < nc; ++c)
    for (int w = 0; w < 4; ++w)
      if (s.coarse_solid[4 * c + w]) B.csolid[c] |= 1u << w;
  // area(ABC)/V of every quad (emitVolumeRay2D.jl:7), evaluated exactly as the
  // reference's expression (no contraction: -ffp-contract=off)
  B.trifrac.assign(nf, 0.0);
  for (size_t f = 0; f < nf; ++f) {
    if (s.fine_nv[f] != 4) continue;
    const double* v = s.fine_xy + 8 * f;
    B.trifrac[f] = 0.5 * (v[0] * (v[3] - v[5]) + v[2] * (v[5] - v[1]) + v[4] * (v[1] - v[3])) / s.fine_volume[f];
  }
  // one convex coarse polygon -> SINGLE kernels (a ray that leaves it is lost)
  if (nc == 1) {
    const double* v = s.coarse_xy;
    int n = s.coarse_nv[0], pos = 0, neg = 0;
    for (int i = 0; i < n; ++i) {
      int j = (i + 1) % n, k = (i + 2) % n;
      double cr = (v[2 * j] - v[2 * i]) * (v[2 * k + 1] - v[2 * j + 1]) - (v[2 * j + 1] - v[2 * i + 1]) * (v[2 * k] - v[2 * j]);
      pos += cr > 0;
      neg += cr < 0;
    }
    B.single_convex = (pos == 0 || neg == 0);
  }
  B.axis_rect = true;
  for (size_t c = 0; c < nc && B.axis_rect; ++c) B.axis_rect = canonical_rect(s.coarse_nv[c], B.cpoly[c]);
  for (size_t f = 0; f < nf && B.axis_rect; ++f) B.axis_rect = canonical_rect(s.fine_nv[f], B.fpoly[f]);
  B.fcoarse.resize(nf);
  for (size_t c = 0; c < nc; ++c)
    for (int f = s.fine_offset[c]; f < s.fine_offset[c + 1]; ++f) B.fcoarse[f] = (int32_t)c;
}

// Device point-location grids (rthx_grid.cpp): the coarse one first, then one
// per coarse polygon.  Cells per mean polygon extent (per axis): at 2 a cell
// holds at most one vertex of a regular mesh.
constexpr double kGridCellsPerPolygon = 2.0;

DevGrid add_grid(const int32_t* nv, const double* xy, int first, int count, Domain2dBuild& B) {
  DevGrid g{};
  g.cell_base = (int32_t)B.gcells.size();
  GridBuild b = build_cell_grid(nv, xy, first, count, kGridCellsPerPolygon, B.gcells, B.glists, B.gitems);
  g.ox = b.ox;
  g.oy = b.oy;
  g.inv_x = b.inv_x;
  g.inv_y = b.inv_y;
  g.nx = b.nx;
  g.ny = b.ny;
  return g;
}

int build_grids(const rthx_domain_desc& s, Domain2dBuild& B, std::string& err) {
  B.c_grid = add_grid(s.coarse_nv, s.coarse_xy, 0, s.n_coarse, B);
  B.fgrids.resize(s.n_coarse);
  for (int c = 0; c < s.n_coarse; ++c)
    B.fgrids[c] = add_grid(s.fine_nv, s.fine_xy, s.fine_offset[c], s.fine_offset[c + 1] - s.fine_offset[c], B);
  if (B.gcells.size() >= (1ull << 30) || B.gitems.size() >= (1ull << 31)) return refuse(err, RTHX_ERANGE, "grids too large");
  if (B.gitems.empty()) B.gitems.push_back(0);
  return RTHX_OK;
}

// (cos, sin)(2 pi j / 256) for the emission azimuth (cos_2pi_u32) and the
// free-path log table (neg_log_tab).  One copy per bin, each followed by the
// bin's 1 / beta_uniform (the kernels' kTabInvBeta slot; +inf when
// beta_uniform <= 0), so that a kernel reading the tables from global memory
// finds a whole kLdsTableDoubles block at bin * kLdsTableDoubles.
void build_tables(const rthx_domain_desc& s, Domain2dBuild& B) {
  B.beta_first.resize(s.n_bins);
  B.tables.resize((size_t)s.n_bins * kLdsTableDoubles);
  for (int b = 0; b < s.n_bins; ++b) {
    B.beta_first[b] = s.beta[(size_t)b * s.n_fine];
    double* t = B.tables.data() + (size_t)b * kLdsTableDoubles;
    fill_tables(t);
    t[kTabInvBeta] = B.beta_first[b] > 0 ? 1.0 / B.beta_first[b] : HUGE_VAL;
  }
}

// Per bin the beta every fine polygon of a coarse polygon shares (-1 when
// they differ).
void coarse_beta(const rthx_domain_desc& s, Domain2dBuild& B) {
  const size_t nc = s.n_coarse, nf = s.n_fine;
  if (nc < 2) return;
  B.c_beta.assign((size_t)s.n_bins * nc, -1.0);
  for (int bn = 0; bn < s.n_bins; ++bn)
    for (size_t c = 0; c < nc; ++c) {
      const int f0 = s.fine_offset[c], f1 = s.fine_offset[c + 1];
      const double* bb = s.beta + (size_t)bn * nf;
      bool same = true;
      for (int f = f0 + 1; f < f1 && same; ++f) same = bb[f] == bb[f0];
      if (same) B.c_beta[(size_t)bn * nc + c] = bb[f0];
    }
}

size_t a16(size_t b) { return (b + 15) & ~(size_t)15; }

// An LDS block under construction: every section starts at the next multiple
// of 16 bytes, the gaps are zero.  Without `fill` only the offsets are laid
// out (a block that may turn out too large for LDS is sized first).
struct Blob {
  bool fill;
  size_t size = 0;
  std::vector<unsigned char> bytes;
  // Appends n records; returns the section's offset.
  template <class T>
  int32_t add(const T* src, size_t n) {
    const size_t off = size;
    size = a16(off + n * sizeof(T));
    if (fill) {
      bytes.resize(size, 0);
      if (n) std::memcpy(bytes.data() + off, src, n * sizeof(T));
    }
    return (int32_t)off;
  }
  template <class T>
  int32_t add(const std::vector<T>& v) {
    return add(v.data(), v.size());
  }
};

// Coarse mesh as the CLDS kernels stage it in LDS (rthx_domain2d.h
// CoarseLayout).  The offsets are filled in any case; the blob is built when
// there is more than one coarse polygon and the block fits.
void layout_coarse_lds(const rthx_domain_desc& s, Domain2dBuild& B) {
  const size_t nc = s.n_coarse;
  CoarseLayout L{};
  auto lay = [&](Blob& blob) {
    blob.add(B.cpoly);
    L.off_fgrid = blob.add(B.fgrids);
    L.off_bbox = blob.add(s.coarse_bbox, 4 * nc);
    L.off_first = blob.add(s.fine_offset, nc + 1);
    L.off_solid = blob.add(B.csolid);
    L.off_cells = blob.add(B.gcells.data(), (size_t)B.c_grid.nx * B.c_grid.ny);  // (the coarse grid's cells come first)
    L.off_beta = L.blob_bytes = (int32_t)blob.size;
  };
  Blob sizes{false};
  lay(sizes);
  const size_t total = a16(sizes.size + nc * sizeof(double));
  if (nc >= 2 && total <= kMaxCoarseLdsBytes) {
    Blob blob{true};
    lay(blob);
    L.bytes = (int32_t)total;
    B.c_blob = std::move(blob.bytes);
  }
  B.cl = L;
}

// The sorted distinct edge coordinates of n canonical rectangles along x or y.
std::vector<double> edge_lines(const std::vector<DevPoly>& q, bool xdir) {
  std::vector<double> v;
  v.reserve(2 * q.size());
  for (const DevPoly& p : q) {
    v.push_back(xdir ? p.x[0] : p.y[0]);
    v.push_back(xdir ? p.x[1] : p.y[2]);
  }
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// The index of x in the sorted v, -1 when it is not there.
int64_t index_of(const std::vector<double>& v, double x) {
  const auto it = std::lower_bound(v.begin(), v.end(), x);
  return (it != v.end() && *it == x) ? (int64_t)(it - v.begin()) : -1;
}

// Whether q is exactly box (i, j) of the lattice (i, j in range).
bool is_box(const DevPoly& q, const std::vector<double>& xs, int64_t i, const std::vector<double>& ys, int64_t j) {
  return q.x[0] == xs[i] && q.x[1] == xs[i + 1] && q.y[0] == ys[j] && q.y[2] == ys[j + 1];
}

// Multi-polygon lattice (rthx_domain2d.h MLatLayout; MLAT kernels): the
// coarse rectangles are the boxes of a coarse lattice, and the fine
// rectangles of each are, x fastest, the boxes of one global fine lattice
// inside it.
void detect_multi_lattice(const rthx_domain_desc& s, Domain2dBuild& B) {
  const size_t nc = s.n_coarse;
  const std::vector<double> xs = edge_lines(B.fpoly, true), ys = edge_lines(B.fpoly, false);
  const std::vector<double> cxs = edge_lines(B.cpoly, true), cys = edge_lines(B.cpoly, false);
  const int64_t nx = (int64_t)xs.size() - 1, ny = (int64_t)ys.size() - 1;
  const int64_t ncx = (int64_t)cxs.size() - 1, ncy = (int64_t)cys.size() - 1;
  if (!(ncx >= 1 && ncy >= 1 && ncx * ncy == (int64_t)nc && nx <= 65536 && ny <= 65536)) return;
  std::vector<int32_t> cmap(nc, -1);
  std::vector<MCoarse> info(nc);
  for (size_t c = 0; c < nc; ++c) {
    const DevPoly& q = B.cpoly[c];
    const int64_t ci = index_of(cxs, q.x[0]), cj = index_of(cys, q.y[0]);
    if (!(ci >= 0 && cj >= 0 && ci < ncx && cj < ncy && is_box(q, cxs, ci, cys, cj) && cmap[cj * ncx + ci] < 0)) return;
    cmap[cj * ncx + ci] = (int32_t)c;
    const int64_t i0 = index_of(xs, q.x[0]), i1 = index_of(xs, q.x[1]);
    const int64_t j0 = index_of(ys, q.y[0]), j1 = index_of(ys, q.y[2]);
    const int f0 = s.fine_offset[c], f1 = s.fine_offset[c + 1];
    if (!(i0 >= 0 && i1 > i0 && j0 >= 0 && j1 > j0 && (i1 - i0) * (j1 - j0) == f1 - f0)) return;
    for (int f = f0; f < f1; ++f)
      if (!is_box(B.fpoly[f], xs, i0 + (f - f0) % (i1 - i0), ys, j0 + (f - f0) / (i1 - i0))) return;
    info[c] = MCoarse{f0, (int32_t)i0, (int32_t)j0, (int32_t)(i1 - i0), (int32_t)(j1 - j0), (int32_t)ci,
                      (int32_t)cj, B.csolid[c]};
  }
  std::vector<uint32_t> bsolid(nc);
  for (size_t bx = 0; bx < nc; ++bx) bsolid[bx] = B.csolid[cmap[bx]];
  MLatLayout G{};
  G.nx = (int32_t)nx;
  G.ny = (int32_t)ny;
  G.ncx = (int32_t)ncx;
  G.ncy = (int32_t)ncy;
  auto lay = [&](Blob& blob) {
    blob.add(xs);
    G.off_ys = blob.add(ys);
    G.off_cxs = blob.add(cxs);
    G.off_cys = blob.add(cys);
    G.off_cmap = blob.add(cmap);
    G.off_cinfo = blob.add(info);
    G.off_bsolid = blob.add(bsolid);
    G.off_beta = G.blob_bytes = (int32_t)blob.size;
  };
  Blob sizes{false};
  lay(sizes);
  size_t total = a16(sizes.size + 8 * nc);  // (the betas: staged per bin)
  if (ncx == 1) {  // layer records (walk_layers), staged per bin
    G.off_lay = (int32_t)total;
    total = a16(total + sizeof(LayerRec) * (size_t)(ncy + 2));  // (sentinels below and above)
  }
  if (total > kMaxCoarseLdsBytes) return;
  Blob blob{true};
  lay(blob);
  G.bytes = (int32_t)total;
  G.inv_x = (double)nx / (xs[nx] - xs[0]);
  G.inv_y = (double)ny / (ys[ny] - ys[0]);
  G.inv_cx = (double)ncx / (cxs[ncx] - cxs[0]);
  G.inv_cy = (double)ncy / (cys[ncy] - cys[0]);
  B.ml = G;
  B.ml_blob = std::move(blob.bytes);
  // c_beta by box, and per bin whether some box has no single beta
  B.ml_bbeta.resize((size_t)s.n_bins * nc);
  B.ml_mixed.assign((size_t)s.n_bins, 0);
  for (int bn = 0; bn < s.n_bins; ++bn)
    for (size_t bx = 0; bx < nc; ++bx) {
      const double beta = B.c_beta[(size_t)bn * nc + cmap[bx]];
      B.ml_bbeta[(size_t)bn * nc + bx] = beta;
      B.ml_mixed[bn] |= beta < 0.0 ? 1 : 0;
    }
}

// Lattice of a single axis-aligned coarse rectangle (rthx_domain2d.h
// LatticeLayout; LAT kernels): the fine cells must be exactly the nx x ny
// boxes between the sorted distinct x and y coordinates, and only boundary
// fine walls may be solid.
void detect_single_lattice(const rthx_domain_desc& s, const Domain2dOptions& opt, Domain2dBuild& B) {
  const size_t nf = s.n_fine;
  const std::vector<double> xs = edge_lines(B.fpoly, true), ys = edge_lines(B.fpoly, false);
  const int64_t nx = (int64_t)xs.size() - 1, ny = (int64_t)ys.size() - 1;
  if (!(nx >= 1 && ny >= 1 && nx * ny == (int64_t)nf && nx <= kLatMaxDim && ny <= kLatMaxDim)) return;  // (lat_cell: 24-bit products)
  std::vector<int32_t> map(nf, -1);
  bool identity = true;
  for (size_t f = 0; f < nf; ++f) {
    const int64_t ix = index_of(xs, B.fpoly[f].x[0]), iy = index_of(ys, B.fpoly[f].y[0]);
    if (!(ix >= 0 && iy >= 0 && ix < nx && iy < ny && is_box(B.fpoly[f], xs, ix, ys, iy) && map[iy * nx + ix] < 0)) return;
    map[iy * nx + ix] = (int32_t)f;
    identity = identity && (int64_t)f == iy * nx + ix;
    // interior fine walls must be open (boundary walls: w 0 bottom, 1 right, 2 top, 3 left)
    const bool bnd[4] = {iy == 0, ix == nx - 1, iy == ny - 1, ix == 0};
    for (int w = 0; w < 4; ++w)
      if (!bnd[w] && s.fine_surface[4 * f + w] >= 0) return;
  }
  LatticeLayout L{};
  L.nx = (int32_t)nx;
  L.ny = (int32_t)ny;
  L.identity = identity ? 1 : 0;
  Blob blob{true};
  blob.add(xs);
  L.off_ys = blob.add(ys);
  L.bytes = (int32_t)blob.size;
  L.inv_x = (double)nx / (xs[nx] - xs[0]);
  L.inv_y = (double)ny / (ys[ny] - ys[0]);
  if (std::isfinite(opt.lat_guess_scale) && opt.lat_guess_scale > 0.0) {
    L.inv_x *= opt.lat_guess_scale;
    L.inv_y *= opt.lat_guess_scale;
  }
  B.lat = L;
  B.lat_blob = std::move(blob.bytes);
  if (!identity) B.lat_map = std::move(map);
}

}  // namespace

int build_domain2d(const rthx_domain_desc& s, const Domain2dOptions& opt, Domain2dBuild& B, std::string& err) {
  B = Domain2dBuild{};
  err.clear();
  if (const int rc = validate_desc(s, B, err)) return rc;
  // (the grids first, as rthx_domain_create always had it: the cell records grow by doubling, and the polygon
  // records then fit the room the last growth leaves in the heap instead of lying under it)
  if (const int rc = build_grids(s, B, err)) return rc;
  B.cpoly = pad_polygons(s.coarse_nv, s.coarse_xy, s.coarse_normal, s.n_coarse);
  B.fpoly = pad_polygons(s.fine_nv, s.fine_xy, s.fine_normal, s.n_fine);
  classify(s, B);
  build_tables(s, B);
  coarse_beta(s, B);
  layout_coarse_lds(s, B);
  if (!B.single_convex && B.axis_rect && s.n_coarse >= 2 && !opt.no_mlat) detect_multi_lattice(s, B);
  if (B.single_convex && B.axis_rect && !opt.no_lat) detect_single_lattice(s, opt, B);
  return RTHX_OK;
}

int mirror_masks(const std::vector<int32_t>& c_nv, const std::vector<double>& c_xy,
                 const std::vector<uint32_t>& c_solid, const uint8_t* mirror, std::vector<uint32_t>& mask, int64_t& n,
                 std::string& err) {
  const size_t nc = c_nv.size();
  mask.assign(nc, 0u);
  n = 0;
  for (size_t c = 0; mirror && c < nc; ++c)
    for (int w = 0; w < 4; ++w) {
      if (!mirror[4 * c + w]) continue;
      if (w >= c_nv[c]) return refuse(err, RTHX_EINVAL, "mirror flag on a wall the coarse polygon does not have");
      if ((c_solid[c] >> w) & 1u) return refuse(err, RTHX_EINVAL, "mirror flag on a solid wall");
      mask[c] |= 1u << w;
      ++n;
    }
  if (n > 0 && nc > 1) {  // the neighbours' walls
    typedef std::array<double, 4> Key;  // the wall's end points, the smaller first
    auto key_of = [&](size_t c, int w) {
      const double* v = c_xy.data() + 8 * c;
      const int w2 = (w + 1) % c_nv[c];
      const std::pair<double, double> a{v[2 * w], v[2 * w + 1]}, b{v[2 * w2], v[2 * w2 + 1]};
      return a < b ? Key{a.first, a.second, b.first, b.second} : Key{b.first, b.second, a.first, a.second};
    };
    std::map<Key, std::vector<std::pair<size_t, int>>> walls;
    for (size_t c = 0; c < nc; ++c)
      for (int w = 0; w < c_nv[c]; ++w) walls[key_of(c, w)].push_back({c, w});
    const std::vector<uint32_t> flagged = mask;
    for (size_t c = 0; c < nc; ++c)
      for (int w = 0; w < c_nv[c]; ++w)
        if ((flagged[c] >> w) & 1u)
          for (const auto& o : walls[key_of(c, w)])
            if (!((c_solid[o.first] >> o.second) & 1u)) mask[o.first] |= 1u << o.second;
  }
  return RTHX_OK;
}

}  // namespace rthx
