// Stand-alone check of the 2D tracer's host-side domain build
// (csrc/rthx_domain2d_build.h build_domain2d, mirror_masks), compiled
// together with csrc/rthx_domain2d_build.cpp and csrc/rthx_grid.cpp under
// -fsanitize=address,undefined by tests/test_domain2d_build_host.py and run
// as a program.
//
// Every tracer fast path (LAT, MLAT, CLDS, AXIS, SINGLE) is chosen by what
// this build decides, and the kernels read its blobs by the layouts' offsets.
// Each is checked here by brute force, on domains generated in this file, each
// the smallest that reaches its branch.  Every refusal of the descriptor is
// provoked but "grids too large" (2^30 cells).  For every domain a 64-bit
// FNV-1a hash over the named fields of the result is printed; the pytest
// compares it with tests/golden/domain2d_build.json.  The lookup tables'
// values depend on the machine's libm, so they are pinned by their
// properties, not by the hash.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_domain2d_build.h"

using namespace rthx;

static int fails = 0;
static const char* current = "";
#define EXPECT(cond, ...)                              \
  do {                                                 \
    if (!(cond)) {                                     \
      if (fails < 30) {                                \
        std::printf("FAIL [%s] %s: ", current, #cond); \
        std::printf(__VA_ARGS__);                      \
        std::printf("\n");                             \
      }                                                \
      ++fails;                                         \
    }                                                  \
  } while (0)

// ---------------------------------------------------------------- domains

struct Poly {
  int n = 0;
  double x[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
  bool solid[4] = {false, false, false, false};
};

static Poly rect(double x0, double x1, double y0, double y1, bool s0, bool s1, bool s2, bool s3) {
  Poly p;
  p.n = 4;
  const double xs[4] = {x0, x1, x1, x0}, ys[4] = {y0, y0, y1, y1};
  const bool s[4] = {s0, s1, s2, s3};
  for (int i = 0; i < 4; ++i) p.x[i] = xs[i], p.y[i] = ys[i], p.solid[i] = s[i];
  return p;
}
static Poly tri(double x0, double y0, double x1, double y1, double x2, double y2, bool s0, bool s1, bool s2) {
  Poly p;
  p.n = 3;
  const double xs[3] = {x0, x1, x2}, ys[3] = {y0, y1, y2};
  const bool s[3] = {s0, s1, s2};
  for (int i = 0; i < 3; ++i) p.x[i] = xs[i], p.y[i] = ys[i], p.solid[i] = s[i];
  return p;
}

// A domain as the caller flattens it (include/rthx.h rthx_domain_desc).  The
// descriptor's own grids are only validated by the build (the device grids
// are built from the polygons), so each is the one-cell grid of its set.
struct Dom {
  std::string name;
  int n_bins = 1;
  std::vector<Poly> coarse;
  std::vector<std::vector<Poly>> fine;  // per coarse polygon
  std::vector<double> beta;             // [n_bins][n_fine]; empty: 0.5 everywhere
  Domain2dOptions opt;
  // flattened
  std::vector<int32_t> c_nv, f_off, f_nv, f_surf;
  std::vector<double> c_xy, c_nrm, c_bbox, f_xy, f_nrm, f_mid, f_vol, f_bbox, ubeta;
  std::vector<uint8_t> c_solid;
  std::vector<std::vector<int32_t>> g_start, g_items;  // [0] coarse, [1 + c] fine
  std::vector<rthx_grid_desc> fgrid;
  rthx_domain_desc d{};

  static void put(const Poly& p, std::vector<int32_t>& nv, std::vector<double>& xy, std::vector<double>& nrm,
                  std::vector<double>& bbox) {
    nv.push_back(p.n);
    double lo[2] = {p.x[0], p.y[0]}, hi[2] = {p.x[0], p.y[0]};
    for (int i = 0; i < 4; ++i) {
      xy.push_back(i < p.n ? p.x[i] : 0.0);
      xy.push_back(i < p.n ? p.y[i] : 0.0);
      if (i < p.n) {
        const int j = (i + 1) % p.n;
        const double dx = p.x[j] - p.x[i], dy = p.y[j] - p.y[i], len = std::sqrt(dx * dx + dy * dy);
        nrm.push_back(dy / len + 0.0);  // (+ 0.0: no negative zeros)
        nrm.push_back(-dx / len + 0.0);
        lo[0] = std::min(lo[0], p.x[i]), hi[0] = std::max(hi[0], p.x[i]);
        lo[1] = std::min(lo[1], p.y[i]), hi[1] = std::max(hi[1], p.y[i]);
      } else {
        nrm.push_back(0.0);
        nrm.push_back(0.0);
      }
    }
    bbox.insert(bbox.end(), {lo[0], hi[0], lo[1], hi[1]});
  }
  rthx_grid_desc one_cell(size_t k, int32_t count) {
    g_start[k] = {0, count};
    g_items[k].resize(count);
    for (int32_t i = 0; i < count; ++i) g_items[k][i] = i;
    return rthx_grid_desc{0.0, 0.0, 1.0, 1, 1, g_start[k].data(), g_items[k].data()};
  }
  void flatten() {
    const size_t nc = coarse.size();
    g_start.assign(nc + 1, {});
    g_items.assign(nc + 1, {});
    fgrid.resize(nc);
    f_off.assign(1, 0);
    int32_t n_surf = 0;
    for (size_t c = 0; c < nc; ++c) {
      put(coarse[c], c_nv, c_xy, c_nrm, c_bbox);
      for (int w = 0; w < 4; ++w) c_solid.push_back(coarse[c].solid[w] ? 1 : 0);
      for (const Poly& p : fine[c]) {
        put(p, f_nv, f_xy, f_nrm, f_bbox);
        double mx = 0, my = 0, a2 = 0;
        for (int i = 0; i < p.n; ++i) {
          const int j = (i + 1) % p.n;
          mx += p.x[i], my += p.y[i], a2 += p.x[i] * p.y[j] - p.x[j] * p.y[i];
        }
        f_mid.insert(f_mid.end(), {mx / p.n, my / p.n});
        f_vol.push_back(0.5 * a2);
        for (int w = 0; w < 4; ++w) f_surf.push_back(w < p.n && p.solid[w] ? n_surf++ : -1);
      }
      f_off.push_back((int32_t)f_nv.size());
      fgrid[c] = one_cell(1 + c, (int32_t)fine[c].size());
    }
    const size_t nf = f_nv.size();
    if (beta.empty()) beta.assign((size_t)n_bins * nf, 0.5);
    ubeta.assign(n_bins, -1.0);
    d = rthx_domain_desc{};
    d.abi_version = RTHX_ABI_VERSION;
    d.n_coarse = (int32_t)nc, d.n_fine = (int32_t)nf, d.n_surfaces = n_surf, d.n_bins = n_bins;
    d.coarse_nv = c_nv.data(), d.coarse_xy = c_xy.data(), d.coarse_normal = c_nrm.data();
    d.coarse_solid = c_solid.data(), d.coarse_bbox = c_bbox.data();
    d.coarse_grid = one_cell(0, (int32_t)nc);
    d.fine_offset = f_off.data(), d.fine_nv = f_nv.data(), d.fine_xy = f_xy.data(), d.fine_normal = f_nrm.data();
    d.fine_mid = f_mid.data(), d.fine_volume = f_vol.data(), d.fine_bbox = f_bbox.data();
    d.fine_surface = f_surf.data(), d.fine_grid = fgrid.data();
    d.beta = beta.data(), d.uniform_beta = ubeta.data();
  }
};

static std::vector<double> edges(double a, double b, int n) {
  std::vector<double> e(n + 1);
  for (int i = 0; i <= n; ++i) e[i] = a + (b - a) * i / n;
  e[n] = b;
  return e;
}

// The fine rectangles of the coarse rectangle `c` between the given edges, x
// fastest; fine walls on c's boundary are solid where c's are.
static std::vector<Poly> rect_cells(const Poly& c, const std::vector<double>& xs, const std::vector<double>& ys) {
  std::vector<Poly> out;
  const int nx = (int)xs.size() - 1, ny = (int)ys.size() - 1;
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i)
      out.push_back(rect(xs[i], xs[i + 1], ys[j], ys[j + 1], j == 0 && c.solid[0], i == nx - 1 && c.solid[1],
                         j == ny - 1 && c.solid[2], i == 0 && c.solid[3]));
  return out;
}

// A triangle cut into four by its edge midpoints: three corner triangles
// (wall 0 and wall 2 on the parent's walls k and k + 2) and the middle one.
static std::vector<Poly> tri_cells(const Poly& c) {
  double mx[3], my[3];
  for (int i = 0; i < 3; ++i) mx[i] = 0.5 * (c.x[i] + c.x[(i + 1) % 3]), my[i] = 0.5 * (c.y[i] + c.y[(i + 1) % 3]);
  std::vector<Poly> out;
  for (int k = 0; k < 3; ++k) {
    const int p = (k + 2) % 3;
    out.push_back(tri(c.x[k], c.y[k], mx[k], my[k], mx[p], my[p], c.solid[k], false, c.solid[p]));
  }
  out.push_back(tri(mx[0], my[0], mx[1], my[1], mx[2], my[2], false, false, false));
  return out;
}

static Dom lat_domain(const char* name, int nx, int ny) {
  Dom D;
  D.name = name;
  D.coarse = {rect(0.0, 1.5, 0.0, 1.0, true, true, true, true)};
  D.fine = {rect_cells(D.coarse[0], edges(0.0, 1.5, nx), edges(0.0, 1.0, ny))};
  return D;
}

static Dom fan_domain(const char* name, int n_wedges) {
  Dom D;
  D.name = name;
  const double two_pi = 6.283185307179586;
  for (int k = 0; k < n_wedges; ++k) {
    const double a0 = two_pi * k / n_wedges, a1 = two_pi * (k + 1) / n_wedges;
    D.coarse.push_back(tri(0.0, 0.0, std::cos(a0), std::sin(a0), std::cos(a1), std::sin(a1), false, true, false));
    D.fine.push_back(tri_cells(D.coarse.back()));
  }
  return D;
}

// An ncx x ncy lattice of coarse rectangles over the unit square (outer walls
// solid), each cut into nxf x nyf fine rectangles of one global lattice;
// `skip`: a coarse box left out.
static Dom mlat_domain(const char* name, int ncx, int ncy, int nxf, int nyf, int skip = -1) {
  Dom D;
  D.name = name;
  const std::vector<double> xs = edges(0.0, 1.0, ncx * nxf), ys = edges(0.0, 1.0, ncy * nyf);
  for (int j = 0; j < ncy; ++j)
    for (int i = 0; i < ncx; ++i) {
      if (j * ncx + i == skip) continue;
      D.coarse.push_back(rect(xs[i * nxf], xs[(i + 1) * nxf], ys[j * nyf], ys[(j + 1) * nyf], j == 0, i == ncx - 1,
                              j == ncy - 1, i == 0));
      D.fine.push_back(rect_cells(D.coarse.back(),
                                  std::vector<double>(xs.begin() + i * nxf, xs.begin() + (i + 1) * nxf + 1),
                                  std::vector<double>(ys.begin() + j * nyf, ys.begin() + (j + 1) * nyf + 1)));
    }
  return D;
}

// ---------------------------------------------------------------- fingerprint

struct Fnv {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  template <class T>
  void val(const T& v) {
    bytes(&v, sizeof(T));
  }
  template <class T>
  void vec(const std::vector<T>& v) {
    val((uint64_t)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
  void grid(const DevGrid& g) { val(g.ox), val(g.oy), val(g.inv_x), val(g.inv_y), val(g.nx), val(g.ny), val(g.cell_base); }
};

static uint64_t fingerprint(const Domain2dBuild& B) {
  Fnv f;
  static_assert(sizeof(DevPoly) == 16 * sizeof(double) && sizeof(CellRec) == 6 * sizeof(double) + 4 * sizeof(int32_t),
                "no padding in the records hashed whole");
  f.vec(B.cpoly), f.vec(B.fpoly), f.vec(B.csolid), f.vec(B.trifrac), f.vec(B.fcoarse), f.vec(B.s_face), f.vec(B.s_wall);
  f.val((int32_t)B.single_convex), f.val((int32_t)B.axis_rect);
  f.grid(B.c_grid);
  f.val((uint64_t)B.fgrids.size());
  for (const DevGrid& g : B.fgrids) f.grid(g);
  f.vec(B.gcells), f.vec(B.glists), f.vec(B.gitems), f.vec(B.beta_first);
  const CoarseLayout& c = B.cl;
  for (int32_t v : {c.bytes, c.blob_bytes, c.off_fgrid, c.off_bbox, c.off_first, c.off_solid, c.off_cells, c.off_beta})
    f.val(v);
  f.vec(B.c_blob), f.vec(B.c_beta);
  const MLatLayout& m = B.ml;
  for (int32_t v : {m.bytes, m.blob_bytes, m.nx, m.ny, m.ncx, m.ncy, m.off_ys, m.off_cxs, m.off_cys, m.off_cmap,
                    m.off_cinfo, m.off_bsolid, m.off_beta, m.off_lay})
    f.val(v);
  for (double v : {m.inv_x, m.inv_y, m.inv_cx, m.inv_cy}) f.val(v);
  f.vec(B.ml_blob), f.vec(B.ml_bbeta), f.vec(B.ml_mixed);
  const LatticeLayout& l = B.lat;
  for (int32_t v : {l.bytes, l.nx, l.ny, l.identity, l.off_ys}) f.val(v);
  f.val(l.inv_x), f.val(l.inv_y);
  f.vec(B.lat_blob), f.vec(B.lat_map);
  return f.h;
}

// ---------------------------------------------------------------- checks

struct Section {
  const char* what;
  int64_t off;
  const void* src;
  size_t bytes;
};

// Offsets ascending, multiples of 16, sections disjoint and inside the blob,
// each byte-equal to its source (no source: the caller checks the content
// itself); `total` (the LDS block) within the limit.
static void check_sections(const std::vector<unsigned char>& blob, const std::vector<Section>& sec, int64_t blob_bytes,
                           int64_t total) {
  EXPECT((int64_t)blob.size() == blob_bytes && blob_bytes % 16 == 0, "%zu %lld", blob.size(), (long long)blob_bytes);
  EXPECT(total % 16 == 0 && total >= blob_bytes && total <= (int64_t)kMaxCoarseLdsBytes, "%lld", (long long)total);
  for (size_t k = 0; k < sec.size(); ++k) {
    const int64_t end = k + 1 < sec.size() ? sec[k + 1].off : blob_bytes;
    EXPECT(sec[k].off % 16 == 0 && sec[k].off >= 0 && sec[k].off + (int64_t)sec[k].bytes <= end, "%s at %lld", sec[k].what,
           (long long)sec[k].off);
    if (sec[k].src && sec[k].off + sec[k].bytes <= blob.size())
      EXPECT(sec[k].bytes == 0 || std::memcmp(blob.data() + sec[k].off, sec[k].src, sec[k].bytes) == 0, "%s", sec[k].what);
  }
}

static int64_t a16(int64_t b) { return (b + 15) / 16 * 16; }

// The distinct x (or y) coordinates of the n polygons' first and third
// vertices, ascending: the lattice lines of a mesh of canonical rectangles,
// from the descriptor's own arrays.
static std::vector<double> lines_of(const double* xy, size_t n, bool xdir) {
  std::set<double> v;
  for (size_t p = 0; p < n; ++p) v.insert(xy[8 * p + (xdir ? 0 : 1)]), v.insert(xy[8 * p + (xdir ? 4 : 5)]);
  return std::vector<double>(v.begin(), v.end());
}

template <class T>
static std::vector<T> section(const std::vector<unsigned char>& blob, int64_t off, size_t n) {
  std::vector<T> v(n);
  if (off >= 0 && off + n * sizeof(T) <= blob.size() && n) std::memcpy(v.data(), blob.data() + off, n * sizeof(T));
  return v;
}

// Whether polygon p of the flattened arrays is the rectangle [x0,x1] x [y0,y1]
// in canonical order with the canonical normals.
static bool is_box(const int32_t* nv, const double* xy, const double* nrm, size_t p, double x0, double x1, double y0,
                   double y1) {
  const double v[8] = {x0, y0, x1, y0, x1, y1, x0, y1}, n[8] = {0, -1, 1, 0, 0, 1, -1, 0};
  bool ok = nv[p] == 4;
  for (int k = 0; k < 8; ++k) ok = ok && xy[8 * p + k] == v[k] && nrm[8 * p + k] == n[k];
  return ok;
}
static bool canonical(const int32_t* nv, const double* xy, const double* nrm, size_t p) {
  return xy[8 * p] < xy[8 * p + 2] && xy[8 * p + 1] < xy[8 * p + 5] &&
         is_box(nv, xy, nrm, p, xy[8 * p], xy[8 * p + 2], xy[8 * p + 1], xy[8 * p + 5]);
}

static void check_polys(const std::vector<DevPoly>& q, const int32_t* nv, const double* xy, const double* nrm, size_t n) {
  EXPECT(q.size() == n, "%zu", q.size());
  for (size_t p = 0; p < n && p < q.size(); ++p)
    for (int i = 0; i < 4; ++i) {
      const int v = std::min(i, nv[p] - 1);
      EXPECT(q[p].x[i] == xy[8 * p + 2 * v] && q[p].y[i] == xy[8 * p + 2 * v + 1], "polygon %zu vertex %d", p, i);
      const bool real = i < nv[p];
      EXPECT(q[p].nx[i] == (real ? nrm[8 * p + 2 * i] : 0.0) && q[p].ny[i] == (real ? nrm[8 * p + 2 * i + 1] : 0.0),
             "polygon %zu normal %d", p, i);
    }
}

static void check_grid_of(const Domain2dBuild& B, const DevGrid& g, int64_t& base, int32_t count) {
  EXPECT(g.cell_base == base && g.nx >= 1 && g.ny >= 1 && g.inv_x > 0 && g.inv_y > 0, "cell_base %d, expected %lld",
         g.cell_base, (long long)base);
  const int64_t n = (int64_t)g.nx * g.ny;
  for (int64_t c = base; c < base + n && c < (int64_t)B.gcells.size(); ++c) {
    const int32_t start = B.glists[2 * c], cnt = B.glists[2 * c + 1];
    EXPECT(start >= 0 && cnt >= 0 && (size_t)start + cnt <= B.gitems.size(), "cell %lld list", (long long)c);
    for (int32_t k = 0; k < cnt; ++k) EXPECT(B.gitems[start + k] >= 0 && B.gitems[start + k] < count, "cell %lld item", (long long)c);
    for (int32_t leaf : B.gcells[c].leaf) EXPECT(leaf >= -2 && leaf < count, "cell %lld leaf %d", (long long)c, leaf);
  }
  base += n;
}

static void check_tables(const Domain2dBuild& B, int n_bins) {
  EXPECT(B.tables.size() == (size_t)n_bins * kLdsTableDoubles && B.beta_first.size() == (size_t)n_bins, "%zu", B.tables.size());
  if (B.tables.size() != (size_t)n_bins * kLdsTableDoubles) return;
  for (int b = 0; b < n_bins; ++b) {
    const double* t = B.tables.data() + (size_t)b * kLdsTableDoubles;
    for (int j = 0; j < kCosTable; ++j) {
      const long double c = t[2 * j], s = t[2 * j + 1];
      EXPECT(fabsl(c * c + s * s - 1.0L) <= 2.0L * DBL_EPSILON, "cos/sin pair %d", j);
    }
    EXPECT(t[0] == 1.0 && t[1] == 0.0, "angle 0");
    for (int i = 0; i < kLogTable; ++i) {
      const double* e = t + kLogTableOffset + 4 * i;
      const long double T = logl((long double)e[0]);
      EXPECT(fabsl(((long double)e[1] + (long double)e[2]) - T) <= LDBL_EPSILON * fabsl(T) && e[1] == (double)T && e[3] == 0.0,
             "log entry %d", i);
      // invc is the reciprocal of the entry's centre: 0.6875 + (i + 0.5) / 128 up to 1, then the [1, 1.375) half
      double z0, z1;
      const uint64_t b0 = kLogOff + ((uint64_t)i << 45), b1 = kLogOff + ((uint64_t)(i + 1) << 45);
      std::memcpy(&z0, &b0, 8), std::memcpy(&z1, &b1, 8);
      EXPECT(e[0] == (double)(2.0L / ((long double)z0 + (long double)z1)), "log entry %d invc", i);
    }
    const double want = B.beta_first[b] > 0 ? 1.0 / B.beta_first[b] : HUGE_VAL;
    EXPECT(t[kTabInvBeta] == want, "bin %d inv beta", b);
  }
}

static void check_domain(const Dom& D, const Domain2dBuild& B) {
  const rthx_domain_desc& s = D.d;
  const size_t nc = s.n_coarse, nf = s.n_fine;
  // s_face / s_wall invert fine_surface
  EXPECT(B.s_face.size() == (size_t)s.n_surfaces && B.s_wall.size() == (size_t)s.n_surfaces, "%zu", B.s_face.size());
  int64_t solid_walls = 0;
  for (size_t f = 0; f < nf; ++f)
    for (int w = 0; w < 4; ++w) {
      const int32_t i = s.fine_surface[4 * f + w];
      if (i < 0) continue;
      ++solid_walls;
      EXPECT(B.s_face[i] == (int32_t)f && B.s_wall[i] == w, "surface %d", i);
    }
  EXPECT(solid_walls == s.n_surfaces, "%lld", (long long)solid_walls);
  // fcoarse inverts fine_offset
  EXPECT(B.fcoarse.size() == nf, "%zu", B.fcoarse.size());
  for (size_t f = 0; f < nf && f < B.fcoarse.size(); ++f) {
    const int32_t c = B.fcoarse[f];
    EXPECT(c >= 0 && (size_t)c < nc && s.fine_offset[c] <= (int32_t)f && (int32_t)f < s.fine_offset[c + 1], "fine %zu", f);
  }
  EXPECT(B.csolid.size() == nc, "%zu", B.csolid.size());
  for (size_t c = 0; c < nc && c < B.csolid.size(); ++c)
    for (int w = 0; w < 4; ++w) EXPECT(((B.csolid[c] >> w) & 1u) == (s.coarse_solid[4 * c + w] ? 1u : 0u), "coarse %zu wall %d", c, w);
  for (size_t c = 0; c < nc && c < B.csolid.size(); ++c) EXPECT(B.csolid[c] < 16u, "coarse %zu", c);
  // trifrac: the reference's expression, bit for bit
  EXPECT(B.trifrac.size() == nf, "%zu", B.trifrac.size());
  for (size_t f = 0; f < nf && f < B.trifrac.size(); ++f) {
    const double* v = s.fine_xy + 8 * f;
    const double want =
        s.fine_nv[f] == 4 ? 0.5 * (v[0] * (v[3] - v[5]) + v[2] * (v[5] - v[1]) + v[4] * (v[1] - v[3])) / s.fine_volume[f] : 0.0;
    EXPECT(std::memcmp(&B.trifrac[f], &want, 8) == 0, "fine %zu: %.17g != %.17g", f, B.trifrac[f], want);
  }
  check_polys(B.cpoly, s.coarse_nv, s.coarse_xy, s.coarse_normal, nc);
  check_polys(B.fpoly, s.fine_nv, s.fine_xy, s.fine_normal, nf);
  // axis_rect, single_convex restated
  bool axis = true;
  for (size_t c = 0; c < nc; ++c) axis = axis && canonical(s.coarse_nv, s.coarse_xy, s.coarse_normal, c);
  for (size_t f = 0; f < nf; ++f) axis = axis && canonical(s.fine_nv, s.fine_xy, s.fine_normal, f);
  EXPECT(B.axis_rect == axis, "%d", (int)B.axis_rect);
  bool convex = nc == 1;
  if (nc == 1) {  // every vertex turns the same way
    const Poly& p = D.coarse[0];
    int left = 0, right = 0;
    for (int i = 0; i < p.n; ++i) {
      const int a = (i + p.n - 1) % p.n, b = (i + 1) % p.n;
      const double t = (p.x[i] - p.x[a]) * (p.y[b] - p.y[i]) - (p.y[i] - p.y[a]) * (p.x[b] - p.x[i]);
      left += t > 0, right += t < 0;
    }
    convex = left == 0 || right == 0;
  }
  EXPECT(B.single_convex == convex, "%d", (int)B.single_convex);
  // grids
  EXPECT(B.fgrids.size() == nc && B.glists.size() == 2 * B.gcells.size() && !B.gitems.empty(), "%zu grids", B.fgrids.size());
  int64_t base = 0;
  if (B.fgrids.size() == nc && B.glists.size() == 2 * B.gcells.size()) {
    check_grid_of(B, B.c_grid, base, s.n_coarse);
    for (size_t c = 0; c < nc; ++c) check_grid_of(B, B.fgrids[c], base, s.fine_offset[c + 1] - s.fine_offset[c]);
    EXPECT(base == (int64_t)B.gcells.size(), "%lld cells of %zu", (long long)base, B.gcells.size());
  }
  check_tables(B, s.n_bins);
  for (int b = 0; b < s.n_bins; ++b) EXPECT(B.beta_first[b] == s.beta[(size_t)b * nf], "bin %d", b);
  // per-coarse betas
  EXPECT(B.c_beta.size() == (nc >= 2 ? (size_t)s.n_bins * nc : 0), "%zu", B.c_beta.size());
  auto shared_beta = [&](int bn, size_t c) {
    const double* bb = s.beta + (size_t)bn * nf;
    for (int f = s.fine_offset[c]; f < s.fine_offset[c + 1]; ++f)
      if (bb[f] != bb[s.fine_offset[c]]) return -1.0;
    return bb[s.fine_offset[c]];
  };
  if (B.c_beta.size() == (size_t)s.n_bins * nc)
    for (int bn = 0; bn < s.n_bins; ++bn)
      for (size_t c = 0; c < nc; ++c) EXPECT(B.c_beta[(size_t)bn * nc + c] == shared_beta(bn, c), "bin %d coarse %zu", bn, c);

  // CLDS layout
  {
    const CoarseLayout& L = B.cl;
    const size_t ncells = (size_t)B.c_grid.nx * B.c_grid.ny;
    const std::vector<Section> sec = {{"cpoly", 0, B.cpoly.data(), nc * sizeof(DevPoly)},
                                      {"fgrids", L.off_fgrid, B.fgrids.data(), nc * sizeof(DevGrid)},
                                      {"bbox", L.off_bbox, s.coarse_bbox, nc * 32},
                                      {"first", L.off_first, s.fine_offset, (nc + 1) * 4},
                                      {"solid", L.off_solid, B.csolid.data(), nc * 4},
                                      {"cells", L.off_cells, B.gcells.data(), ncells * sizeof(CellRec)}};
    const int64_t total = a16(L.off_beta + (int64_t)nc * 8);
    EXPECT(L.off_beta == L.blob_bytes && L.off_beta == a16(L.off_cells + (int64_t)(ncells * sizeof(CellRec))), "%d", L.off_beta);
    const bool staged = nc >= 2 && total <= (int64_t)kMaxCoarseLdsBytes;
    EXPECT(L.bytes == (staged ? total : 0), "bytes %d, block %lld", L.bytes, (long long)total);
    if (L.bytes)
      check_sections(B.c_blob, sec, L.blob_bytes, L.bytes);
    else
      EXPECT(B.c_blob.empty(), "%zu", B.c_blob.size());
  }
  // LAT
  {
    const LatticeLayout& L = B.lat;
    if (L.bytes) {
      const std::vector<double> xs = lines_of(s.fine_xy, nf, true), ys = lines_of(s.fine_xy, nf, false);
      EXPECT((int64_t)xs.size() == L.nx + 1 && (int64_t)ys.size() == L.ny + 1, "%zu x %zu lines", xs.size(), ys.size());
      if ((int64_t)xs.size() != L.nx + 1 || (int64_t)ys.size() != L.ny + 1) return;
      check_sections(B.lat_blob, {{"xs", 0, xs.data(), xs.size() * 8}, {"ys", L.off_ys, ys.data(), ys.size() * 8}}, L.bytes,
                     L.bytes);
      EXPECT(L.off_ys == a16(8 * (L.nx + 1)) && L.bytes == a16(L.off_ys + 8 * (L.ny + 1)), "%d %d", L.off_ys, L.bytes);
      EXPECT(B.single_convex && B.axis_rect && !D.opt.no_lat && (int64_t)L.nx * L.ny == (int64_t)nf && L.nx <= kLatMaxDim &&
                 L.ny <= kLatMaxDim,
             "%d x %d", L.nx, L.ny);
      EXPECT(B.lat_map.size() == (L.identity ? 0 : nf), "%zu", B.lat_map.size());
      std::vector<int> seen(nf, 0);
      for (int j = 0; j < L.ny; ++j)
        for (int i = 0; i < L.nx; ++i) {
          const size_t cell = (size_t)j * L.nx + i;
          const int32_t f = L.identity ? (int32_t)cell : (cell < B.lat_map.size() ? B.lat_map[cell] : -1);
          EXPECT(f >= 0 && (size_t)f < nf, "cell %zu", cell);
          if (f < 0 || (size_t)f >= nf) continue;
          ++seen[f];
          EXPECT(is_box(s.fine_nv, s.fine_xy, s.fine_normal, f, xs[i], xs[i + 1], ys[j], ys[j + 1]), "cell %zu", cell);
          const bool bnd[4] = {j == 0, i == L.nx - 1, j == L.ny - 1, i == 0};
          for (int w = 0; w < 4; ++w) EXPECT(bnd[w] || s.fine_surface[4 * f + w] < 0, "cell %zu wall %d", cell, w);
        }
      for (size_t f = 0; f < nf; ++f) EXPECT(seen[f] == 1, "fine %zu", f);
      const double sc = D.opt.lat_guess_scale > 0 ? D.opt.lat_guess_scale : 1.0;
      EXPECT(L.inv_x == (double)L.nx / (xs[L.nx] - xs[0]) * sc && L.inv_y == (double)L.ny / (ys[L.ny] - ys[0]) * sc, "%g %g",
             L.inv_x, L.inv_y);
      for (int32_t r : L.reserved) EXPECT(r == 0, "%d", r);
    } else {
      EXPECT(B.lat_blob.empty() && B.lat_map.empty() && L.nx == 0 && L.ny == 0, "%zu", B.lat_blob.size());
    }
  }
  // MLAT
  {
    const MLatLayout& G = B.ml;
    if (G.bytes) {
      const std::vector<double> xs = lines_of(s.fine_xy, nf, true), ys = lines_of(s.fine_xy, nf, false);
      const std::vector<double> cxs = lines_of(s.coarse_xy, nc, true), cys = lines_of(s.coarse_xy, nc, false);
      EXPECT((int64_t)xs.size() == G.nx + 1 && (int64_t)ys.size() == G.ny + 1 && (int64_t)cxs.size() == G.ncx + 1 &&
                 (int64_t)cys.size() == G.ncy + 1,
             "%zu x %zu, %zu x %zu lines", xs.size(), ys.size(), cxs.size(), cys.size());
      if ((int64_t)xs.size() != G.nx + 1 || (int64_t)ys.size() != G.ny + 1 || (int64_t)cxs.size() != G.ncx + 1 ||
          (int64_t)cys.size() != G.ncy + 1)
        return;
      // (cmap, the MCoarse records and bsolid are read out of the blob and checked by content below)
      const std::vector<int32_t> cmap = section<int32_t>(B.ml_blob, G.off_cmap, nc);
      const std::vector<MCoarse> info = section<MCoarse>(B.ml_blob, G.off_cinfo, nc);
      const std::vector<uint32_t> bsolid = section<uint32_t>(B.ml_blob, G.off_bsolid, nc);
      check_sections(B.ml_blob,
                     {{"xs", 0, xs.data(), xs.size() * 8},
                      {"ys", G.off_ys, ys.data(), ys.size() * 8},
                      {"cxs", G.off_cxs, cxs.data(), cxs.size() * 8},
                      {"cys", G.off_cys, cys.data(), cys.size() * 8},
                      {"cmap", G.off_cmap, nullptr, nc * 4},
                      {"cinfo", G.off_cinfo, nullptr, nc * sizeof(MCoarse)},
                      {"bsolid", G.off_bsolid, nullptr, nc * 4}},
                     G.blob_bytes, G.bytes);
      EXPECT(G.off_ys == a16(8 * (G.nx + 1)) && G.off_cxs == a16(G.off_ys + 8 * (G.ny + 1)) &&
                 G.off_cys == a16(G.off_cxs + 8 * (G.ncx + 1)) && G.off_cmap == a16(G.off_cys + 8 * (G.ncy + 1)) &&
                 G.off_cinfo == a16(G.off_cmap + 4 * (int64_t)nc) && G.off_bsolid == a16(G.off_cinfo + 32 * (int64_t)nc) &&
                 G.off_beta == a16(G.off_bsolid + 4 * (int64_t)nc) && G.off_beta == G.blob_bytes,
             "section offsets");
      const int64_t after_beta = a16(G.off_beta + 8 * (int64_t)nc);
      if (G.ncx == 1)
        EXPECT(G.off_lay == after_beta && G.bytes == a16(G.off_lay + (int64_t)sizeof(LayerRec) * (G.ncy + 2)), "%d %d", G.off_lay,
               G.bytes);
      else
        EXPECT(G.off_lay == 0 && G.bytes == after_beta, "%d %d", G.off_lay, G.bytes);
      EXPECT(!B.single_convex && B.axis_rect && nc >= 2 && !D.opt.no_mlat && (int64_t)G.ncx * G.ncy == (int64_t)nc, "%d x %d",
             G.ncx, G.ncy);
      std::vector<int> cseen(nc, 0);
      std::vector<int> cover((size_t)G.nx * G.ny, 0), fseen(nf, 0);
      for (size_t b = 0; b < nc; ++b) {
        const int32_t c = cmap[b];
        EXPECT(c >= 0 && (size_t)c < nc, "box %zu", b);
        if (c < 0 || (size_t)c >= nc) continue;
        ++cseen[c];
        const MCoarse& m = info[c];
        const int ci = (int)(b % G.ncx), cj = (int)(b / G.ncx);
        EXPECT(m.ci == ci && m.cj == cj && m.solid == B.csolid[c] && m.first == s.fine_offset[c] &&
                   m.nxf * m.nyf == s.fine_offset[c + 1] - s.fine_offset[c],
               "box %zu record", b);
        EXPECT(is_box(s.coarse_nv, s.coarse_xy, s.coarse_normal, c, cxs[ci], cxs[ci + 1], cys[cj], cys[cj + 1]), "box %zu", b);
        EXPECT(m.i0 >= 0 && m.j0 >= 0 && m.nxf >= 1 && m.nyf >= 1 && m.i0 + m.nxf <= G.nx && m.j0 + m.nyf <= G.ny, "box %zu", b);
        if (!(m.i0 >= 0 && m.j0 >= 0 && m.nxf >= 1 && m.nyf >= 1 && m.i0 + m.nxf <= G.nx && m.j0 + m.nyf <= G.ny)) continue;
        EXPECT(xs[m.i0] == cxs[ci] && xs[m.i0 + m.nxf] == cxs[ci + 1] && ys[m.j0] == cys[cj] && ys[m.j0 + m.nyf] == cys[cj + 1],
               "box %zu fine range", b);
        for (int j = 0; j < m.nyf; ++j)
          for (int i = 0; i < m.nxf; ++i) {
            ++cover[(size_t)(m.j0 + j) * G.nx + m.i0 + i];
            const int32_t f = m.first + j * m.nxf + i;
            if (f < 0 || (size_t)f >= nf) continue;
            ++fseen[f];
            EXPECT(is_box(s.fine_nv, s.fine_xy, s.fine_normal, f, xs[m.i0 + i], xs[m.i0 + i + 1], ys[m.j0 + j], ys[m.j0 + j + 1]),
                   "fine %d", f);
          }
        EXPECT(bsolid[b] == B.csolid[c], "box %zu solid", b);
        for (int bn = 0; bn < s.n_bins; ++bn) {
          const double bb = B.ml_bbeta[(size_t)bn * nc + b];
          EXPECT(bb == shared_beta(bn, c) && (bb < 0) == (shared_beta(bn, c) == -1.0), "bin %d box %zu", bn, b);
        }
      }
      for (size_t c = 0; c < nc; ++c) EXPECT(cseen[c] == 1, "coarse %zu", c);
      for (size_t k = 0; k < cover.size(); ++k) EXPECT(cover[k] == 1, "lattice cell %zu", k);
      for (size_t f = 0; f < nf; ++f) EXPECT(fseen[f] == 1, "fine %zu", f);
      EXPECT(B.ml_bbeta.size() == (size_t)s.n_bins * nc && B.ml_mixed.size() == (size_t)s.n_bins, "%zu", B.ml_bbeta.size());
      for (int bn = 0; bn < s.n_bins && B.ml_mixed.size() == (size_t)s.n_bins; ++bn) {
        bool mixed = false;
        for (size_t b = 0; b < nc; ++b) mixed = mixed || B.ml_bbeta[(size_t)bn * nc + b] < 0;
        EXPECT(B.ml_mixed[bn] == (mixed ? 1 : 0), "bin %d", bn);
      }
      EXPECT(G.inv_x == (double)G.nx / (xs[G.nx] - xs[0]) && G.inv_y == (double)G.ny / (ys[G.ny] - ys[0]) &&
                 G.inv_cx == (double)G.ncx / (cxs[G.ncx] - cxs[0]) && G.inv_cy == (double)G.ncy / (cys[G.ncy] - cys[0]),
             "first guesses");
    } else {
      EXPECT(B.ml_blob.empty() && B.ml_bbeta.empty() && B.ml_mixed.empty() && G.nx == 0 && G.blob_bytes == 0, "%zu",
             B.ml_blob.size());
    }
  }
}

static Domain2dBuild run(Dom D) {
  current = D.name.c_str();
  D.flatten();
  Domain2dBuild B;
  std::string err;
  const int rc = build_domain2d(D.d, D.opt, B, err);
  EXPECT(rc == RTHX_OK && err.empty(), "%d %s", rc, err.c_str());
  if (rc != RTHX_OK) return B;
  check_domain(D, B);
  std::printf("domain %s hash %016llx single %d axis %d lat %d %d %d ml %d %d %d %d %d cl %d cells %zu\n", current,
              (unsigned long long)fingerprint(B), (int)B.single_convex, (int)B.axis_rect, B.lat.nx, B.lat.ny,
              B.lat.bytes ? B.lat.identity : -1, B.ml.nx, B.ml.ny, B.ml.ncx, B.ml.ncy, B.ml.bytes, B.cl.bytes, B.gcells.size());
  return B;
}

// ---------------------------------------------------------------- refusals

static int n_refusals = 0;
static void refuse(const char* what, int code, const std::function<void(Dom&)>& spoil) {
  current = what;
  Dom D = lat_domain("refusal", 3, 2);
  D.flatten();
  spoil(D);
  Domain2dBuild B;
  std::string err;
  const int rc = build_domain2d(D.d, D.opt, B, err);
  EXPECT(rc == code && err == what, "%d '%s'", rc, err.c_str());
  ++n_refusals;
}

static void check_refusals() {
  static const double nan = std::nan(""), inf = HUGE_VAL;
  refuse("empty or negative domain sizes", RTHX_EINVAL, [](Dom& D) { D.d.n_bins = 0; });
  refuse("empty or negative domain sizes", RTHX_EINVAL, [](Dom& D) { D.d.n_surfaces = -1; });
  // (tested before any array is read: the sizes alone)
  refuse("too many elements", RTHX_ERANGE, [](Dom& D) {
    D.d = rthx_domain_desc{};
    D.d.n_coarse = 1, D.d.n_bins = 1, D.d.n_fine = 1 << 30, D.d.n_surfaces = 1 << 30;
  });
  refuse("null descriptor array", RTHX_EINVAL, [](Dom& D) { D.d.fine_mid = nullptr; });
  refuse("null descriptor array", RTHX_EINVAL, [](Dom& D) { D.d.uniform_beta = nullptr; });
  refuse("coarse polygon with n not in {3,4}", RTHX_EINVAL, [](Dom& D) { D.c_nv[0] = 5; });
  refuse("fine_offset must run from 0 to n_fine", RTHX_EINVAL, [](Dom& D) { D.f_off[1] = 5; });
  refuse("fine_offset must run from 0 to n_fine", RTHX_EINVAL, [](Dom& D) { D.f_off[0] = 1; });
  refuse("coarse polygon without fine polygons", RTHX_EINVAL, [](Dom& D) {
    D.c_nv.push_back(4), D.d.coarse_nv = D.c_nv.data();
    D.f_off = {0, 6, 6}, D.d.fine_offset = D.f_off.data();
    D.d.n_coarse = 2;
  });
  refuse("fine polygon with n not in {3,4}", RTHX_EINVAL, [](Dom& D) { D.f_nv[5] = 2; });
  refuse("fine_surface index out of range", RTHX_EINVAL, [](Dom& D) { D.f_surf[0] = D.d.n_surfaces; });
  refuse("fine_surface index out of range", RTHX_EINVAL, [](Dom& D) { D.f_surf[1] = -2; });
  refuse("fine_surface index out of range", RTHX_EINVAL, [](Dom& D) { D.f_nv[0] = 3; });  // (its wall 3 is solid)
  refuse("surface index used twice", RTHX_EINVAL, [](Dom& D) { D.f_surf[4 * 5 + 1] = D.f_surf[0]; });
  refuse("surface index without a solid fine wall", RTHX_EINVAL, [](Dom& D) { D.f_surf[0] = -1; });
  refuse("non-finite or negative extinction", RTHX_EINVAL, [](Dom& D) { D.beta[3] = -0.1; });
  refuse("non-finite or negative extinction", RTHX_EINVAL, [](Dom& D) { D.beta[5] = inf; });
  refuse("non-finite fine geometry", RTHX_EINVAL, [](Dom& D) { D.f_xy[17] = nan; });
  refuse("non-finite fine geometry", RTHX_EINVAL, [](Dom& D) { D.f_nrm[47] = inf; });
  refuse("invalid grid: coarse grid", RTHX_EINVAL, [](Dom& D) { D.d.coarse_grid.nx = 0; });
  refuse("invalid grid: coarse grid", RTHX_EINVAL, [](Dom& D) { D.d.coarse_grid.inv_cell_size = nan; });
  refuse("invalid grid: fine grid", RTHX_EINVAL, [](Dom& D) { D.fgrid[0].cell_start = nullptr; });
  // (tested before cell_start is read: the sizes alone)
  refuse("grid too large: fine grid", RTHX_ERANGE, [](Dom& D) { D.fgrid[0].nx = D.fgrid[0].ny = 65536; });
  refuse("grid cell_start[0] != 0: coarse grid", RTHX_EINVAL, [](Dom& D) { D.g_start[0][0] = 1; });
  refuse("grid cell_start not monotone: fine grid", RTHX_EINVAL, [](Dom& D) { D.g_start[1][1] = -1; });
  refuse("null grid items: fine grid", RTHX_EINVAL, [](Dom& D) { D.fgrid[0].cell_items = nullptr; });
  refuse("grid item out of range: fine grid", RTHX_EINVAL, [](Dom& D) { D.g_items[1][2] = 6; });
  refuse("grid item out of range: coarse grid", RTHX_EINVAL, [](Dom& D) { D.g_items[0][0] = -1; });
}

// ---------------------------------------------------------------- mirror masks

static void check_mirror_masks() {
  current = "mirror_masks";
  // two unit squares side by side and a triangle on top of the first; the
  // squares share the wall x = 1 (wall 1 of square 0, wall 3 of square 1)
  auto flat = [](const std::vector<Poly>& polys, std::vector<int32_t>& nv, std::vector<double>& xy, std::vector<uint32_t>& solid) {
    for (const Poly& p : polys) {
      nv.push_back(p.n);
      uint32_t m = 0;
      for (int i = 0; i < 4; ++i) {
        xy.push_back(i < p.n ? p.x[i] : 0.0), xy.push_back(i < p.n ? p.y[i] : 0.0);
        m |= (i < p.n && p.solid[i]) ? 1u << i : 0u;
      }
      solid.push_back(m);
    }
  };
  for (int neighbour_solid = 0; neighbour_solid < 2; ++neighbour_solid) {
    std::vector<int32_t> nv;
    std::vector<double> xy;
    std::vector<uint32_t> solid, mask;
    flat({rect(0, 1, 0, 1, true, false, false, false), rect(1, 2, 0, 1, true, true, true, neighbour_solid != 0),
          tri(0, 1, 1, 1, 0.5, 2, false, true, true)},
         nv, xy, solid);
    std::vector<uint8_t> flags(12, 0);
    int64_t n = -1;
    std::string err;
    EXPECT(mirror_masks(nv, xy, solid, nullptr, mask, n, err) == RTHX_OK && n == 0 && mask == std::vector<uint32_t>(3, 0u), "no flags");
    flags[1] = 1;  // square 0, wall 1: shared with square 1
    flags[3] = 1;  // square 0, wall 3: nobody's neighbour
    EXPECT(mirror_masks(nv, xy, solid, flags.data(), mask, n, err) == RTHX_OK && n == 2, "%lld %s", (long long)n, err.c_str());
    EXPECT(mask.size() == 3 && mask[0] == (2u | 8u) && mask[1] == (neighbour_solid ? 0u : 8u) && mask[2] == 0u, "%u %u %u", mask[0],
           mask[1], mask[2]);
    flags.assign(12, 0);
    flags[4 * 2 + 0] = 1;  // the triangle's wall 0 = square 0's wall 2, reversed
    EXPECT(mirror_masks(nv, xy, solid, flags.data(), mask, n, err) == RTHX_OK && n == 1 && mask[0] == 4u && mask[1] == 0u &&
               mask[2] == 1u,
           "%lld", (long long)n);
    flags.assign(12, 0);
    flags[4 * 2 + 3] = 1;
    EXPECT(mirror_masks(nv, xy, solid, flags.data(), mask, n, err) == RTHX_EINVAL &&
               err == "mirror flag on a wall the coarse polygon does not have",
           "%s", err.c_str());
    flags.assign(12, 0);
    flags[0] = 1;
    EXPECT(mirror_masks(nv, xy, solid, flags.data(), mask, n, err) == RTHX_EINVAL && err == "mirror flag on a solid wall", "%s",
           err.c_str());
  }
}

// ---------------------------------------------------------------- main

int main() {
  // LAT
  const Domain2dBuild lat_3x2 = run(lat_domain("lat_3x2", 3, 2));
  {
    Dom D = lat_domain("lat_3x2_permuted", 3, 2);
    std::swap(D.fine[0][1], D.fine[0][4]);
    run(D);
  }
  {
    Dom D = lat_domain("lat_3x2_interior_wall", 3, 2);
    D.fine[0][1].solid[2] = true;  // (the wall between cells (1, 0) and (1, 1))
    run(D);
  }
  {  // cell (0, 0) split in two along x only: 7 fine cells on a 4 x 2 lattice of edges
    Dom D = lat_domain("lat_split_cell", 3, 2);
    const Poly p = D.fine[0][0];
    D.fine[0][0] = rect(p.x[0], 0.25, p.y[0], p.y[2], true, false, false, true);
    D.fine[0].push_back(rect(0.25, p.x[1], p.y[0], p.y[2], true, false, false, false));
    run(D);
  }
  {
    Dom D = lat_domain("lat_3x2_no_lat", 3, 2);
    D.opt.no_lat = true;
    run(D);
  }
  {
    Dom D = lat_domain("lat_3x2_guess_half", 3, 2);
    D.opt.lat_guess_scale = 0.5;
    Domain2dBuild B = run(D);
    // the first guess is scaled and nothing else moves
    EXPECT(B.lat.inv_x == 0.5 * lat_3x2.lat.inv_x && B.lat.inv_y == 0.5 * lat_3x2.lat.inv_y, "%g %g", B.lat.inv_x, B.lat.inv_y);
    B.lat.inv_x = lat_3x2.lat.inv_x, B.lat.inv_y = lat_3x2.lat.inv_y;
    EXPECT(fingerprint(B) == fingerprint(lat_3x2) && B.tables == lat_3x2.tables && B.lat.bytes > 0, "something else moved");
  }
  // one coarse polygon that is no rectangle
  {
    Dom D;
    D.name = "single_triangle";
    D.coarse = {tri(0, 0, 2, 0, 0.5, 1.5, true, true, true)};
    D.fine = {tri_cells(D.coarse[0])};
    run(D);
  }
  {  // a quad with a reflex vertex, cut along the diagonal through it
    Dom D;
    D.name = "single_nonconvex_quad";
    Poly q;
    q.n = 4;
    const double x[4] = {0, 2, 0.5, 0}, y[4] = {0, 0, 0.5, 2};
    for (int i = 0; i < 4; ++i) q.x[i] = x[i], q.y[i] = y[i], q.solid[i] = true;
    D.coarse = {q};
    D.fine = {{tri(0, 0, 2, 0, 0.5, 0.5, true, true, false), tri(0, 0, 0.5, 0.5, 0, 2, false, true, true)}};
    run(D);
  }
  // CLDS
  run(fan_domain("fan_4", 4));
  run(fan_domain("fan_16", 16));
  // MLAT
  {
    Dom D = mlat_domain("mlat_2x3_of_4x3", 2, 3, 4, 3);  // (tests/helpers.py quad_lattice_domain, its betas too)
    for (size_t c = 0; c < D.coarse.size(); ++c)
      D.beta.insert(D.beta.end(), D.fine[c].size(), 0.8 * (1 + 0.3 * ((c % 2 + c / 2) % 2)));
    run(D);
  }
  {  // the coarse polygons out of box order (cmap no identity), their solid walls and betas all different
    Dom D = mlat_domain("mlat_2x3_coarse_permuted", 2, 3, 4, 3);
    std::swap(D.coarse[0], D.coarse[4]), std::swap(D.fine[0], D.fine[4]);
    std::swap(D.coarse[1], D.coarse[2]), std::swap(D.fine[1], D.fine[2]);
    for (size_t c = 0; c < D.coarse.size(); ++c) D.beta.insert(D.beta.end(), D.fine[c].size(), 0.25 * (c + 1));
    run(D);
  }
  run(mlat_domain("mlat_column_3_layers", 1, 3, 5, 2));
  {
    Dom D = mlat_domain("mlat_column_2_bins_mixed", 1, 3, 5, 2);
    D.n_bins = 2;
    D.beta.assign(2 * 30, 0.5);
    for (int f = 10; f < 20; ++f) D.beta[f] = 0.7;  // bin 0: layer 1 differs from the others, uniform inside
    D.beta[30 + 13] = 0.9;                          // bin 1: one fine cell of layer 1 differs
    const Domain2dBuild B = run(D);
    EXPECT(B.ml_mixed == std::vector<uint8_t>({0, 1}) && B.ml_bbeta == std::vector<double>({0.5, 0.7, 0.5, 0.5, -1.0, 0.5}),
           "mixed bins");
    EXPECT(B.ml.off_lay > 0 && B.ml.bytes - B.ml.off_lay == (int32_t)sizeof(LayerRec) * (3 + 2), "%d", B.ml.off_lay);
  }
  {
    Dom D = mlat_domain("mlat_2x3_no_mlat", 2, 3, 4, 3);
    D.opt.no_mlat = true;
    run(D);
  }
  run(mlat_domain("mlat_2x3_box_missing", 2, 3, 4, 3, 3));
  {  // the boxes in place, one coarse polygon's fine cells y fastest
    Dom D = mlat_domain("mlat_2x3_y_fastest", 2, 3, 4, 3);
    std::vector<Poly> t;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 3; ++j) t.push_back(D.fine[2][j * 4 + i]);
    D.fine[2] = t;
    run(D);
  }
  // too big for LDS: the coarse mesh alone, then the lattice's block too
  // (the smallest that are: 9 x 9 still stages the coarse mesh, 31 x 31 the lattice)
  run(mlat_domain("mlat_10x10_of_1x1", 10, 10, 1, 1));
  run(mlat_domain("mlat_32x32_of_1x1", 32, 32, 1, 1));

  check_refusals();
  check_mirror_masks();
  std::printf("refusals provoked: %d; not provoked: \"grids too large\" (2^30 grid cells)\n", n_refusals);
  if (fails) {
    std::printf("domain2d check FAILED: %d\n", fails);
    return 1;
  }
  std::printf("domain2d check ok\n");
  return 0;
}
