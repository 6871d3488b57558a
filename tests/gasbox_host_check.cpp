// Stand-alone check of the gas-box ray's classification (csrc/rthx_gasbox.h
// classify, the function the kernel calls), built with
// -fsanitize=address,undefined by tests/test_gasbox_host.py.  The kernel adds
// to histogram counter classify(...) without a bounds test, so the range
// [0, N) is what keeps its atomics inside the row: it is checked here for 1e6
// random rays in each of three boxes and for hand-made edge cases (origins on
// faces, edges and corners, zero direction components, ties in the exit
// distance, S == t, S = +inf, end points on cell boundaries, and -- range
// only -- inputs no emitter produces: origins outside the box, huge and
// non-finite values).
// Wall hits must land on the face the direction points at, and random rays
// must agree with a long-double restatement written here, except where that
// restatement's end point lies within 1e-12 h of a cell boundary; the share
// of such exceptions is printed and must stay under 1e-6.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>

#include "rthx_gasbox.h"

namespace gb = rthx::gasbox;
typedef long double ld;

static int fails = 0;
#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      if (fails < 20) {            \
        std::printf("FAIL %s: ", #cond); \
        std::printf(__VA_ARGS__);  \
        std::printf("\n");         \
      }                            \
      ++fails;                     \
    }                              \
  } while (0)

// Face of a wall column (or -1 for a volume).
static int face_of(const gb::Box& B, int32_t col) {
  if (col >= B.n_surfaces) return -1;
  int f = 0;
  for (int k = 1; k < 6; ++k)
    if (col >= B.face_offset[k]) f = k;
  return f;
}

// The restatement: exit distance, end point and cell indices in long double.
// near: the end point (or, for a wall hit, the point o + S d along the exit
// axis) lies within 1e-12 h of a cell boundary.
static int32_t restate(const gb::Box& B, const double* o, const double* d, double S, bool* near) {
  const ld inf = std::numeric_limits<ld>::infinity();
  ld t = inf;
  int ax = 0;
  for (int k = 0; k < 3; ++k) {
    const ld tk = d[k] == 0.0 ? inf : ((ld)(d[k] > 0.0 ? B.hi[k] : B.lo[k]) - (ld)o[k]) / (ld)d[k];
    if (tk < t) {
      t = tk;
      ax = k;
    }
  }
  const bool gas = (ld)S < t;
  const ld e = gas ? (ld)S : t;
  int32_t c[3];
  *near = false;
  for (int k = 0; k < 3; ++k) {
    const ld h = ((ld)B.hi[k] - (ld)B.lo[k]) / (ld)B.n[k];
    const ld x = ((ld)o[k] + e * (ld)d[k] - (ld)B.lo[k]) / h;
    ld fl = floorl(x);
    if (!(gas == false && k == ax) && fabsl(x - roundl(x)) < 1e-12L) *near = true;
    if (fl < 0) fl = 0;
    if (fl > B.n[k] - 1) fl = B.n[k] - 1;
    c[k] = (int32_t)fl;
  }
  if (!gas && std::isfinite(S)) {  // (S barely at or above t: fp64 may round it below)
    const ld h = ((ld)B.hi[ax] - (ld)B.lo[ax]) / (ld)B.n[ax];
    if (fabsl(((ld)S - t) * (ld)d[ax]) < 1e-12L * h) *near = true;
  }
  if (gas) return B.n_surfaces + c[0] + B.n[0] * (c[1] + B.n[1] * c[2]);
  const int f = 2 * ax + (d[ax] > 0.0 ? 1 : 0);
  const int p = ax == 0 ? 1 : 0, q = ax == 2 ? 1 : 2;
  return B.face_offset[f] + c[p] + B.n[p] * c[q];
}

// Range, and (face: inputs with a finite exit distance) the face a wall hit lands on.
static int32_t checked(const gb::Box& B, const double* o, const double* d, double S, const char* what,
                       bool face = true) {
  const int32_t col = gb::classify(B, o, d, S);
  EXPECT(col >= 0 && col < B.n_elements, "%s: column %d of %d (o %g %g %g d %g %g %g S %g)", what, col, B.n_elements,
         o[0], o[1], o[2], d[0], d[1], d[2], S);
  const int f = face_of(B, col);
  if (face && f >= 0 && (d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0)) {
    const double da = d[f >> 1];
    EXPECT((f & 1) ? da > 0.0 : da < 0.0, "%s: hit face %d with d along its axis %g", what, f, da);
  }
  return col;
}

static gb::Box box_of(int nx, int ny, int nz) {
  const double lo[3] = {-0.25, 0.5, 0.0}, hi[3] = {0.75, 1.4, 0.5};
  const int32_t n[3] = {nx, ny, nz};
  gb::Box B{};
  if (!gb::make_box(lo, hi, n, &B)) {
    std::printf("make_box failed\n");
    std::exit(2);
  }
  return B;
}

static long random_rays(const gb::Box& B, uint64_t seed, long n_rays, long* n_near) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  long checked_n = 0;
  for (long i = 0; i < n_rays; ++i) {
    double o[3], d[3];
    for (int k = 0; k < 3; ++k) {
      o[k] = B.lo[k] + U(rng) * (B.hi[k] - B.lo[k]);
      d[k] = G(rng);
    }
    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (len == 0.0) continue;
    for (int k = 0; k < 3; ++k) d[k] /= len;
    const double S = (rng() & 31u) == 0 ? std::numeric_limits<double>::infinity() : -std::log(1.0 - U(rng)) / 2.0;
    const int32_t col = checked(B, o, d, S, "random ray");
    bool near;
    const int32_t want = restate(B, o, d, S, &near);
    if (near)
      ++*n_near;
    else
      EXPECT(col == want, "random ray: column %d, restatement %d (o %.17g %.17g %.17g d %.17g %.17g %.17g S %.17g)", col,
             want, o[0], o[1], o[2], d[0], d[1], d[2], S);
    ++checked_n;
  }
  return checked_n;
}

static void edge_cases(const gb::Box& B) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double mid[3] = {0.5 * (B.lo[0] + B.hi[0]), 0.5 * (B.lo[1] + B.hi[1]), 0.5 * (B.lo[2] + B.hi[2])};
  const double dirs[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 1, 0}, {-1, 0, 1},
                            {0, -1, -1}, {1, 1, 1}, {-1, -1, -1}, {1, -1, 1}, {0.6, 0.8, 0}, {1e-300, 1, 0},
                            {-0.0, 0.0, 1}, {0, 0, 0}};
  const double paths[] = {0.0, 1e-300, 1e-9, 0.1, 0.25, 1.0, 1e9, 1e300, inf};
  // origins on faces, edges, corners, cell boundaries and the centre
  for (int ix = 0; ix <= 2 * B.n[0]; ++ix)
    for (int iy = 0; iy <= 2 * B.n[1]; ++iy)
      for (int iz = 0; iz <= 2 * B.n[2]; ++iz) {
        const double o[3] = {B.lo[0] + 0.5 * ix * B.h[0], B.lo[1] + 0.5 * iy * B.h[1], B.lo[2] + 0.5 * iz * B.h[2]};
        for (const auto& dd : dirs)
          for (double S : paths) checked(B, o, dd, S, "lattice origin");
      }
  // two- and three-axis ties in t from the centre, S == t exactly, beta = 0 (S = +inf)
  {
    const double d2[3] = {B.hi[0] - mid[0], B.hi[1] - mid[1], 0.0};  // reaches the x+ / y+ edge at t = 1
    int32_t col = checked(B, mid, d2, inf, "two-axis tie");
    EXPECT(face_of(B, col) == 1, "two-axis tie: face %d, the lowest axis wins (x+)", face_of(B, col));
    const double d3[3] = {mid[0] - B.lo[0], mid[1] - B.lo[1], mid[2] - B.lo[2]};
    const double d3n[3] = {-d3[0], -d3[1], -d3[2]};  // reaches the corner lo at t = 1
    col = checked(B, mid, d3n, inf, "three-axis tie");
    EXPECT(col == B.face_offset[0], "three-axis tie: column %d, expected x- cell (0, 0)", col);
    col = checked(B, mid, d3n, 1.0, "S == t");
    EXPECT(col == B.face_offset[0], "S == t goes to the wall: column %d", col);
    col = checked(B, mid, d3n, std::nextafter(1.0, 0.0), "S just below t");
    EXPECT(col == B.n_surfaces, "S just below t stays in voxel (0, 0, 0): column %d", col);
  }
  // an end point exactly on a cell boundary belongs to the upper cell (floor)
  if (B.n[0] >= 2) {
    const double o[3] = {B.lo[0], mid[1], mid[2]}, d[3] = {1.0, 0.0, 0.0};
    const int32_t col = checked(B, o, d, B.h[0], "end point on a cell boundary");
    const int32_t cy = (int32_t)((mid[1] - B.lo[1]) * B.inv_h[1]), cz = (int32_t)((mid[2] - B.lo[2]) * B.inv_h[2]);
    EXPECT(col == B.n_surfaces + 1 + B.n[0] * (cy + B.n[1] * cz), "boundary end point: column %d", col);
  }
  // inputs no emitter produces: the range must hold all the same
  const double wild[] = {-inf, -1e308, -1e30, -1.0, -0.0, 0.0, 1e-310, 0.3, 1.0, 1e30, 1e308, inf, nan};
  for (double a : wild)
    for (double b : wild)
      for (double S : wild) {
        const double o1[3] = {a, mid[1], b}, d1[3] = {b, a, 1.0}, o2[3] = {mid[0], a, a}, d2[3] = {a, b, b};
        checked(B, o1, d1, S, "wild input", false);
        checked(B, o2, d1, S, "wild input", false);
        checked(B, mid, d2, S, "wild input", false);
        checked(B, o1, d2, S, "wild input", false);
      }
}

int main() {
  const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {7, 1, 3}};
  long total = 0, n_near = 0;
  for (int s = 0; s < 3; ++s) {
    const gb::Box B = box_of(shapes[s][0], shapes[s][1], shapes[s][2]);
    int64_t ns, nv, off[7];
    gb::layout(B.n, &ns, &nv, off);
    EXPECT(ns == B.n_surfaces && ns + nv == B.n_elements, "layout: %lld + %lld", (long long)ns, (long long)nv);
    // every emitter's own ray starts inside its element: a vanishing free path from a voxel stays there
    for (int32_t g = 0; g < B.n_elements; ++g) {
      const gb::Emitter E = gb::make_emitter(B, g);
      const double u[3] = {0.5, 0.25, 0.75};
      double o[3], d[3];
      gb::emit(E, u, 0.6, 0.8, 0.6, 0.8, o, d);
      const int32_t col = checked(B, o, d, 0.0, "emitter");
      if (g >= B.n_surfaces) EXPECT(col == g, "voxel %d: a ray of length 0 ends in %d", g, col);
      else EXPECT(col >= B.n_surfaces, "wall %d: a ray of length 0 ends at %d, not in the gas", g, col);
      const int32_t far = checked(B, o, d, std::numeric_limits<double>::infinity(), "emitter");
      EXPECT(far < B.n_surfaces && far != g, "emitter %d: an unattenuated ray ends at %d", g, far);
    }
    total += random_rays(B, 1234u + s, 1000000, &n_near);
    edge_cases(B);
  }
  const double share = (double)n_near / (double)total;
  std::printf("gasbox rays %ld, near a cell boundary %ld (share %.3g)\n", total, n_near, share);
  EXPECT(share < 1e-6, "share of boundary exceptions %.3g", share);
  if (fails) {
    std::printf("gasbox check: %d failures\n", fails);
    return 1;
  }
  std::printf("gasbox check ok\n");
  return 0;
}
