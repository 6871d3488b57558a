// Stand-alone check of the per-voxel gas box's ray (csrc/rthx_gasbox_walk.h
// walk, the function the kernel calls), built with
// -fsanitize=address,undefined by tests/test_gasbox_field_host.py.  The
// kernel gathers beta at the walk's voxel index and adds to histogram counter
// walk(...) without a bounds test, so the ranges [0, Nv) and [0, N) are what
// keep its loads and atomics inside their arrays: the field handed to walk
// here is a heap array of exactly Nv doubles (AddressSanitizer sees a read
// outside it), and the column is checked for 1e6 random rays in each of three
// boxes, with random fields that include zeros, and for hand-made cases: the
// uniform check's (origins on faces, edges and corners, zero direction
// components, ties in the exit distance, tau = +inf), tau exactly at a
// voxel's far boundary, a ray along an edge, an all-zero field and -- range
// only -- inputs no emitter produces: origins outside the box, huge and
// non-finite origins, directions, depths and fields.
// No ray may take more than n_x + n_y + n_z trips, wall hits must land on the
// face the direction points at, and random rays must agree with a long-double
// restatement written here (all plane crossings sorted, segments located by
// their midpoints), except where that restatement has two crossings, the
// origin and a plane, or the absorption threshold and a crossing within 1e-12
// relative; the share of such exceptions is printed and must stay under 1e-6.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "rthx_gasbox_walk.h"

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

static ld cell_width(const gb::Box& B, int k) { return ((ld)B.hi[k] - (ld)B.lo[k]) / (ld)B.n[k]; }

static int32_t located(const gb::Box& B, int k, ld x) {
  ld fl = floorl((x - (ld)B.lo[k]) / cell_width(B, k));
  if (fl < 0) fl = 0;
  if (fl > B.n[k] - 1) fl = B.n[k] - 1;
  return (int32_t)fl;
}

// The restatement.  Exit as classify's (distance to the box face per axis,
// the lowest axis on a tie); every interior plane crossed before it, sorted;
// optical depth summed over the segments between crossings, each located by
// its midpoint.  near: see the head of the file.
static int32_t restate(const gb::Box& B, const std::vector<double>& beta, const double* o, const double* d, double tau,
                       bool* near) {
  const ld inf = std::numeric_limits<ld>::infinity(), tiny = 1e-12L;
  *near = false;
  ld t_exit = inf;
  int ax = 0;
  for (int k = 0; k < 3; ++k) {
    const ld tk = d[k] == 0.0 ? inf : ((ld)(d[k] > 0.0 ? B.hi[k] : B.lo[k]) - (ld)o[k]) / (ld)d[k];
    if (tk < t_exit) {
      t_exit = tk;
      ax = k;
    }
  }
  static std::vector<ld> cross;  // (reused: one allocation for all rays)
  cross.clear();
  for (int k = 0; k < 3; ++k) {
    const ld h = cell_width(B, k);
    const ld x = ((ld)o[k] - (ld)B.lo[k]) / h;
    if (fabsl(x - roundl(x)) < tiny && !(x < 0.5L && d[k] > 0.0) && !(x > B.n[k] - 0.5L && d[k] < 0.0))
      *near = true;  // (an origin on an interior plane, or on a face it leaves through)
    if (d[k] == 0.0) continue;
    for (int32_t i = 0; i <= B.n[k]; ++i) {
      const ld t = ((ld)B.lo[k] + (ld)i * h - (ld)o[k]) / (ld)d[k];
      if (k == ax && (i == 0 || i == B.n[k])) continue;  // (the exit itself, and the face behind the ray)
      if (t > 0 && fabsl(t - t_exit) < tiny * (1 + fabsl(t_exit))) *near = true;
      if (t > 0 && t < t_exit && i > 0 && i < B.n[k]) cross.push_back(t);
    }
  }
  std::sort(cross.begin(), cross.end());
  for (size_t i = 1; i < cross.size(); ++i)
    if (cross[i] - cross[i - 1] < tiny * (1 + cross[i])) *near = true;
  if (!cross.empty() && cross[0] < tiny) *near = true;
  cross.push_back(t_exit);
  ld t_prev = 0, acc = 0;
  for (const ld t : cross) {
    const ld mid = 0.5L * (t_prev + t);
    const int32_t c0 = located(B, 0, (ld)o[0] + mid * (ld)d[0]), c1 = located(B, 1, (ld)o[1] + mid * (ld)d[1]),
                  c2 = located(B, 2, (ld)o[2] + mid * (ld)d[2]);
    const int32_t v = c0 + B.n[0] * (c1 + B.n[1] * c2);
    const ld next = acc + (ld)beta[v] * (t - t_prev);
    if (fabsl((ld)tau - next) < tiny * (1 + next)) *near = true;
    if ((ld)tau < next) return B.n_surfaces + v;
    acc = next;
    t_prev = t;
  }
  int32_t c[3];
  for (int k = 0; k < 3; ++k) c[k] = located(B, k, (ld)o[k] + t_exit * (ld)d[k]);
  const int f = 2 * ax + (d[ax] > 0.0 ? 1 : 0);
  const int p = ax == 0 ? 1 : 0, q = ax == 2 ? 1 : 2;
  return B.face_offset[f] + c[p] + B.n[p] * c[q];
}

// Range and trips, and (face: inputs with a finite exit distance) the face a wall hit lands on.
static int32_t checked(const gb::Box& B, const std::vector<double>& beta, const double* o, const double* d, double tau,
                       const char* what, bool face = true) {
  int32_t trips = -1;
  const int32_t col = gb::walk(B, beta.data(), o, d, tau, &trips);
  EXPECT(col >= 0 && col < B.n_elements, "%s: column %d of %d (o %g %g %g d %g %g %g tau %g)", what, col, B.n_elements,
         o[0], o[1], o[2], d[0], d[1], d[2], tau);
  EXPECT(trips >= 1 && trips <= B.n[0] + B.n[1] + B.n[2], "%s: %d trips in a %d x %d x %d lattice", what, trips, B.n[0],
         B.n[1], B.n[2]);
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

static int64_t n_volumes(const gb::Box& B) { return (int64_t)B.n_elements - B.n_surfaces; }

// A field of Nv entries: a third of the voxels transparent, the rest spread over three decades.
static std::vector<double> random_field(const gb::Box& B, std::mt19937_64& rng) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::vector<double> beta((size_t)n_volumes(B));
  for (double& b : beta) b = U(rng) < 1.0 / 3.0 ? 0.0 : std::pow(10.0, -1.0 + 3.0 * U(rng));
  return beta;
}

static long random_rays(const gb::Box& B, uint64_t seed, long n_rays, long* n_near) {
  std::mt19937_64 rng(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> G(0.0, 1.0);
  long checked_n = 0;
  std::vector<double> beta;
  for (long i = 0; i < n_rays; ++i) {
    if (i % 1000 == 0) beta = random_field(B, rng);
    double o[3], d[3];
    for (int k = 0; k < 3; ++k) {
      o[k] = B.lo[k] + U(rng) * (B.hi[k] - B.lo[k]);
      d[k] = G(rng);
    }
    const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (len == 0.0) continue;
    for (int k = 0; k < 3; ++k) d[k] /= len;
    const double tau = (rng() & 31u) == 0 ? std::numeric_limits<double>::infinity() : -std::log(1.0 - U(rng));
    const int32_t col = checked(B, beta, o, d, tau, "random ray");
    bool near;
    const int32_t want = restate(B, beta, o, d, tau, &near);
    if (near)
      ++*n_near;
    else
      EXPECT(col == want, "random ray: column %d, restatement %d (o %.17g %.17g %.17g d %.17g %.17g %.17g tau %.17g)",
             col, want, o[0], o[1], o[2], d[0], d[1], d[2], tau);
    ++checked_n;
  }
  return checked_n;
}

static void edge_cases(const gb::Box& B) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double mid[3] = {0.5 * (B.lo[0] + B.hi[0]), 0.5 * (B.lo[1] + B.hi[1]), 0.5 * (B.lo[2] + B.hi[2])};
  const size_t nv = (size_t)n_volumes(B);
  std::mt19937_64 rng(99);
  const std::vector<double> zero(nv, 0.0), one(nv, 1.0), mixed = random_field(B, rng);
  const double dirs[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 1, 0}, {-1, 0, 1},
                            {0, -1, -1}, {1, 1, 1}, {-1, -1, -1}, {1, -1, 1}, {0.6, 0.8, 0}, {1e-300, 1, 0},
                            {-0.0, 0.0, 1}, {0, 0, 0}};
  const double depths[] = {0.0, 1e-300, 1e-9, 0.1, 0.25, 1.0, 1e9, 1e300, inf};
  // origins on faces, edges, corners, cell boundaries and the centre
  for (int ix = 0; ix <= 2 * B.n[0]; ++ix)
    for (int iy = 0; iy <= 2 * B.n[1]; ++iy)
      for (int iz = 0; iz <= 2 * B.n[2]; ++iz) {
        const double o[3] = {B.lo[0] + 0.5 * ix * B.h[0], B.lo[1] + 0.5 * iy * B.h[1], B.lo[2] + 0.5 * iz * B.h[2]};
        for (const auto& dd : dirs)
          for (double tau : depths) {
            checked(B, mixed, o, dd, tau, "lattice origin");
            // an all-zero field absorbs nothing: every ray with a direction ends at a wall
            const int32_t col = checked(B, zero, o, dd, tau, "lattice origin, zero field");
            if (dd[0] != 0.0 || dd[1] != 0.0 || dd[2] != 0.0)
              EXPECT(col < B.n_surfaces, "zero field: a ray ended in voxel column %d", col);
          }
      }
  // two- and three-axis ties at the exit from the centre: the lowest axis wins
  {
    // (towards lo: the exit planes lo + 0 h are exact, so both distances are exactly 1)
    const double d2[3] = {B.lo[0] - mid[0], B.lo[1] - mid[1], 0.0};  // reaches the x- / y- edge at t = 1
    int32_t col = checked(B, zero, mid, d2, inf, "two-axis tie");
    EXPECT(face_of(B, col) == 0, "two-axis tie: face %d, the lowest axis wins (x-)", face_of(B, col));
    const double d3n[3] = {B.lo[0] - mid[0], B.lo[1] - mid[1], B.lo[2] - mid[2]};  // reaches the corner lo at t = 1
    col = checked(B, one, mid, d3n, inf, "three-axis tie");
    EXPECT(col == B.face_offset[0], "three-axis tie: column %d, expected x- cell (0, 0)", col);
  }
  // tau exactly at a voxel's far boundary is not absorbed there (strict): with
  // beta = 1 the depth of the first cell is its segment, tau_next = 0 + 1 * seg
  {
    const double o[3] = {B.lo[0], mid[1], mid[2]}, d[3] = {1.0, 0.0, 0.0};
    const int32_t cy = gb::cell_of(B, 1, mid[1]), cz = gb::cell_of(B, 2, mid[2]);
    const int32_t first = B.n_surfaces + B.n[0] * (cy + B.n[1] * cz);
    const double seg = gb::plane_t(B.lo[0], B.h[0], 0, 1, o[0], d[0]);
    int32_t col = checked(B, one, o, d, seg, "tau at the far boundary");
    if (B.n[0] >= 2)
      EXPECT(col == first + 1, "tau at the far boundary: column %d, expected the next voxel %d", col, first + 1);
    else
      EXPECT(face_of(B, col) == 1, "tau at the far boundary of the only cell: column %d, expected the x+ wall", col);
    col = checked(B, one, o, d, std::nextafter(seg, 0.0), "tau just inside");
    EXPECT(col == first, "tau just inside the far boundary: column %d, expected voxel %d", col, first);
    col = checked(B, one, o, d, 0.0, "tau 0");  // (0 < 0 + seg: absorbed where it starts)
    EXPECT(col == first, "tau 0: column %d, expected voxel %d", col, first);
  }
  // a ray along an edge of the box stays in the edge's cells and leaves through the end wall's corner cell
  {
    const double o[3] = {B.lo[0], B.lo[1], mid[2]}, up[3] = {0.0, 0.0, 1.0}, down[3] = {0.0, 0.0, -1.0};
    int32_t col = checked(B, zero, o, up, 1.0, "along an edge");
    EXPECT(col == B.face_offset[5], "along an edge: column %d, expected z+ cell (0, 0)", col);
    col = checked(B, zero, o, down, 1.0, "along an edge");
    EXPECT(col == B.face_offset[4], "along an edge: column %d, expected z- cell (0, 0)", col);
    col = checked(B, one, o, up, 1e-9, "along an edge");
    EXPECT(col == B.n_surfaces + B.n[0] * B.n[1] * gb::cell_of(B, 2, mid[2]), "along an edge: absorbed in column %d", col);
    const double o2[3] = {B.hi[0], B.hi[1], B.lo[2]};  // the far edge, from its lower end
    col = checked(B, zero, o2, up, inf, "along the far edge");
    EXPECT(col == B.face_offset[5] + B.n[0] * B.n[1] - 1, "along the far edge: column %d, expected the last z+ cell", col);
  }
  // inputs no emitter produces: the ranges must hold all the same
  const double wild[] = {-inf, -1e308, -1e30, -1.0, -0.0, 0.0, 1e-310, 0.3, 1.0, 1e30, 1e308, inf, nan};
  std::vector<double> wild_field(nv);
  for (size_t v = 0; v < nv; ++v) wild_field[v] = wild[(7 * v + 3) % 13];
  const std::vector<double>* const fields[2] = {&mixed, &wild_field};
  for (const std::vector<double>* field : fields)
    for (double a : wild)
      for (double b : wild)
        for (double tau : wild) {
          const double o1[3] = {a, mid[1], b}, d1[3] = {b, a, 1.0}, o2[3] = {mid[0], a, a}, d2[3] = {a, b, b};
          checked(B, *field, o1, d1, tau, "wild input", false);
          checked(B, *field, o2, d1, tau, "wild input", false);
          checked(B, *field, mid, d2, tau, "wild input", false);
          checked(B, *field, o1, d2, tau, "wild input", false);
        }
}

int main() {
  const int shapes[3][3] = {{4, 3, 2}, {1, 1, 1}, {7, 1, 3}};
  long total = 0, n_near = 0;
  for (int s = 0; s < 3; ++s) {
    const gb::Box B = box_of(shapes[s][0], shapes[s][1], shapes[s][2]);
    // wall_column's face offsets (from n) are layout's
    for (int f = 0; f < 6; ++f)
      EXPECT(gb::wall_column(B, f >> 1, f & 1, 0, 0, 0) == B.face_offset[f], "face %d starts at %d, not %d", f,
             gb::wall_column(B, f >> 1, f & 1, 0, 0, 0), B.face_offset[f]);
    // every emitter's own ray: depth 0 is absorbed where it starts, an unattenuated ray reaches another wall
    const std::vector<double> one((size_t)n_volumes(B), 1.0);
    for (int32_t g = 0; g < B.n_elements; ++g) {
      const gb::Emitter E = gb::make_emitter(B, g);
      const double u[3] = {0.5, 0.25, 0.75};
      double o[3], d[3];
      gb::emit(E, u, 0.6, 0.8, 0.6, 0.8, o, d);
      const int32_t col = checked(B, one, o, d, 0.0, "emitter");
      if (g >= B.n_surfaces) EXPECT(col == g, "voxel %d: a ray of depth 0 ends in %d", g, col);
      else EXPECT(col >= B.n_surfaces, "wall %d: a ray of depth 0 ends at %d, not in the gas", g, col);
      const int32_t far = checked(B, one, o, d, std::numeric_limits<double>::infinity(), "emitter");
      EXPECT(far < B.n_surfaces && far != g, "emitter %d: an unattenuated ray ends at %d", g, far);
      EXPECT(far == gb::classify(B, o, d, std::numeric_limits<double>::infinity()),
             "emitter %d: the walk leaves at %d, the uniform ray at %d", g, far,
             gb::classify(B, o, d, std::numeric_limits<double>::infinity()));
    }
    total += random_rays(B, 4321u + s, 1000000, &n_near);
    edge_cases(B);
  }
  const double share = (double)n_near / (double)total;
  std::printf("gasbox walk rays %ld, near a crossing %ld (share %.3g)\n", total, n_near, share);
  EXPECT(share < 1e-6, "share of near-crossing exceptions %.3g", share);
  if (fails) {
    std::printf("gasbox walk check: %d failures\n", fails);
    return 1;
  }
  std::printf("gasbox walk check ok\n");
  return 0;
}
