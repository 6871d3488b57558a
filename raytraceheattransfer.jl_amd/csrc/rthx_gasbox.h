// rthx_gasbox.h -- the ray of the 3D gas-box exchange tracer (include/rthx.h
// rthx_gasbox_*): an axis-aligned box lo < hi of n[0] x n[1] x
// n[2] uniform cells filled with one grey medium of extinction beta, all six
// faces walls.  Element order, emission geometry and the classification of a
// ray's end point, as plain host and device code: the kernel
// (rthx_gasbox_kernels.hip) and the host check (tests/gasbox_host_check.cpp)
// call the same functions, so the column range that makes the kernel's
// histogram atomics safe is proved on the CPU.
//
// Elements: surfaces first, then volumes.  Face f = 2 axis + side (x-, x+,
// y-, y+, z-, z+); on a face of axis a with the other two axes p < q, cell
// (c_p, c_q) is element face_offset[f] + c_p + n_p c_q.  Volume (c_x, c_y,
// c_z) is element Ns + c_x + n_x (c_y + n_y c_z).
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef RTHX_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTHX_HD __host__ __device__
#else
#define RTHX_HD
#endif
#endif

namespace rthx {
namespace gasbox {

// The two axes p < q other than a.
RTHX_HD inline int axis_p(int a) { return a == 0 ? 1 : 0; }
RTHX_HD inline int axis_q(int a) { return a == 2 ? 1 : 2; }

// Sizes of the lattice n (every n[k] >= 1): Ns, Nv and the first element of
// each face, face_offset[6] = Ns.
RTHX_HD inline void layout(const int32_t n[3], int64_t* n_surfaces, int64_t* n_volumes, int64_t face_offset[7]) {
  int64_t off = 0;
  for (int f = 0; f < 6; ++f) {
    const int a = f >> 1;
    face_offset[f] = off;
    off += (int64_t)n[axis_p(a)] * n[axis_q(a)];
  }
  face_offset[6] = off;
  *n_surfaces = off;
  *n_volumes = (int64_t)n[0] * n[1] * n[2];
}

// The box as the kernel takes it (a kernel argument: wave-uniform).
struct Box {
  double lo[3], hi[3];
  double h[3];        // (hi - lo) / n
  double inv_h[3];    // n / (hi - lo)
  int32_t n[3];
  int32_t face_offset[6];
  int32_t n_surfaces;  // Ns
  int32_t n_elements;  // N = Ns + Nv < 2^31
};

// Fills a Box; false when N >= 2^31.  (lo, hi, n are the caller's, checked.)
inline bool make_box(const double lo[3], const double hi[3], const int32_t n[3], Box* B) {
  // (the product in double first: up to 2^93, it would overflow layout's int64)
  if ((double)n[0] * (double)n[1] * (double)n[2] >= 2147483648.0) return false;
  int64_t ns, nv, off[7];
  layout(n, &ns, &nv, off);
  if (ns + nv >= (int64_t(1) << 31)) return false;
  for (int k = 0; k < 3; ++k) {
    B->lo[k] = lo[k];
    B->hi[k] = hi[k];
    B->h[k] = (hi[k] - lo[k]) / (double)n[k];
    B->inv_h[k] = (double)n[k] / (hi[k] - lo[k]);
    B->n[k] = n[k];
  }
  for (int f = 0; f < 6; ++f) B->face_offset[f] = (int32_t)off[f];
  B->n_surfaces = (int32_t)ns;
  B->n_elements = (int32_t)(ns + nv);
  return true;
}

// Cell of coordinate x along axis k: floor((x - lo) / h) clamped to
// [0, n - 1], as (x - lo) * (n / (hi - lo)).  The comparisons come before the
// conversion, so a NaN or an infinite x gives a cell too (0, or an end cell).
RTHX_HD inline int32_t cell_of(const Box& B, int k, double x) {
  const double c = (x - B.lo[k]) * B.inv_h[k];
  if (!(c >= 0.0)) return 0;
  if (c >= (double)B.n[k]) return B.n[k] - 1;
  return (int32_t)c;  // (0 <= c < n: truncation is floor)
}

// Emitter g as the ray body reads it: a ray leaves from base + u * span (u
// the three position draws; a wall's span is 0 along its own axis, where base
// is the face's plane).
struct Emitter {
  double base[3], span[3];
  int32_t axis;  // a wall's axis; -1: a volume
  double sgn;    // a wall's inward normal along its axis: +1 (side 0) or -1 (side 1)
};

// g in [0, N).
RTHX_HD inline Emitter make_emitter(const Box& B, int32_t g) {
  Emitter E;
  int32_t c[3];
  if (g >= B.n_surfaces) {
    int32_t v = g - B.n_surfaces;
    c[0] = v % B.n[0];
    v /= B.n[0];
    c[1] = v % B.n[1];
    c[2] = v / B.n[1];
    E.axis = -1;
    E.sgn = 0.0;
  } else {
    int f = 0;
    int32_t off = B.face_offset[0];
    for (int k = 1; k < 6; ++k)
      if (g >= B.face_offset[k]) {
        f = k;
        off = B.face_offset[k];
      }
    const int a = f >> 1;
    const int32_t local = g - off;
    const int32_t np = a == 0 ? B.n[1] : B.n[0];  // n_p: p = 1 for a = 0, else 0
    const int32_t cp = local % np, cq = local / np;
    c[0] = a == 0 ? 0 : cp;                       // (p == 0 unless a == 0)
    c[1] = a == 0 ? cp : a == 1 ? 0 : cq;
    c[2] = a == 2 ? 0 : cq;                       // (q == 2 unless a == 2)
    E.axis = a;
    E.sgn = (f & 1) ? -1.0 : 1.0;
  }
  for (int k = 0; k < 3; ++k) {
    const bool own = E.axis == k;
    E.base[k] = own ? ((E.sgn < 0.0) ? B.hi[k] : B.lo[k]) : B.lo[k] + (double)c[k] * B.h[k];
    E.span[k] = own ? 0.0 : B.h[k];
  }
  return E;
}

// Origin and direction of one ray.  u[k]: the position draw along axis k in
// [0, 1) (unused along a wall's own axis); (ct, st): cosine and sine of the
// polar angle -- about the inward normal for a wall (cosine law:
// ct = sqrt(1 - u), st = sqrt(u)), about z for a volume (isotropic:
// ct = 1 - 2u); (cphi, sphi): the azimuth, measured from axis p towards axis q
// for a wall, from x towards y for a volume.
RTHX_HD inline void emit(const Emitter& E, const double u[3], double ct, double st, double cphi, double sphi,
                         double o[3], double d[3]) {
  o[0] = E.base[0] + u[0] * E.span[0];
  o[1] = E.base[1] + u[1] * E.span[1];
  o[2] = E.base[2] + u[2] * E.span[2];
  const double a = st * cphi, b = st * sphi, c = E.axis < 0 ? ct : E.sgn * ct;
  d[0] = E.axis == 0 ? c : a;
  d[1] = E.axis == 0 ? a : E.axis == 1 ? c : b;
  d[2] = E.axis == 0 || E.axis == 1 ? b : c;
}

// Distance along d_k from o_k to the face of axis k that d_k points at; +inf for d_k == 0.
RTHX_HD inline double exit_t(const Box& B, int k, double ok, double dk) {
  const double q = ((dk > 0.0 ? B.hi[k] : B.lo[k]) - ok) / dk;
  return dk == 0.0 ? __builtin_inf() : q;
}

// The element that absorbs the ray o + s d with free path S (>= 0, +inf in a
// transparent medium).  Exit distance: per axis t_a = ((d_a > 0 ? hi_a :
// lo_a) - o_a) / d_a, +inf where d_a == 0 (a select, not the quotient);
// t = min t_a, the lowest axis on a tie.  S < t: the voxel holding o + S d.
// Otherwise the wall cell of the exit face (axis of t, the side d points at)
// holding o + t d.  The result lies in [0, N) for every input, NaN and
// infinities included: every cell index goes through cell_of's clamp.
RTHX_HD inline int32_t classify(const Box& B, const double o[3], const double d[3], double S) {
  // (written out per axis: constant indices only, nothing the device would keep in scratch)
  const double t0 = exit_t(B, 0, o[0], d[0]), t1 = exit_t(B, 1, o[1], d[1]), t2 = exit_t(B, 2, o[2], d[2]);
  double t = __builtin_inf();
  int ax = 0;
  if (t0 < t) t = t0;  // (strict: the lowest axis keeps a tie; a NaN never wins)
  if (t1 < t) {
    t = t1;
    ax = 1;
  }
  if (t2 < t) {
    t = t2;
    ax = 2;
  }
  if (S < t) {
    const int32_t cx = cell_of(B, 0, o[0] + S * d[0]);
    const int32_t cy = cell_of(B, 1, o[1] + S * d[1]);
    const int32_t cz = cell_of(B, 2, o[2] + S * d[2]);
    return B.n_surfaces + cx + B.n[0] * (cy + B.n[1] * cz);
  }
  // (per-axis values by selects on ax, not by indexing: no scratch arrays on the device)
  const double x0 = o[0] + t * d[0], x1 = o[1] + t * d[1], x2 = o[2] + t * d[2];
  const double dax = ax == 0 ? d[0] : ax == 1 ? d[1] : d[2];
  const int f = 2 * ax + (dax > 0.0 ? 1 : 0);
  const int32_t c0 = cell_of(B, 0, x0), c1 = cell_of(B, 1, x1), c2 = cell_of(B, 2, x2);
  const int32_t cp = ax == 0 ? c1 : c0, cq = ax == 2 ? c1 : c2;
  const int32_t np = ax == 0 ? B.n[1] : B.n[0];
  const int32_t off = f == 0 ? B.face_offset[0] : f == 1 ? B.face_offset[1] : f == 2 ? B.face_offset[2]
                    : f == 3 ? B.face_offset[3] : f == 4 ? B.face_offset[4] : B.face_offset[5];
  return off + cp + np * cq;
}

// Philox counter word 3 of the gas-box tracer: apart from the 2D tracer's
// bins, kTrace3dTag (rthx_trace3d.h) and kDirectTag (rthx_direct.h).
constexpr uint32_t kTag = 0x20000000u;
constexpr int kThreads = 256;  // lanes per workgroup

}  // namespace gasbox
}  // namespace rthx

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace rthx {
namespace gasbox {

// Row tally of a launch: an LDS histogram of N u32 counters, of N u16
// counters packed two per word (fewer than 65536 rays per workgroup), or one
// returnless agent-scope atomic per ray into the dense row in global memory.
enum Tally : int { kU32 = 0, kU16 = 1, kGlobal = 2 };

// Grid: n_rows * split workgroups; workgroup (slot, part) traces rays
// ray_base + [part * chunk, ...) of emitter g_begin + slot * g_stride, its
// lanes striding the range.
struct Launch {
  Box B;
  double beta;             // >= 0
  const double* tables;    // kTableDoubles doubles (rthx_domain2d.h), device memory
  int64_t R, ray_base;
  int64_t g_begin, g_stride, n_rows;
  int32_t split;
  uint32_t key0, key1;     // Philox key (seed)
  uint32_t* dense;         // [n_rows][N], zeroed: the parts add into it
  uint32_t* row_tallied;   // [n_rows], zeroed
  bool faithful;
  int tally;               // Tally
  hipStream_t stream;
};

// Dynamic LDS of a launch (0 for kGlobal).
inline size_t lds_bytes(int tally, int64_t N) {
  return tally == kGlobal ? 0 : 4 * (size_t)(tally == kU16 ? (N + 1) / 2 : N);
}

hipError_t launch(const Launch& L);

}  // namespace gasbox
}  // namespace rthx
#endif
