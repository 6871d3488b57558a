// rthx_gasbox_walk.h -- the ray of the gas box with one extinction
// coefficient per voxel (include/rthx.h rthx_gasbox_trace_field, DESIGN.md
// §7m).  Emission is the uniform box's (rthx_gasbox.h make_emitter, emit);
// with beta varying from voxel to voxel the ray can no longer end by locating
// one point, so it crosses the lattice cell by cell (a 3D DDA) and spends its
// optical depth tau* = -ln u on the way.  Plain host and device code like
// classify: the kernel (rthx_gasbox_field_kernels.hip) and the host check
// (tests/gasbox_walk_host_check.cpp) call the same function, so the column
// range that makes the kernel's histogram atomics safe, and the range of the
// voxel index it gathers beta from, are proved on the CPU.
#pragma once

#include "rthx_gasbox.h"

namespace rthx {
namespace gasbox {

// Distance along d_k from o_k to the plane that bounds cell c of axis k on the
// side d_k points at, lo_k + (c + (d_k > 0)) h_k: from the integer cell every
// time, never by adding h, so the planes do not drift.  +inf for d_k == 0 (a
// select, not the quotient).  up = (d_k > 0) as 0 / 1.
RTHX_HD inline double plane_t(double lo, double h, int32_t c, int32_t up, double ok, double dk) {
  const double plane = lo + (double)(c + up) * h;
  const double q = (plane - ok) / dk;
  return dk == 0.0 ? __builtin_inf() : q;
}

// The wall cell behind cell (c0, c1, c2) on the face of axis ax, side up (0:
// the lo face, 1: the hi face).  Per-axis values by selects on ax, as in
// classify: nothing runtime-indexed.  The face's first element comes from n
// (layout's sums: faces x-, x+ hold n_y n_z cells each, y-, y+ n_x n_z, z-,
// z+ n_x n_y) rather than from face_offset: six fewer box constants live
// across the kernel's ray loop.
RTHX_HD inline int32_t wall_column(const Box& B, int ax, int32_t up, int32_t c0, int32_t c1, int32_t c2) {
  const int32_t ax_cells = B.n[1] * B.n[2], ay_cells = B.n[0] * B.n[2], az_cells = B.n[0] * B.n[1];
  const int32_t before = ax == 0 ? 0 : ax == 1 ? 2 * ax_cells : 2 * (ax_cells + ay_cells);
  const int32_t own = ax == 0 ? ax_cells : ax == 1 ? ay_cells : az_cells;
  const int32_t cp = ax == 0 ? c1 : c0, cq = ax == 2 ? c1 : c2;
  const int32_t np = ax == 0 ? B.n[1] : B.n[0];
  return before + up * own + cp + np * cq;
}

// The element that absorbs the ray o + s d of optical depth tau (>= 0, +inf:
// never absorbed in the gas) in the field beta_v (Nv values >= 0 in volume
// element order; zeros are legal and never absorb).
//
// From the cell c = cell_of(o) the ray crosses one cell a trip: t_a is the
// distance to the plane that bounds c_a on the side d_a points at (plane_t),
// t_out = min t_a with the lowest axis on a tie, and the segment inside the
// cell is seg = max(t_out - t_cur, 0) (an origin that rounding put a hair
// outside its own cell gives one segment of length 0).  The ray is absorbed
// in c iff tau < tau_acc + beta_c seg -- strict, as classify's S < t; its
// column is then Ns + c_x + n_x (c_y + n_y c_z) from the walk's own indices.
// Otherwise tau_acc takes the sum, c_ax steps by sign(d_ax), and when it
// leaves [0, n_ax) the ray ends on face 2 ax + (d_ax > 0), at the wall cell
// of the walk's two other indices.  Only the axis that stepped gets a new
// t_a: the other two cells did not change, so neither did their planes.
//
// Every trip moves one index one step in a fixed direction, so a ray leaves
// the lattice after at most sum (n_a - 1) + 1 trips whatever the input -- NaN
// and infinities included, where every comparison is false and the walk
// steps along x.  The loop is bounded by sum n_a all the same (a wave-uniform
// trip count); a ray that came out of it would end at a wall cell of the x
// face.  The indices stay in [0, n_a) while the loop runs, so beta_v is read
// inside [0, Nv) and the result lies in [0, N).  trips (optional): the trips
// taken.
RTHX_HD inline int32_t walk(const Box& B, const double* beta_v, const double o[3], const double d[3], double tau,
                            int32_t* trips = nullptr) {
  int32_t c0 = cell_of(B, 0, o[0]), c1 = cell_of(B, 1, o[1]), c2 = cell_of(B, 2, o[2]);
  // (0 / 1 integers, not flags: a flag a lane is a pair of scalar registers on the device)
  const int32_t up0 = d[0] > 0.0 ? 1 : 0, up1 = d[1] > 0.0 ? 1 : 0, up2 = d[2] > 0.0 ? 1 : 0;
  double t0 = plane_t(B.lo[0], B.h[0], c0, up0, o[0], d[0]);
  double t1 = plane_t(B.lo[1], B.h[1], c1, up1, o[1], d[1]);
  double t2 = plane_t(B.lo[2], B.h[2], c2, up2, o[2], d[2]);
  double t_cur = 0.0, tau_acc = 0.0;
  const int32_t cap = B.n[0] + B.n[1] + B.n[2];
  int32_t trip = 0;
  for (; trip < cap; ++trip) {
    double t_out = __builtin_inf();
    int ax = 0;
    if (t0 < t_out) t_out = t0;  // (strict: the lowest axis keeps a tie; a NaN never wins)
    if (t1 < t_out) {
      t_out = t1;
      ax = 1;
    }
    if (t2 < t_out) {
      t_out = t2;
      ax = 2;
    }
    const double ahead = t_out - t_cur;
    const double seg = ahead > 0.0 ? ahead : 0.0;  // (a NaN gives 0)
    const int32_t v = c0 + B.n[0] * (c1 + B.n[1] * c2);
    const double tau_next = tau_acc + beta_v[v] * seg;
    if (tau < tau_next) {
      if (trips) *trips = trip + 1;
      return B.n_surfaces + v;
    }
    tau_acc = tau_next;
    t_cur = t_out;
    const int32_t up = ax == 0 ? up0 : ax == 1 ? up1 : up2;
    const int32_t c = (ax == 0 ? c0 : ax == 1 ? c1 : c2) + 2 * up - 1;
    const int32_t n = ax == 0 ? B.n[0] : ax == 1 ? B.n[1] : B.n[2];
    if (c < 0 || c >= n) {
      if (trips) *trips = trip + 1;
      return wall_column(B, ax, up, c0, c1, c2);
    }
    const double t_new = plane_t(ax == 0 ? B.lo[0] : ax == 1 ? B.lo[1] : B.lo[2], ax == 0 ? B.h[0] : ax == 1 ? B.h[1] : B.h[2],
                                 c, up, ax == 0 ? o[0] : ax == 1 ? o[1] : o[2], ax == 0 ? d[0] : ax == 1 ? d[1] : d[2]);
    c0 = ax == 0 ? c : c0;
    c1 = ax == 1 ? c : c1;
    c2 = ax == 2 ? c : c2;
    t0 = ax == 0 ? t_new : t0;
    t1 = ax == 1 ? t_new : t1;
    t2 = ax == 2 ? t_new : t2;
  }
  if (trips) *trips = trip;
  return wall_column(B, 0, up0, c0, c1, c2);
}

}  // namespace gasbox
}  // namespace rthx

#if defined(__HIPCC__)
namespace rthx {
namespace gasbox {

// A launch of the walk: the uniform tracer's (Launch, whose beta is unused)
// and the field, Nv doubles in device memory in volume element order.
struct FieldLaunch {
  Launch L;
  const double* beta_v;
};

hipError_t launch_field(const FieldLaunch& F);

}  // namespace gasbox
}  // namespace rthx
#endif
