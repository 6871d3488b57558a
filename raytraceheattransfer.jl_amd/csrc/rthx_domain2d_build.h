// rthx_domain2d_build.h -- the 2D tracer's host-side domain build
// (rthx_domain2d_build.cpp): the flattened descriptor in, every array the
// device domain is made of beyond the descriptor's own out, with the choice
// of the tracer's fast paths (SINGLE, AXIS, CLDS, MLAT, LAT).  No HIP, no
// environment, no global error state: the C ABI (rthx_api.cpp
// rthx_domain_create) reads the knobs, calls build_domain2d and uploads the
// result; tests/domain2d_host_check.cpp calls it on the host and checks the
// result by brute force.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rthx.h"
#include "rthx_domain2d.h"
#include "rthx_grid.h"

namespace rthx {

// What the environment's knobs set (rthx_domain_create reads them).
struct Domain2dOptions {
  bool no_mlat = false;         // RTHX_NO_MLAT=1: never the multi-polygon lattice
  bool no_lat = false;          // RTHX_NO_LAT=1: never the single-rectangle lattice
  double lat_guess_scale = 0;   // RTHX_LAT_GUESS_SCALE: the LAT first guess scaled (0, or not finite and positive: as it is)
};

// The blobs are the LDS blocks as the kernels stage them (rthx_domain2d.h
// CoarseLayout, MLatLayout, LatticeLayout): bytes, a multiple of 16 of them,
// empty when the layout's `bytes` is 0.
struct Domain2dBuild {
  std::vector<DevPoly> cpoly, fpoly;     // padded to 4 slots
  std::vector<uint32_t> csolid;          // [n_coarse] bit w = coarse wall w solid
  std::vector<double> trifrac;           // [n_fine] area(ABC)/V of quads, 0 for triangles
  std::vector<int32_t> fcoarse;          // [n_fine] inverse of fine_offset
  std::vector<int32_t> s_face, s_wall;   // [n_surfaces] inverse of fine_surface
  bool single_convex = false;            // one convex coarse polygon (SINGLE kernels)
  bool axis_rect = false;                // every polygon an axis-aligned rectangle in canonical order (AXIS kernels)
  // point-location grids: the coarse one first, then one per coarse polygon
  DevGrid c_grid{};
  std::vector<DevGrid> fgrids;
  std::vector<CellRec> gcells;
  std::vector<int32_t> glists, gitems;   // (gitems: never empty)
  // per bin a kLdsTableDoubles block: the tables, then 1 / beta_first (+inf when beta_first <= 0)
  std::vector<double> tables;
  std::vector<double> beta_first;        // beta of fine face 0 per bin
  CoarseLayout cl{};                     // (offsets filled even when not staged)
  std::vector<unsigned char> c_blob;
  std::vector<double> c_beta;            // [n_bins][n_coarse] (n_coarse >= 2) the beta the coarse polygon's fine ones share, else -1
  MLatLayout ml{};
  std::vector<unsigned char> ml_blob;
  std::vector<double> ml_bbeta;          // [n_bins][n_coarse] c_beta by lattice box
  std::vector<uint8_t> ml_mixed;         // per bin, 1 if some box has no single beta
  LatticeLayout lat{};
  std::vector<unsigned char> lat_blob;
  std::vector<int32_t> lat_map;          // [nx ny] when !lat.identity
};

// Validates the descriptor and builds the domain.  Returns RTHX_OK, or an
// RTHX_E* code with its message in `err`.
int build_domain2d(const rthx_domain_desc& s, const Domain2dOptions& opt, Domain2dBuild& out, std::string& err);

// rthx_domain_set_mirror_walls: the coarse polygons' mirror masks (bit w =
// wall w reflects) from the caller's flags mirror[n_coarse * 4] (nullptr:
// none), and the number n of walls the caller flagged.  A flagged wall
// between two coarse polygons reflects from both sides: the neighbour's wall
// with the same two end points takes the flag too (unless it is solid, where
// the ray ends anyway).
int mirror_masks(const std::vector<int32_t>& c_nv, const std::vector<double>& c_xy,
                 const std::vector<uint32_t>& c_solid, const uint8_t* mirror, std::vector<uint32_t>& mask, int64_t& n,
                 std::string& err);

// The device lookup tables (rthx_domain2d.h kTableDoubles doubles):
// cos/sin(2 pi j/256) for cos_2pi_u32, and for neg_log_tab per entry i the
// centre c of its z interval, invc = fl(1/c) and ln(invc) split into hi + lo,
// evaluated in long double.
void fill_tables(double* t);

}  // namespace rthx
