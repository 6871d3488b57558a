// rthx_domain2d.h — the records of the flattened 2D domain that the host
// builds and the kernels read (DESIGN.md "Data layout in HBM"): grids,
// polygons, cells, the three LDS layouts and the lookup tables' sizes.  Plain
// C++, no HIP: rthx_device.h includes it for the kernels (DevDomain, which
// holds the device pointers, stays there), rthx_domain2d_build.h for the host
// builder and its stand-alone check.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rthx {

struct DevGrid {
  double ox, oy;        // origin
  double inv_x, inv_y;  // 1/cell size in x and y
  int32_t nx, ny;
  int32_t cell_base;    // offset of this grid's cells in grid_cells (and grid_lists / 2)
  int32_t reserved;
};

// Polygon record (128 B): vertices and unit inward normals
// (calculateInwardNormal.jl:1-12), always 4 slots.  A triangle repeats its
// last vertex in slot 3 and has a zero normal there, so every loop below runs
// over 4 edges without a vertex-count test: the repeated vertex adds a
// horizontal zero-length edge that never crosses (point in polygon), and the
// zero normal gives |d.n| = 0 < 1e-10, which distToSurface2D treats as
// parallel (no hit).
struct alignas(16) DevPoly {
  double x[4], y[4];
  double nx[4], ny[4];
};

// Point-location cell record (built by rthx_grid.cpp, layout = CellRec):
// code = (a0 x + b0 y + c0 < 0) | (a1 x + b1 y + c1 < 0) << 1 selects leaf[code]:
// >= 0 polygon, -1 outside all polygons, -2 test the cell's candidate list.
struct alignas(16) DevCell {
  double a0, b0, c0;
  double a1, b1, c1;
  int32_t leaf[4];
};

constexpr int kCosTable = 256;  // cos/sin(2 pi j / 256), j < 256
constexpr int kLogTable = 128;  // neg_log_tab entries
constexpr int kLogTableOffset = 2 * kCosTable;
constexpr int kTableDoubles = kLogTableOffset + 4 * kLogTable;
// The kernels' LDS copy of the tables holds one more double: the launch's
// TraceParams::inv_beta_uniform, which the free path reads at its point of
// use (a kernel-argument double kept live across the ray loop is spilled
// with the SGPRs loaded beside it and reloaded by v_readlane every ray).
constexpr int kTabInvBeta = kTableDoubles;
constexpr int kLdsTableDoubles = kTableDoubles + 1;
// neg_log_tab (rthx_device.h): table entry i covers the z interval that
// starts at the double with bits kLogOff + (i << 45).
constexpr uint64_t kLogOff = 0x3FE6000000000000ull;  // bits of 0.6875

constexpr size_t kMaxCoarseLdsBytes = 48 * 1024; // largest coarse mesh the CLDS kernels stage in LDS

// Byte layout of the coarse mesh as multi-polygon trace kernels stage it in
// LDS (CLDS kernels): DevPoly records at 0, then fine grids,
// bounding boxes, fine-polygon offsets, solid-wall masks, the coarse grid's
// cell records and one beta per coarse polygon for the traced bin.  Every
// offset is a multiple of 16.  bytes == 0: not staged (too large).
struct CoarseLayout {
  int32_t bytes;      // whole LDS block, beta included
  int32_t blob_bytes; // copied from c_blob (everything before beta)
  int32_t off_fgrid, off_bbox, off_first, off_solid, off_cells, off_beta;
};

// Lattice form of a single axis-aligned coarse rectangle whose fine cells
// are the nx x ny rectangles [xs[i], xs[i+1]) x [ys[j], ys[j+1]) (meshQuad
// on a rectangle, meshQuad.jl:139-179).  LAT kernels stage the blob in LDS:
// xs[nx+1], ys[ny+1] (f64; every interior fine wall is open, the boundary
// walls' surface indices come from f_surf).  Fine cell (i, j) is polygon
// j nx + i when `identity`, else lat_map[j nx + i].  bytes == 0: not a
// lattice.
constexpr int kLatMaxDim = 4096;  // most boxes a side (host: no lattice beyond it); cell indices then fit 24-bit multiplies
struct LatticeLayout {
  int32_t bytes;             // blob bytes (multiple of 16)
  int32_t nx, ny;
  int32_t identity;
  int32_t off_ys;
  int32_t reserved[5];
  double inv_x, inv_y;       // nx / (xs[nx] - xs[0]), ny / (ys[ny] - ys[0]): first guess of the cell
};

// Lattice form of a multi-polygon domain (MLAT kernels): the coarse polygons
// are the ncx x ncy boxes of a coarse lattice (cxs, cys) and the fine
// polygons of every coarse box are the boxes of one global fine lattice (xs,
// ys) inside it, x fastest (meshQuad.jl:139-179) -- a layered medium such as
// the greenhouse (67 layers of 201 x 3 cells: one 201 x 201 lattice).  Blob:
// xs[nx+1], ys[ny+1], cxs[ncx+1], cys[ncy+1] (f64), cmap[ncy ncx] (i32:
// coarse polygon of box b = cj ncx + ci), MCoarse[n_coarse], bsolid[nbox]
// (u32: solid walls of box b), then (staged per bin from ml_bbeta) one beta
// per box (-1 when the fine betas of its polygon differ).
struct MCoarse {
  int32_t first;     // first fine polygon
  int32_t i0, j0;    // its fine lattice box
  int32_t nxf, nyf;  // fine boxes per row / column
  int32_t ci, cj;    // coarse lattice box
  uint32_t solid;    // bit w: coarse wall w solid
};

struct MLatLayout {
  int32_t bytes;       // LDS block incl. the betas (0: not a lattice)
  int32_t blob_bytes;  // staged from ml_blob
  int32_t nx, ny, ncx, ncy;
  int32_t off_ys, off_cxs, off_cys, off_cmap, off_cinfo, off_bsolid, off_beta;
  int32_t off_lay;     // one coarse column (ncx == 1): LayerRec[ncy + 2] (a sentinel, the layers, a sentinel) staged per bin after the betas; else 0
  double inv_x, inv_y, inv_cx, inv_cy;  // first guesses of lattice_index
};

// One layer of a one-column lattice as walk_layers reads it: its bounds,
// this bin's beta and its solid walls in one 32-byte LDS record (two
// ds_read_b128 per segment).
struct alignas(16) LayerRec {
  double y0, y1;
  double beta;     // -1: the fine betas of the layer differ (MIXED)
  uint32_t solid;  // bit w: wall w solid
  uint32_t pad;
};

}  // namespace rthx
