// rthx_transpose_plan.h -- host-only planning of the device CSR -> CSC
// transpose (rthx_transpose_kernels.hip): from the number of
// columns and entries, the radix passes and their digit shifts, the tiling of
// the entries, and the layout of the scratch block.  Used by the launcher
// (rthx_transpose.cpp) and by a CPU test (tests/transpose_plan_check.cpp);
// no HIP in here.
#pragma once

#include <stdint.h>

namespace rthx {
namespace tp {

constexpr int kDigitBits = 8;
constexpr int kDigits = 1 << kDigitBits;  // bins per pass
constexpr int kLanes = 256;               // lanes of a tile's workgroup (one entry each per round)
constexpr int kRounds = 16;               // rounds per tile
constexpr int64_t kTile = (int64_t)kLanes * kRounds;
constexpr int kMaxPasses = 4;             // n_cols < 2^31
constexpr int kScanLanes = 256;           // the table scan: lanes per block ...
constexpr int kScanPer = 8;               // ... and words per lane
constexpr int64_t kScanBlock = (int64_t)kScanLanes * kScanPer;
constexpr int64_t kAlign = 256;           // alignment of the scratch parts

struct Plan {
  int64_t n_cols = 0, nnz = 0;
  int key_bits = 0;            // bits that hold 0 .. n_cols - 1 (0 for one column)
  int passes = 1;              // at least one: a pass is also what moves the entries
  int shift[kMaxPasses] = {0, 0, 0, 0};
  int64_t n_tiles = 0;         // tiles of kTile entries, the last one partial
  int64_t table_words = 0;     // kDigits x n_tiles, digit-major (int64 words)
  int64_t scan_blocks = 0;     // blocks of kScanBlock table words
  int payload_bytes = 8;       // 8: double values, 4: uint32 counts
  // byte offsets into the scratch block (each a multiple of kAlign)
  int64_t off_table = 0, off_sums = 0, off_scol = 0;
  int64_t off_col[2] = {0, 0}, off_row[2] = {0, 0}, off_pay[2] = {0, 0};  // record buffers (passes > 1 / > 2)
  int64_t scratch_bytes = 0;
};

inline int key_bits_for(int64_t n_cols) {  // bits of n_cols - 1
  int b = 0;
  while (b < 62 && (int64_t(1) << b) < n_cols) ++b;
  return b;
}

inline int64_t align_up(int64_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

// n_cols >= 1 (0 is planned like 1), 0 <= nnz < 2^31.
inline Plan plan_transpose(int64_t n_cols, int64_t nnz, int payload_bytes) {
  Plan p;
  p.n_cols = n_cols;
  p.nnz = nnz;
  p.payload_bytes = payload_bytes;
  p.key_bits = key_bits_for(n_cols < 1 ? 1 : n_cols);
  p.passes = (p.key_bits + kDigitBits - 1) / kDigitBits;
  if (p.passes < 1) p.passes = 1;
  for (int k = 0; k < kMaxPasses; ++k) p.shift[k] = k * kDigitBits;
  p.n_tiles = (nnz + kTile - 1) / kTile;
  p.table_words = p.n_tiles * kDigits;
  p.scan_blocks = (p.table_words + kScanBlock - 1) / kScanBlock;
  int64_t at = 0;
  auto take = [&at](int64_t bytes) {
    const int64_t o = at;
    at += align_up(bytes < 1 ? 1 : bytes);
    return o;
  };
  p.off_table = take(p.table_words * 8);
  p.off_sums = take((p.scan_blocks + 1) * 8);
  p.off_scol = take(nnz * 4);
  for (int b = 0; b < 2; ++b) {
    const bool used = p.passes > b + 1;
    p.off_col[b] = take(used ? nnz * 4 : 0);
    p.off_row[b] = take(used ? nnz * 4 : 0);
    p.off_pay[b] = take(used ? nnz * payload_bytes : 0);
  }
  p.scratch_bytes = at;
  return p;
}

}  // namespace tp
}  // namespace rthx
