// Checks plan_transpose (csrc/rthx_transpose_plan.h), the host-side planning
// of the device CSR -> CSC transpose: the radix passes cover the column bits
// and no more, the tiles tile [0, nnz) exactly, and the scan-table and
// scratch sizes are consistent.  Built for the host with ASan + UBSan by
// tests/test_transpose_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rthx_transpose_plan.h"

using namespace rthx::tp;

static long g_cases = 0;

#define CHECK(cond)                                                                             \
  do {                                                                                          \
    if (!(cond)) {                                                                              \
      std::printf("FAILED %s (n_cols %lld, nnz %lld)\n", #cond, (long long)n_cols, (long long)nnz); \
      std::exit(1);                                                                             \
    }                                                                                           \
  } while (0)

static void check(int64_t n_cols, int64_t nnz, int payload) {
  const Plan p = plan_transpose(n_cols, nnz, payload);
  ++g_cases;
  // the passes' digits cover every bit of the largest column, and the last
  // pass is needed (one pass at least: it is also what moves the entries)
  const int64_t top = n_cols - 1;
  CHECK(p.passes >= 1 && p.passes <= kMaxPasses);
  CHECK(top >> (kDigitBits * p.passes) == 0);
  CHECK(p.passes == 1 || (top >> (kDigitBits * (p.passes - 1))) != 0);
  for (int k = 0; k < p.passes; ++k) CHECK(p.shift[k] == k * kDigitBits);
  // a column is rebuilt from its digits
  for (int64_t c : {int64_t(0), top / 2, top}) {
    int64_t back = 0;
    for (int k = 0; k < p.passes; ++k) back |= ((c >> p.shift[k]) & (kDigits - 1)) << p.shift[k];
    CHECK(back == c);
  }
  // tiles: [t * kTile, min((t + 1) * kTile, nnz)) are non-empty and cover [0, nnz)
  CHECK(kTile == (int64_t)kLanes * kRounds);
  CHECK(p.n_tiles * kTile >= nnz);
  CHECK(p.n_tiles == 0 ? nnz == 0 : (p.n_tiles - 1) * kTile < nnz);
  int64_t covered = 0;
  for (int64_t t = 0; t < p.n_tiles && t < 8; ++t) {
    const int64_t e0 = t * kTile, e1 = e0 + kTile < nnz ? e0 + kTile : nnz;
    CHECK(e0 == covered && e1 > e0);
    covered = e1;
  }
  if (p.n_tiles <= 8) CHECK(covered == nnz);
  // table and its scan blocks
  CHECK(p.table_words == p.n_tiles * kDigits);
  CHECK(p.scan_blocks * kScanBlock >= p.table_words);
  CHECK(p.scan_blocks == 0 ? p.table_words == 0 : (p.scan_blocks - 1) * kScanBlock < p.table_words);
  // scratch parts: aligned, in order, disjoint, inside scratch_bytes
  struct Part {
    int64_t off, bytes;
  };
  std::vector<Part> parts = {{p.off_table, p.table_words * 8}, {p.off_sums, (p.scan_blocks + 1) * 8},
                             {p.off_scol, nnz * 4}};
  for (int b = 0; b < 2; ++b) {
    const bool used = p.passes > b + 1;
    parts.push_back({p.off_col[b], used ? nnz * 4 : 0});
    parts.push_back({p.off_row[b], used ? nnz * 4 : 0});
    parts.push_back({p.off_pay[b], used ? nnz * payload : 0});
  }
  int64_t end = 0;
  for (const Part& q : parts) {
    CHECK(q.off % kAlign == 0);
    CHECK(q.off >= end);
    end = q.off + q.bytes;
  }
  CHECK(end <= p.scratch_bytes);
  CHECK(p.scratch_bytes % kAlign == 0);
}

int main() {
  const int64_t T = kTile;
  const int64_t nnzs[] = {0, 1, T - 1, T, T + 1, 3 * T + 5};
  for (int64_t n_cols = 1; n_cols <= 70000; ++n_cols)
    for (int payload : {4, 8}) check(n_cols, (n_cols * 37) % (5 * T), payload);
  for (int64_t n_cols : {int64_t(1), int64_t(255), int64_t(256), int64_t(257), int64_t(65536), int64_t(65537),
                         int64_t(1) << 24, (int64_t(1) << 24) + 1, (int64_t(1) << 31) - 1})
    for (int64_t nnz : nnzs)
      for (int payload : {4, 8}) check(n_cols, nnz, payload);
  // the pass counts at the edges, spelled out
  const int64_t nnz = 0, n_cols = 0;
  CHECK(plan_transpose(1, 0, 8).passes == 1);
  CHECK(plan_transpose(256, 0, 8).passes == 1);
  CHECK(plan_transpose(257, 0, 8).passes == 2);
  CHECK(plan_transpose(65536, 0, 8).passes == 2);
  CHECK(plan_transpose(65537, 0, 8).passes == 3);
  CHECK(plan_transpose(10605, 0, 4).passes == 2 && plan_transpose(41205, 0, 4).passes == 2);
  std::printf("transpose plan ok: %ld cases\n", g_cases);
  return 0;
}
