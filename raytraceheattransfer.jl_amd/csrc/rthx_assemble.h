// rthx_assemble.h -- launcher of the row-shard merge kernels
// (rthx_assemble_kernels.hip), driven by rthx_assemble.cpp
// (rthx_merge_row_shards).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rthx {
namespace asmb {

constexpr int kMaxShards = 64;

// W CSR blocks of an n_rows-row matrix: block k holds rows k, k + W, ...
// (row_off local to the block: n_k + 1 entries, n_k = ceil((n_rows - k) / W)).
// Passed by value as the kernels' argument (3 x 64 pointers).
struct ShardSet {
  const int64_t* row_off[kMaxShards];
  const uint32_t* cols[kMaxShards];
  const uint32_t* counts[kMaxShards];
  int64_t n_rows;
  int32_t n_shards;
};

// row_ptr (n_rows + 1), cols and counts of the merged CSR, enqueued on st.
hipError_t merge_row_shards(const ShardSet& S, int64_t* row_ptr, uint32_t* cols, uint32_t* counts, hipStream_t st);

// Sum of two count matrices over the same rows (rthx_result_accumulate):
// A (the result) and B (the added block) as CSR with column-ascending rows;
// the sum has a row's columns merged, equal columns adding their counts.
struct AccJob {
  int64_t n_rows, n_cols;
  const int64_t* a_off;
  const uint32_t* a_cols;
  const uint32_t* a_cnt;
  const int64_t* b_off;
  const uint32_t* b_cols;
  const uint32_t* b_cnt;
  int64_t rays;  // rays per row of the sum (lost rays of a row: rays - its counts' sum)
  int32_t wide;  // 1: one 256-lane workgroup per row (long rows), 0: one wave per row
};
// Totals words of an accumulate: nnz of the sum, lost rays, max lost rays of
// one row, and entries of B that break its layout (a row of negative length,
// a column >= n_cols).
constexpr int kAccTotals = 4;
// Pass 1: mark[k] (over B's entries) = entries before k in its row that match
// a column of A's row; len[row] = the merged row's length.  Pass 2: off =
// exclusive scan of len (n_rows + 1), totals[0] = nnz.
hipError_t acc_lengths(const AccJob& J, uint32_t* mark, int64_t* len, int64_t* off, unsigned long long* totals,
                       hipStream_t st);
// Pass 3: the merged rows into cols / cnt at off, tallied[row] = the row's
// counts' sum, totals[1..2] = lost rays and their maximum over the rows.
hipError_t acc_write(const AccJob& J, const uint32_t* mark, const int64_t* off, uint32_t* cols, uint32_t* cnt,
                     uint32_t* tallied, unsigned long long* totals, hipStream_t st);

// Binomial sampling error of count / tallied (rthx_result_sampling_error):
// s[row] = (1 - sum_j p_j^2) / n with n the row's counts' sum and
// p_j = count_j / n (0 where n = 0); out[0] = sum of s, out[1] = max of s.
hipError_t sampling_error(const int64_t* row_off, const uint32_t* cnt, int64_t n_rows, double* s, double* out,
                          hipStream_t st);

}  // namespace asmb
}  // namespace rthx
