// rthx_transpose_kernels.hip -- stable CSR -> CSC transpose on the device
// (DESIGN.md §7h): F' for the sparse GERT operators (k_spmv, the banded
// spectral apply) and Julia's SparseMatrixCSC for the seam
// (rthx_result_copy_F_csc).
//
// The entries of a CSR block lie in row-major order, so a stable sort by
// column alone leaves every column's rows ascending and equal (row, column)
// pairs in their input order: the row never enters the key.  The sort is an
// LSD radix sort, 8 bits per pass, ceil(bits(n_cols - 1) / 8) passes (two for
// 256 < n_cols <= 65536).  A pass over tiles of 256 lanes x 16 rounds:
//  * k_tp_hist: the tile's histogram of the pass's digit in LDS (integer
//    atomics: sums, order-free), written digit-major to a 256 x n_tiles table;
//  * k_tp_scan_sum / k_tp_scan_top / k_tp_scan_apply: exclusive scan of the
//    table in three launches (block sums, one workgroup over the sums, the
//    blocks again) -- no workgroup waits on another;
//  * k_tp_scatter: the tile again in entry order.  An entry's place is
//    table[digit][tile] + its rank among the tile's earlier entries of that
//    digit: within a wave from 8 ballots on the digit's bits and mbcnt of
//    the peers below the lane, across the waves from per-wave digit counts
//    in LDS, across the rounds from a running per-digit offset.  No atomic
//    places an entry: the permutation is fixed, the result bit-reproducible.
//    The entries are staged in LDS in their new order, 2048 at a time, so
//    that a wave's stores cover a few runs of neighbours, not 64 places.
// The first pass reads the CSR block (an entry's row by a search of the row
// offsets, narrowed to the rows its tile touches), middle passes move
// (column, row, payload) records, and the last pass writes the final row
// index and value types and the sorted columns, from whose boundaries
// k_tp_offsets writes t_off.
//
// HBM traffic per entry, two passes, counts payload, int64 rows: 4 (hist) +
// 8 read + 12 written, then 4 (hist) + 12 read + 20 written (row 8, value 8,
// sorted column 4) + 4 (offsets) = 64 B.
//
// A column never indexes memory: a digit is masked to 8 bits before it
// indexes LDS, places come from the scan, and k_tp_offsets clamps a column
// to n_cols.  Built without fast-math: count / tallied is the correctly
// rounded quotient of rthx_result_copy_F.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_transpose.h"

namespace rthx {
namespace tp {

namespace {

constexpr int kWaves = kLanes / 64;
constexpr int kRowThreads = 256;    // k_tp_rows: one wave per row
constexpr int kTopThreads = 1024;   // one-workgroup scans (k_shard_scan's form)

// (column, row, payload) records between two passes
template <class P>
struct Rec {
  uint32_t* col;
  uint32_t* row;
  P* pay;
};

// last index r in [lo, hi] with off[r] <= e (off[lo] <= e holds)
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ off, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// Per-tile digit histogram.  CSR: the columns come from the CSR block.
template <bool CSR>
__global__ __launch_bounds__(kLanes) void k_tp_hist(Source S, const uint32_t* __restrict__ rcol, int shift,
                                                    int64_t n_tiles, int64_t* __restrict__ table) {
  __shared__ uint32_t hist[kDigits];
  const int tid = threadIdx.x;
  const int64_t tile = blockIdx.x;
  const int64_t e0 = tile * kTile;
  const int64_t e1 = e0 + kTile < S.nnz ? e0 + kTile : S.nnz;
  hist[tid] = 0;
  __syncthreads();
  int64_t lo = 0, hi = 0;
  if (CSR && !S.whole) {
    lo = row_of(S.off, 0, S.n_rows - 1, e0);
    hi = row_of(S.off, lo, S.n_rows - 1, e1 - 1);
  }
#pragma unroll 4
  for (int r = 0; r < kRounds; ++r) {
    const int64_t e = e0 + (int64_t)r * kLanes + tid;
    if (e < e1) {
      uint32_t c;
      if (!CSR) {
        c = rcol[e];
      } else if (S.whole) {
        c = S.cols[e];
      } else {
        const int64_t row = row_of(S.off, lo, hi, e);
        c = S.cols[S.src[row] + (e - S.off[row])];
      }
      atomicAdd(&hist[(c >> shift) & (kDigits - 1)], 1u);
    }
  }
  __syncthreads();
  table[(int64_t)tid * n_tiles + tile] = (int64_t)hist[tid];
}

// Exclusive scan of the table, part 1: sums[b] = sum of block b's words.
__global__ __launch_bounds__(kScanLanes) void k_tp_scan_sum(const int64_t* __restrict__ table, int64_t words,
                                                            int64_t* __restrict__ sums) {
  __shared__ int64_t part[kScanLanes / 64];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kScanBlock + (int64_t)tid * kScanPer;
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) s += i0 + k < words ? table[i0 + k] : 0;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t t = 0;
    for (int w = 0; w < kScanLanes / 64; ++w) t += part[w];
    sums[blockIdx.x] = t;
  }
}

// Part 2, one workgroup: v[0 .. n) -> its exclusive scan in place, v[n] = total.
__global__ __launch_bounds__(kTopThreads) void k_tp_scan_top(int64_t* __restrict__ v, int64_t n) {
  __shared__ int64_t part[kTopThreads];
  const int t = threadIdx.x;
  const int64_t per = (n + kTopThreads - 1) / kTopThreads;
  const int64_t g0 = t * per < n ? t * per : n;
  const int64_t g1 = g0 + per < n ? g0 + per : n;
  int64_t s = 0;
  for (int64_t g = g0; g < g1; ++g) s += v[g];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < kTopThreads; o <<= 1) {
    const int64_t x = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t g = g0; g < g1; ++g) {
    const int64_t x = v[g];
    v[g] = run;
    run += x;
  }
  if (t == kTopThreads - 1) v[n] = part[t];
}

// Part 3: every block scans its words from its sum's scan value.
__global__ __launch_bounds__(kScanLanes) void k_tp_scan_apply(int64_t* __restrict__ table, int64_t words,
                                                              const int64_t* __restrict__ sums) {
  __shared__ int64_t part[kScanLanes];
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kScanBlock + (int64_t)tid * kScanPer;
  int64_t x[kScanPer];
  int64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    x[k] = i0 + k < words ? table[i0 + k] : 0;
    s += x[k];
  }
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < kScanLanes; o <<= 1) {
    const int64_t y = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += y;
    __syncthreads();
  }
  int64_t run = sums[blockIdx.x] + part[tid] - s;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (i0 + k < words) table[i0 + k] = run;
    run += x[k];
  }
}

// The tile's entries to their places.  CSR: read from the CSR block, else
// from the records `in`; LAST: written as the final arrays, else as records.
// The tile goes in chunks of kChunkRounds rounds.  A chunk's entries are
// loaded into registers at once, counted per digit in LDS, ranked round by
// round as described above into a chunk-local order (by digit, then entry
// order), staged in LDS in that order, and written out from there: lanes
// next to each other then write next to each other, a digit's run at a time.
constexpr int kChunkRounds = 8;
constexpr int kChunk = kLanes * kChunkRounds;
static_assert(kRounds % kChunkRounds == 0, "a tile is a whole number of chunks");

template <class P, bool CSR, bool LAST>
__global__ __launch_bounds__(kLanes) void k_tp_scatter(Source S, Dest D, Rec<P> in, Rec<P> out,
                                                       uint32_t* __restrict__ scol, int shift, int64_t n_tiles,
                                                       const int64_t* __restrict__ table) {
  __shared__ int64_t gbase[kDigits];           // global place of the digit's first entry of this chunk
  __shared__ uint32_t lstart[kDigits];         // the digit's first place in the chunk-local order
  __shared__ uint32_t lnext[kDigits];          // chunk-local place of the digit's next entry
  __shared__ uint32_t scan[kDigits];           // the chunk's entries per digit, then their inclusive scan
  __shared__ uint32_t wcnt[kWaves][kDigits];   // the round's entries per wave and digit
  __shared__ uint32_t s_col[kChunk];
  __shared__ uint32_t s_row[kChunk];
  __shared__ P s_pay[kChunk];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t e0 = tile * kTile;
  const int64_t e1 = e0 + kTile < S.nnz ? e0 + kTile : S.nnz;
  gbase[tid] = table[(int64_t)tid * n_tiles + tile];
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wcnt[w][tid] = 0;
  int64_t lo = 0, hi = 0;
  if (CSR) {
    lo = row_of(S.off, 0, S.n_rows - 1, e0);
    hi = row_of(S.off, lo, S.n_rows - 1, e1 - 1);
  }
  for (int64_t c0 = e0; c0 < e1; c0 += kChunk) {  // (uniform over the workgroup)
    const int64_t c1 = c0 + kChunk < e1 ? c0 + kChunk : e1;
    const uint32_t n_chunk = (uint32_t)(c1 - c0);
    uint32_t col[kChunkRounds], row[kChunkRounds];
    P pay[kChunkRounds];
    scan[tid] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kChunkRounds; ++r) {
      const int64_t e = c0 + (int64_t)r * kLanes + tid;
      col[r] = 0;
      row[r] = 0;
      pay[r] = P(0);
      if (e < c1) {
        if (CSR) {
          const int64_t rr = row_of(S.off, lo, hi, e);
          const int64_t i = S.src[rr] + (e - S.off[rr]);
          row[r] = (uint32_t)rr;
          col[r] = S.cols[i];
          if constexpr (sizeof(P) == 8) pay[r] = S.vals[i];
          else pay[r] = S.counts[i];
        } else {
          col[r] = in.col[e];
          row[r] = in.row[e];
          pay[r] = in.pay[e];
        }
        atomicAdd(&scan[(col[r] >> shift) & (kDigits - 1)], 1u);  // (a count: order-free)
      }
    }
    __syncthreads();
    const uint32_t mine = scan[tid];
    __syncthreads();
    for (int o = 1; o < kDigits; o <<= 1) {  // inclusive scan of the chunk's digit counts
      const uint32_t v = tid >= o ? scan[tid - o] : 0u;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    lstart[tid] = scan[tid] - mine;
    lnext[tid] = scan[tid] - mine;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kChunkRounds; ++r) {
      const bool valid = c0 + (int64_t)r * kLanes + tid < c1;
      const uint32_t digit = (col[r] >> shift) & (kDigits - 1);
      // the wave's valid lanes of the same digit
      uint64_t peers = __ballot(valid);
#pragma unroll
      for (int b = 0; b < kDigitBits; ++b) {
        const bool bit = (digit >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
      }
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32),
                                                       __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
      if (valid && below == 0) wcnt[wave][digit] = (uint32_t)__popcll(peers);  // (the digit's first lane of the wave)
      __syncthreads();
      if (valid) {
        uint32_t q = lnext[digit] + below;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) q += w < wave ? wcnt[w][digit] : 0u;
        s_col[q] = col[r];  // (q < n_chunk: a place in the chunk's order)
        s_row[q] = row[r];
        s_pay[q] = pay[r];
      }
      __syncthreads();
      {  // lane d owns digit d: advance its place, clear its counts
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
          t += wcnt[w][tid];
          wcnt[w][tid] = 0;
        }
        lnext[tid] += t;
      }
      __syncthreads();
    }
    // the chunk in its local order: entry q of digit d goes to gbase[d] + (q - lstart[d])
#pragma unroll
    for (int k = 0; k < kChunkRounds; ++k) {
      const uint32_t q = (uint32_t)k * kLanes + tid;
      if (q < n_chunk) {
        const uint32_t c = s_col[q], rw = s_row[q];
        const P py = s_pay[q];
        const uint32_t digit = (c >> shift) & (kDigits - 1);
        const int64_t p = gbase[digit] + (int64_t)(q - lstart[digit]);
        if (LAST) {
          scol[p] = c;
          if (D.rows64) D.rows64[p] = D.begin + (int64_t)rw * D.stride + D.base;
          else D.rows32[p] = (int32_t)rw;
          if constexpr (sizeof(P) == 8) D.vals[p] = py;
          else D.vals[p] = (double)py / S.tallied[rw];  // (count / tallied: rthx_result_copy_F's quotient)
        } else {
          out.col[p] = c;
          out.row[p] = rw;
          out.pay[p] = py;
        }
      }
    }
    __syncthreads();
    gbase[tid] += mine;  // (read by every lane in the next chunk, after its first barrier)
  }
}

// t_off from the sorted columns: columns (prev, c] start at entry i, and the
// last entry closes the rest.  A column is clamped to
// n_cols before it bounds the loop.
__global__ __launch_bounds__(256) void k_tp_offsets(const uint32_t* __restrict__ scol, int64_t nnz, int64_t n_cols,
                                                    int64_t base, int64_t* __restrict__ t_off) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= nnz; i += (int64_t)gridDim.x * 256) {
    int64_t c = n_cols, prev = -1;
    if (i < nnz) {
      c = (int64_t)scol[i];
      c = c < n_cols ? c : n_cols - 1;
    }
    if (i > 0) {
      prev = (int64_t)scol[i - 1];
      prev = prev < n_cols ? prev : n_cols - 1;
    }
    for (int64_t q = prev + 1; q <= c; ++q) t_off[q] = i + base;
  }
}

// One wave per row of a trace result's counts: the row's tallied rays, its
// start, and the length of its prefix of columns < n_keep.
__global__ __launch_bounds__(kRowThreads) void k_tp_rows(const int64_t* __restrict__ row_off,
                                                         const uint32_t* __restrict__ cols,
                                                         const uint32_t* __restrict__ counts, int64_t n_rows,
                                                         int64_t n_keep, int64_t n_cols, double* __restrict__ tallied,
                                                         int64_t* __restrict__ src, int64_t* __restrict__ len) {
  const int64_t k = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  if (k >= n_rows) return;
  const int lane = threadIdx.x & 63;
  const int64_t first = row_off[0];
  const int64_t b = row_off[k] - first, e = row_off[k + 1] - first;
  uint64_t t = 0;
  for (int64_t i = b + lane; i < e; i += 64) t += counts[i];
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) {
    int64_t lo = b, hi = e;  // first entry with a column >= n_keep (columns ascend)
    if (n_keep < n_cols) {
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)cols[mid] < n_keep) lo = mid + 1;
        else hi = mid;
      }
    } else {
      lo = e;
    }
    tallied[k] = (double)t;
    src[k] = b;
    len[k] = lo - b;
  }
}

// One workgroup: off = exclusive scan of len (n + 1 words).
__global__ __launch_bounds__(kTopThreads) void k_tp_scan_rows(const int64_t* __restrict__ len, int64_t n,
                                                              int64_t* __restrict__ off) {
  __shared__ int64_t part[kTopThreads];
  const int t = threadIdx.x;
  const int64_t per = (n + kTopThreads - 1) / kTopThreads;
  const int64_t g0 = t * per < n ? t * per : n;
  const int64_t g1 = g0 + per < n ? g0 + per : n;
  int64_t s = 0;
  for (int64_t g = g0; g < g1; ++g) s += len[g];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < kTopThreads; o <<= 1) {
    const int64_t x = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t g = g0; g < g1; ++g) {
    off[g] = run;
    run += len[g];
  }
  if (t == kTopThreads - 1) off[n] = part[t];
}

template <class P>
hipError_t run_passes(const Source& S, const Dest& D, const Plan& P_, char* scratch, hipStream_t st) {
  int64_t* table = reinterpret_cast<int64_t*>(scratch + P_.off_table);
  int64_t* sums = reinterpret_cast<int64_t*>(scratch + P_.off_sums);
  uint32_t* scol = reinterpret_cast<uint32_t*>(scratch + P_.off_scol);
  Rec<P> buf[2];
  for (int b = 0; b < 2; ++b) {
    buf[b].col = reinterpret_cast<uint32_t*>(scratch + P_.off_col[b]);
    buf[b].row = reinterpret_cast<uint32_t*>(scratch + P_.off_row[b]);
    buf[b].pay = reinterpret_cast<P*>(scratch + P_.off_pay[b]);
  }
  const dim3 tiles((unsigned)P_.n_tiles), lanes(kLanes);
  const dim3 sblocks((unsigned)P_.scan_blocks), slanes(kScanLanes);
  for (int k = 0; k < P_.passes; ++k) {
    const bool first = k == 0, last = k == P_.passes - 1;
    const Rec<P> in = first ? Rec<P>{nullptr, nullptr, nullptr} : buf[(k - 1) & 1];
    const Rec<P> out = last ? Rec<P>{nullptr, nullptr, nullptr} : buf[k & 1];
    const int shift = P_.shift[k];
    if (first) hipLaunchKernelGGL(k_tp_hist<true>, tiles, lanes, 0, st, S, nullptr, shift, P_.n_tiles, table);
    else hipLaunchKernelGGL(k_tp_hist<false>, tiles, lanes, 0, st, S, in.col, shift, P_.n_tiles, table);
    hipLaunchKernelGGL(k_tp_scan_sum, sblocks, slanes, 0, st, table, P_.table_words, sums);
    hipLaunchKernelGGL(k_tp_scan_top, dim3(1), dim3(kTopThreads), 0, st, sums, P_.scan_blocks);
    hipLaunchKernelGGL(k_tp_scan_apply, sblocks, slanes, 0, st, table, P_.table_words, sums);
    if (first && last)
      hipLaunchKernelGGL((k_tp_scatter<P, true, true>), tiles, lanes, 0, st, S, D, in, out, scol, shift, P_.n_tiles, table);
    else if (first)
      hipLaunchKernelGGL((k_tp_scatter<P, true, false>), tiles, lanes, 0, st, S, D, in, out, scol, shift, P_.n_tiles, table);
    else if (last)
      hipLaunchKernelGGL((k_tp_scatter<P, false, true>), tiles, lanes, 0, st, S, D, in, out, scol, shift, P_.n_tiles, table);
    else
      hipLaunchKernelGGL((k_tp_scatter<P, false, false>), tiles, lanes, 0, st, S, D, in, out, scol, shift, P_.n_tiles, table);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t transpose(const Source& S, const Dest& D, const Plan& P, void* scratch, hipStream_t st) {
  char* sc = static_cast<char*>(scratch);
  if (S.nnz > 0) {
    const hipError_t e = S.counts ? run_passes<uint32_t>(S, D, P, sc, st) : run_passes<double>(S, D, P, sc, st);
    if (e != hipSuccess) return e;
  }
  const int64_t work = S.nnz + 1;
  const unsigned grid = (unsigned)(work < 65536 * 256 ? (work + 255) / 256 : 65536);
  hipLaunchKernelGGL(k_tp_offsets, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(sc + P.off_scol),
                     S.nnz, S.n_cols, D.base, D.t_off);
  return hipGetLastError();
}

hipError_t block_rows(const int64_t* row_off, const uint32_t* cols, const uint32_t* counts, int64_t n_rows,
                      int64_t n_keep, int64_t n_cols, double* tallied, int64_t* src, int64_t* len, int64_t* off,
                      hipStream_t st) {
  if (n_rows > 0) {
    const int64_t blocks = (n_rows + kRowThreads / 64 - 1) / (kRowThreads / 64);
    hipLaunchKernelGGL(k_tp_rows, dim3((unsigned)blocks), dim3(kRowThreads), 0, st, row_off, cols, counts, n_rows,
                       n_keep, n_cols, tallied, src, len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tp_scan_rows, dim3(1), dim3(kTopThreads), 0, st, len, n_rows, off);
  return hipGetLastError();
}

}  // namespace tp
}  // namespace rthx
