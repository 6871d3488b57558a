// rthx_assemble_kernels.hip -- assembly of a row-sharded count matrix on one
// device (BASELINE config C5 over W GPUs: every rank traces the rows
// g = k, k + W, k + 2W, ... of a band and the band's owner merges the W
// blocks).  This replaces, for blocks that come from several GPUs, the
// reference's merge of its per-thread COO triplets into one sparse matrix
// (parallelRayTracing.jl:128-145).
//
// Two passes, both HBM-bound copies with no arithmetic to speak of:
//  * k_shard_scan: one workgroup; row g's length is read from its block's
//    offsets, each lane sums a contiguous run of rows, an LDS scan over the
//    lanes gives every run its start, and the lanes write row_ptr.  Reads
//    8 B and writes 8 B per row (a C5 band: 41,205 rows, ~0.7 MB).
//  * k_shard_copy: one workgroup per row (grid-stride), copying the row's
//    (column, count) pairs from its block to their place in the merged CSR;
//    16 B of HBM traffic per nonzero (8 read + 8 written) -- a transparent C5
//    band: 221 M nonzeros, 3.5 GB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_assemble.h"

namespace rthx {
namespace asmb {

constexpr int kScanThreads = 1024;
constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;  // independent loads in flight per lane

__device__ __forceinline__ int64_t row_len(const ShardSet& S, int64_t g, int64_t* src) {
  const int k = (int)(g % S.n_shards);
  const int64_t i = g / S.n_shards;
  const int64_t a = S.row_off[k][i];
  *src = a;
  return S.row_off[k][i + 1] - a;
}

__global__ __launch_bounds__(kScanThreads) void k_shard_scan(ShardSet S, int64_t* __restrict__ row_ptr) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t n = S.n_rows;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t g0 = t * per < n ? t * per : n;
  const int64_t g1 = g0 + per < n ? g0 + per : n;
  int64_t s = 0, src;
  for (int64_t g = g0; g < g1; ++g) s += row_len(S, g, &src);
  part[t] = s;
  __syncthreads();
  // Hillis-Steele inclusive scan over the lanes' sums (1024 entries, 10 steps)
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int64_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;  // exclusive start of this lane's rows
  for (int64_t g = g0; g < g1; ++g) {
    row_ptr[g] = run;
    run += row_len(S, g, &src);
  }
  if (t == kScanThreads - 1) row_ptr[n] = part[t];
}

__global__ __launch_bounds__(kCopyThreads) void k_shard_copy(ShardSet S, const int64_t* __restrict__ row_ptr,
                                                             uint32_t* __restrict__ cols,
                                                             uint32_t* __restrict__ counts) {
  for (int64_t g = blockIdx.x; g < S.n_rows; g += gridDim.x) {
    int64_t src;
    const int64_t len = row_len(S, g, &src);
    const int k = (int)(g % S.n_shards);
    const uint32_t* __restrict__ sc = S.cols[k] + src;
    const uint32_t* __restrict__ sn = S.counts[k] + src;
    uint32_t* __restrict__ dc = cols + row_ptr[g];
    uint32_t* __restrict__ dn = counts + row_ptr[g];
    int64_t j = threadIdx.x;
    for (; j + (kCopyUnroll - 1) * kCopyThreads < len; j += kCopyUnroll * kCopyThreads) {
      uint32_t c[kCopyUnroll], v[kCopyUnroll];
#pragma unroll
      for (int u = 0; u < kCopyUnroll; ++u) {
        c[u] = __builtin_nontemporal_load(sc + j + u * kCopyThreads);
        v[u] = __builtin_nontemporal_load(sn + j + u * kCopyThreads);
      }
#pragma unroll
      for (int u = 0; u < kCopyUnroll; ++u) {
        dc[j + u * kCopyThreads] = c[u];
        dn[j + u * kCopyThreads] = v[u];
      }
    }
    for (; j < len; j += kCopyThreads) {
      dc[j] = sc[j];
      dn[j] = sn[j];
    }
  }
}

hipError_t merge_row_shards(const ShardSet& S, int64_t* row_ptr, uint32_t* cols, uint32_t* counts,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_shard_scan, dim3(1), dim3(kScanThreads), 0, st, S, row_ptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || S.n_rows == 0) return e;
  // one workgroup per row up to 64 per CU's worth of rows (grid-stride beyond)
  const int64_t grid = S.n_rows < 16384 ? S.n_rows : 16384;
  hipLaunchKernelGGL(k_shard_copy, dim3((unsigned)grid), dim3(kCopyThreads), 0, st, S, row_ptr, cols, counts);
  return hipGetLastError();
}

}  // namespace asmb
}  // namespace rthx

// ---------------------------------------------------------------------------
// Sum of two count matrices (rthx_result_accumulate): a progressive trace
// adds the counts of its next ray range to what it holds, and a ray-sharded
// trace's owner folds the W blocks of its gather.  Per row two
// column-ascending lists are merged, equal columns adding their counts.
//
// An entry's place in the merged row follows from ranks alone: with r the
// number of B's columns below an A entry's column (binary search in B's row)
// and m the number of those that match a column of A, A's entry j lands at
// j + r - m; an unmatched B entry k with m matches before it and r columns of
// A below its own lands at k - m + r (a matched one adds its count to A's
// entry).  m is a prefix count over B's row:
//  * k_acc_mark: a group of G lanes (one wave, or one 256-lane workgroup for
//    long rows) walks B's row G entries at a time; each lane looks its column
//    up in A's row, and a ballot scan with a running carry gives mark[k].
//    The row's merged length is lenA + lenB - matches.
//  * k_acc_scan: one workgroup scans the lengths into row offsets
//    (k_shard_scan's form).
//  * k_acc_write: every entry of A and every unmatched entry of B computes
//    its place and is written once; the row's counts' sum goes to tallied.
//  * k_acc_lost: lost rays per row from tallied, their sum and maximum.
// HBM traffic per call: A and B read twice (columns in pass 1, columns and
// counts in pass 3; the binary searches hit rows that are in L2), 4 B of mark
// written and read per B entry, and the sum written once.
// ---------------------------------------------------------------------------
namespace rthx {
namespace asmb {

constexpr int kAccThreads = 256;

// first index in c[0, n) whose column is >= key
__device__ __forceinline__ int64_t acc_lower_bound(const uint32_t* __restrict__ c, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Rows of the launch: group `grp` of G lanes takes rows grp, grp + n_grp, ...
template <int G>
__global__ __launch_bounds__(kAccThreads) void k_acc_mark(AccJob J, uint32_t* __restrict__ mark,
                                                          int64_t* __restrict__ len,
                                                          unsigned long long* __restrict__ totals) {
  __shared__ uint32_t wave_m[kAccThreads / 64];
  constexpr int per_block = kAccThreads / G;
  const int tid = threadIdx.x;
  const int gl = tid % G;  // lane of the group
  const int lane = tid & 63, wave = tid >> 6;
  const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t row = (int64_t)blockIdx.x * per_block + tid / G; row < J.n_rows; row += (int64_t)gridDim.x * per_block) {
    const int64_t a0 = J.a_off[row], la = J.a_off[row + 1] - a0;
    const int64_t b0 = J.b_off[row];
    int64_t lb = J.b_off[row + 1] - b0;
    bool bad = lb < 0 || b0 < 0;
    if (bad) lb = 0;
    const uint32_t* __restrict__ ac = J.a_cols + a0;
    const uint32_t* __restrict__ bc = J.b_cols + b0;
    uint32_t carry = 0;
    for (int64_t t0 = 0; t0 < lb; t0 += G) {  // (uniform over the group: a workgroup's barriers below)
      const int64_t k = t0 + gl;
      bool m = false;
      if (k < lb) {
        const uint32_t c = bc[k];
        if ((int64_t)c >= J.n_cols) bad = true;
        const int64_t r = acc_lower_bound(ac, la, c);
        m = r < la && ac[r] == c;
      }
      const uint64_t b = __ballot(m);
      uint32_t excl = (uint32_t)__popcll(b & lt_mask), total = (uint32_t)__popcll(b);
      if (G > 64) {
        if (lane == 0) wave_m[wave] = total;
        __syncthreads();
        total = 0;
        for (int w = 0; w < G / 64; ++w) {
          const uint32_t s = wave_m[w];
          excl += w < wave ? s : 0u;
          total += s;
        }
        __syncthreads();
      }
      if (k < lb) mark[b0 + k] = carry + excl;
      carry += total;
    }
    if (gl == 0) len[row] = la + lb - (int64_t)carry;
    if (__ballot(bad) != 0ull && lane == 0) atomicAdd(&totals[3], 1ull);
  }
}

__global__ __launch_bounds__(kScanThreads) void k_acc_scan(const int64_t* __restrict__ len, int64_t n,
                                                           int64_t* __restrict__ off,
                                                           unsigned long long* __restrict__ totals) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t g0 = t * per < n ? t * per : n;
  const int64_t g1 = g0 + per < n ? g0 + per : n;
  int64_t s = 0;
  for (int64_t g = g0; g < g1; ++g) s += len[g];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {
    const int64_t v = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - s;
  for (int64_t g = g0; g < g1; ++g) {
    off[g] = run;
    run += len[g];
  }
  if (t == kScanThreads - 1) {
    off[n] = part[t];
    totals[0] = (unsigned long long)part[t];
  }
}

template <int G>
__global__ __launch_bounds__(kAccThreads) void k_acc_write(AccJob J, const uint32_t* __restrict__ mark,
                                                           const int64_t* __restrict__ off,
                                                           uint32_t* __restrict__ cols, uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ tallied) {
  constexpr int per_block = kAccThreads / G;
  const int tid = threadIdx.x;
  const int gl = tid % G;
  for (int64_t row = (int64_t)blockIdx.x * per_block + tid / G; row < J.n_rows; row += (int64_t)gridDim.x * per_block) {
    const int64_t a0 = J.a_off[row], la = J.a_off[row + 1] - a0;
    const int64_t b0 = J.b_off[row];
    int64_t lb = J.b_off[row + 1] - b0;
    if (lb < 0 || b0 < 0) lb = 0;  // (flagged by k_acc_mark)
    const int64_t o = off[row];
    const int64_t matches = la + lb - (off[row + 1] - o);
    const uint32_t* __restrict__ ac = J.a_cols + a0;
    const uint32_t* __restrict__ an = J.a_cnt + a0;
    const uint32_t* __restrict__ bc = J.b_cols + b0;
    const uint32_t* __restrict__ bn = J.b_cnt + b0;
    const uint32_t* __restrict__ bm = mark + b0;
    uint32_t* __restrict__ oc = cols + o;
    uint32_t* __restrict__ on = cnt + o;
    uint64_t sum = 0;
    for (int64_t j = gl; j < la; j += G) {
      const uint32_t c = ac[j];
      const int64_t r = acc_lower_bound(bc, lb, c);
      uint32_t v = an[j];
      if (r < lb && bc[r] == c) v += bn[r];
      const int64_t m = r < lb ? (int64_t)bm[r] : matches;
      oc[j + r - m] = c;
      on[j + r - m] = v;
      sum += v;
    }
    for (int64_t k = gl; k < lb; k += G) {
      const uint32_t c = bc[k];
      const int64_t r = acc_lower_bound(ac, la, c);
      if (r < la && ac[r] == c) continue;  // (added to A's entry above)
      const uint32_t v = bn[k];
      const int64_t p = k - (int64_t)bm[k] + r;
      oc[p] = c;
      on[p] = v;
      sum += v;
    }
    for (int o2 = 32; o2 > 0; o2 >>= 1) sum += __shfl_xor(sum, o2);
    // (the sum of a row's counts is at most the rays it traced, below 2^32)
    if ((tid & 63) == 0 && sum) atomicAdd(&tallied[row], (uint32_t)sum);
  }
}

__global__ __launch_bounds__(kAccThreads) void k_acc_lost(const uint32_t* __restrict__ tallied, int64_t n_rows,
                                                          int64_t rays, unsigned long long* __restrict__ totals) {
  unsigned long long ls = 0, lm = 0;
  for (int64_t row = (int64_t)blockIdx.x * kAccThreads + threadIdx.x; row < n_rows;
       row += (int64_t)gridDim.x * kAccThreads) {
    const int64_t lost = rays - (int64_t)tallied[row];
    const unsigned long long l = lost > 0 ? (unsigned long long)lost : 0ull;
    ls += l;
    lm = l > lm ? l : lm;
  }
  for (int o = 32; o > 0; o >>= 1) {
    ls += __shfl_xor(ls, o);
    const unsigned long long x = __shfl_xor(lm, o);
    lm = x > lm ? x : lm;
  }
  if ((threadIdx.x & 63) == 0 && ls) {
    atomicAdd(&totals[1], ls);
    atomicMax(&totals[2], lm);
  }
}

static unsigned acc_grid(const AccJob& J) {
  const int64_t per_block = J.wide ? 1 : kAccThreads / 64;
  const int64_t blocks = (J.n_rows + per_block - 1) / per_block;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

hipError_t acc_lengths(const AccJob& J, uint32_t* mark, int64_t* len, int64_t* off, unsigned long long* totals,
                       hipStream_t st) {
  if (J.n_rows > 0) {
    if (J.wide)
      hipLaunchKernelGGL(k_acc_mark<kAccThreads>, dim3(acc_grid(J)), dim3(kAccThreads), 0, st, J, mark, len, totals);
    else
      hipLaunchKernelGGL(k_acc_mark<64>, dim3(acc_grid(J)), dim3(kAccThreads), 0, st, J, mark, len, totals);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_acc_scan, dim3(1), dim3(kScanThreads), 0, st, len, J.n_rows, off, totals);
  return hipGetLastError();
}

hipError_t acc_write(const AccJob& J, const uint32_t* mark, const int64_t* off, uint32_t* cols, uint32_t* cnt,
                     uint32_t* tallied, unsigned long long* totals, hipStream_t st) {
  if (J.n_rows <= 0) return hipSuccess;
  if (J.wide)
    hipLaunchKernelGGL(k_acc_write<kAccThreads>, dim3(acc_grid(J)), dim3(kAccThreads), 0, st, J, mark, off, cols, cnt,
                       tallied);
  else
    hipLaunchKernelGGL(k_acc_write<64>, dim3(acc_grid(J)), dim3(kAccThreads), 0, st, J, mark, off, cols, cnt, tallied);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t blocks = (J.n_rows + kAccThreads - 1) / kAccThreads;
  hipLaunchKernelGGL(k_acc_lost, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kAccThreads), 0, st, tallied,
                     J.n_rows, J.rays, totals);
  return hipGetLastError();
}

// One wave per row, in fp64: n exactly (integer sum), then sum_j (c_j / n)^2.
__global__ __launch_bounds__(kAccThreads) void k_err_rows(const int64_t* __restrict__ row_off,
                                                          const uint32_t* __restrict__ cnt, int64_t n_rows,
                                                          double* __restrict__ s) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * (kAccThreads / 64) + (threadIdx.x >> 6); row < n_rows;
       row += (int64_t)gridDim.x * (kAccThreads / 64)) {
    const int64_t b = row_off[row], e = row_off[row + 1];
    uint64_t n = 0;
    for (int64_t k = b + lane; k < e; k += 64) n += cnt[k];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    const double nd = (double)n;
    double q = 0.0;
    for (int64_t k = b + lane; k < e; k += 64) {
      const double p = (double)cnt[k] / nd;
      q += p * p;
    }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if (lane == 0) s[row] = n ? (1.0 - q) / nd : 0.0;
  }
}

// One workgroup: the rows' variances summed and maximised in a fixed order.
__global__ __launch_bounds__(kScanThreads) void k_err_reduce(const double* __restrict__ s, int64_t n_rows,
                                                             double* __restrict__ out) {
  __shared__ double ps[kScanThreads], pm[kScanThreads];
  const int t = threadIdx.x;
  double a = 0.0, m = 0.0;
  for (int64_t i = t; i < n_rows; i += kScanThreads) {
    const double v = s[i];
    a += v;
    m = v > m ? v : m;
  }
  ps[t] = a;
  pm[t] = m;
  __syncthreads();
  for (int o = kScanThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      ps[t] += ps[t + o];
      pm[t] = pm[t + o] > pm[t] ? pm[t + o] : pm[t];
    }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = ps[0];
    out[1] = pm[0];
  }
}

hipError_t sampling_error(const int64_t* row_off, const uint32_t* cnt, int64_t n_rows, double* s, double* out,
                          hipStream_t st) {
  if (n_rows > 0) {
    const int64_t blocks = (n_rows + kAccThreads / 64 - 1) / (kAccThreads / 64);
    hipLaunchKernelGGL(k_err_rows, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kAccThreads), 0, st,
                       row_off, cnt, n_rows, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_err_reduce, dim3(1), dim3(kScanThreads), 0, st, s, n_rows, out);
  return hipGetLastError();
}

}  // namespace asmb
}  // namespace rthx
