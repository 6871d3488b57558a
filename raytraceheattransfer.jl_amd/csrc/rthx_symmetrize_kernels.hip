// rthx_symmetrize_kernels.hip -- X = (Diagonal(w) A + (Diagonal(w) A)') / 2
// of a square CSR matrix on the device, the set-up of the
// sparse exchange-factor smoothing (smoothExchangeFactors.jl:474-477).
//
// Row i of X is the union of row i of A and row i of A', both strictly
// column-ascending, so an entry's place follows from ranks alone, as in the
// sum of two count matrices (rthx_assemble_kernels.hip): with r the number of
// columns of A' below an A entry's column and m the number of those that are
// also stored in A's row, A's entry j lands at j + r - m; an unmatched entry k
// of A' with m matches before it and r columns of A below its own lands at
// k - m + r.  Three passes, one wave per row throughout:
//  * k_sym_mark: the wave walks the row of A' 64 entries at a time, each lane
//    looks its column up in A's row, and a ballot scan with a running carry
//    gives mark[k]; the row's merged length is lenA + lenT - matches.  No
//    barrier and no LDS: the loop's trip count is uniform over the wave, which
//    is all the ballot needs.
//  * k_sym_scan: one workgroup scans the lengths into x_off (k_acc_scan's form).
//  * k_sym_write: every entry of A and every unmatched entry of A' computes
//    its place and its value and is written once.
// Built without fast-math and with -ffp-contract=off: w * v, the sum and the
// halving are three separately rounded fp64 operations, count / tallied is
// the correctly rounded quotient, and x + 0.0 is kept (it turns -0.0 into
// +0.0), so X is bit-equal to the host build of rthx_smooth.cpp.
// Entry indices are 64-bit; a column indexes w only after it is bounded by n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_symmetrize.h"

namespace rthx {
namespace sym {

namespace {

constexpr int kScanThreads = 1024;

// first index in c[0, n) whose column is >= key
__device__ __forceinline__ int64_t lower_bound(const uint32_t* __restrict__ c, int64_t n, uint32_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Row `row` of both matrices: A's entries at ac[0, la) (base a0 of the
// payload arrays), those of A' at index t0 + [0, lt).
struct Row {
  int64_t a0, la, t0, lt;
};

__device__ __forceinline__ Row row_of(const Pair& J, int64_t row) {
  Row R;
  const int64_t o = J.A.off[row];
  R.la = J.A.off[row + 1] - o;
  R.a0 = J.A.whole ? o : J.A.src[row];
  R.t0 = J.t_off[row];
  R.lt = J.t_off[row + 1] - R.t0;
  if (R.la < 0) R.la = 0;
  if (R.lt < 0 || R.t0 < 0) R.lt = 0;
  return R;
}

__global__ __launch_bounds__(kThreads) void k_sym_mark(Pair J, uint32_t* __restrict__ mark,
                                                       int64_t* __restrict__ len) {
  constexpr int per_block = kThreads / kGroup;
  const int lane = threadIdx.x & 63;
  const uint64_t lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const uint32_t* __restrict__ tcols = reinterpret_cast<const uint32_t*>(J.t_cols);
  for (int64_t row = (int64_t)blockIdx.x * per_block + (threadIdx.x >> 6); row < J.A.n_rows;
       row += (int64_t)gridDim.x * per_block) {
    const Row R = row_of(J, row);
    const uint32_t* __restrict__ ac = J.A.cols + R.a0;
    const uint32_t* __restrict__ tc = tcols + R.t0;
    uint32_t carry = 0;
    for (int64_t k0 = 0; k0 < R.lt; k0 += kGroup) {  // (uniform over the wave: the ballot below)
      const int64_t k = k0 + lane;
      bool m = false;
      if (k < R.lt) {
        const uint32_t c = tc[k];
        const int64_t r = lower_bound(ac, R.la, c);
        m = r < R.la && ac[r] == c;
      }
      const uint64_t b = __ballot(m);
      if (k < R.lt) mark[R.t0 + k] = carry + (uint32_t)__popcll(b & lt_mask);
      carry += (uint32_t)__popcll(b);
    }
    if (lane == 0) len[row] = R.la + R.lt - (int64_t)carry;
  }
}

__global__ __launch_bounds__(kScanThreads) void k_sym_scan(const int64_t* __restrict__ len, int64_t n,
                                                           int64_t* __restrict__ off) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t g0 = t * per < n ? t * per : n;
  const int64_t g1 = g0 + per < n ? g0 + per : n;
  int64_t s = 0;
  for (int64_t g = g0; g < g1; ++g) s += len[g];
  part[t] = s;
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {  // (10 steps for every lane)
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
  if (t == kScanThreads - 1) off[n] = part[t];
}

__global__ __launch_bounds__(kThreads) void k_sym_write(Pair J, const double* __restrict__ w,
                                                        const uint32_t* __restrict__ mark,
                                                        const int64_t* __restrict__ x_off,
                                                        int32_t* __restrict__ x_cols, double* __restrict__ x_vals) {
  constexpr int per_block = kThreads / kGroup;
  const int lane = threadIdx.x & 63;
  const int64_t n = J.A.n_rows;
  const uint32_t* __restrict__ tcols = reinterpret_cast<const uint32_t*>(J.t_cols);
  for (int64_t row = (int64_t)blockIdx.x * per_block + (threadIdx.x >> 6); row < n;
       row += (int64_t)gridDim.x * per_block) {
    const Row R = row_of(J, row);
    const int64_t o = x_off[row], lx = x_off[row + 1] - o;
    const int64_t matches = R.la + R.lt - lx;
    const uint32_t* __restrict__ ac = J.A.cols + R.a0;
    const uint32_t* __restrict__ tc = tcols + R.t0;
    const double* __restrict__ tv = J.t_vals + R.t0;
    const uint32_t* __restrict__ tm = mark + R.t0;
    int32_t* __restrict__ xc = x_cols + o;
    double* __restrict__ xv = x_vals + o;
    const double wi = w ? w[row] : 1.0;
    const double tal = J.A.counts ? J.A.tallied[row] : 1.0;
    for (int64_t j = lane; j < R.la; j += kGroup) {
      const uint32_t c = ac[j];
      const int64_t r = lower_bound(tc, R.lt, c);
      const double v = J.A.counts ? (double)J.A.counts[R.a0 + j] / tal : J.A.vals[R.a0 + j];
      const double a = wi * v;
      double b = 0.0;
      if (r < R.lt && tc[r] == c) b = (w && (int64_t)c < n ? w[c] : 1.0) * tv[r];
      const int64_t m = r < R.lt ? (int64_t)tm[r] : matches;
      const int64_t p = j + r - m;
      if (p >= 0 && p < lx) {  // (holds for ascending rows)
        xc[p] = (int32_t)c;
        xv[p] = 0.5 * (a + b);
      }
    }
    for (int64_t k = lane; k < R.lt; k += kGroup) {
      const uint32_t c = tc[k];
      const int64_t r = lower_bound(ac, R.la, c);
      if (r < R.la && ac[r] == c) continue;  // (written with A's entry above)
      const double b = (w && (int64_t)c < n ? w[c] : 1.0) * tv[k];
      const int64_t p = k - (int64_t)tm[k] + r;
      if (p >= 0 && p < lx) {
        xc[p] = (int32_t)c;
        xv[p] = 0.5 * (0.0 + b);
      }
    }
  }
}

unsigned grid_of(int64_t n_rows) {
  const int64_t per_block = kThreads / kGroup;
  const int64_t blocks = (n_rows + per_block - 1) / per_block;
  return (unsigned)(blocks < 65536 ? blocks : 65536);
}

}  // namespace

hipError_t lengths(const Pair& J, uint32_t* mark, int64_t* len, int64_t* x_off, hipStream_t st) {
  if (J.A.n_rows > 0) {
    hipLaunchKernelGGL(k_sym_mark, dim3(grid_of(J.A.n_rows)), dim3(kThreads), 0, st, J, mark, len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_sym_scan, dim3(1), dim3(kScanThreads), 0, st, len, J.A.n_rows, x_off);
  return hipGetLastError();
}

hipError_t write(const Pair& J, const double* w, const uint32_t* mark, const int64_t* x_off, int32_t* x_cols,
                 double* x_vals, hipStream_t st) {
  if (J.A.n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sym_write, dim3(grid_of(J.A.n_rows)), dim3(kThreads), 0, st, J, w, mark, x_off, x_cols,
                     x_vals);
  return hipGetLastError();
}

}  // namespace sym
}  // namespace rthx
