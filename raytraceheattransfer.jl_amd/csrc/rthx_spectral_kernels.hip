// rthx_spectral_kernels.hip -- device kernels of the spectral GERT solve
// (DESIGN.md §7f): the banded operator g_k = F_k' x_k with its mix over the
// bands, the emission update, and the Planck band fractions with the
// per-element temperature inversion.  The banded F' x is the only large pass
// (K n^2 doubles for distinct dense matrices, n^2 for a shared one: HBM-bound);
// everything else is K n long.  Every reduction runs in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_spectral.h"

namespace rthx {
namespace sp {

constexpr int kCols = 256;   // columns per workgroup of the dense F' x
constexpr int kChunk = 128;  // rows per workgroup of the dense F' x
constexpr int kShare = 8;    // bands per pass over a shared dense F

// Dense row-major F_k, one matrix per band (blockIdx.z = band):
// part[k][chunk][j] = sum_{i in chunk} F_k[i][j] x_k[i].  Each lane owns a
// column, rows are streamed (coalesced along j), x_k[i] is wave-uniform.
__global__ __launch_bounds__(kCols) void k_part_bands(const BandMat* __restrict__ mats, const double* __restrict__ x,
                                                      int64_t n, int64_t chunks, double* __restrict__ part) {
  const int64_t k = blockIdx.z;
  const double* __restrict__ F = mats[k].F;
  if (!F) return;  // a sparse band: k_spmv_bands
  const int64_t j = (int64_t)blockIdx.x * kCols + threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * kChunk;
  const int64_t i1 = i0 + kChunk < n ? i0 + kChunk : n;
  if (j >= n) return;
  const double* __restrict__ xk = x + k * n;
  double s = 0.0;
#pragma unroll 8
  for (int64_t i = i0; i < i1; ++i) s += F[i * n + j] * xk[i];
  part[(k * chunks + blockIdx.y) * n + j] = s;
}

// One dense F shared by every band: each loaded F[i][j] serves KB bands from
// registers (blockIdx.z = group of KB bands), so K <= KB bands cost one pass
// over F.  Bands past K - 1 in the last group repeat band K - 1 and are not
// stored.
template <int KB>
__global__ __launch_bounds__(kCols) void k_part_shared(const double* __restrict__ F, const double* __restrict__ x,
                                                       int64_t n, int K, int64_t chunks, double* __restrict__ part) {
  const int k0 = (int)blockIdx.z * KB;
  const int64_t j = (int64_t)blockIdx.x * kCols + threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.y * kChunk;
  const int64_t i1 = i0 + kChunk < n ? i0 + kChunk : n;
  if (j >= n) return;
  const double* xq[KB];
  double acc[KB];
#pragma unroll
  for (int q = 0; q < KB; ++q) {
    const int k = k0 + q < K ? k0 + q : K - 1;
    xq[q] = x + (int64_t)k * n;
    acc[q] = 0.0;
  }
#pragma unroll 4
  for (int64_t i = i0; i < i1; ++i) {
    const double a = F[i * n + j];
#pragma unroll
    for (int q = 0; q < KB; ++q) acc[q] += a * xq[q][i];
  }
#pragma unroll
  for (int q = 0; q < KB; ++q)
    if (k0 + q < K) part[((int64_t)(k0 + q) * chunks + blockIdx.y) * n + j] = acc[q];
}

// Sparse bands, F' as CSR, one wave per row (blockIdx.y = band): g_k = F_k' x_k.
__global__ __launch_bounds__(256) void k_spmv_bands(const BandMat* __restrict__ mats, int n_mats,
                                                    const double* __restrict__ x, int64_t n, double* __restrict__ g) {
  const int64_t k = blockIdx.y;
  const BandMat M = mats[n_mats == 1 ? 0 : k];
  if (M.F) return;  // a dense band: k_part_*
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int lane = threadIdx.x & 63;
  const double* __restrict__ xk = x + k * n;
  double s = 0.0;
  for (int64_t p = M.rp[i] + lane; p < M.rp[i + 1]; p += 64) s += M.v[p] * xk[M.ci[p]];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) g[k * n + i] = s;
}

// One lane per element, looping over the bands: g_ik from the partial sums of
// a dense band (fixed order) or as k_spmv_bands left it; then, when y is
// given, y_ik = x_ik - b_ik g_ik - radeq_i f_ik sum_l (1 - b_il) g_il.
__global__ void k_mix(const BandMat* __restrict__ mats, int n_mats, const double* __restrict__ part, int64_t chunks,
                      int64_t n, int K, const double* __restrict__ x, const double* __restrict__ b,
                      const double* __restrict__ f, const uint8_t* __restrict__ radeq, double* g, double* y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double absorbed = 0.0;
  for (int64_t k = 0; k < K; ++k) {
    double gk;
    if (mats[n_mats == 1 ? 0 : k].F) {
      gk = 0.0;
      for (int64_t c = 0; c < chunks; ++c) gk += part[(k * chunks + c) * n + i];
      g[k * n + i] = gk;
    } else {
      gk = g[k * n + i];
    }
    if (y) absorbed += (1.0 - b[k * n + i]) * gk;
  }
  if (!y) return;
  const bool re = radeq && radeq[i];
  for (int64_t k = 0; k < K; ++k) {
    const int64_t q = k * n + i;
    double out = x[q] - b[q] * g[q];
    if (re) out -= f[q] * absorbed;
    y[q] = out;
  }
}

__global__ void k_emission(const double* __restrict__ j, const double* __restrict__ b, const double* __restrict__ g,
                           const uint8_t* __restrict__ radeq, int64_t n, int K, double* __restrict__ e) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !radeq[i]) return;
  double s = 0.0;
  for (int64_t k = 0; k < K; ++k) s += j[k * n + i] - b[k * n + i] * g[k * n + i];
  const double floor_e = 10.0 * 2.220446049250313e-16;
  e[i] = s > floor_e ? s : floor_e;
}

constexpr double kC2 = 1.4387768775039337e-2;  // h c / k_B [m K] (src/RayTraceHeatTransfer.jl:25)
constexpr double kSigma = 5.670374419e-8;      // src/RayTraceHeatTransfer.jl:20
constexpr double kPi = 3.141592653589793;

// emitFracBlackBodySpectrum (emitFracBlackBodySpectrum.jl:1-42): F(0 -> lambda T).
__device__ double planck_cumulative(double lambda, double T) {
  if (!isfinite(T) || T <= 0.0) return 0.0;
  const double xi = kC2 / (lambda * T);
  if (xi > 50.0) return 0.0;
  if (xi < 1e-8) return 1.0;
  double F = 0.0;
  for (int mi = 1; mi <= 100; ++mi) {
    const double m = (double)mi;
    const double ex = exp(-m * xi);
    if (ex < 1e-16) break;
    const double poly = xi * xi * xi + 3.0 * (xi * xi) / m + 6.0 * xi / (m * m) + 6.0 / (m * m * m);
    const double term = (ex / m) * poly;
    if (isfinite(term)) F += term;
  }
  F *= 15.0 / (kPi * kPi * kPi * kPi);
  return F < 0.0 ? 0.0 : (F > 1.0 ? 1.0 : F);
}

// _fill_emission_fractions! (getBinsEmissionFractions.jl): band k spans
// limits[k] .. limits[k + 1], the first band from 0, the last to infinity.
// Calls use(k, w_k) for k = 0 .. K - 1.
template <class Use>
__device__ void band_fractions(const double* __restrict__ limits, int K, double T, Use use) {
  double prev = 0.0;
  for (int k = 0; k < K; ++k) {
    if (k == K - 1) {
      use(k, 1.0 - prev);
    } else {
      const double cur = planck_cumulative(limits[k + 1], T);
      use(k, cur - prev);
      prev = cur;
    }
  }
}

__global__ void k_fractions(const double* __restrict__ limits, int K, const double* __restrict__ T,
                            const double* __restrict__ prop, int64_t n, double* plain, double* __restrict__ weighted) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  band_fractions(limits, K, T[i], [&](int k, double w) {
    const int64_t q = (int64_t)k * n + i;
    plain[q] = w;
    s += (prop ? prop[q] : 1.0) * w;
  });
  if (!weighted) return;
  for (int64_t k = 0; k < K; ++k) {  // getWeightedEmissionFractions: left as prop .* w when the sum is 0
    const int64_t q = k * n + i;
    const double v = (prop ? prop[q] : 1.0) * plain[q];
    weighted[q] = s > 0.0 ? v / s : v;
  }
}

__device__ double emitting_sum(const double* __restrict__ limits, int K, const double* __restrict__ prop, int64_t n,
                               int64_t i, double T) {
  double s = 0.0;
  band_fractions(limits, K, T, [&](int k, double w) { s += prop[(int64_t)k * n + i] * w; });
  return s;
}

__global__ void k_temperatures(const double* __restrict__ limits, int K, const double* __restrict__ prop,
                               const double* __restrict__ size, const double* __restrict__ T_in,
                               const uint8_t* __restrict__ radeq, int invert, int64_t n, double* __restrict__ e,
                               double* __restrict__ T) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (!radeq[i]) {  // setupBoundaryConditions.jl:31-54
    const double t = T_in[i];
    T[i] = t;
    e[i] = size[i] * kSigma * (t * t * t * t) * emitting_sum(limits, K, prop, n, i, t);
    return;
  }
  if (!invert) return;
  double t = T[i];
  const double ei = e[i];
  for (int it = 0; it < 60; ++it) {
    const double den = size[i] * kSigma * emitting_sum(limits, K, prop, n, i, t);
    const double tn = den > 0.0 ? sqrt(sqrt(ei / den)) : 0.0;
    const double d = fabs(tn - t);
    t = tn;
    if (d <= 1e-13 * fabs(tn)) break;
  }
  T[i] = t;
}

__global__ void k_rhs(const double* __restrict__ f, const double* __restrict__ e, const double* __restrict__ q,
                      const uint8_t* __restrict__ radeq, int64_t n, int64_t total, double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const int64_t i = p % n;
  out[p] = f[p] * (radeq[i] ? q[i] : e[i]);
}

static unsigned g1(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

int64_t part_doubles(int64_t n) { return ((n + kChunk - 1) / kChunk) * n; }

template <int KB>
static void launch_shared(const double* F, const double* x, int64_t n, int K, int64_t chunks, double* part,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_part_shared<KB>, dim3(g1(n, kCols), (unsigned)chunks, g1(K, KB)), dim3(kCols), 0, s, F, x, n, K,
                     chunks, part);
}

hipError_t apply(const BandedOp& op, const double* x, const double* b, const double* f, const uint8_t* radeq,
                 double* g, double* y, hipStream_t s) {
  const int64_t n = op.n;
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  if (op.any_dense) {
    if (op.n_mats == 1) {
      if (op.K >= kShare) launch_shared<kShare>(op.shared_F, x, n, op.K, chunks, op.part, s);
      else if (op.K > 2) launch_shared<4>(op.shared_F, x, n, op.K, chunks, op.part, s);
      else if (op.K == 2) launch_shared<2>(op.shared_F, x, n, op.K, chunks, op.part, s);
      else launch_shared<1>(op.shared_F, x, n, op.K, chunks, op.part, s);
    } else {
      hipLaunchKernelGGL(k_part_bands, dim3(g1(n, kCols), (unsigned)chunks, (unsigned)op.K), dim3(kCols), 0, s,
                         op.mats, x, n, chunks, op.part);
    }
  }
  if (op.any_sparse)
    hipLaunchKernelGGL(k_spmv_bands, dim3(g1(n, 4), (unsigned)op.K), dim3(256), 0, s, op.mats, op.n_mats, x, n, g);
  hipLaunchKernelGGL(k_mix, dim3(g1(n, 256)), dim3(256), 0, s, op.mats, op.n_mats, op.part, chunks, n, op.K, x, b, f,
                     radeq, g, y);
  return hipGetLastError();
}

hipError_t emission(const double* j, const double* b, const double* g, const uint8_t* radeq, int64_t n, int K,
                    double* e, hipStream_t s) {
  hipLaunchKernelGGL(k_emission, dim3(g1(n, 256)), dim3(256), 0, s, j, b, g, radeq, n, K, e);
  return hipGetLastError();
}

hipError_t fractions(const double* limits, int K, const double* T, const double* prop, int64_t n, double* plain,
                     double* weighted, hipStream_t s) {
  hipLaunchKernelGGL(k_fractions, dim3(g1(n, 64)), dim3(64), 0, s, limits, K, T, prop, n, plain, weighted);
  return hipGetLastError();
}

hipError_t temperatures(const double* limits, int K, const double* prop, const double* size, const double* T_in,
                        const uint8_t* radeq, bool invert, int64_t n, double* e, double* T, hipStream_t s) {
  hipLaunchKernelGGL(k_temperatures, dim3(g1(n, 64)), dim3(64), 0, s, limits, K, prop, size, T_in, radeq,
                     invert ? 1 : 0, n, e, T);
  return hipGetLastError();
}

hipError_t rhs(const double* f, const double* e, const double* q, const uint8_t* radeq, int64_t n, int K, double* out,
               hipStream_t s) {
  const int64_t total = n * K;
  hipLaunchKernelGGL(k_rhs, dim3(g1(total, 256)), dim3(256), 0, s, f, e, q, radeq, n, total, out);
  return hipGetLastError();
}

}  // namespace sp
}  // namespace rthx
