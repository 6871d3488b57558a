// rthx_gasbox_kernels.hip -- Monte Carlo exchange factors of a gas-filled box
// on gfx950 (include/rthx.h rthx_gasbox_trace): the 3D
// analogue of the 2D tracer's uniform grey lattice.  With one extinction
// coefficient a ray needs no walk through the voxels: it ends after one free
// path or at the box's wall, whichever comes first, and its absorber is found
// by locating that point (rthx_gasbox.h classify).  The ray body is straight
// line code: two Philox blocks, the emission, one exit distance, one select.
//
// A workgroup traces a slice of one emitter's rays and tallies them in an LDS
// histogram that it then adds to the row's dense counts, or -- where N does
// not fit LDS, or the slice has fewer rays than the row has columns -- adds
// every ray straight to the dense row.  The box is closed, so every ray is
// tallied, at a column that classify keeps inside [0, N).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_device.h"
#include "rthx_gasbox.h"

namespace rthx {
namespace gasbox {

// Box constants, beta and the launch's scalars arrive as kernel arguments
// (wave-uniform, in SGPRs); no device record is loaded.
struct KernelArgs {
  Box B;
  double beta, inv_beta;   // inv_beta = +inf for beta == 0: every free path is +inf
  const double* tables;
  int64_t R, ray_base, g_begin, g_stride;
  int32_t split;
  uint32_t key0, key1;
  uint32_t* dense;
  uint32_t* row_tallied;
};

// Ray (g, ray id r) draws from the two Philox blocks of RayDraws, counter
// (r, g, 0 / 1, kTag); the words are listed beside RayDraws (rthx_device.h).
template <bool FAITHFUL>
__device__ __forceinline__ int32_t trace_ray(const Box& B, const Emitter& E, const KernelArgs& A, uint32_t g,
                                             uint32_t r) {
  const RayDraws rd(r, g, 0u, kTag, A.key0, A.key1);
  const double* tab = A.tables;
  const double u[3] = {u32(rd.a[0]), u32(rd.a[1]), u32(rd.a[2])};
  const uint32_t w_th = rd.a[3], w_ph = rd.c[0], w_path = rd.c[1];
  double ct, st, cphi, sphi, S;
  if (E.axis >= 0) {  // wall: cosine law about the inward normal (wave-uniform branch)
    const double ut = u32(w_th);
    if (FAITHFUL) {
      ct = sqrt(1.0 - ut);
      st = sqrt(ut);
    } else {
      ct = sqrt_unit(1.0 - ut);  // (1 - u is exact and >= 2^-32)
      st = sqrt_unit(ut);
    }
  } else {  // volume: isotropic
    ct = 1.0 - 2.0 * u32(w_th);
    if (FAITHFUL) {
      const double th = acos(ct);
      ct = cos(th);
      st = sin(th);
    } else {
      st = sin_theta_u32(w_th);
    }
  }
  if (FAITHFUL) {
    cphi = cos(RTHX_TWO_PI * u32(w_ph));
    sphi = sin(RTHX_TWO_PI * u32(w_ph));
    S = A.beta > 0.0 ? -log(u32(w_path)) / A.beta : __builtin_inf();  // (word 0: -log(0) = +inf)
  } else {
    cphi = cos_2pi_u32(w_ph, tab);
    sphi = cos_2pi_u32(w_ph - 0x40000000u, tab);  // cos(2 pi u - pi/2) = sin(2 pi u)
    S = neg_log_u32(w_path, tab + kLogTableOffset) * A.inv_beta;  // (-ln u > 0: never 0 * inf)
  }
  double o[3], d[3];
  emit(E, u, ct, st, cphi, sphi, o, d);
  return classify(B, o, d, S);
}

template <bool FAITHFUL, int TALLY>
__global__ __launch_bounds__(kThreads) void gasbox_trace_kernel(KernelArgs A) {
  extern __shared__ uint32_t hist[];  // kU32: N words; kU16: (N + 1) / 2; kGlobal: none
  const Box& B = A.B;
  const int tid = threadIdx.x;
  const int64_t slot = blockIdx.x / A.split, part = blockIdx.x % A.split;
  const int64_t chunk = (A.R + A.split - 1) / A.split;
  const int64_t r_begin = part * chunk;
  const int64_t r_end = r_begin + chunk < A.R ? r_begin + chunk : A.R;
  const int64_t g = A.g_begin + slot * A.g_stride;
  const int64_t N = B.n_elements;
  const int64_t words = TALLY == kGlobal ? 0 : TALLY == kU16 ? (N + 1) / 2 : N;
  uint32_t* dense = A.dense + slot * N;
  if (TALLY != kGlobal) {
    for (int64_t i = tid; i < words; i += kThreads) hist[i] = 0u;
    __syncthreads();
  }
  const Emitter E = make_emitter(B, (int32_t)g);
  for (int64_t r = r_begin + tid; r < r_end; r += kThreads) {
    // (col in [0, N): rthx_gasbox.h classify, tests/gasbox_host_check.cpp)
    const int32_t col = trace_ray<FAITHFUL>(B, E, A, (uint32_t)g, (uint32_t)(A.ray_base + r));
    if (TALLY == kGlobal)
      __hip_atomic_fetch_add(&dense[col], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (TALLY == kU16)
      atomicAdd(&hist[col >> 1], 1u << ((col & 1) * 16));  // (fewer than 65536 rays here: no carry)
    else
      atomicAdd(&hist[col], 1u);
  }
  if (TALLY != kGlobal) {
    __syncthreads();
    for (int64_t i = tid; i < N; i += kThreads) {
      const uint32_t v = TALLY == kU16 ? (hist[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu : hist[i];
      if (v) __hip_atomic_fetch_add(&dense[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // every ray of the slice was tallied
  if (tid == 0 && r_end > r_begin)
    __hip_atomic_fetch_add(&A.row_tallied[slot], (uint32_t)(r_end - r_begin), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

namespace {

template <bool FAITHFUL, int TALLY>
hipError_t launch_variant(const Launch& L, const KernelArgs& A) {
  const size_t lds = lds_bytes(TALLY, L.B.n_elements);
  auto kern = gasbox_trace_kernel<FAITHFUL, TALLY>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int64_t blocks = L.n_rows * L.split;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, L.stream, A);
  return hipGetLastError();
}

template <bool FAITHFUL>
hipError_t launch_tally(const Launch& L, const KernelArgs& A) {
  switch (L.tally) {
    case kU32: return launch_variant<FAITHFUL, kU32>(L, A);
    case kU16: return launch_variant<FAITHFUL, kU16>(L, A);
    default: return launch_variant<FAITHFUL, kGlobal>(L, A);
  }
}

}  // namespace

hipError_t launch(const Launch& L) {
  KernelArgs A{};
  A.B = L.B;
  A.beta = L.beta;
  A.inv_beta = L.beta > 0.0 ? 1.0 / L.beta : __builtin_inf();
  A.tables = L.tables;
  A.R = L.R;
  A.ray_base = L.ray_base;
  A.g_begin = L.g_begin;
  A.g_stride = L.g_stride;
  A.split = L.split;
  A.key0 = L.key0;
  A.key1 = L.key1;
  A.dense = L.dense;
  A.row_tallied = L.row_tallied;
  return L.faithful ? launch_tally<true>(L, A) : launch_tally<false>(L, A);
}

}  // namespace gasbox
}  // namespace rthx
