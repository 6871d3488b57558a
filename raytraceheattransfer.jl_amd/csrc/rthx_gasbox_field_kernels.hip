// rthx_gasbox_field_kernels.hip -- Monte Carlo exchange factors of a gas box
// with one extinction coefficient per voxel on gfx950 (include/rthx.h
// rthx_gasbox_trace_field).  The uniform box's ray
// (rthx_gasbox_kernels.hip) ends by locating one point; here the ray walks the
// lattice (rthx_gasbox_walk.h walk) and gathers beta from the field in device
// memory, one fp64 load a cell.  Trip counts differ between the lanes of a
// wave, so the loop body is short: one min over three distances, one load, one
// fma-shaped update, one quotient for the axis that stepped.
//
// Emission, the Philox words and their order are the uniform tracer's, so a
// uniform field sends the uniform kernel's rays.  Grid, row split and the
// three row tallies are its too: a workgroup traces a slice of one emitter's
// rays into an LDS histogram (u16 or u32 counters) that it adds to the row's
// dense counts, or adds every ray straight to the dense row.  The box is
// closed, so every ray is tallied, at a column that walk keeps inside [0, N).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_device.h"
#include "rthx_gasbox_walk.h"

namespace rthx {
namespace gasbox {

// Box constants and the launch's scalars arrive as kernel arguments
// (wave-uniform, in SGPRs); the field is the one array the lanes gather from.
struct FieldKernelArgs {
  Box B;
  const double* beta_v;    // [Nv], >= 0
  const double* tables;
  int64_t R, ray_base, g_begin, g_stride;
  int32_t split;
  uint32_t key0, key1;
  uint32_t* dense;
  uint32_t* row_tallied;
};

// Ray (g, ray id r): the two Philox blocks of RayDraws at counter
// (r, g, 0 / 1, kTag) and the words of the uniform tracer's trace_ray, word
// c[1] giving the optical depth -ln u instead of the free path -ln u / beta.
template <bool FAITHFUL>
__device__ __forceinline__ int32_t trace_field_ray(const Box& Bw, const Emitter& E, const FieldKernelArgs& A, uint32_t g,
                                                   uint32_t r) {
  const RayDraws rd(r, g, 0u, kTag, A.key0, A.key1);
  const double* tab = A.tables;
  const double u[3] = {u32(rd.a[0]), u32(rd.a[1]), u32(rd.a[2])};
  const uint32_t w_th = rd.a[3], w_ph = rd.c[0], w_path = rd.c[1];
  double ct, st, cphi, sphi, tau;
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
    tau = -log(u32(w_path));  // (word 0: -log(0) = +inf)
  } else {
    cphi = cos_2pi_u32(w_ph, tab);
    sphi = cos_2pi_u32(w_ph - 0x40000000u, tab);  // cos(2 pi u - pi/2) = sin(2 pi u)
    tau = neg_log_u32(w_path, tab + kLogTableOffset);  // (word 0: +inf)
  }
  double o[3], d[3];
  emit(E, u, ct, st, cphi, sphi, o, d);
  return walk(Bw, A.beta_v, o, d, tau);
}

template <bool FAITHFUL, int TALLY>
__global__ __launch_bounds__(kThreads) void gasbox_field_trace_kernel(FieldKernelArgs A) {
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
  const Box& Bw = B;
  const Emitter E = make_emitter(B, (int32_t)g);
  // Ray ids and the lane's trip count in 32 bits (ray_base + R < 2^32, checked
  // by the host): 64-bit loop counters cost the scalar registers that the
  // FAITHFUL instances, full of libm's constants, no longer have.  The id is
  // not compared, so its last increment may wrap.
  const uint32_t n_part = (uint32_t)(r_end > r_begin ? r_end - r_begin : 0);
  const uint32_t n_lane = n_part > (uint32_t)tid ? (n_part - (uint32_t)tid + (kThreads - 1)) / kThreads : 0u;
  uint32_t id = (uint32_t)(A.ray_base + r_begin) + (uint32_t)tid;
  for (uint32_t it = 0; it < n_lane; ++it, id += kThreads) {
    // (col in [0, N): rthx_gasbox_walk.h walk, tests/gasbox_walk_host_check.cpp)
    const int32_t col = trace_field_ray<FAITHFUL>(Bw, E, A, (uint32_t)g, id);
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
hipError_t launch_variant(const Launch& L, const FieldKernelArgs& A) {
  const size_t lds = lds_bytes(TALLY, L.B.n_elements);
  auto kern = gasbox_field_trace_kernel<FAITHFUL, TALLY>;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const int64_t blocks = L.n_rows * L.split;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, L.stream, A);
  return hipGetLastError();
}

template <bool FAITHFUL>
hipError_t launch_tally(const Launch& L, const FieldKernelArgs& A) {
  switch (L.tally) {
    case kU32: return launch_variant<FAITHFUL, kU32>(L, A);
    case kU16: return launch_variant<FAITHFUL, kU16>(L, A);
    default: return launch_variant<FAITHFUL, kGlobal>(L, A);
  }
}

}  // namespace

hipError_t launch_field(const FieldLaunch& F) {
  const Launch& L = F.L;
  FieldKernelArgs A{};
  A.B = L.B;
  A.beta_v = F.beta_v;
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
