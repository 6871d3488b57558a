// rthx_spectral.h -- launchers of the spectral GERT solve kernels
// (rthx_spectral_kernels.hip), driven by rthx_spectral.cpp.  Vectors of
// length K n are band-major (x[k n + i]): every band's slice is contiguous.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rthx {
namespace sp {

// One band's matrix on the device: dense row-major F (n x n), or F' as CSR
// (rows of F' = columns of F) when F is nullptr.
struct BandMat {
  const double* F = nullptr;
  const int64_t* rp = nullptr;
  const int32_t* ci = nullptr;
  const double* v = nullptr;
};

// The banded operator: K bands over n_mats matrices (1: one shared matrix,
// else K).  mats: device array [n_mats]; part: K * part_doubles(n) doubles
// when any matrix is dense.
struct BandedOp {
  int64_t n = 0;
  int K = 0;
  int n_mats = 0;
  bool any_dense = false, any_sparse = false;
  const BandMat* mats = nullptr;
  const double* shared_F = nullptr;  // mats[0].F when n_mats == 1 and it is dense
  double* part = nullptr;
};
int64_t part_doubles(int64_t n);

// g_k = F_k' x_k for every band (g: [K n]); then, when y is not nullptr,
//   y_ik = x_ik - b_ik g_ik - radeq_i f_ik sum_l (1 - b_il) g_il.
hipError_t apply(const BandedOp& op, const double* x, const double* b, const double* f, const uint8_t* radeq,
                 double* g, double* y, hipStream_t s);
// e_i = max(sum_k (j_ik - b_ik g_ik), 10 eps) on radiative-equilibrium elements.
hipError_t emission(const double* j, const double* b, const double* g, const uint8_t* radeq, int64_t n, int K,
                    double* e, hipStream_t s);
// Planck band fractions of T (limits: K + 1 band limits, device): plain
// w[K n] and, when weighted is not nullptr, prop .* w normalised per element
// (prop nullptr: 1).
hipError_t fractions(const double* limits, int K, const double* T, const double* prop, int64_t n, double* plain,
                     double* weighted, hipStream_t s);
// Prescribed elements (radeq 0): T = T_in, e = size sigma T^4 sum_k prop_k w_k(T).
// Radiative-equilibrium elements, when invert: T from e by the fixed point
// T <- (e / (size sigma sum_k prop_k w_k(T)))^(1/4) started at the T there.
hipError_t temperatures(const double* limits, int K, const double* prop, const double* size, const double* T_in,
                        const uint8_t* radeq, bool invert, int64_t n, double* e, double* T, hipStream_t s);
// rhs_ik = f_ik (radeq_i ? q_i : e_i).
hipError_t rhs(const double* f, const double* e, const double* q, const uint8_t* radeq, int64_t n, int K, double* out,
               hipStream_t s);

}  // namespace sp
}  // namespace rthx
