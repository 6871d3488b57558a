// rthx_solve.h -- launchers of the grey GERT solve kernels
// (rthx_solve_kernels.hip), driven by rthx_solve.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "rthx_common.h"

namespace rthx {
namespace gs {

// The operator F' x: a dense row-major F (n x n) with a partial-sum buffer of
// part_doubles(n), or F' as CSR (rows of F' = columns of F).
struct Op {
  bool dense = true;
  int64_t n = 0;
  const double* F = nullptr;
  double* part = nullptr;
  const int64_t* rp = nullptr;
  const int32_t* ci = nullptr;
  const double* v = nullptr;
};

// out = x - c .* (F' x) when c != nullptr, else out = F' x.
hipError_t apply(const Op& op, const double* x, const double* c, double* out, hipStream_t s);
int64_t part_doubles(int64_t n);
hipError_t multidot(const double* V, const double* w, int m, int64_t n, double* out, hipStream_t s);
hipError_t combine(const double* V, const double* coef, int m, double sign, int64_t n, double* w, hipStream_t s);
hipError_t scale(const double* a, double alpha, int64_t n, double* out, hipStream_t s);
hipError_t sub(const double* a, const double* b, int64_t n, double* out, hipStream_t s);

// Restarted GMRES (rthx_solve.cpp) on vectors of length n: the right-hand
// side in h, the solution in x.  The operator is a callback out = M x on the
// stream s; with warm = true the iteration starts from the x already there
// (and takes no step when that x meets the tolerance), else from zero.
struct Krylov {
  hipStream_t s = nullptr;
  int64_t n = 0;
  DevBuf h, x, r, w, V, small;
  int reserve(int memory);
  int d2h(double* dst, const double* src, size_t count);  // copy and wait
  int norm(const double* v, double* out);
};
using Apply = std::function<hipError_t(const double* x, double* out)>;
int gmres(Krylov& S, const Apply& M, const rthx_solve_args& a, bool warm, rthx_solve_info& info);

}  // namespace gs
}  // namespace rthx
