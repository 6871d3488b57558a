// rthx_solve.cpp -- C ABI of the grey GERT solve (include/rthx.h,
// rthx_solve_grey*): the linear system of equilibriumGrey2D!
// (src/HeatTransfer/equilibrium/equilibriumGrey2D.jl:136-166)
//     (I - Diagonal(coeff) F') j = h,   g = F' j   (:176-201)
// by restarted GMRES on the device, as the reference's sparse branch
// (Krylov.jl gmres!, memory = 50, restart = true, rtol = 1e-12, default
// atol = sqrt(eps), zero initial guess).  Orthogonalisation is classical
// Gram-Schmidt applied twice (two batched kernels per step, one host sync)
// instead of Krylov.jl's modified Gram-Schmidt; both keep the basis
// orthogonal to working precision.  The Hessenberg least-squares problem
// (Givens rotations, back substitution) is solved on the host.  A caller's
// sparse F is checked and transposed on the host by rthx_csr_host.h, before
// the device is opened, and uploaded as a tp::DeviceCsr (rthx_transpose.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "rthx_common.h"
#include "rthx_domain.h"
#include "rthx_smooth.h"
#include "rthx_solve.h"
#include "rthx_transpose.h"

using rthx::DevBuf;
using rthx::fail;
using rthx::now_ms;

namespace {

struct Solver : rthx::gs::Krylov {
  rthx::gs::Op op;
  DevBuf c, part;
};

}  // namespace

namespace rthx {
namespace gs {

int Krylov::reserve(int memory) {
  const int m = std::max(1, memory);
  HIP_TRY(h.reserve(n * 8), "hipMalloc");
  HIP_TRY(x.reserve(n * 8), "hipMalloc");
  HIP_TRY(r.reserve(n * 8), "hipMalloc");
  HIP_TRY(w.reserve(n * 8), "hipMalloc");
  HIP_TRY(V.reserve((size_t)(m + 1) * n * 8), "hipMalloc Krylov basis");
  HIP_TRY(small.reserve((size_t)(2 * (m + 1) + 1) * 8), "hipMalloc");
  return RTHX_OK;
}

int Krylov::d2h(double* dst, const double* src, size_t count) {
  HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyDeviceToHost, s), "hipMemcpy");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return RTHX_OK;
}

int Krylov::norm(const double* v, double* out) {
  HIP_TRY(multidot(v, v, 1, n, small.as<double>(), s), "multidot");
  double t;
  RTHX_TRY(d2h(&t, small.as<double>(), 1));
  *out = std::sqrt(t);
  return RTHX_OK;
}

int gmres(Krylov& S, const Apply& A, const rthx_solve_args& a, bool warm, rthx_solve_info& info) {
  const int64_t n = S.n;
  const int m = std::max(1, a.memory);
  const int64_t itmax = a.itmax > 0 ? a.itmax : 2 * n;
  hipStream_t s = S.s;
  double* x = S.x.as<double>();
  double* r = S.r.as<double>();
  double* w = S.w.as<double>();
  double* V = S.V.as<double>();
  double* h = S.h.as<double>();
  double* sm = S.small.as<double>();  // [2(m+1) + 1]: h1, h2, |w|^2
  double hnorm;
  RTHX_TRY(S.norm(h, &hnorm));
  const double tol = a.atol + a.rtol * hnorm;
  double beta = hnorm;
  if (warm) {  // r = h - M x0
    HIP_TRY(A(x, w), "apply");
    HIP_TRY(sub(h, w, n, r, s), "sub");
    RTHX_TRY(S.norm(r, &beta));
  } else {
    HIP_TRY(hipMemsetAsync(x, 0, n * 8, s), "hipMemset");
    HIP_TRY(hipMemcpyAsync(r, h, n * 8, hipMemcpyDeviceToDevice, s), "hipMemcpy");
  }
  int64_t iters = 0;
  int cycles = 0;
  std::vector<double> H((size_t)(m + 1) * m), cs(m), sn(m), g(m + 1), y(m), hh(2 * (m + 1) + 1);
  auto Hat = [&](int i, int k) -> double& { return H[(size_t)k * (m + 1) + i]; };
  while (beta > tol && iters < itmax) {
    ++cycles;
    HIP_TRY(scale(r, 1.0 / beta, n, V, s), "scale");
    std::fill(g.begin(), g.end(), 0.0);
    g[0] = beta;
    int k = 0;
    while (k < m && iters < itmax) {
      double* vk = V + (int64_t)k * n;
      HIP_TRY(A(vk, w), "apply");
      HIP_TRY(multidot(V, w, k + 1, n, sm, s), "multidot");
      HIP_TRY(combine(V, sm, k + 1, -1.0, n, w, s), "combine");
      HIP_TRY(multidot(V, w, k + 1, n, sm + (m + 1), s), "multidot");
      HIP_TRY(combine(V, sm + (m + 1), k + 1, -1.0, n, w, s), "combine");
      HIP_TRY(multidot(w, w, 1, n, sm + 2 * (m + 1), s), "multidot");
      RTHX_TRY(S.d2h(hh.data(), sm, 2 * (m + 1) + 1));
      for (int i = 0; i <= k; ++i) Hat(i, k) = hh[i] + hh[(m + 1) + i];
      const double hn = std::sqrt(hh[2 * (m + 1)]);
      Hat(k + 1, k) = hn;
      if (hn > 0) HIP_TRY(scale(w, 1.0 / hn, n, V + (int64_t)(k + 1) * n, s), "scale");
      for (int i = 0; i < k; ++i) {  // earlier rotations
        const double t = cs[i] * Hat(i, k) + sn[i] * Hat(i + 1, k);
        Hat(i + 1, k) = -sn[i] * Hat(i, k) + cs[i] * Hat(i + 1, k);
        Hat(i, k) = t;
      }
      const double den = std::hypot(Hat(k, k), Hat(k + 1, k));
      cs[k] = den > 0 ? Hat(k, k) / den : 1.0;
      sn[k] = den > 0 ? Hat(k + 1, k) / den : 0.0;
      Hat(k, k) = den;
      Hat(k + 1, k) = 0.0;
      g[k + 1] = -sn[k] * g[k];
      g[k] = cs[k] * g[k];
      ++iters;
      ++k;
      if (std::fabs(g[k]) <= tol || hn == 0.0) break;
    }
    for (int i = k - 1; i >= 0; --i) {  // H y = g
      double t = g[i];
      for (int q = i + 1; q < k; ++q) t -= Hat(i, q) * y[q];
      y[i] = t / Hat(i, i);
    }
    HIP_TRY(hipMemcpyAsync(sm, y.data(), k * 8, hipMemcpyHostToDevice, s), "hipMemcpy");
    HIP_TRY(combine(V, sm, k, 1.0, n, x, s), "combine");
    HIP_TRY(A(x, w), "apply");  // true residual h - M x
    HIP_TRY(sub(h, w, n, r, s), "sub");
    RTHX_TRY(S.norm(r, &beta));
  }
  info.iterations = (int32_t)iters;
  info.cycles = cycles;
  info.converged = beta <= tol ? 1 : 0;
  info.residual = beta;
  info.tolerance = tol;
  return RTHX_OK;
}

}  // namespace gs
}  // namespace rthx

namespace {

// Solve with the operator already set up on S; writes j and g to the host.
int run(Solver& S, const double* coeff, const double* h, const rthx_solve_args* args, double* j_out, double* g_out,
        rthx_solve_info* info, double t0) {
  const int64_t n = S.n;
  HIP_TRY(S.c.reserve(n * 8), "hipMalloc");
  RTHX_TRY(S.reserve(args->memory));
  HIP_TRY(hipMemcpyAsync(S.c.p, coeff, n * 8, hipMemcpyHostToDevice, S.s), "hipMemcpy");
  HIP_TRY(hipMemcpyAsync(S.h.p, h, n * 8, hipMemcpyHostToDevice, S.s), "hipMemcpy");
  rthx_solve_info I{};
  I.n = n;
  const double* c = S.c.as<double>();
  const rthx::gs::Apply M = [&S, c](const double* x, double* out) { return rthx::gs::apply(S.op, x, c, out, S.s); };
  RTHX_TRY(rthx::gs::gmres(S, M, *args, false, I));
  HIP_TRY(rthx::gs::apply(S.op, S.x.as<double>(), nullptr, S.w.as<double>(), S.s), "apply");  // g = F' j
  RTHX_TRY(S.d2h(j_out, S.x.as<double>(), n));
  RTHX_TRY(S.d2h(g_out, S.w.as<double>(), n));
  I.ms_total = now_ms() - t0;
  if (info) *info = I;
  return RTHX_OK;
}

int check_args(int64_t n, const double* coeff, const double* h, const rthx_solve_args* args, double* j_out,
               double* g_out) {
  if (n < 1 || !coeff || !h || !args || !j_out || !g_out) return fail(RTHX_EINVAL, "bad solve arguments");
  if (!(args->rtol >= 0) || !(args->atol >= 0) || args->memory < 1) return fail(RTHX_EINVAL, "bad tolerances");
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(coeff[i]) || !std::isfinite(h[i])) return fail(RTHX_EINVAL, "non-finite coeff or h");
  return RTHX_OK;
}

}  // namespace

RTHX_EXPORT int rthx_solve_grey(const int64_t* row_ptr, const int32_t* cols, const double* vals,
                                const double* dense, int64_t n, const double* coeff, const double* h,
                                const rthx_solve_args* args, double* j_out, double* g_out,
                                rthx_solve_info* info) {
  const double t0 = now_ms();
  RTHX_TRY(check_args(n, coeff, h, args, j_out, g_out));
  if (n >= (1ll << 31)) return fail(RTHX_ERANGE, "system too large");
  rthx::csr::Host Ft;  // F' of a sparse F
  if (!dense) {
    RTHX_TRY(rthx::check_host_csr(row_ptr, cols, vals, n, n, false, false));
    rthx::csr::transposed(row_ptr, cols, vals, n, n, Ft);
  }
  Solver S;
  S.n = n;
  RTHX_TRY(rthx::open_device(args->device, &S.s));
  DevBuf Fd;
  rthx::tp::DeviceCsr T;
  S.op.n = n;
  if (dense) {
    for (int64_t k = 0; k < n * n; ++k)
      if (!std::isfinite(dense[k])) return fail(RTHX_EINVAL, "non-finite F entry");
    HIP_TRY(Fd.reserve((size_t)n * n * 8), "hipMalloc dense F");
    HIP_TRY(hipMemcpyAsync(Fd.p, dense, (size_t)n * n * 8, hipMemcpyHostToDevice, S.s), "hipMemcpy F");
    HIP_TRY(S.part.reserve((size_t)rthx::gs::part_doubles(n) * 8), "hipMalloc");
    S.op.dense = true;
    S.op.F = Fd.as<double>();
    S.op.part = S.part.as<double>();
  } else {
    RTHX_TRY(T.upload(Ft.rp.data(), Ft.ci.data(), Ft.v.data(), n, Ft.nnz(), S.s));
    HIP_TRY(hipStreamSynchronize(S.s), "upload");
    S.op.dense = false;
    S.op.rp = T.rp.as<int64_t>();
    S.op.ci = T.ci.as<int32_t>();
    S.op.v = T.v.as<double>();
  }
  return run(S, coeff, h, args, j_out, g_out, info, t0);
}

RTHX_EXPORT int rthx_solve_grey_smoothed(const rthx_smooth_result* F, const double* coeff, const double* h,
                                         const rthx_solve_args* args, double* j_out, double* g_out,
                                         rthx_solve_info* info) {
  const double t0 = now_ms();
  if (!F) return fail(RTHX_EINVAL, "null smoothing result");
  RTHX_TRY(check_args(F->n, coeff, h, args, j_out, g_out));
  if (args->device != F->device) return fail(RTHX_EINVAL, "args.device differs from the result's device");
  HIP_TRY(hipSetDevice(F->device), "hipSetDevice");
  Solver S;
  S.n = F->n;
  HIP_TRY(rthx::device_stream(F->device, &S.s), "hipStreamCreate");
  S.op.n = S.n;
  if (F->dense) {
    HIP_TRY(S.part.reserve((size_t)rthx::gs::part_doubles(S.n) * 8), "hipMalloc");
    S.op.dense = true;
    S.op.F = F->F.as<double>();
    S.op.part = S.part.as<double>();
  } else {  // F' from the handle's device CSR (formed once, kept in the handle)
    S.op.dense = false;
    RTHX_TRY(rthx::tp::smooth_transposed(F, S.s, &S.op.rp, &S.op.ci, &S.op.v));
  }
  return run(S, coeff, h, args, j_out, g_out, info, t0);
}

RTHX_EXPORT int rthx_solve_grey_result(const rthx_result* counts, int64_t n, const double* coeff, const double* h,
                                       const rthx_solve_args* args, double* j_out, double* g_out,
                                       rthx_solve_info* info) {
  const double t0 = now_ms();
  if (!counts) return fail(RTHX_EINVAL, "null result");
  RTHX_TRY(rthx::result_ready(counts));  // (RTHX_ESTATE without a trace; completes a pending one)
  RTHX_TRY(check_args(n, coeff, h, args, j_out, g_out));
  if (!counts->parts.empty() || counts->device < 0)
    return fail(RTHX_EINVAL, "rthx_solve_grey_result needs a single-device result");
  if (counts->begin != 0 || counts->stride != 1 || n > counts->n_rows || n > counts->N)
    return fail(RTHX_EINVAL, "rthx_solve_grey_result needs a trace of every emitter row below n");
  if (args->device != counts->device) return fail(RTHX_EINVAL, "args.device differs from the result's device");
  if (counts->R < 1) return fail(RTHX_EINVAL, "a trace with R = 0 rays per emitter has no F_raw");
  HIP_TRY(hipSetDevice(counts->device), "hipSetDevice");
  Solver S;
  S.n = n;
  HIP_TRY(rthx::device_stream(counts->device, &S.s), "hipStreamCreate");
  rthx::tp::DeviceCsr Ft;
  RTHX_TRY(rthx::tp::transpose_result_block(counts, n, S.s, Ft));
  S.op.dense = false;
  S.op.n = n;
  S.op.rp = Ft.rp.as<int64_t>();
  S.op.ci = Ft.ci.as<int32_t>();
  S.op.v = Ft.v.as<double>();
  return run(S, coeff, h, args, j_out, g_out, info, t0);
}
