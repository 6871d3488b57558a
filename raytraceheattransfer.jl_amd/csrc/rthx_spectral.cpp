// rthx_spectral.cpp -- C ABI of the spectral GERT solve (include/rthx.h,
// rthx_solve_spectral, rthx_spectral_apply, rthx_spectral_fractions;
// DESIGN.md §7f).  The reference (equilibriumSpectral2D.jl,
// equilibriumSurfacesSpectral3D.jl) reaches its converged state by a Picard
// iteration on the emitted power with a least-squares solve per step; here
// the radiative-equilibrium rows are substituted, which leaves one square
// system in the stacked radiosities per outer iteration, solved by the
// restarted GMRES of rthx_solve.cpp (warm-started), and the outer loop only
// refreshes the emission fractions f(T).  All arguments are validated on the
// host before the first GPU call; a sparse band is checked and transposed
// there by rthx_csr_host.h and uploaded as a tp::DeviceCsr (rthx_transpose.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "rthx_common.h"
#include "rthx_smooth.h"
#include "rthx_solve.h"
#include "rthx_spectral.h"
#include "rthx_transpose.h"

using rthx::DevBuf;
using rthx::fail;
using rthx::now_ms;

namespace {

using HostCsr = rthx::csr::Host;  // F' of one sparse band on the host (validated), ready for upload

bool all_finite(const double* a, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

int check_sizes(int64_t n, int32_t n_bands, int32_t n_matrices) {
  if (n < 1 || n_bands < 1) return fail(RTHX_EINVAL, "n and n_bands must be positive");
  if (n_matrices != 1 && n_matrices != n_bands) return fail(RTHX_EINVAL, "n_matrices must be 1 or n_bands");
  if (n >= (1ll << 31)) return fail(RTHX_ERANGE, "system too large");
  if (n_bands > 65535) return fail(RTHX_ERANGE, "too many bands");
  return RTHX_OK;
}

int check_limits(const double* lim, int32_t n_bands) {
  if (!lim) return fail(RTHX_EINVAL, "null band limits");
  for (int k = 0; k <= n_bands; ++k) {
    if (!std::isfinite(lim[k]) || !(lim[k] > 0.0)) return fail(RTHX_EINVAL, "band limits must be positive");
    if (k > 0 && !(lim[k] > lim[k - 1])) return fail(RTHX_EINVAL, "band limits must be strictly increasing");
  }
  return RTHX_OK;
}

// Every band has exactly one form; sparse bands are transposed here (host).
int check_bands(const rthx_spectral_band* F, int32_t n_mats, int64_t n, int32_t device, std::vector<HostCsr>& csr) {
  if (!F) return fail(RTHX_EINVAL, "null band matrices");
  csr.resize(n_mats);
  for (int k = 0; k < n_mats; ++k) {
    const bool sparse = F[k].row_ptr || F[k].cols || F[k].vals;
    const int forms = (sparse ? 1 : 0) + (F[k].dense ? 1 : 0) + (F[k].smoothed ? 1 : 0);
    if (forms != 1) return fail(RTHX_EINVAL, "band " + std::to_string(k) + ": exactly one matrix form expected");
    if (F[k].smoothed) {
      if (F[k].smoothed->device != device) return fail(RTHX_EINVAL, "smoothing result lies on another device");
      if (F[k].smoothed->n != n) return fail(RTHX_EINVAL, "smoothing result of another size");
    } else if (F[k].dense) {
      if (!all_finite(F[k].dense, n * n)) return fail(RTHX_EINVAL, "non-finite F entry");
    } else {
      RTHX_TRY(rthx::check_host_csr(F[k].row_ptr, F[k].cols, F[k].vals, n, n, false, false));
      rthx::csr::transposed(F[k].row_ptr, F[k].cols, F[k].vals, n, n, csr[k]);
    }
  }
  return RTHX_OK;
}

int upload(DevBuf& d, const void* src, size_t bytes, hipStream_t s) {
  HIP_TRY(d.reserve(bytes), "hipMalloc");
  HIP_TRY(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, s), "hipMemcpy");
  return RTHX_OK;
}

// The band matrices on the device and the launch description of the operator.
struct Operator {
  std::vector<std::unique_ptr<DevBuf>> bufs;
  std::vector<std::unique_ptr<rthx::tp::DeviceCsr>> sparse;
  DevBuf mats, part;
  rthx::sp::BandedOp op;

  int put(const void* src, size_t bytes, hipStream_t s, void** out) {
    bufs.emplace_back(new DevBuf);
    RTHX_TRY(upload(*bufs.back(), src, bytes, s));
    *out = bufs.back()->p;
    return RTHX_OK;
  }

  int setup(const rthx_spectral_band* F, int32_t n_mats, int64_t n, int32_t K, const std::vector<HostCsr>& csr,
            hipStream_t s) {
    std::vector<rthx::sp::BandMat> host(n_mats);
    op.n = n;
    op.K = K;
    op.n_mats = n_mats;
    for (int k = 0; k < n_mats; ++k) {
      void* p = nullptr;
      if (F[k].smoothed && !F[k].smoothed->dense) {  // F' from the handle's device CSR
        RTHX_TRY(rthx::tp::smooth_transposed(F[k].smoothed, s, &host[k].rp, &host[k].ci, &host[k].v));
        op.any_sparse = true;
      } else if (F[k].smoothed) {
        host[k].F = F[k].smoothed->F.as<double>();
        op.any_dense = true;
      } else if (F[k].dense) {
        RTHX_TRY(put(F[k].dense, (size_t)n * n * 8, s, &p));
        host[k].F = static_cast<const double*>(p);
        op.any_dense = true;
      } else {
        sparse.emplace_back(new rthx::tp::DeviceCsr);
        rthx::tp::DeviceCsr& T = *sparse.back();
        RTHX_TRY(T.upload(csr[k].rp.data(), csr[k].ci.data(), csr[k].v.data(), n, csr[k].nnz(), s));
        host[k].rp = T.rp.as<int64_t>();
        host[k].ci = T.ci.as<int32_t>();
        host[k].v = T.v.as<double>();
        op.any_sparse = true;
      }
    }
    RTHX_TRY(upload(mats, host.data(), host.size() * sizeof(rthx::sp::BandMat), s));
    HIP_TRY(hipStreamSynchronize(s), "upload");
    op.mats = mats.as<rthx::sp::BandMat>();
    op.shared_F = n_mats == 1 ? host[0].F : nullptr;
    if (op.any_dense) {
      HIP_TRY(part.reserve((size_t)K * rthx::sp::part_doubles(n) * 8), "hipMalloc");
      op.part = part.as<double>();
    }
    return RTHX_OK;
  }
};

// HIP-event time summed over the banded applies.  Every apply is followed by
// a stream synchronisation (a norm or a Hessenberg column read back) before
// the next one, so the pending pair is complete when it is read.
struct ApplyTimer {
  rthx::EventPair ev;
  bool pending = false;
  double ms = 0.0;
  hipError_t collect() {
    if (!pending) return hipSuccess;
    hipError_t e = hipEventSynchronize(ev.e[1]);
    if (e != hipSuccess) return e;
    float t = 0.f;
    e = ev.elapsed(&t);
    if (e != hipSuccess) return e;
    ms += t;
    pending = false;
    return hipSuccess;
  }
};

}  // namespace

RTHX_EXPORT int rthx_solve_spectral(const rthx_spectral_band* F, int32_t n_matrices, int64_t n, int32_t n_bands,
                                    const double* band_limits, const double* b, const double* prop,
                                    const double* size, const double* T_in, const double* q_in,
                                    const rthx_spectral_args* args, double* j_out, double* g_out, double* T_out,
                                    double* e_out, rthx_spectral_info* info) {
  namespace sp = rthx::sp;
  namespace gs = rthx::gs;
  const double t0 = now_ms();
  if (!F || !b || !prop || !size || !T_in || !q_in || !args || !j_out || !g_out || !T_out || !e_out)
    return fail(RTHX_EINVAL, "bad spectral solve arguments");
  RTHX_TRY(check_sizes(n, n_bands, n_matrices));
  if (!(args->rtol >= 0) || !(args->atol >= 0) || args->memory < 1 || args->max_outer < 1 ||
      !(args->convergence_tol >= 0))
    return fail(RTHX_EINVAL, "bad tolerances");
  RTHX_TRY(check_limits(band_limits, n_bands));
  const int K = n_bands;
  const int64_t N = (int64_t)K * n;
  if (!all_finite(b, N) || !all_finite(prop, N) || !all_finite(size, n) || !all_finite(T_in, n) ||
      !all_finite(q_in, n))
    return fail(RTHX_EINVAL, "non-finite input");
  for (int64_t p = 0; p < N; ++p)
    if (b[p] < 0.0 || b[p] > 1.0) return fail(RTHX_EINVAL, "b outside [0, 1]");
  // P: prescribed temperature (T_in > -0.1); R: radiative equilibrium
  std::vector<uint8_t> radeq(n);
  std::vector<double> T0(n);
  double t_max = -1.0;
  for (int64_t i = 0; i < n; ++i) {
    radeq[i] = T_in[i] > -0.1 ? 0 : 1;
    if (!radeq[i]) t_max = std::max(t_max, T_in[i]);
  }
  if (t_max < -0.1) return fail(RTHX_EINVAL, "no element with a prescribed temperature");
  const double t_start = t_max > 0.0 ? t_max : 1000.0;  // first iterate of the unknown temperatures
  for (int64_t i = 0; i < n; ++i) T0[i] = radeq[i] ? t_start : T_in[i];
  std::vector<HostCsr> csr;
  RTHX_TRY(check_bands(F, n_matrices, n, args->device, csr));

  hipStream_t s = nullptr;
  RTHX_TRY(rthx::open_device(args->device, &s));
  Operator A;
  RTHX_TRY(A.setup(F, n_matrices, n, K, csr, s));
  gs::Krylov S;
  S.s = s;
  S.n = N;
  RTHX_TRY(S.reserve(args->memory));
  DevBuf db, dprop, dsize, dTin, dq, dradeq, dlim, dT, de, df, dplain, dg, dprev;
  RTHX_TRY(upload(db, b, N * 8, s));
  RTHX_TRY(upload(dprop, prop, N * 8, s));
  RTHX_TRY(upload(dsize, size, n * 8, s));
  RTHX_TRY(upload(dTin, T_in, n * 8, s));
  RTHX_TRY(upload(dq, q_in, n * 8, s));
  RTHX_TRY(upload(dradeq, radeq.data(), n, s));
  RTHX_TRY(upload(dlim, band_limits, (size_t)(K + 1) * 8, s));
  RTHX_TRY(upload(dT, T0.data(), n * 8, s));
  HIP_TRY(de.reserve(n * 8), "hipMalloc");
  HIP_TRY(df.reserve(N * 8), "hipMalloc");
  HIP_TRY(dplain.reserve(N * 8), "hipMalloc");
  HIP_TRY(dg.reserve(N * 8), "hipMalloc");
  HIP_TRY(dprev.reserve(N * 8), "hipMalloc");
  HIP_TRY(hipMemsetAsync(de.p, 0, n * 8, s), "hipMemset");
  HIP_TRY(hipMemsetAsync(S.x.p, 0, N * 8, s), "hipMemset");
  HIP_TRY(hipStreamSynchronize(s), "upload");
  const double* pb = db.as<double>();
  const double* pprop = dprop.as<double>();
  const double* plim = dlim.as<double>();
  const uint8_t* pre = dradeq.as<uint8_t>();
  double* pT = dT.as<double>();
  double* pe = de.as<double>();
  double* pf = df.as<double>();
  double* pg = dg.as<double>();
  double* x = S.x.as<double>();
  double* sm = S.small.as<double>();

  ApplyTimer timer;
  HIP_TRY(timer.ev.create(), "hipEventCreate");
  auto timed_apply = [&](const double* in, double* out) -> hipError_t {
    hipError_t e = timer.collect();
    if (e != hipSuccess) return e;
    if ((e = timer.ev.start(s)) != hipSuccess) return e;
    if ((e = sp::apply(A.op, in, pb, pf, pre, pg, out, s)) != hipSuccess) return e;
    if ((e = timer.ev.stop(s)) != hipSuccess) return e;
    timer.pending = true;
    return hipSuccess;
  };
  const gs::Apply M = timed_apply;

  rthx_solve_args sa{};
  sa.device = args->device;
  sa.memory = args->memory;
  sa.itmax = args->itmax;
  sa.rtol = args->rtol;
  sa.atol = args->atol;
  rthx_spectral_info I{};
  I.n = n;
  I.n_bands = K;
  // prescribed elements: T = T_in and their emitted power, once
  HIP_TRY(sp::temperatures(plim, K, pprop, dsize.as<double>(), dTin.as<double>(), pre, false, n, pe, pT, s),
          "temperatures");
  for (int outer = 1; outer <= args->max_outer; ++outer) {
    HIP_TRY(sp::fractions(plim, K, pT, pprop, n, dplain.as<double>(), pf, s), "fractions");
    HIP_TRY(sp::rhs(pf, pe, dq.as<double>(), pre, n, K, S.h.as<double>(), s), "rhs");
    HIP_TRY(hipMemcpyAsync(dprev.p, x, N * 8, hipMemcpyDeviceToDevice, s), "hipMemcpy");
    rthx_solve_info L{};
    RTHX_TRY(gs::gmres(S, M, sa, outer > 1, L));
    I.outer_iterations = outer;
    I.gmres_iterations += L.iterations;
    I.residual = L.residual;
    I.tolerance = L.tolerance;
    HIP_TRY(timed_apply(x, nullptr), "apply");  // g = F' j
    HIP_TRY(gs::sub(x, dprev.as<double>(), N, S.r.as<double>(), s), "sub");
    HIP_TRY(gs::multidot(S.r.as<double>(), S.r.as<double>(), 1, N, sm, s), "multidot");
    HIP_TRY(gs::multidot(x, x, 1, N, sm + 1, s), "multidot");
    HIP_TRY(sp::emission(x, pb, pg, pre, n, K, pe, s), "emission");
    HIP_TRY(sp::temperatures(plim, K, pprop, dsize.as<double>(), dTin.as<double>(), pre, true, n, pe, pT, s),
            "temperatures");
    double d[2];
    RTHX_TRY(S.d2h(d, sm, 2));
    I.change = d[1] > 0.0 ? std::sqrt(d[0] / d[1]) : 0.0;
    // converged: the reference's criterion, or a warm start that already
    // solves the system of the refreshed fractions (GMRES took no step)
    if (L.converged && (I.change < args->convergence_tol || (outer > 1 && L.iterations == 0))) {
      I.converged = 1;
      break;
    }
  }
  HIP_TRY(timer.collect(), "hipEventElapsedTime");
  RTHX_TRY(S.d2h(j_out, x, N));
  RTHX_TRY(S.d2h(g_out, pg, N));
  RTHX_TRY(S.d2h(T_out, pT, n));
  RTHX_TRY(S.d2h(e_out, pe, n));
  I.ms_apply = timer.ms;
  I.ms_total = now_ms() - t0;
  if (info) *info = I;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_spectral_apply(const rthx_spectral_band* F, int32_t n_matrices, int64_t n, int32_t n_bands,
                                    int32_t device, const double* x, const double* b, const double* f,
                                    const uint8_t* is_radeq, double* g_out, double* y_out) {
  if (!F || !x || !g_out || (y_out && (!b || !f))) return fail(RTHX_EINVAL, "bad spectral apply arguments");
  RTHX_TRY(check_sizes(n, n_bands, n_matrices));
  const int64_t N = (int64_t)n_bands * n;
  if (!all_finite(x, N) || (y_out && (!all_finite(b, N) || !all_finite(f, N))))
    return fail(RTHX_EINVAL, "non-finite input");
  std::vector<HostCsr> csr;
  RTHX_TRY(check_bands(F, n_matrices, n, device, csr));
  hipStream_t s = nullptr;
  RTHX_TRY(rthx::open_device(device, &s));
  Operator A;
  RTHX_TRY(A.setup(F, n_matrices, n, n_bands, csr, s));
  DevBuf dx, db, df, dre, dg, dy;
  RTHX_TRY(upload(dx, x, N * 8, s));
  HIP_TRY(dg.reserve(N * 8), "hipMalloc");
  std::vector<uint8_t> none;
  if (y_out) {
    RTHX_TRY(upload(db, b, N * 8, s));
    RTHX_TRY(upload(df, f, N * 8, s));
    if (!is_radeq) none.assign(n, 0);
    RTHX_TRY(upload(dre, is_radeq ? is_radeq : none.data(), n, s));
    HIP_TRY(dy.reserve(N * 8), "hipMalloc");
  }
  HIP_TRY(rthx::sp::apply(A.op, dx.as<double>(), db.as<double>(), df.as<double>(), dre.as<uint8_t>(), dg.as<double>(),
                          y_out ? dy.as<double>() : nullptr, s),
          "apply");
  HIP_TRY(hipMemcpyAsync(g_out, dg.p, N * 8, hipMemcpyDeviceToHost, s), "hipMemcpy");
  if (y_out) HIP_TRY(hipMemcpyAsync(y_out, dy.p, N * 8, hipMemcpyDeviceToHost, s), "hipMemcpy");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return RTHX_OK;
}

RTHX_EXPORT int rthx_spectral_fractions(const double* band_limits, int32_t n_bands, const double* T,
                                        const double* prop, int64_t n, int32_t device, double* plain_out,
                                        double* weighted_out) {
  if (!T || !plain_out) return fail(RTHX_EINVAL, "bad spectral fractions arguments");
  RTHX_TRY(check_sizes(n, n_bands, 1));
  RTHX_TRY(check_limits(band_limits, n_bands));
  const int64_t N = (int64_t)n_bands * n;
  if (prop && !all_finite(prop, N)) return fail(RTHX_EINVAL, "non-finite input");
  hipStream_t s = nullptr;
  RTHX_TRY(rthx::open_device(device, &s));
  DevBuf dlim, dT, dprop, dplain, dw;
  RTHX_TRY(upload(dlim, band_limits, (size_t)(n_bands + 1) * 8, s));
  RTHX_TRY(upload(dT, T, n * 8, s));
  if (prop) RTHX_TRY(upload(dprop, prop, N * 8, s));
  HIP_TRY(dplain.reserve(N * 8), "hipMalloc");
  if (weighted_out) HIP_TRY(dw.reserve(N * 8), "hipMalloc");
  HIP_TRY(rthx::sp::fractions(dlim.as<double>(), n_bands, dT.as<double>(), prop ? dprop.as<double>() : nullptr, n,
                              dplain.as<double>(), weighted_out ? dw.as<double>() : nullptr, s),
          "fractions");
  HIP_TRY(hipMemcpyAsync(plain_out, dplain.p, N * 8, hipMemcpyDeviceToHost, s), "hipMemcpy");
  if (weighted_out) HIP_TRY(hipMemcpyAsync(weighted_out, dw.p, N * 8, hipMemcpyDeviceToHost, s), "hipMemcpy");
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  return RTHX_OK;
}

// The operator alone, timed call by call with HIP events, for
// tools/bench_spectral_solve.py; not part of include/rthx.h.  mode 0: the
// banded apply (every element in radiative equilibrium: the full mix); mode 1:
// the same K products as K launches of the grey operator x_k - c_k .* F_k' x_k
// (rthx_solve.h apply), dense matrices only.  ms_out[reps].
RTHX_EXPORT int rthx_debug_spectral_apply_times(const rthx_spectral_band* F, int32_t n_matrices, int64_t n,
                                                int32_t n_bands, int32_t device, int32_t mode, int32_t warmup,
                                                int32_t reps, double* ms_out) {
  if (!F || !ms_out || reps < 1 || warmup < 0 || (mode != 0 && mode != 1))
    return fail(RTHX_EINVAL, "bad apply timing arguments");
  RTHX_TRY(check_sizes(n, n_bands, n_matrices));
  std::vector<HostCsr> csr;
  RTHX_TRY(check_bands(F, n_matrices, n, device, csr));
  hipStream_t s = nullptr;
  RTHX_TRY(rthx::open_device(device, &s));
  Operator A;
  RTHX_TRY(A.setup(F, n_matrices, n, n_bands, csr, s));
  if (mode == 1 && A.op.any_sparse) return fail(RTHX_EINVAL, "sequential grey applies: dense matrices only");
  const int64_t N = (int64_t)n_bands * n;
  std::vector<double> half(N, 0.5);
  std::vector<uint8_t> ones(n, 1);
  DevBuf dx, db, df, dre, dg, dy, gpart;
  RTHX_TRY(upload(dx, half.data(), N * 8, s));
  RTHX_TRY(upload(db, half.data(), N * 8, s));
  RTHX_TRY(upload(df, half.data(), N * 8, s));
  RTHX_TRY(upload(dre, ones.data(), n, s));
  HIP_TRY(dg.reserve(N * 8), "hipMalloc");
  HIP_TRY(dy.reserve(N * 8), "hipMalloc");
  HIP_TRY(gpart.reserve((size_t)rthx::gs::part_doubles(n) * 8), "hipMalloc");
  std::vector<rthx::sp::BandMat> mats(n_matrices);
  HIP_TRY(hipMemcpyAsync(mats.data(), A.mats.p, mats.size() * sizeof(rthx::sp::BandMat), hipMemcpyDeviceToHost, s),
          "hipMemcpy");
  HIP_TRY(hipStreamSynchronize(s), "upload");
  std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e), "hipEventCreate");
  for (int it = -warmup; it < reps; ++it) {
    if (it >= 0) HIP_TRY(hipEventRecord(ev[2 * it], s), "hipEventRecord");
    if (mode == 0) {
      HIP_TRY(rthx::sp::apply(A.op, dx.as<double>(), db.as<double>(), df.as<double>(), dre.as<uint8_t>(),
                              dg.as<double>(), dy.as<double>(), s),
              "apply");
    } else {
      for (int k = 0; k < n_bands; ++k) {
        rthx::gs::Op op;
        op.n = n;
        op.F = mats[n_matrices == 1 ? 0 : k].F;
        op.part = gpart.as<double>();
        HIP_TRY(rthx::gs::apply(op, dx.as<double>() + (int64_t)k * n, db.as<double>() + (int64_t)k * n,
                                dy.as<double>() + (int64_t)k * n, s),
                "apply");
      }
    }
    if (it >= 0) HIP_TRY(hipEventRecord(ev[2 * it + 1], s), "hipEventRecord");
  }
  HIP_TRY(hipStreamSynchronize(s), "hipStreamSynchronize");
  for (int it = 0; it < reps; ++it) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, ev[2 * it], ev[2 * it + 1]), "hipEventElapsedTime");
    ms_out[it] = t;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return RTHX_OK;
}
