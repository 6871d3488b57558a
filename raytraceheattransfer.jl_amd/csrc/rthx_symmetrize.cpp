// rthx_symmetrize.cpp -- host side of the device CSR symmetrisation
// (rthx_symmetrize_kernels.hip): the steps of one build, shared
// with the sparse smoothing set-up (rthx_smooth.cpp), and the C ABI of the
// primitive (include/rthx.h rthx_csr_symmetrize).  The caller's matrix is
// checked by rthx_csr_host.h; the device CSR, the transpose's reserve and
// enqueue steps and the device opening come from rthx_transpose.h and
// rthx_common.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "rthx_symmetrize.h"

using rthx::DevBuf;
using rthx::fail;

namespace rthx {
namespace sym {

int reserve(const tp::Source& A, Work& W) {
  RTHX_TRY(tp::reserve_transpose(A, W.ts, W.T));
  HIP_TRY(W.mark.reserve((size_t)std::max<int64_t>(A.nnz, 1) * 4), "hipMalloc symmetrise marks");
  HIP_TRY(W.len.reserve((size_t)std::max<int64_t>(A.n_rows, 1) * 8), "hipMalloc symmetrise lengths");
  return RTHX_OK;
}

static Pair pair_of(const tp::Source& A, const Work& W) {
  Pair J;
  J.A = A;
  J.t_off = W.T.rp.as<int64_t>();
  J.t_cols = W.T.ci.as<int32_t>();
  J.t_vals = W.T.v.as<double>();
  return J;
}

hipError_t enqueue_lengths(const tp::Source& A, Work& W, int64_t* x_off, hipStream_t st) {
  const hipError_t e = tp::enqueue_transpose(A, W.ts, W.T, st);
  if (e != hipSuccess) return e;
  return lengths(pair_of(A, W), W.mark.as<uint32_t>(), W.len.as<int64_t>(), x_off, st);
}

hipError_t enqueue_write(const tp::Source& A, const Work& W, const double* w, const int64_t* x_off, int32_t* x_cols,
                         double* x_vals, hipStream_t st) {
  return write(pair_of(A, W), w, W.mark.as<uint32_t>(), x_off, x_cols, x_vals, st);
}

}  // namespace sym
}  // namespace rthx

RTHX_EXPORT int rthx_csr_symmetrize(int32_t device, int64_t n, const int64_t* row_ptr, const int32_t* cols,
                                    const double* vals, const double* w, int64_t x_cap, int64_t* x_row_ptr,
                                    int32_t* x_cols, double* x_vals, int64_t* x_nnz, double* device_ms) {
  namespace tp = rthx::tp;
  namespace sym = rthx::sym;
  if (n < 0 || !row_ptr || !x_row_ptr || !x_nnz) return fail(RTHX_EINVAL, "bad symmetrise arguments");
  if (n >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "n must be below 2^31");
  RTHX_TRY(rthx::check_host_csr(row_ptr, cols, vals, n, n, true, true));
  const int64_t nnz = row_ptr[n];
  if (w)
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(w[i])) return fail(RTHX_EINVAL, "weights must be finite");
  if (x_cap < 0) x_cap = 0;
  if (x_cap > 0 && (!x_cols || !x_vals)) return fail(RTHX_EINVAL, "null output arrays");
  rthx::DeviceGuard keep_device;
  hipStream_t st = nullptr;
  RTHX_TRY(rthx::open_device(device, &st));
  // everything is allocated before the timed stretch; 2 nnz entries always suffice for X
  const int64_t cap = std::min<int64_t>(x_cap, 2 * nnz);
  tp::DeviceCsr A, X;
  DevBuf dw;
  RTHX_TRY(A.upload(row_ptr, cols, vals, n, nnz, st));
  RTHX_TRY(X.reserve(n, cap));
  if (w && n) {
    HIP_TRY(dw.reserve((size_t)n * 8), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(dw.p, w, (size_t)n * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  }
  const tp::Source S = A.source(n, n);
  sym::Work W;
  RTHX_TRY(sym::reserve(S, W));
  rthx::EventPair ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  int64_t total = 0;
  bool fits = false;
  hipError_t e = ev.start(st);
  if (e == hipSuccess) e = sym::enqueue_lengths(S, W, X.rp.as<int64_t>(), st);
  // (the host reads the total between the passes: the event time includes that round trip)
  if (e == hipSuccess) e = hipMemcpyAsync(&total, X.rp.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) {
    fits = total <= cap;
    if (fits) e = sym::enqueue_write(S, W, w && n ? dw.as<double>() : nullptr, X.rp.as<int64_t>(), X.ci.as<int32_t>(),
                                     X.v.as<double>(), st);
  }
  if (e == hipSuccess) e = ev.stop(st);
  if (e == hipSuccess) e = hipMemcpyAsync(x_row_ptr, X.rp.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && fits && total) {
    e = hipMemcpyAsync(x_cols, X.ci.p, (size_t)total * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(x_vals, X.v.p, (size_t)total * 8, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  float ms = 0.f;
  if (e == hipSuccess) e = ev.elapsed(&ms);
  if (e != hipSuccess) return rthx::hip_fail(e, "CSR symmetrise");
  *x_nnz = total;
  if (device_ms) *device_ms = ms;
  if (!fits)
    return fail(RTHX_ERANGE, "x_cap = " + std::to_string(x_cap) + " is below the " + std::to_string(total) +
                                 " entries of X");
  return RTHX_OK;
}
