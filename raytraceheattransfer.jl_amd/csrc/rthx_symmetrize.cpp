// rthx_symmetrize.cpp -- host side of the device CSR symmetrisation
// (rthx_symmetrize_kernels.hip): the steps of one build, shared
// with the sparse smoothing set-up (rthx_smooth.cpp), and the C ABI of the
// primitive (include/rthx.h rthx_csr_symmetrize).
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
  const int64_t n = A.n_rows, nnz = A.nnz;
  const size_t m = (size_t)std::max<int64_t>(nnz, 1);
  W.P = tp::plan_transpose(n, nnz, A.counts ? 4 : 8);
  HIP_TRY(W.tscratch.reserve((size_t)W.P.scratch_bytes), "hipMalloc transpose scratch");
  HIP_TRY(W.T.rp.reserve((size_t)(n + 1) * 8), "hipMalloc");
  HIP_TRY(W.T.ci.reserve(m * 4), "hipMalloc");
  HIP_TRY(W.T.v.reserve(m * 8), "hipMalloc");
  HIP_TRY(W.mark.reserve(m * 4), "hipMalloc symmetrise marks");
  HIP_TRY(W.len.reserve((size_t)std::max<int64_t>(n, 1) * 8), "hipMalloc symmetrise lengths");
  W.T.nnz = nnz;
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
  tp::Dest D;
  D.t_off = W.T.rp.as<int64_t>();
  D.rows32 = W.T.ci.as<int32_t>();
  D.vals = W.T.v.as<double>();
  const hipError_t e = tp::transpose(A, D, W.P, W.tscratch.p, st);
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
  if (row_ptr[0] != 0) return fail(RTHX_EINVAL, "row_ptr[0] != 0");
  for (int64_t i = 0; i < n; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return fail(RTHX_EINVAL, "row_ptr not monotone");
    if (row_ptr[i + 1] >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31");
  }
  const int64_t nnz = row_ptr[n];
  if (nnz > 0 && (!cols || !vals)) return fail(RTHX_EINVAL, "null CSR arrays");
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      if (cols[k] < 0 || cols[k] >= n || !std::isfinite(vals[k])) return fail(RTHX_EINVAL, "bad CSR entry");
      if (k > row_ptr[i] && !(cols[k - 1] < cols[k]))
        return fail(RTHX_EINVAL, "row " + std::to_string(i) + " is not strictly column-ascending");
    }
  if (w)
    for (int64_t i = 0; i < n; ++i)
      if (!std::isfinite(w[i])) return fail(RTHX_EINVAL, "weights must be finite");
  if (x_cap < 0) x_cap = 0;
  if (x_cap > 0 && (!x_cols || !x_vals)) return fail(RTHX_EINVAL, "null output arrays");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(RTHX_EDEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RTHX_EINVAL, "device ordinal out of range");
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIP_TRY(rthx::device_stream(device, &st), "device stream");
  // everything is allocated before the timed stretch; 2 nnz entries always suffice for X
  const size_t m = (size_t)std::max<int64_t>(nnz, 1);
  const int64_t cap = std::min<int64_t>(x_cap, 2 * nnz);
  DevBuf rp, ci, v, dw, xrp, xci, xv;
  HIP_TRY(rp.reserve((size_t)(n + 1) * 8), "hipMalloc");
  HIP_TRY(ci.reserve(m * 4), "hipMalloc");
  HIP_TRY(v.reserve(m * 8), "hipMalloc");
  HIP_TRY(xrp.reserve((size_t)(n + 1) * 8), "hipMalloc");
  HIP_TRY(xci.reserve((size_t)std::max<int64_t>(cap, 1) * 4), "hipMalloc");
  HIP_TRY(xv.reserve((size_t)std::max<int64_t>(cap, 1) * 8), "hipMalloc");
  HIP_TRY(hipMemcpyAsync(rp.p, row_ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  if (nnz) {
    HIP_TRY(hipMemcpyAsync(ci.p, cols, (size_t)nnz * 4, hipMemcpyHostToDevice, st), "hipMemcpy");
    HIP_TRY(hipMemcpyAsync(v.p, vals, (size_t)nnz * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  }
  if (w && n) {
    HIP_TRY(dw.reserve((size_t)n * 8), "hipMalloc");
    HIP_TRY(hipMemcpyAsync(dw.p, w, (size_t)n * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  }
  tp::Source S;
  S.n_rows = n;
  S.n_cols = n;
  S.nnz = nnz;
  S.off = rp.as<int64_t>();
  S.src = S.off;
  S.cols = ci.as<uint32_t>();
  S.vals = v.as<double>();
  sym::Work W;
  if (int rc = sym::reserve(S, W)) return rc;
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(hipEventCreate(&ev[0]), "hipEventCreate");
  HIP_TRY(hipEventCreate(&ev[1]), "hipEventCreate");
  int64_t total = 0;
  bool fits = false;
  hipError_t e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) e = sym::enqueue_lengths(S, W, xrp.as<int64_t>(), st);
  // (the host reads the total between the passes: the event time includes that round trip)
  if (e == hipSuccess) e = hipMemcpyAsync(&total, xrp.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) {
    fits = total <= cap;
    if (fits) e = sym::enqueue_write(S, W, w && n ? dw.as<double>() : nullptr, xrp.as<int64_t>(), xci.as<int32_t>(),
                                     xv.as<double>(), st);
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], st);
  if (e == hipSuccess) e = hipMemcpyAsync(x_row_ptr, xrp.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && fits && total) {
    e = hipMemcpyAsync(x_cols, xci.p, (size_t)total * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(x_vals, xv.p, (size_t)total * 8, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (e != hipSuccess) return rthx::hip_fail(e, "CSR symmetrise");
  *x_nnz = total;
  if (device_ms) *device_ms = ms;
  if (!fits)
    return fail(RTHX_ERANGE, "x_cap = " + std::to_string(x_cap) + " is below the " + std::to_string(total) +
                                 " entries of X");
  return RTHX_OK;
}
