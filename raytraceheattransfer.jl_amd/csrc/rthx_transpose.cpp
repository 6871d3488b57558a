// rthx_transpose.cpp -- host side of the device CSR -> CSC transpose
// (rthx_transpose_kernels.hip): the C ABI of the primitive
// (include/rthx.h rthx_csr_transpose) and the helpers that form F' for the
// sparse GERT operators from a trace result's counts and from a sparse
// smoothing result, where they lie.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rthx_domain.h"
#include "rthx_smooth.h"
#include "rthx_transpose.h"

using rthx::DevBuf;
using rthx::fail;

namespace rthx {
namespace tp {

int result_block(const rthx_result* res, int64_t n, hipStream_t st, Block& B) {
  if (res->info.nnz >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31 for the device transpose");
  DevBuf len;
  HIP_TRY(B.tallied.reserve((size_t)n * 8), "hipMalloc tallied");
  HIP_TRY(B.src.reserve((size_t)n * 8), "hipMalloc row starts");
  HIP_TRY(len.reserve((size_t)n * 8), "hipMalloc row lengths");
  HIP_TRY(B.off.reserve((size_t)(n + 1) * 8), "hipMalloc row offsets");
  HIP_TRY(block_rows(res->row_off.as<int64_t>(), res->cols.as<uint32_t>(), res->cnt.as<uint32_t>(), n, n, res->N,
                     B.tallied.as<double>(), B.src.as<int64_t>(), len.as<int64_t>(), B.off.as<int64_t>(), st),
          "block rows launch");
  int64_t nnz = 0;
  HIP_TRY(hipMemcpyAsync(&nnz, B.off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st), "hipMemcpy block nnz");
  HIP_TRY(hipStreamSynchronize(st), "block rows");
  Source& S = B.S;
  S.n_rows = n;
  S.n_cols = n;
  S.nnz = nnz;
  S.off = B.off.as<int64_t>();
  S.src = B.src.as<int64_t>();
  S.whole = 0;
  S.cols = res->cols.as<uint32_t>();
  S.counts = res->cnt.as<uint32_t>();
  S.tallied = B.tallied.as<double>();
  return RTHX_OK;
}

int transpose_result_block(const rthx_result* res, int64_t n, hipStream_t st, Transposed& out) {
  Block B;
  if (int rc = result_block(res, n, st, B)) return rc;
  const Source& S = B.S;
  const int64_t nnz = S.nnz;
  DevBuf scratch;
  const Plan P = plan_transpose(n, nnz, 4);
  HIP_TRY(scratch.reserve((size_t)P.scratch_bytes), "hipMalloc transpose scratch");
  HIP_TRY(out.rp.reserve((size_t)(n + 1) * 8), "hipMalloc");
  HIP_TRY(out.ci.reserve((size_t)std::max<int64_t>(nnz, 1) * 4), "hipMalloc");
  HIP_TRY(out.v.reserve((size_t)std::max<int64_t>(nnz, 1) * 8), "hipMalloc");
  out.nnz = nnz;
  Dest D;
  D.t_off = out.rp.as<int64_t>();
  D.rows32 = out.ci.as<int32_t>();
  D.vals = out.v.as<double>();
  HIP_TRY(transpose(S, D, P, scratch.p, st), "transpose launch");
  HIP_TRY(hipStreamSynchronize(st), "transpose");  // (the scratch is freed on return)
  return RTHX_OK;
}

int smooth_transposed(const rthx_smooth_result* cF, hipStream_t st, const int64_t** rp, const int32_t** ci,
                      const double** v) {
  rthx_smooth_result* F = const_cast<rthx_smooth_result*>(cF);
  if (!F->have_t) {
    const int64_t n = F->n, nnz = F->nnz;
    if (nnz >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31 for the device transpose");
    const Plan P = plan_transpose(n, nnz, 8);
    DevBuf scratch;
    HIP_TRY(scratch.reserve((size_t)P.scratch_bytes), "hipMalloc transpose scratch");
    HIP_TRY(F->trp.reserve((size_t)(n + 1) * 8), "hipMalloc");
    HIP_TRY(F->tci.reserve((size_t)std::max<int64_t>(nnz, 1) * 4), "hipMalloc");
    HIP_TRY(F->tv.reserve((size_t)std::max<int64_t>(nnz, 1) * 8), "hipMalloc");
    Source S;
    S.n_rows = n;
    S.n_cols = n;
    S.nnz = nnz;
    S.off = F->rp.as<int64_t>();
    S.src = S.off;
    S.cols = F->ci.as<uint32_t>();
    S.vals = F->F.as<double>();
    Dest D;
    D.t_off = F->trp.as<int64_t>();
    D.rows32 = F->tci.as<int32_t>();
    D.vals = F->tv.as<double>();
    HIP_TRY(transpose(S, D, P, scratch.p, st), "transpose launch");
    HIP_TRY(hipStreamSynchronize(st), "transpose");
    F->have_t = true;
  }
  *rp = F->trp.as<int64_t>();
  *ci = F->tci.as<int32_t>();
  *v = F->tv.as<double>();
  return RTHX_OK;
}

}  // namespace tp
}  // namespace rthx

RTHX_EXPORT int rthx_csr_transpose(int32_t device, int64_t n_rows, int64_t n_cols, const int64_t* row_ptr,
                                   const int32_t* cols, const double* vals, int64_t* t_row_ptr, int32_t* t_cols,
                                   double* t_vals, double* device_ms) {
  namespace tp = rthx::tp;
  if (n_rows < 0 || n_cols < 0 || !row_ptr || !t_row_ptr) return fail(RTHX_EINVAL, "bad transpose arguments");
  if (n_rows >= (int64_t(1) << 31) || n_cols >= (int64_t(1) << 31))
    return fail(RTHX_ERANGE, "n_rows and n_cols must be below 2^31");
  if (row_ptr[0] != 0) return fail(RTHX_EINVAL, "row_ptr[0] != 0");
  for (int64_t i = 0; i < n_rows; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return fail(RTHX_EINVAL, "row_ptr not monotone");
    if (row_ptr[i + 1] >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31");
  }
  const int64_t nnz = row_ptr[n_rows];
  if (nnz > 0 && (!cols || !vals || !t_cols || !t_vals)) return fail(RTHX_EINVAL, "null CSR arrays");
  for (int64_t k = 0; k < nnz; ++k)
    if (cols[k] < 0 || cols[k] >= n_cols || !std::isfinite(vals[k])) return fail(RTHX_EINVAL, "bad CSR entry");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(RTHX_EDEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(RTHX_EINVAL, "device ordinal out of range");
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIP_TRY(rthx::device_stream(device, &st), "device stream");
  const tp::Plan P = tp::plan_transpose(n_cols, nnz, 8);
  const size_t m = (size_t)std::max<int64_t>(nnz, 1);
  DevBuf rp, ci, v, trp, tci, tv, scratch;
  HIP_TRY(rp.reserve((size_t)(n_rows + 1) * 8), "hipMalloc");
  HIP_TRY(ci.reserve(m * 4), "hipMalloc");
  HIP_TRY(v.reserve(m * 8), "hipMalloc");
  HIP_TRY(trp.reserve((size_t)(n_cols + 1) * 8), "hipMalloc");
  HIP_TRY(tci.reserve(m * 4), "hipMalloc");
  HIP_TRY(tv.reserve(m * 8), "hipMalloc");
  HIP_TRY(scratch.reserve((size_t)P.scratch_bytes), "hipMalloc transpose scratch");
  HIP_TRY(hipMemcpyAsync(rp.p, row_ptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  if (nnz) {
    HIP_TRY(hipMemcpyAsync(ci.p, cols, (size_t)nnz * 4, hipMemcpyHostToDevice, st), "hipMemcpy");
    HIP_TRY(hipMemcpyAsync(v.p, vals, (size_t)nnz * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  }
  tp::Source S;
  S.n_rows = n_rows;
  S.n_cols = n_cols;
  S.nnz = nnz;
  S.off = rp.as<int64_t>();
  S.src = S.off;
  S.cols = ci.as<uint32_t>();
  S.vals = v.as<double>();
  tp::Dest D;
  D.t_off = trp.as<int64_t>();
  D.rows32 = tci.as<int32_t>();
  D.vals = tv.as<double>();
  hipEvent_t ev[2] = {nullptr, nullptr};
  HIP_TRY(hipEventCreate(&ev[0]), "hipEventCreate");
  HIP_TRY(hipEventCreate(&ev[1]), "hipEventCreate");
  hipError_t e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) e = tp::transpose(S, D, P, scratch.p, st);
  if (e == hipSuccess) e = hipEventRecord(ev[1], st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_row_ptr, trp.p, (size_t)(n_cols + 1) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(t_cols, tci.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(t_vals, tv.p, (size_t)nnz * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  float ms = 0.f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (e != hipSuccess) return rthx::hip_fail(e, "CSR transpose");
  if (device_ms) *device_ms = ms;
  return RTHX_OK;
}
