// rthx_transpose.cpp -- host side of the device CSR -> CSC transpose
// (rthx_transpose_kernels.hip): the device CSR and the
// reserve / enqueue steps of one transpose (rthx_transpose.h), which every
// user of the kernels goes through; the helpers that form F' for the sparse
// GERT operators from a trace result's counts and from a sparse smoothing
// result, where they lie; and the C ABI of the primitive (include/rthx.h
// rthx_csr_transpose).  A caller's host matrix is checked by rthx_csr_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rthx_domain.h"
#include "rthx_smooth.h"
#include "rthx_transpose.h"

using rthx::fail;

namespace rthx {
namespace tp {

int DeviceCsr::reserve(int64_t n_rows, int64_t nnz_) {
  const size_t m = (size_t)std::max<int64_t>(nnz_, 1);
  HIP_TRY(rp.reserve((size_t)(n_rows + 1) * 8), "hipMalloc");
  HIP_TRY(ci.reserve(m * 4), "hipMalloc");
  HIP_TRY(v.reserve(m * 8), "hipMalloc");
  nnz = nnz_;
  return RTHX_OK;
}

int DeviceCsr::upload(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows, int64_t nnz_,
                      hipStream_t st) {
  RTHX_TRY(reserve(n_rows, nnz_));
  HIP_TRY(hipMemcpyAsync(rp.p, row_ptr, (size_t)(n_rows + 1) * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  if (nnz) {
    HIP_TRY(hipMemcpyAsync(ci.p, cols, (size_t)nnz * 4, hipMemcpyHostToDevice, st), "hipMemcpy");
    HIP_TRY(hipMemcpyAsync(v.p, vals, (size_t)nnz * 8, hipMemcpyHostToDevice, st), "hipMemcpy");
  }
  return RTHX_OK;
}

int reserve_transpose(const Source& S, Scratch& W, DeviceCsr& T) {
  W.P = plan_transpose(S.n_cols, S.nnz, S.counts ? 4 : 8);
  HIP_TRY(W.buf.reserve((size_t)W.P.scratch_bytes), "hipMalloc transpose scratch");
  return T.reserve(S.n_cols, S.nnz);
}

hipError_t enqueue_transpose(const Source& S, const Scratch& W, const DeviceCsr& T, hipStream_t st) {
  return transpose(S, T.dest(), W.P, W.buf.p, st);
}

hipError_t counts_source(const rthx_result* res, int64_t n_rows, int64_t n_keep, double* tallied, int64_t* src,
                         int64_t* len, int64_t* off, hipStream_t st, Source& S) {
  S.n_rows = n_rows;
  S.n_cols = n_keep;
  S.off = off;
  S.src = src;
  S.cols = res->cols.as<uint32_t>();
  S.counts = res->cnt.as<uint32_t>();
  S.tallied = tallied;
  return block_rows(res->row_off.as<int64_t>(), S.cols, S.counts, n_rows, n_keep, res->N, tallied, src, len, off, st);
}

int result_block(const rthx_result* res, int64_t n, hipStream_t st, Block& B) {
  if (res->info.nnz >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31 for the device transpose");
  DevBuf len;
  HIP_TRY(B.tallied.reserve((size_t)n * 8), "hipMalloc tallied");
  HIP_TRY(B.src.reserve((size_t)n * 8), "hipMalloc row starts");
  HIP_TRY(len.reserve((size_t)n * 8), "hipMalloc row lengths");
  HIP_TRY(B.off.reserve((size_t)(n + 1) * 8), "hipMalloc row offsets");
  HIP_TRY(counts_source(res, n, n, B.tallied.as<double>(), B.src.as<int64_t>(), len.as<int64_t>(),
                        B.off.as<int64_t>(), st, B.S),
          "block rows launch");
  B.S.whole = 0;
  HIP_TRY(hipMemcpyAsync(&B.S.nnz, B.off.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, st), "hipMemcpy block nnz");
  HIP_TRY(hipStreamSynchronize(st), "block rows");
  return RTHX_OK;
}

int transpose_result_block(const rthx_result* res, int64_t n, hipStream_t st, DeviceCsr& out) {
  Block B;
  Scratch W;
  RTHX_TRY(result_block(res, n, st, B));
  RTHX_TRY(reserve_transpose(B.S, W, out));
  HIP_TRY(enqueue_transpose(B.S, W, out, st), "transpose launch");
  HIP_TRY(hipStreamSynchronize(st), "transpose");  // (the scratch is freed on return)
  return RTHX_OK;
}

int smooth_transposed(const rthx_smooth_result* cF, hipStream_t st, const int64_t** rp, const int32_t** ci,
                      const double** v) {
  rthx_smooth_result* F = const_cast<rthx_smooth_result*>(cF);
  if (!F->have_t) {
    if (F->nnz >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31 for the device transpose");
    const Source S = whole_source(F->n, F->n, F->nnz, F->rp.as<int64_t>(), F->ci.as<uint32_t>(), F->F.as<double>());
    Scratch W;
    RTHX_TRY(reserve_transpose(S, W, F->t));
    HIP_TRY(enqueue_transpose(S, W, F->t, st), "transpose launch");
    HIP_TRY(hipStreamSynchronize(st), "transpose");
    F->have_t = true;
  }
  *rp = F->t.rp.as<int64_t>();
  *ci = F->t.ci.as<int32_t>();
  *v = F->t.v.as<double>();
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
  RTHX_TRY(rthx::check_host_csr(row_ptr, cols, vals, n_rows, n_cols, true, false));
  const int64_t nnz = row_ptr[n_rows];
  if (nnz > 0 && (!t_cols || !t_vals)) return fail(RTHX_EINVAL, "null CSR arrays");
  rthx::DeviceGuard keep_device;
  hipStream_t st = nullptr;
  RTHX_TRY(rthx::open_device(device, &st));
  // everything is allocated before the timed stretch
  tp::DeviceCsr A, T;
  tp::Scratch W;
  RTHX_TRY(A.upload(row_ptr, cols, vals, n_rows, nnz, st));
  const tp::Source S = A.source(n_rows, n_cols);
  RTHX_TRY(tp::reserve_transpose(S, W, T));
  rthx::EventPair ev;
  HIP_TRY(ev.create(), "hipEventCreate");
  hipError_t e = ev.start(st);
  if (e == hipSuccess) e = tp::enqueue_transpose(S, W, T, st);
  if (e == hipSuccess) e = ev.stop(st);
  if (e == hipSuccess) e = hipMemcpyAsync(t_row_ptr, T.rp.p, (size_t)(n_cols + 1) * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(t_cols, T.ci.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && nnz) e = hipMemcpyAsync(t_vals, T.v.p, (size_t)nnz * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  float ms = 0.f;
  if (e == hipSuccess) e = ev.elapsed(&ms);
  if (e != hipSuccess) return rthx::hip_fail(e, "CSR transpose");
  if (device_ms) *device_ms = ms;
  return RTHX_OK;
}
