// rthx_assemble.cpp -- C ABI of the row-shard merge (include/rthx.h
// rthx_merge_row_shards): a C5 band traced as W row shards, one per GPU, is
// put together on the band's owner GPU from the blocks its RCCL gather
// received (rthx.distributed.trace_bands_row_sharded).
#include <hip/hip_runtime.h>

#include "rthx_assemble.h"
#include "rthx_common.h"

RTHX_EXPORT int rthx_merge_row_shards(int32_t device, int32_t n_shards, int64_t n_rows,
                                      const int64_t* const* shard_row_off, const uint32_t* const* shard_cols,
                                      const uint32_t* const* shard_counts, int64_t* row_ptr, uint32_t* cols,
                                      uint32_t* counts, void* stream) {
  using rthx::fail;
  if (n_shards < 1 || n_shards > rthx::asmb::kMaxShards) return fail(RTHX_ERANGE, "n_shards must be in [1, 64]");
  if (n_rows < 0) return fail(RTHX_EINVAL, "negative n_rows");
  if (!shard_row_off || !shard_cols || !shard_counts || !row_ptr) return fail(RTHX_EINVAL, "null pointer");
  rthx::asmb::ShardSet S{};
  S.n_rows = n_rows;
  S.n_shards = n_shards;
  for (int k = 0; k < n_shards; ++k) {
    const bool has_rows = k < n_rows;
    if (!shard_row_off[k] || (has_rows && (!shard_cols[k] || !shard_counts[k])))
      return fail(RTHX_EINVAL, "null shard pointer");
    S.row_off[k] = shard_row_off[k];
    S.cols[k] = shard_cols[k];
    S.counts[k] = shard_counts[k];
  }
  if (n_rows > 0 && (!cols || !counts)) return fail(RTHX_EINVAL, "null output");
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!st) HIP_TRY(rthx::device_stream(device, &st), "device stream");
  HIP_TRY(rthx::asmb::merge_row_shards(S, row_ptr, cols, counts, st), "row-shard merge launch");
  if (!stream) HIP_TRY(hipStreamSynchronize(st), "row-shard merge");
  return RTHX_OK;
}

// F_raw in CSC (include/rthx.h rthx_result_copy_F_csc).  One-device results:
// the transpose kernels of rthx_transpose_kernels.hip on the counts where
// they lie (counts payload, int64 rows), then three D2H copies.  Several
// devices' parts: F_raw as CSR on the host (rthx_result_copy_F) and the host
// transpose of rthx_csr_host.h.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "rthx_domain.h"
#include "rthx_transpose.h"

namespace {

int csc_on_host(rthx_result* res, int64_t base, int64_t* colptr, int64_t* rowval, double* nzval) {
  const int64_t N = res->N, nnz = res->info.nnz;
  std::vector<int64_t> rp((size_t)N + 1);
  std::vector<int32_t> cols((size_t)std::max<int64_t>(nnz, 1));
  std::vector<double> vals((size_t)std::max<int64_t>(nnz, 1));
  if (int rc = rthx_result_copy_F(res, rp.data(), cols.data(), vals.data())) return rc;
  std::vector<int64_t> own_colptr(colptr ? 0 : (size_t)N + 1);
  rthx::csr::transpose(rp.data(), cols.data(), vals.data(), N, N, base, colptr ? colptr : own_colptr.data(), rowval,
                       nzval);
  return RTHX_OK;
}

}  // namespace

RTHX_EXPORT int rthx_result_copy_F_csc(const rthx_result* cres, int32_t index_base, int64_t* colptr, int64_t* rowval,
                                       double* nzval) {
  using rthx::fail;
  if (!cres) return fail(RTHX_EINVAL, "null result");
  if (index_base != 0 && index_base != 1) return fail(RTHX_EINVAL, "index_base must be 0 or 1");
  if (int rc = rthx::result_ready(cres)) return rc;
  rthx_result* res = const_cast<rthx_result*>(cres);
  if (!res->parts.empty()) return csc_on_host(res, index_base, colptr, rowval, nzval);
  const int64_t N = res->N, nnz = res->info.nnz, n_rows = res->n_rows;
  if (nnz >= (int64_t(1) << 31)) return fail(RTHX_ERANGE, "nnz must be below 2^31 for the device transpose");
  namespace tp = rthx::tp;
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(res->device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIP_TRY(rthx::device_stream(res->device, &st), "device stream");
  const tp::Plan P = tp::plan_transpose(N, nnz, 4);
  const size_t m = (size_t)std::max<int64_t>(nnz, 1), mr = (size_t)std::max<int64_t>(n_rows, 1);
  HIP_TRY(res->csc_scratch.reserve((size_t)P.scratch_bytes), "hipMalloc transpose scratch");
  HIP_TRY(res->csc_rowsum.reserve(mr * 8), "hipMalloc row sums");
  HIP_TRY(res->csc_src.reserve(mr * 8), "hipMalloc row starts");
  HIP_TRY(res->csc_len.reserve(mr * 8), "hipMalloc row lengths");
  HIP_TRY(res->csc_off.reserve((mr + 1) * 8), "hipMalloc row offsets");
  HIP_TRY(res->csc_colptr.reserve((size_t)(N + 1) * 8), "hipMalloc colptr");
  HIP_TRY(res->csc_rowval.reserve(m * 8), "hipMalloc rowval");
  HIP_TRY(res->csc_nz.reserve(m * 8), "hipMalloc nzval");
  // every traced row whole (n_keep = N): the rows' tallied rays, and offsets from 0
  tp::Source S;
  HIP_TRY(tp::counts_source(res, n_rows, N, res->csc_rowsum.as<double>(), res->csc_src.as<int64_t>(),
                            res->csc_len.as<int64_t>(), res->csc_off.as<int64_t>(), st, S),
          "CSC rows launch");
  S.nnz = nnz;
  tp::Dest D;
  D.t_off = res->csc_colptr.as<int64_t>();
  D.rows64 = res->csc_rowval.as<int64_t>();
  D.vals = res->csc_nz.as<double>();
  D.begin = res->begin;
  D.stride = res->stride;
  D.base = index_base;
  HIP_TRY(tp::transpose(S, D, P, res->csc_scratch.p, st), "CSC transpose launch");
  if (colptr) HIP_TRY(hipMemcpyAsync(colptr, res->csc_colptr.p, (size_t)(N + 1) * 8, hipMemcpyDeviceToHost, st), "hipMemcpy colptr");
  if (rowval && nnz) HIP_TRY(hipMemcpyAsync(rowval, res->csc_rowval.p, (size_t)nnz * 8, hipMemcpyDeviceToHost, st), "hipMemcpy rowval");
  if (nzval && nnz) HIP_TRY(hipMemcpyAsync(nzval, res->csc_nz.p, (size_t)nnz * 8, hipMemcpyDeviceToHost, st), "hipMemcpy nzval");
  HIP_TRY(hipStreamSynchronize(st), "F_raw CSC");
  return RTHX_OK;
}

// ---------------------------------------------------------------------------
// Sum of two count matrices (include/rthx.h rthx_result_accumulate,
// rthx_result_accumulate_csr) and the sampling error of a result
// (rthx_result_sampling_error).  Kernels: rthx_assemble_kernels.hip.
// ---------------------------------------------------------------------------
namespace {

// dst += the block (b_off, b_cols, b_cnt) of dst->n_rows rows, nnz_b entries
// and rays_b rays per row, on dst's device (dst is ready, single-device).
int accumulate_block(rthx_result* dst, const int64_t* b_off, const uint32_t* b_cols, const uint32_t* b_cnt,
                     int64_t nnz_b, int64_t rays_b) {
  using rthx::fail;
  const int64_t n_rows = dst->n_rows;
  hipStream_t st = nullptr;
  HIP_TRY(rthx::device_stream(dst->device, &st), "device stream");
  for (auto& e : dst->acc_ev)
    if (!e) HIP_TRY(hipEventCreate(&e), "hipEventCreate");
  rthx::asmb::AccJob J{};
  J.n_rows = n_rows;
  J.n_cols = dst->N;
  J.a_off = dst->row_off.as<int64_t>();
  J.a_cols = dst->cols.as<uint32_t>();
  J.a_cnt = dst->cnt.as<uint32_t>();
  J.b_off = b_off;
  J.b_cols = b_cols;
  J.b_cnt = b_cnt;
  J.rays = dst->R + rays_b;
  // long rows (a mean of 512 entries or more in either operand): a workgroup per row
  J.wide = n_rows > 0 && std::max<int64_t>(dst->info.nnz, nnz_b) / n_rows >= 512 ? 1 : 0;
  HIP_TRY(dst->acc_len.reserve((size_t)std::max<int64_t>(n_rows, 1) * 8), "hipMalloc merged row lengths");
  HIP_TRY(dst->acc_off.reserve((size_t)(n_rows + 1) * 8), "hipMalloc merged row offsets");
  HIP_TRY(dst->acc_mark.reserve((size_t)std::max<int64_t>(nnz_b, 1) * 4), "hipMalloc match ranks");
  HIP_TRY(dst->acc_totals.reserve(8 * rthx::asmb::kAccTotals), "hipMalloc totals");
  HIP_TRY(dst->row_tallied.reserve((size_t)std::max<int64_t>(n_rows, 1) * 4), "hipMalloc row_tallied");
  HIP_TRY(dst->h_totals.reserve(8 * 8), "hipHostMalloc totals");
  unsigned long long* totals = dst->acc_totals.as<unsigned long long>();
  HIP_TRY(hipMemsetAsync(totals, 0, 8 * rthx::asmb::kAccTotals, st), "hipMemset totals");
  HIP_TRY(hipEventRecord(dst->acc_ev[0], st), "hipEventRecord");
  HIP_TRY(rthx::asmb::acc_lengths(J, dst->acc_mark.as<uint32_t>(), dst->acc_len.as<int64_t>(),
                                  dst->acc_off.as<int64_t>(), totals, st),
          "accumulate length launch");
  HIP_TRY(hipMemcpyAsync(dst->h_totals.p, totals, 8 * rthx::asmb::kAccTotals, hipMemcpyDeviceToHost, st),
          "hipMemcpy totals");
  HIP_TRY(hipStreamSynchronize(st), "accumulate lengths");
  const int64_t* ht = static_cast<const int64_t*>(dst->h_totals.p);
  if (ht[3] != 0) return fail(RTHX_EINVAL, "the added CSR block has a negative row length or a column >= N");
  const int64_t nnz = ht[0];
  HIP_TRY(dst->acc_cols.reserve((size_t)std::max<int64_t>(nnz, 1) * 4), "hipMalloc merged cols");
  HIP_TRY(dst->acc_cnt.reserve((size_t)std::max<int64_t>(nnz, 1) * 4), "hipMalloc merged counts");
  HIP_TRY(hipMemsetAsync(dst->row_tallied.p, 0, (size_t)std::max<int64_t>(n_rows, 1) * 4, st), "hipMemset row_tallied");
  HIP_TRY(rthx::asmb::acc_write(J, dst->acc_mark.as<uint32_t>(), dst->acc_off.as<int64_t>(),
                                dst->acc_cols.as<uint32_t>(), dst->acc_cnt.as<uint32_t>(),
                                dst->row_tallied.as<uint32_t>(), totals, st),
          "accumulate write launch");
  HIP_TRY(hipEventRecord(dst->acc_ev[1], st), "hipEventRecord");
  HIP_TRY(hipMemcpyAsync(dst->h_totals.p, totals, 8 * rthx::asmb::kAccTotals, hipMemcpyDeviceToHost, st),
          "hipMemcpy totals");
  HIP_TRY(hipStreamSynchronize(st), "accumulate");
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, dst->acc_ev[0], dst->acc_ev[1]), "hipEventElapsedTime");
  dst->acc_ms = ms;
  // the sum takes the result's place; the old arrays serve the next accumulate
  dst->row_off.swap(dst->acc_off);
  dst->cols.swap(dst->acc_cols);
  dst->cnt.swap(dst->acc_cnt);
  dst->host_row_off = false;
  dst->R += rays_b;
  dst->info.rays_per_emitter = dst->R;
  dst->info.rays_traced = n_rows * dst->R;
  dst->info.nnz = nnz;
  dst->info.lost_total = ht[1];
  dst->info.lost_max_row = ht[2];
  return RTHX_OK;
}

int check_sum_rays(int64_t a, int64_t b) {
  if (a + b > 0xFFFFFFFFll) return rthx::fail(RTHX_ERANGE, "the summed rays per emitter must be below 2^32");
  return RTHX_OK;
}

}  // namespace

RTHX_EXPORT int rthx_result_accumulate(rthx_result* dst, const rthx_result* src) {
  using rthx::fail;
  if (!dst || !src) return fail(RTHX_EINVAL, "null argument");
  if (dst == src) return fail(RTHX_EINVAL, "a result cannot be accumulated into itself");
  if (int rc = rthx::result_ready(dst)) return rc;
  if (int rc = rthx::result_ready(src)) return rc;
  if (!dst->parts.empty() || !src->parts.empty())
    return fail(RTHX_EINVAL, "rthx_result_accumulate needs single-device results");
  if (dst->device != src->device) return fail(RTHX_EINVAL, "the results are on different devices");
  if (dst->N != src->N || dst->begin != src->begin || dst->stride != src->stride || dst->n_rows != src->n_rows)
    return fail(RTHX_EINVAL, "the results cover different rows");
  if (int rc = check_sum_rays(dst->R, src->R)) return rc;
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(dst->device), "hipSetDevice");
  return accumulate_block(dst, src->row_off.as<int64_t>(), src->cols.as<uint32_t>(), src->cnt.as<uint32_t>(),
                          src->info.nnz, src->R);
}

RTHX_EXPORT int rthx_result_accumulate_csr(rthx_result* dst, int64_t n_rows, const int64_t* row_off,
                                           const uint32_t* cols, const uint32_t* counts, int64_t rays_per_emitter) {
  using rthx::fail;
  if (!dst || !row_off) return fail(RTHX_EINVAL, "null argument");
  if (n_rows < 0 || rays_per_emitter < 0) return fail(RTHX_EINVAL, "negative n_rows or rays_per_emitter");
  if (int rc = rthx::result_ready(dst)) return rc;
  if (!dst->parts.empty()) return fail(RTHX_EINVAL, "rthx_result_accumulate_csr needs a single-device result");
  if (n_rows != dst->n_rows) return fail(RTHX_EINVAL, "the block's row count differs from the result's");
  if (int rc = check_sum_rays(dst->R, rays_per_emitter)) return rc;
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(dst->device), "hipSetDevice");
  // the block's first and last offsets: from 0, nnz entries
  int64_t ends[2] = {0, 0};
  HIP_TRY(hipMemcpy(&ends[0], row_off, 8, hipMemcpyDeviceToHost), "hipMemcpy row_off");
  HIP_TRY(hipMemcpy(&ends[1], row_off + n_rows, 8, hipMemcpyDeviceToHost), "hipMemcpy row_off");
  if (ends[0] != 0 || ends[1] < 0) return fail(RTHX_EINVAL, "the block's row offsets must run from 0 to its nnz");
  if (ends[1] > 0 && (!cols || !counts)) return fail(RTHX_EINVAL, "null cols or counts");
  return accumulate_block(dst, row_off, cols, counts, ends[1], rays_per_emitter);
}

RTHX_EXPORT int rthx_result_accumulate_ms(const rthx_result* res, double* ms_out) {
  if (!res || !ms_out) return rthx::fail(RTHX_EINVAL, "null argument");
  *ms_out = res->acc_ms;
  return RTHX_OK;
}

RTHX_EXPORT int rthx_result_sampling_error(const rthx_result* cres, double* rms_out, double* max_row_out) {
  using rthx::fail;
  if (!cres) return fail(RTHX_EINVAL, "null argument");
  if (int rc = rthx::result_ready(cres)) return rc;
  rthx_result* res = const_cast<rthx_result*>(cres);
  if (!res->parts.empty()) return fail(RTHX_EINVAL, "rthx_result_sampling_error needs a single-device result");
  rthx::DeviceGuard keep_device;
  HIP_TRY(hipSetDevice(res->device), "hipSetDevice");
  hipStream_t st = nullptr;
  HIP_TRY(rthx::device_stream(res->device, &st), "device stream");
  const int64_t n_rows = res->n_rows;
  HIP_TRY(res->acc_err.reserve((size_t)(n_rows + 2) * 8), "hipMalloc row variances");
  double* s = res->acc_err.as<double>();
  HIP_TRY(rthx::asmb::sampling_error(res->row_off.as<int64_t>(), res->cnt.as<uint32_t>(), n_rows, s, s + n_rows, st),
          "sampling error launch");
  double out[2] = {0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(out, s + n_rows, 16, hipMemcpyDeviceToHost, st), "hipMemcpy sampling error");
  HIP_TRY(hipStreamSynchronize(st), "sampling error");
  const double cells = (double)n_rows * (double)res->N;
  if (rms_out) *rms_out = cells > 0 ? std::sqrt(out[0] / cells) : 0.0;
  if (max_row_out) *max_row_out = std::sqrt(out[1]);
  return RTHX_OK;
}
