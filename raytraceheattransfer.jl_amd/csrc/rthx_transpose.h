// rthx_transpose.h -- the device CSR -> CSC transpose:
// launchers of rthx_transpose_kernels.hip and the host helpers of
// rthx_transpose.cpp that put the library's sparse consumers on it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_common.h"
#include "rthx_transpose_plan.h"

struct rthx_result;
struct rthx_smooth_result;

namespace rthx {
namespace tp {

// A CSR block in device memory.  Kept entry e of the block (0 <= e < nnz,
// row-major) belongs to the row r with off[r] <= e < off[r + 1] and lies at
// index src[r] + (e - off[r]) of cols / vals / counts.  A whole matrix has
// src == off; a leading block of a trace result keeps a prefix of every row
// (off = scan of the kept lengths, src = the rows' own starts).
struct Source {
  int64_t n_rows = 0, n_cols = 0, nnz = 0;
  const int64_t* off = nullptr;   // n_rows + 1, off[0] = 0, off[n_rows] = nnz
  const int64_t* src = nullptr;   // n_rows
  int32_t whole = 1;              // src[r] == off[r] for every row
  const uint32_t* cols = nullptr;  // < n_cols (int32 columns are read as they are: non-negative)
  const double* vals = nullptr;    // payload: values, or ...
  const uint32_t* counts = nullptr;  // ... counts, written as count / tallied[row]
  const double* tallied = nullptr;   // n_rows
};

// The transpose as CSR: t_off[n_cols + 1] (+ base), and per entry the row it
// came from -- rows32[nnz] (the row r) or rows64[nnz] (begin + r * stride +
// base) -- and its value.  Rows ascend within a column; equal (row, column)
// pairs keep their input order.
struct Dest {
  int64_t* t_off = nullptr;
  int32_t* rows32 = nullptr;
  int64_t* rows64 = nullptr;
  double* vals = nullptr;
  int64_t begin = 0, stride = 1, base = 0;
};

// Enqueues the transpose on st; scratch: P.scratch_bytes of device memory.
hipError_t transpose(const Source& S, const Dest& D, const Plan& P, void* scratch, hipStream_t st);

// Leading block of a trace result's counts (rows < n_rows, columns < n_keep;
// rows column-ascending): tallied[r] = the whole row's counts' sum, src[r] =
// the row's start relative to row 0, off = scan of the kept lengths
// (off[n_rows] = the block's nnz).  len: n_rows words of scratch.
hipError_t block_rows(const int64_t* row_off, const uint32_t* cols, const uint32_t* counts, int64_t n_rows,
                      int64_t n_keep, int64_t n_cols, double* tallied, int64_t* src, int64_t* len, int64_t* off,
                      hipStream_t st);

// F' (CSR: the operator of rthx_solve.h) of a CSR matrix on the device.
struct Transposed {
  DevBuf rp, ci, v;  // n + 1 int64, nnz int32, nnz double
  int64_t nnz = 0;
};

// The n x n leading block of a trace result's F_raw (count / tallied) as a
// Source over the counts where they lie, with the row arrays it points to.
// The result is ready, single-device and holds every row < n (checked by the
// caller).
struct Block {
  DevBuf tallied, src, off;
  Source S;
};
int result_block(const rthx_result* res, int64_t n, hipStream_t st, Block& B);

// That block transposed on the result's device.  The result is ready, single-device and
// holds every row < n (checked by the caller).
int transpose_result_block(const rthx_result* res, int64_t n, hipStream_t st, Transposed& out);
// A sparse smoothing result's F', formed on first use and kept in the handle.
int smooth_transposed(const rthx_smooth_result* F, hipStream_t st, const int64_t** rp, const int32_t** ci,
                      const double** v);

}  // namespace tp
}  // namespace rthx
