// rthx_transpose.h -- the device CSR -> CSC transpose:
// launchers of rthx_transpose_kernels.hip, the one owner of a CSR matrix in
// device memory (DeviceCsr) with the builders of the kernels' Source / Dest
// from it, and the host helpers of rthx_transpose.cpp that put the library's
// sparse consumers on the transpose.
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

// A whole matrix with a values payload as a Source (src == off).
inline Source whole_source(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* off, const uint32_t* cols,
                           const double* vals) {
  Source S;
  S.n_rows = n_rows;
  S.n_cols = n_cols;
  S.nnz = nnz;
  S.off = S.src = off;
  S.cols = cols;
  S.vals = vals;
  return S;
}

// Enqueues the transpose on st; scratch: P.scratch_bytes of device memory.
hipError_t transpose(const Source& S, const Dest& D, const Plan& P, void* scratch, hipStream_t st);

// Leading block of a trace result's counts (rows < n_rows, columns < n_keep;
// rows column-ascending): tallied[r] = the whole row's counts' sum, src[r] =
// the row's start relative to row 0, off = scan of the kept lengths
// (off[n_rows] = the block's nnz).  len: n_rows words of scratch.
hipError_t block_rows(const int64_t* row_off, const uint32_t* cols, const uint32_t* counts, int64_t n_rows,
                      int64_t n_keep, int64_t n_cols, double* tallied, int64_t* src, int64_t* len, int64_t* off,
                      hipStream_t st);

// A CSR matrix in device memory (int64 row pointers, int32 columns, double
// values): an uploaded host matrix, or F' -- the operator of rthx_solve.h --
// as the transpose writes it.
struct DeviceCsr {
  DevBuf rp, ci, v;  // n_rows + 1 int64, nnz int32, nnz double
  int64_t nnz = 0;
  int reserve(int64_t n_rows, int64_t nnz);  // (an empty matrix still gets its three buffers)
  // reserve, then the three copies from the host enqueued on st
  int upload(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows, int64_t nnz,
             hipStream_t st);
  // the whole matrix (n_rows x n_cols, columns non-negative) as a Source, and as the Dest of int32 rows
  Source source(int64_t n_rows, int64_t n_cols) const {
    return whole_source(n_rows, n_cols, nnz, rp.as<int64_t>(), ci.as<uint32_t>(), v.as<double>());
  }
  Dest dest() const {
    Dest D;
    D.t_off = rp.as<int64_t>();
    D.rows32 = ci.as<int32_t>();
    D.vals = v.as<double>();
    return D;
  }
};

// The transpose of one Source: its plan and scratch.  reserve_transpose
// allocates them and T (n_cols rows, S.nnz entries; no launch);
// enqueue_transpose launches into T.  S.nnz is below 2^31.
struct Scratch {
  Plan P;
  DevBuf buf;
};
int reserve_transpose(const Source& S, Scratch& W, DeviceCsr& T);
hipError_t enqueue_transpose(const Source& S, const Scratch& W, const DeviceCsr& T, hipStream_t st);

// A trace result's counts as a Source (value = count / tallied[row]): rows <
// n_rows, of each the leading columns < n_keep.  Enqueues block_rows into
// tallied / src / off (n_rows, n_rows, n_rows + 1 words; len: n_rows words of
// scratch) and points S at them; S.nnz and S.whole are the caller's.
hipError_t counts_source(const rthx_result* res, int64_t n_rows, int64_t n_keep, double* tallied, int64_t* src,
                         int64_t* len, int64_t* off, hipStream_t st, Source& S);

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
int transpose_result_block(const rthx_result* res, int64_t n, hipStream_t st, DeviceCsr& out);
// A sparse smoothing result's F', formed on first use and kept in the handle.
int smooth_transposed(const rthx_smooth_result* F, hipStream_t st, const int64_t** rp, const int32_t** ci,
                      const double** v);

}  // namespace tp
}  // namespace rthx
