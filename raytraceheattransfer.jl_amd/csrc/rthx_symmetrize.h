// rthx_symmetrize.h -- the symmetric part of a square CSR matrix on the
// device: X = (Diagonal(w) A + (Diagonal(w) A)') / 2 from A
// and its transpose (rthx_transpose.h), in one fixed layout.  Launchers of
// rthx_symmetrize_kernels.hip and the host helpers of rthx_symmetrize.cpp
// that the C ABI (rthx_csr_symmetrize) and the sparse smoothing set-up
// (rthx_smooth.cpp) share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rthx_common.h"
#include "rthx_transpose.h"

namespace rthx {
namespace sym {

constexpr int kGroup = 64;      // lanes that share a row: one wave
constexpr int kThreads = 256;   // per workgroup: kThreads / kGroup rows at a time

// A (n x n; every row strictly column-ascending) as a tp::Source and A' as
// the CSR that tp::transpose writes from it with int32 rows and the unscaled
// payload (values, or count / tallied of the source row).
struct Pair {
  tp::Source A;
  const int64_t* t_off = nullptr;   // n + 1
  const int32_t* t_cols = nullptr;  // nnz: the source rows, ascending within a row of A'
  const double* t_vals = nullptr;   // nnz
};

// mark[e], e an entry of A': the entries of its row before it whose column is
// also stored in the same row of A.  len[i] = lenA + lenT - matches, x_off =
// exclusive scan of len (n + 1 words; x_off[n] = nnz of X).
hipError_t lengths(const Pair& J, uint32_t* mark, int64_t* len, int64_t* x_off, hipStream_t st);

// Every entry of A and every unmatched entry of A' placed by its ranks and
// written once: x_ij = 0.5 * (w_i v_ij + w_j v_ji), an absent term +0.0
// (w == nullptr: ones).  No atomics; the same bytes on every run.
hipError_t write(const Pair& J, const double* w, const uint32_t* mark, const int64_t* x_off, int32_t* x_cols,
                 double* x_vals, hipStream_t st);

// Device memory of one build: A', the transpose's scratch, mark and len
// (freed when it goes out of scope).
struct Work {
  tp::Scratch ts;
  tp::DeviceCsr T;
  DevBuf mark, len;
};

// Allocates what a build over A needs (no launch).
int reserve(const tp::Source& A, Work& W);
// Enqueues the transpose of A and the mark and scan passes; x_off: n + 1 words.
hipError_t enqueue_lengths(const tp::Source& A, Work& W, int64_t* x_off, hipStream_t st);
// Enqueues the write pass (x_cols / x_vals hold x_off[n] entries).
hipError_t enqueue_write(const tp::Source& A, const Work& W, const double* w, const int64_t* x_off, int32_t* x_cols,
                         double* x_vals, hipStream_t st);

}  // namespace sym
}  // namespace rthx
