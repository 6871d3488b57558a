// rthx_csr_host.h -- a CSR matrix in host memory (int64 row pointers, int32
// columns, double values): the one check of a caller's matrix, the one
// counting-sort transpose, and the symmetric part that the host route of the
// sparse smoothing builds from them.  Pure host code without
// HIP or the library's error state, so tests/csr_host_check.cpp includes it
// alone.
#pragma once

#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/rthx.h"

namespace rthx {
namespace csr {

struct NoVisit {
  void operator()(int64_t, int64_t) const {}
};

// RTHX_OK, or the code and message of the first defect.  All of row_ptr is
// validated (row_ptr[0] == 0, monotone; below_2g: every row end, so nnz too,
// below 2^31) before any entry is read, so that no row reaches past nnz =
// row_ptr[n_rows]; cols / vals are read only when nnz > 0 and both are there.
// Every entry has a column in [0, n_cols) and a finite value; ascending:
// columns strictly ascend within a row.  (*visitor)(row, k) sees every
// checked entry once, in storage order: the pass runs on a local copy of the
// visitor, so that its state stays in registers, and hands the copy back when
// the matrix is accepted.
template <class Visit = NoVisit>
int check(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows, int64_t n_cols,
          bool below_2g, bool ascending, std::string& msg, Visit* visitor = nullptr) {
  Visit visit = visitor ? *visitor : Visit();
  auto refuse = [&msg](int code, const std::string& why) {
    msg = why;
    return code;
  };
  if (!row_ptr) return refuse(RTHX_EINVAL, "null CSR arrays");
  if (row_ptr[0] != 0) return refuse(RTHX_EINVAL, "row_ptr[0] != 0");
  for (int64_t i = 0; i < n_rows; ++i) {
    if (row_ptr[i + 1] < row_ptr[i]) return refuse(RTHX_EINVAL, "row_ptr not monotone");
    if (below_2g && row_ptr[i + 1] >= (int64_t(1) << 31)) return refuse(RTHX_ERANGE, "nnz must be below 2^31");
  }
  if (row_ptr[n_rows] > 0 && (!cols || !vals)) return refuse(RTHX_EINVAL, "null CSR arrays");
  for (int64_t i = 0; i < n_rows; ++i)
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      if (cols[k] < 0 || cols[k] >= n_cols || !std::isfinite(vals[k])) return refuse(RTHX_EINVAL, "bad CSR entry");
      if (ascending && k > row_ptr[i] && !(cols[k - 1] < cols[k]))
        return refuse(RTHX_EINVAL, "row " + std::to_string(i) + " is not strictly column-ascending");
      visit(i, k);
    }
  if (visitor) *visitor = visit;
  return RTHX_OK;
}

// The transpose of a checked n_rows x n_cols matrix by a stable counting
// sort: t_ptr[n_cols + 1] (+ base), and per entry the row it came from
// (+ base) and its value, either of which may be left out (nullptr).  Rows
// are visited in ascending order, so they ascend within a column and equal
// (row, column) pairs keep their input order.
template <class Row>
void transpose(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows, int64_t n_cols,
               int64_t base, int64_t* t_ptr, Row* t_rows, double* t_vals) {
  const int64_t nnz = row_ptr[n_rows];
  for (int64_t c = 0; c <= n_cols; ++c) t_ptr[c] = 0;
  for (int64_t k = 0; k < nnz; ++k) t_ptr[cols[k] + 1]++;
  for (int64_t c = 0; c < n_cols; ++c) t_ptr[c + 1] += t_ptr[c];
  std::vector<int64_t> next(t_ptr, t_ptr + n_cols);
  for (int64_t i = 0; i < n_rows; ++i)
    for (int64_t k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
      const int64_t q = next[cols[k]]++;
      if (t_rows) t_rows[q] = (Row)(i + base);
      if (t_vals) t_vals[q] = vals[k];
    }
  if (base)
    for (int64_t c = 0; c <= n_cols; ++c) t_ptr[c] += base;
}

// A matrix owned on the host.
struct Host {
  std::vector<int64_t> rp;
  std::vector<int32_t> ci;
  std::vector<double> v;
  int64_t nnz() const { return rp.empty() ? 0 : rp.back(); }
};

inline void transposed(const int64_t* row_ptr, const int32_t* cols, const double* vals, int64_t n_rows,
                       int64_t n_cols, Host& T) {
  const int64_t nnz = row_ptr[n_rows];
  T.rp.resize(n_cols + 1);
  T.ci.resize(nnz);
  T.v.resize(nnz);
  transpose(row_ptr, cols, vals, n_rows, n_cols, 0, T.rp.data(), T.ci.data(), T.v.data());
}

// X = (Diagonal(w) A + (Diagonal(w) A)') / 2 of a square A with ascending rows
// (smoothExchangeFactors.jl:474-477): union pattern, columns ascending,
// x_ij = 0.5 * (w_i a_ij + w_j a_ji) with an absent term +0.0 -- the layout and
// the roundings of rthx_symmetrize_kernels.hip.
inline void symmetric_part(const int64_t* rp, const int32_t* ci, const double* v, const double* w, int64_t n, Host& X) {
  Host T;
  transposed(rp, ci, v, n, n, T);
  const int64_t nnz = T.nnz();
  X.rp.assign(n + 1, 0);
  X.ci.clear();
  X.v.clear();
  X.ci.reserve(2 * nnz);
  X.v.reserve(2 * nnz);
  for (int64_t i = 0; i < n; ++i) {
    int64_t a = rp[i], ae = rp[i + 1], b = T.rp[i], be = T.rp[i + 1];
    while (a < ae || b < be) {
      const int32_t ca = a < ae ? ci[a] : INT32_MAX, cb = b < be ? T.ci[b] : INT32_MAX;
      if (ca == cb) {  // (branches, not selects: a traced F is nearly symmetric and the matched case predicts well)
        X.ci.push_back(ca);
        X.v.push_back(0.5 * (w[i] * v[a++] + w[cb] * T.v[b++]));
      } else if (ca < cb) {
        X.ci.push_back(ca);
        X.v.push_back(0.5 * (w[i] * v[a++] + 0.0));
      } else {
        X.ci.push_back(cb);
        X.v.push_back(0.5 * (0.0 + w[cb] * T.v[b++]));
      }
    }
    X.rp[i + 1] = (int64_t)X.ci.size();
  }
}

}  // namespace csr
}  // namespace rthx
