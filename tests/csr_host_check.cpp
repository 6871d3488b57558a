// Checks csrc/rthx_csr_host.h, the host side of every sparse entry point: the
// one CSR check (every refusal with its code; all of row_ptr before any
// entry), the one counting-sort transpose and the symmetric part, the latter
// two against dense brute force.  Arrays are heap blocks of exactly the size
// a well-formed caller passes, so an over-read aborts under AddressSanitizer.
// Built for the host with ASan + UBSan by tests/test_csr_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "rthx_csr_host.h"

namespace csr = rthx::csr;
using Rp = std::vector<int64_t>;
using Ci = std::vector<int32_t>;
using Vv = std::vector<double>;

static long g_cases = 0;
static uint64_t g_lcg = 20240531;

#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAILED %s (line %d)\n", #cond, __LINE__); \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

static uint32_t lcg() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_lcg >> 33);
}
static double uniform() { return (lcg() + 1.0) / 2147483649.0; }  // (0, 1)

// cols / vals on the heap with exactly `len` entries (nullptr for none)
struct Exact {
  int32_t* c = nullptr;
  double* v = nullptr;
  Exact(const Ci& ci, const Vv& vv, size_t len) {
    if (!len) return;
    c = (int32_t*)std::malloc(len * 4);
    v = (double*)std::malloc(len * 8);
    std::memcpy(c, ci.data(), len * 4);
    std::memcpy(v, vv.data(), len * 8);
  }
  ~Exact() {
    std::free(c);
    std::free(v);
  }
};

// ---- the check ------------------------------------------------------------
struct Record {  // a visitor that keeps what it is shown
  std::vector<std::pair<int64_t, int64_t>> seen;
  void operator()(int64_t i, int64_t k) { seen.emplace_back(i, k); }
};

static void refused(const Rp& rp, const Ci& ci, const Vv& vv, size_t len, int64_t n_rows, int64_t n_cols, bool lim,
                    bool asc, int code, const char* part) {
  Exact e(ci, vv, len);
  std::string msg;
  Record rec;
  const int rc = csr::check(rp.data(), e.c, e.v, n_rows, n_cols, lim, asc, msg, &rec);
  ++g_cases;
  CHECK(rc == code);
  CHECK(msg.find(part) != std::string::npos);
  CHECK(rec.seen.empty());  // (a refused matrix hands no visitor state back)
}

static void accepted(const Rp& rp, const Ci& ci, const Vv& vv, int64_t n_rows, int64_t n_cols, bool asc) {
  Exact e(ci, vv, (size_t)rp[n_rows]);
  std::string msg = "untouched";
  Record rec;
  const int rc = csr::check(rp.data(), e.c, e.v, n_rows, n_cols, true, asc, msg, &rec);
  const std::vector<std::pair<int64_t, int64_t>>& seen = rec.seen;
  ++g_cases;
  CHECK(rc == RTHX_OK && msg == "untouched");
  // the visitor sees every (row, k) once, in order
  CHECK((int64_t)seen.size() == rp[n_rows]);
  size_t q = 0;
  for (int64_t i = 0; i < n_rows; ++i)
    for (int64_t k = rp[i]; k < rp[i + 1]; ++k, ++q) CHECK(seen[q].first == i && seen[q].second == k);
}

static void check_cases() {
  const int E = RTHX_EINVAL, R = RTHX_ERANGE;
  const Ci c3 = {0, 2, 1};
  const Vv v3 = {1.0, 2.0, 3.0};
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // every refusal, with its code
  {
    std::string msg;
    ++g_cases;
    CHECK(csr::check(nullptr, c3.data(), v3.data(), 2, 3, true, true, msg) == E && msg == "null CSR arrays");
  }
  refused({1, 2, 3}, c3, v3, 3, 2, 3, true, false, E, "row_ptr[0]");
  refused({0, 3, 2}, c3, v3, 3, 2, 3, true, false, E, "monotone");
  refused({0, int64_t(1) << 31}, c3, v3, 3, 1, 3, true, false, R, "nnz must be below 2^31");
  refused({0, 1, int64_t(1) << 31}, c3, v3, 3, 2, 3, true, false, R, "2^31");
  refused({0, 2, 3}, c3, v3, 0, 2, 3, true, false, E, "null CSR arrays");  // both absent
  {
    std::string msg;
    const Rp rp = {0, 2, 3};
    g_cases += 2;
    CHECK(csr::check(rp.data(), nullptr, v3.data(), 2, 3, true, false, msg) == E && msg == "null CSR arrays");
    CHECK(csr::check(rp.data(), c3.data(), nullptr, 2, 3, true, false, msg) == E && msg == "null CSR arrays");
  }
  refused({0, 2, 3}, c3, v3, 3, 2, 2, true, false, E, "bad CSR entry");            // column == n_cols
  refused({0, 2, 3}, {0, -1, 1}, v3, 3, 2, 3, true, false, E, "bad CSR entry");    // negative column
  refused({0, 2, 3}, c3, {1.0, nan, 3.0}, 3, 2, 3, true, false, E, "bad CSR entry");
  refused({0, 2, 3}, c3, {1.0, 2.0, -inf}, 3, 2, 3, true, false, E, "bad CSR entry");
  // confined row-pointer jump: row 0 would run to entry 5 of two; refused with no entry read
  refused({0, 5, 2}, c3, v3, 2, 2, 3, false, false, E, "monotone");
  refused({0, 5, 2}, c3, v3, 2, 2, 3, true, true, E, "monotone");
  // (row_ptr = [0, 2, 3] over two-entry arrays cannot be told from a well-formed matrix: row_ptr[n] is all the
  // check knows of the arrays' size, so there is no honest case for it)
  // the ascending switch: an equal and a descending pair, the row named
  const Rp rp4 = {0, 1, 3, 3};
  refused(rp4, {0, 1, 1}, v3, 3, 3, 3, true, true, E, "row 1 is not strictly column-ascending");
  refused(rp4, {0, 2, 1}, v3, 3, 3, 3, true, true, E, "row 1 is not strictly column-ascending");
  refused({0, 2, 3, 3}, {2, 0, 1}, v3, 3, 3, 3, true, true, E, "row 0 is not strictly column-ascending");
  accepted(rp4, {0, 1, 1}, v3, 3, 3, false);
  accepted(rp4, {0, 2, 1}, v3, 3, 3, false);
  // n = 0, nnz = 0 (arrays absent), an empty first, middle and last row
  accepted({0}, {}, {}, 0, 3, true);
  accepted({0, 0, 0}, {}, {}, 2, 3, true);
  accepted({0, 0, 2, 3}, c3, v3, 3, 3, true);
  accepted({0, 2, 2, 3}, c3, v3, 3, 3, true);
  accepted({0, 2, 3, 3}, c3, v3, 3, 3, true);
  // without the 2^31 switch a large row end is no defect of row_ptr (no entry is read: the arrays are absent)
  refused({0, int64_t(1) << 31}, {}, {}, 0, 1, 3, false, false, E, "null CSR arrays");
}

// ---- the transpose --------------------------------------------------------
struct Mat {
  int64_t n_rows = 0, n_cols = 0;
  Rp rp;
  Ci ci;
  Vv v;
};

// density 0, about 0.3 or 1; unsorted: a row's entries in a shuffled order, with repeated (row, column) pairs
static Mat random_matrix(int64_t n_rows, int64_t n_cols, double density, bool unsorted) {
  Mat A;
  A.n_rows = n_rows;
  A.n_cols = n_cols;
  A.rp.assign(1, 0);
  for (int64_t i = 0; i < n_rows; ++i) {
    const size_t r0 = A.ci.size();
    for (int rep = 0; rep < (unsorted ? 2 : 1); ++rep)
      for (int64_t c = 0; c < n_cols; ++c)
        if (density >= 1.0 || uniform() < density) {
          A.ci.push_back((int32_t)c);
          A.v.push_back(uniform() - 0.5);
        }
    if (unsorted)
      for (size_t k = A.ci.size(); k > r0 + 1; --k) {
        const size_t j = r0 + lcg() % (k - r0);
        std::swap(A.ci[k - 1], A.ci[j]);
        std::swap(A.v[k - 1], A.v[j]);
      }
    A.rp.push_back((int64_t)A.ci.size());
  }
  return A;
}

// brute force: per column, the rows in order and within a row the entries in order
template <class Row>
static void transpose_case(const Mat& A, int64_t base, bool with_rows, bool with_vals) {
  const int64_t nnz = A.rp[A.n_rows];
  Rp want_ptr(1, base);
  std::vector<Row> want_rows;
  Vv want_vals;
  for (int64_t c = 0; c < A.n_cols; ++c) {
    for (int64_t i = 0; i < A.n_rows; ++i)
      for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k)
        if (A.ci[k] == c) {
          want_rows.push_back((Row)(i + base));
          want_vals.push_back(A.v[k]);
        }
    want_ptr.push_back((int64_t)want_rows.size() + base);
  }
  Exact in(A.ci, A.v, (size_t)nnz);
  Rp t_ptr(A.n_cols + 1, -7);
  std::vector<Row> t_rows(nnz, (Row)-7);
  Vv t_vals(nnz, -7.0);
  csr::transpose<Row>(A.rp.data(), in.c, in.v, A.n_rows, A.n_cols, base, t_ptr.data(),
                      with_rows ? t_rows.data() : nullptr, with_vals ? t_vals.data() : nullptr);
  ++g_cases;
  CHECK(t_ptr == want_ptr);
  if (with_rows) CHECK(t_rows == want_rows);
  if (with_vals) CHECK(nnz == 0 || std::memcmp(t_vals.data(), want_vals.data(), (size_t)nnz * 8) == 0);
}

static void transpose_cases() {
  for (int64_t n_rows : {0, 1, 2, 3, 5})
    for (int64_t n_cols : {1, 2, 3, 7})
      for (double density : {0.0, 0.3, 1.0})
        for (bool unsorted : {false, true}) {
          const Mat A = random_matrix(n_rows, n_cols, density, unsorted);
          transpose_case<int32_t>(A, 0, true, true);
          transpose_case<int64_t>(A, 0, true, true);
          transpose_case<int64_t>(A, 1, true, true);    // the index base of a Julia SparseMatrixCSC
          transpose_case<int64_t>(A, 1, false, true);   // null rowval
          transpose_case<int64_t>(A, 1, true, false);   // null nzval
          transpose_case<int64_t>(A, 0, false, false);  // the column pointers alone
        }
  // one column in every row
  Mat A;
  A.n_rows = 5;
  A.n_cols = 7;
  A.rp = {0, 1, 2, 3, 4, 5};
  A.ci = {3, 3, 3, 3, 3};
  A.v = {1.0, 2.0, 3.0, 4.0, 5.0};
  transpose_case<int32_t>(A, 0, true, true);
  transpose_case<int64_t>(A, 1, true, true);
  // Host-owned form
  csr::Host T;
  csr::transposed(A.rp.data(), A.ci.data(), A.v.data(), 5, 7, T);
  ++g_cases;
  CHECK(T.nnz() == 5 && T.rp == Rp({0, 0, 0, 0, 5, 5, 5, 5}) && T.ci == Ci({0, 1, 2, 3, 4}) && T.v == A.v);
}

// ---- the symmetric part ---------------------------------------------------
static void symmetric_case(const Mat& A) {
  const int64_t n = A.n_rows;
  Vv w(n);
  for (double& x : w) x = 0.25 + 4.0 * uniform();
  // dense: presence and value
  std::vector<char> has((size_t)(n * n), 0);
  Vv a((size_t)(n * n), 0.0);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      has[i * n + A.ci[k]] = 1;
      a[i * n + A.ci[k]] = A.v[k];
    }
  Rp want_rp(1, 0);
  Ci want_ci;
  std::vector<uint64_t> want_bits;
  for (int64_t i = 0; i < n; ++i) {
    for (int64_t j = 0; j < n; ++j) {
      if (!has[i * n + j] && !has[j * n + i]) continue;
      const double t1 = has[i * n + j] ? w[i] * a[i * n + j] : 0.0;
      const double t2 = has[j * n + i] ? w[j] * a[j * n + i] : 0.0;
      const double x = 0.5 * (t1 + t2);
      uint64_t bits;
      std::memcpy(&bits, &x, 8);
      want_ci.push_back((int32_t)j);
      want_bits.push_back(bits);
    }
    want_rp.push_back((int64_t)want_ci.size());
  }
  Exact in(A.ci, A.v, (size_t)A.rp[n]);
  csr::Host X;
  X.ci.assign(3, 9);  // (stale contents are replaced)
  csr::symmetric_part(A.rp.data(), in.c, in.v, w.data(), n, X);
  ++g_cases;
  CHECK(X.rp == want_rp && X.ci == want_ci && X.v.size() == want_bits.size());
  CHECK(want_bits.empty() || std::memcmp(X.v.data(), want_bits.data(), want_bits.size() * 8) == 0);
}

static void symmetric_cases() {
  for (int64_t n : {1, 2, 3, 5, 7})
    for (double density : {0.0, 0.3, 1.0})
      for (int rep = 0; rep < 3; ++rep) symmetric_case(random_matrix(n, n, density, false));
  // a symmetric pattern (every entry matched) and a strictly upper one (no matched pair)
  Mat S = random_matrix(7, 7, 0.3, false), P, U;
  P.n_rows = P.n_cols = U.n_rows = U.n_cols = 7;
  P.rp.assign(1, 0);
  U.rp.assign(1, 0);
  std::vector<char> has(49, 0);
  for (int64_t i = 0; i < 7; ++i)
    for (int64_t k = S.rp[i]; k < S.rp[i + 1]; ++k) has[i * 7 + S.ci[k]] = has[S.ci[k] * 7 + i] = 1;
  for (int64_t i = 0; i < 7; ++i) {
    for (int64_t j = 0; j < 7; ++j) {
      if (has[i * 7 + j]) {
        P.ci.push_back((int32_t)j);
        P.v.push_back(uniform() - 0.5);
      }
      if (has[i * 7 + j] && j > i) {
        U.ci.push_back((int32_t)j);
        U.v.push_back(uniform() - 0.5);
      }
    }
    P.rp.push_back((int64_t)P.ci.size());
    U.rp.push_back((int64_t)U.ci.size());
  }
  CHECK(P.ci.size() > 7 && U.ci.size() > 2);
  symmetric_case(P);
  symmetric_case(U);
}

int main() {
  check_cases();
  transpose_cases();
  symmetric_cases();
  std::printf("csr host ok: %ld cases\n", g_cases);
  return 0;
}
