// Host-only program: the master QP (csrc/master.hip) and the NNLS (csrc/nnls.hip) through their C entry points, on a problem
// read from a file.  No HIP runtime call.  Built together with those two sources under the address and undefined-behaviour
// sanitizers by tests/test_master_qp.py; every array is allocated at exactly its size, so an entry point that reads or writes
// outside its arguments is reported.  The outputs are compared bit for bit with the library's.
//
//   master_host IN OUT
// IN (a sequence of master solves): int64 0, n, m_eq, rows, solves; p_diag [n], q [n], A_eq [m_eq][n], b_eq [m_eq], R [rows][n],
//      r [rows]; int64 chunks [solves]: the row count at which solve i runs (non-decreasing)
// OUT: create status; per solve: status, rato_master_rows, z [n], lam [rows] (zero beyond the rows added so far).  A refused
//      create writes its status alone.
// IN (one NNLS): int64 1, m, n, maxiter; A column-major [n][m], b [m]; int64 passive [n]
// OUT: status, y [n], passive [n]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "rato_saa.h"

static bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static bool write_all(FILE* f, const std::vector<double>& v) { return v.empty() || fwrite(v.data(), 8, v.size(), f) == v.size(); }
// exactly `count` doubles on the heap (count = 0: a null pointer, as a caller without equalities passes)
static bool read_doubles(FILE* f, std::vector<double>& v, int64_t count) {
  v.resize((size_t)count);
  v.shrink_to_fit();
  return read_all(f, v.data(), sizeof(double) * (size_t)count);
}

static int run_master(FILE* in, std::vector<double>& out) {
  int64_t hd[4];
  if (!read_all(in, hd, sizeof hd)) return 4;
  const int64_t n = hd[0], m = hd[1], rows = hd[2], solves = hd[3];
  if (n < 0 || m < 0 || rows < 0 || solves < 0) return 5;
  std::vector<double> p, q, A, b, R, r;
  if (!read_doubles(in, p, n) || !read_doubles(in, q, n) || !read_doubles(in, A, m * n) || !read_doubles(in, b, m) ||
      !read_doubles(in, R, rows * n) || !read_doubles(in, r, rows))
    return 6;
  std::vector<int64_t> chunks((size_t)solves);
  if (!read_all(in, chunks.data(), sizeof(int64_t) * (size_t)solves)) return 7;
  rato_master* M = nullptr;
  const int rc = rato_master_create(&M, (int32_t)n, p.data(), q.data(), (int32_t)m, m ? A.data() : nullptr, m ? b.data() : nullptr);
  out.push_back(rc);
  if (rc != RATO_OK) return M ? 8 : 0;
  int64_t done = 0;
  for (int64_t s = 0; s < solves; ++s) {
    const int64_t upto = chunks[(size_t)s];
    if (upto < done || upto > rows) return 9;
    // (k = 0 goes through the entry point too, with the pointers of an empty chunk)
    const int ra = rato_master_add_rows(M, (int32_t)(upto - done), R.data() + done * n, r.data() + done);
    if (ra != RATO_OK) return 10;
    done = upto;
    std::vector<double> z((size_t)n, 0.0), lam((size_t)done, 0.0);   // lam at exactly the rows so far
    const int st = rato_master_solve(M, z.data(), done ? lam.data() : nullptr);
    out.push_back(st);
    out.push_back(rato_master_rows(M));
    out.insert(out.end(), z.begin(), z.end());
    lam.resize((size_t)rows, 0.0);
    out.insert(out.end(), lam.begin(), lam.end());
  }
  rato_master_destroy(M);
  return 0;
}

static int run_nnls(FILE* in, std::vector<double>& out) {
  int64_t hd[3];
  if (!read_all(in, hd, sizeof hd)) return 4;
  const int64_t m = hd[0], n = hd[1], maxiter = hd[2];
  if (m < 1 || n < 1) return 5;
  std::vector<double> A, b;
  if (!read_doubles(in, A, m * n) || !read_doubles(in, b, m)) return 6;
  std::vector<int64_t> p64((size_t)n);
  if (!read_all(in, p64.data(), sizeof(int64_t) * (size_t)n)) return 7;
  std::vector<uint8_t> passive((size_t)n);
  for (int64_t j = 0; j < n; ++j) passive[(size_t)j] = p64[(size_t)j] != 0;
  std::vector<double> y((size_t)n, 0.0);
  out.push_back(rato_nnls_warm(A.data(), (int32_t)m, (int32_t)n, b.data(), passive.data(), y.data(), (int32_t)maxiter));
  out.insert(out.end(), y.begin(), y.end());
  for (int64_t j = 0; j < n; ++j) out.push_back(passive[(size_t)j]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t kind;
  std::vector<double> out;
  int rc = read_all(in, &kind, sizeof kind) ? (kind == 0 ? run_master(in, out) : kind == 1 ? run_nnls(in, out) : 5) : 4;
  fclose(in);
  if (rc != 0) return rc;
  FILE* f = fopen(argv[2], "wb");
  if (!f) return 11;
  const bool ok = write_all(f, out);
  if (fclose(f) != 0 || !ok) return 12;
  printf("master host ok\n");
  return 0;
}
