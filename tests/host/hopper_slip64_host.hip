// Host-only program: every lane of both grids of csrc/hopper_slip64.hip, executed in loops with the kernels' own per-lane
// functions (csrc/rato_hopper_slip64.h) and the kernels' order of sums.  No HIP runtime call.  Built with the address and
// undefined-behaviour sanitizers by tests/test_hopper_slip64_host.py; every array is allocated at exactly its size, so a lane
// that reads or writes outside its problem is reported.
//
//   hopper_slip64_host IN OUT
// IN : int64 S, time_jump, time_land, M, K, ldz, ldlam, lam_r0, has_lam, want_zmax; double mu_nom; Z [K][ldz]; a, theta, tau
//      [30][M]; with has_lam: lam [K][ldlam], add [K][S+1][78]
// OUT: h [K][C][M], dh_dfz [K][C][M], dh_dx [K][C][3][M]; with want_zmax: Zmax [K][M]; with has_lam: D [K][C][3], add
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rato_hopper_slip64.h"

static bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }
static bool write_all(FILE* f, const std::vector<double>& v) { return v.empty() || fwrite(v.data(), 8, v.size(), f) == v.size(); }

// the order of sum_partials_kernel<double> (csrc/stats.hip): 64 row lanes stride over the tiles with four accumulators,
// then a tree over the row lanes
static double second_stage(const double* part, int64_t nblocks, int64_t ncols, int64_t col) {
  const int ROWS = 64;
  double red[ROWS];
  for (int ry = 0; ry < ROWS; ++ry) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t b = ry;
    for (; b + 3 * ROWS < nblocks; b += 4 * ROWS) {
      a0 += part[b * ncols + col];
      a1 += part[(b + ROWS) * ncols + col];
      a2 += part[(b + 2 * ROWS) * ncols + col];
      a3 += part[(b + 3 * ROWS) * ncols + col];
    }
    for (; b < nblocks; b += ROWS) a0 += part[b * ncols + col];
    red[ry] = (a0 + a1) + (a2 + a3);
  }
  for (int half = ROWS / 2; half > 0; half >>= 1)
    for (int ry = 0; ry < half; ++ry) red[ry] += red[ry + half];
  return red[0];
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t hd[10];
  double mu_nom;
  if (!read_all(in, hd, sizeof hd) || !read_all(in, &mu_nom, 8)) return 4;
  const int S = (int)hd[0], tj = (int)hd[1], tl = (int)hd[2];
  const int64_t M = hd[3], K = hd[4], ldz = hd[5], ldlam = hd[6], r0 = hd[7];
  const bool has_lam = hd[8] != 0, want_zmax = hd[9] != 0;
  if (S < 1 || M < 1 || K < 1 || tj < 0 || tj > tl || tl > S || ldz < 8 * (S + 1) + 4 * S) return 5;
  const rato_slip64_phases P = {S, tj, tl, tj + (S - tl)};
  const int C = P.C;
  if (has_lam && (r0 < 0 || ldlam < r0 + M * C)) return 5;
  std::vector<double> Z(K * ldz), a(30 * M), th(30 * M), tau(30 * M), lam(has_lam ? K * ldlam : 0),
      add(has_lam ? K * (S + 1) * 78 : 0);
  if (!read_all(in, Z.data(), 8 * Z.size()) || !read_all(in, a.data(), 8 * a.size()) || !read_all(in, th.data(), 8 * th.size()) ||
      !read_all(in, tau.data(), 8 * tau.size()) || !read_all(in, lam.data(), 8 * lam.size()) ||
      !read_all(in, add.data(), 8 * add.size()))
    return 4;
  fclose(in);

  const int log2ti = rato_slip64_log2_ti(M);
  const int64_t nblk = rato_slip64_nblocks(M);
  const int ti = 1 << log2ti, mask = ti - 1, tc = RATO_S64_BLOCK >> log2ti;
  const int ncg = (C + tc - 1) / tc;
  const int gy = want_zmax ? 1 : ncg;
  std::vector<double> h(K * C * M), dfz(K * C * M), dx(K * C * 3 * M), Zmax(want_zmax ? K * M : 0),
      part(has_lam ? nblk * K * C * 3 : 0), D(has_lam ? K * C * 3 : 0);
  const rato_slip64_args A = {P,  mu_nom,   M,        log2ti,     Z.data(), ldz, a.data(), th.data(), tau.data(), has_lam ? lam.data() : nullptr,
                              ldlam, r0, h.data(), dfz.data(), dx.data()};
  // ---- the slip kernel's grid (sample tiles, contact groups, K), workgroup by workgroup --------------------------------------
  for (int64_t k = 0; C > 0 && k < K; ++k)
    for (int64_t bx = 0; bx < nblk; ++bx)
      for (int by = 0; by < gy; ++by) {
        double red[3][RATO_S64_BLOCK], zmax[RATO_S64_BLOCK];
        for (int tid = 0; tid < RATO_S64_BLOCK; ++tid) zmax[tid] = -INFINITY;
        for (int cg = by; cg < ncg; cg += gy) {
          for (int tid = 0; tid < RATO_S64_BLOCK; ++tid) {
            double t[3];
            rato_slip64_run_lane(A, k, bx * ti + (tid & mask), cg * tc + (tid >> log2ti), t, zmax[tid]);
            for (int j = 0; j < 3; ++j) red[j][tid] = t[j];
          }
          if (!has_lam) continue;
          for (int half = ti >> 1; half > 0; half >>= 1)
            for (int tid = 0; tid < RATO_S64_BLOCK; ++tid)
              for (int j = 0; j < 3; ++j) rato_slip64_tree_step(red[j], tid, mask, half);
          for (int tid = 0; tid < RATO_S64_BLOCK; ++tid) {
            const int c = cg * tc + (tid >> log2ti);
            if ((tid & mask) == 0 && c < C)
              for (int j = 0; j < 3; ++j) part[((bx * K + k) * C + c) * 3 + j] = red[j][tid];
          }
        }
        if (want_zmax) {
          for (int half = tc >> 1; half > 0; half >>= 1)
            for (int tid = 0; tid < RATO_S64_BLOCK; ++tid)
              if ((tid >> log2ti) < half) zmax[tid] = fmax(zmax[tid], zmax[tid + half * ti]);
          for (int tid = 0; tid < RATO_S64_BLOCK; ++tid) {
            const int64_t i = bx * ti + (tid & mask);
            if ((tid >> log2ti) == 0 && i < M) Zmax[k * M + i] = zmax[tid];
          }
        }
      }
  // ---- the second stage, then the Hessian-block grid -----------------------------------------------------------------------
  if (has_lam && C > 0) {
    for (int64_t col = 0; col < K * C * 3; ++col) D[col] = second_stage(part.data(), nblk, K * C * 3, col);
    for (int64_t idx = 0; idx < K * C * RATO_S64_ENTRIES; ++idx) rato_slip64_hess_lane(P, idx, Z.data(), ldz, D.data(), add.data());
  }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 3;
  if (!write_all(out, h) || !write_all(out, dfz) || !write_all(out, dx) || !write_all(out, Zmax) || !write_all(out, D) ||
      !write_all(out, add))
    return 6;
  fclose(out);
  printf("slip64 host ok\n");
  return 0;
}
