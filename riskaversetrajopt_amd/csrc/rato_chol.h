// The workgroup Cholesky, fp64: device functions for ONE workgroup of CHOL_BLOCK = 256 lanes, every lane of which calls them
// together.  csrc/chol.hip wraps them in kernels of their own (rato_chol_factor_batch_f64 / rato_chol_solve_batch_f64);
// csrc/qp_ipm.hip calls them from inside its solve, which must not leave the workgroup.
//
// Row-major, lower triangle: L[i][j] = A[i * lda + j], j <= i.  Right-looking over panels of CHOL_NB = 32 columns:
//   1. the 32 x 32 diagonal block is factored by wave 0 in registers (lane r owns row r; the pivot column travels by
//      __shfl), which needs no barrier; a non-positive or non-finite pivot j ends the factorization with j + 1;
//   2. the rows below are solved against it, one lane per row, the block read from LDS (broadcast reads);
//   3. the trailing matrix is updated in 64 x 64 tiles; the two 64 x 32 slices of the panel a tile needs are staged in LDS
//      (the matrix itself stays in global memory: 1.28 MB at n = 400, L2 resident), each lane owns a 4 x 4 micro-tile whose
//      columns are consecutive across lanes (coalesced rows).
// Only entries with j <= i < n are ever read or written: the strict upper triangle and the padding may hold anything.
// The register budget is tight (the callers compile to 255 / 256 VGPRs without scratch): the sched_barriers below are what
// keeps it there.
#pragma once
#include "rato_common.h"

#include <math.h>

namespace rato {

constexpr int CHOL_BLOCK = 256;
constexpr int CHOL_NB = 32;              // panel width
constexpr int CHOL_TILE = 64;            // trailing-update tile
constexpr int CHOL_LD = CHOL_NB + 1;     // LDS row stride of a staged slice (odd: no two rows of a column share a bank pair)
// doubles of LDS chol_factor needs: Ld [CHOL_NB * CHOL_LD], then Li and Lj [CHOL_TILE * CHOL_LD] each
constexpr int CHOL_LDS_DOUBLES = CHOL_NB * CHOL_LD + 2 * CHOL_TILE * CHOL_LD;

// In-place Cholesky of the lower triangle of A (n x n, leading dimension lda).  Ld, Li, Lj: the LDS staging areas (the factored
// diagonal block; the panel slices of a trailing tile: its rows and its columns); word: one LDS int32.  -> 0, or j + 1 for the
// first pivot j that is not positive and finite (what lies right of and below that panel is then left half done), the same
// value in every lane.  Ends behind a barrier: the caller may reset the word or reuse the tiles at once.
__device__ __forceinline__ int chol_factor(double* A, int n, int64_t lda, double* Ld, double* Li, double* Lj, int32_t* word) {
  const int tid = threadIdx.x;
  if (tid == 0) *word = 0;
  __syncthreads();
  int info = 0;
  for (int j0 = 0; j0 < n; j0 += CHOL_NB) {
    const int nb = min(CHOL_NB, n - j0);
    // 1. the diagonal block, wave 0, registers; rows and columns past n act as the identity
    if (tid < RATO_WAVE) {
      const int r = tid;
      double row[CHOL_NB];
#pragma unroll
      for (int c = 0; c < CHOL_NB; ++c)
        row[c] = (r < nb && c <= r && c < nb) ? A[(int64_t)(j0 + r) * lda + j0 + c] : ((r == c) ? 1.0 : 0.0);
      int fail = 0;
#pragma unroll
      for (int j = 0; j < CHOL_NB; ++j) {
        const double piv = __shfl(row[j], j, RATO_WAVE);
        if (!fail && !(piv > 0.0 && piv <= 1.79769313486231570815e308)) fail = j0 + j + 1;   // wave-uniform
        const double dj = sqrt(piv);
        if (r == j) row[j] = dj;
        else if (r > j) row[j] = row[j] / dj;
#pragma unroll
        for (int c = j + 1; c < CHOL_NB; ++c) {
          const double lcj = __shfl(row[j], c, RATO_WAVE);
          if (r >= c) row[c] -= row[j] * lcj;
        }
        __builtin_amdgcn_sched_barrier(0);   // keeps the next column's shuffles from being hoisted (no scratch)
      }
      if (fail) {
        if (tid == 0) *word = fail;
      } else if (r < CHOL_NB) {
#pragma unroll
        for (int c = 0; c < CHOL_NB; ++c) {
          Ld[r * CHOL_LD + c] = row[c];
          if (r < nb && c <= r) A[(int64_t)(j0 + r) * lda + j0 + c] = row[c];
        }
      }
    }
    __syncthreads();
    info = *word;                                  // every lane reads the same word after the barrier
    if (info) break;
    const int i0 = j0 + CHOL_NB;                   // first row below the block
    if (i0 >= n) break;
    // 2. rows below: x L11' = a, one lane per row
    for (int i = i0 + tid; i < n; i += CHOL_BLOCK) {
      double* a = A + (int64_t)i * lda + j0;
      double x[CHOL_NB];
#pragma unroll
      for (int c = 0; c < CHOL_NB; ++c) x[c] = a[c];
#pragma unroll
      for (int c = 0; c < CHOL_NB; ++c) {
        double s = x[c];
#pragma unroll
        for (int p = 0; p < c; ++p) s -= x[p] * Ld[c * CHOL_LD + p];
        x[c] = s / Ld[c * CHOL_LD + c];
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int c = 0; c < CHOL_NB; ++c) a[c] = x[c];
    }
    __syncthreads();
    // 3. trailing update, 64 x 64 tiles of the lower triangle
    const int tx = tid & 15, ty = tid >> 4;
    for (int ti = i0; ti < n; ti += CHOL_TILE) {
      for (int tj = i0; tj <= ti; tj += CHOL_TILE) {
        for (int e = tid; e < CHOL_TILE * CHOL_NB; e += CHOL_BLOCK) {
          const int r = e / CHOL_NB, c = e - r * CHOL_NB;
          Li[r * CHOL_LD + c] = (ti + r < n) ? A[(int64_t)(ti + r) * lda + j0 + c] : 0.0;
          Lj[r * CHOL_LD + c] = (tj + r < n) ? A[(int64_t)(tj + r) * lda + j0 + c] : 0.0;
        }
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
#pragma unroll 4
        for (int p = 0; p < CHOL_NB; ++p) {
          double li[4], lj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            li[u] = Li[(ty + 16 * u) * CHOL_LD + p];
            lj[u] = Lj[(tx + 16 * u) * CHOL_LD + p];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] += li[u] * lj[v];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = ti + ty + 16 * u, j = tj + tx + 16 * v;
            if (i < n && j <= i) A[(int64_t)i * lda + j] -= acc[u][v];
          }
        __syncthreads();
      }
    }
  }
  __syncthreads();                                 // nobody resets the word before everyone has read it
  return info;
}

// L L' x = b in place on xs (LDS, n doubles), L as chol_factor leaves it.  Begins with a barrier (the caller's writes to xs
// are visible) and ends behind one.
__device__ __forceinline__ void chol_solve(const double* L, int n, int64_t lda, double* xs) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += CHOL_NB) {        // L y = b
    const int nb = min(CHOL_NB, n - j0);
    if (tid < RATO_WAVE) {                         // the diagonal block, wave 0: lane r owns row j0 + r
      const int r = tid;
      double x = (r < nb) ? xs[j0 + r] : 0.0;
      for (int c = 0; c < nb; ++c) {
        if (r == c) x = x / L[(int64_t)(j0 + c) * lda + j0 + c];
        const double xc = __shfl(x, c, RATO_WAVE);
        if (r > c && r < nb) x -= L[(int64_t)(j0 + r) * lda + j0 + c] * xc;
      }
      if (r < nb) xs[j0 + r] = x;
    }
    __syncthreads();
    for (int i = j0 + CHOL_NB + tid; i < n; i += CHOL_BLOCK) {   // rows below: contiguous reads of their own row
      const double* l = L + (int64_t)i * lda + j0;
      double s = xs[i];
      for (int p = 0; p < CHOL_NB; ++p) s -= l[p] * xs[j0 + p];
      xs[i] = s;
    }
    __syncthreads();
  }
  for (int j0 = ((n - 1) / CHOL_NB) * CHOL_NB; j0 >= 0; j0 -= CHOL_NB) {   // L' x = y, blocks from the end
    const int nb = min(CHOL_NB, n - j0);
    if (tid < RATO_WAVE) {
      const int r = tid;
      double x = (r < nb) ? xs[j0 + r] : 0.0;
      for (int c = nb - 1; c >= 0; --c) {
        if (r == c) x = x / L[(int64_t)(j0 + c) * lda + j0 + c];
        const double xc = __shfl(x, c, RATO_WAVE);
        if (r < c) x -= L[(int64_t)(j0 + c) * lda + j0 + r] * xc;
      }
      if (r < nb) xs[j0 + r] = x;
    }
    __syncthreads();
    for (int i = tid; i < j0; i += CHOL_BLOCK) {   // rows above: column i of the block's rows, consecutive across lanes
      double s = xs[i];
      for (int p = 0; p < nb; ++p) s -= L[(int64_t)(j0 + p) * lda + i] * xs[j0 + p];
      xs[i] = s;
    }
    __syncthreads();
  }
}

}  // namespace rato
