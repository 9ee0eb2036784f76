// Grid-parallel batched Cholesky, fp64: the arithmetic of csrc/rato_chol.h (same operations per entry, in the same order, so
// the results are bitwise those of csrc/chol.hip) spread over the device as a stream-ordered sequence of launches.
//
//   rato_chol_factor_grid_batch_f64  right-looking over panels of CHOL_NB = 32 columns, ONE launch per panel.  Launch q (panel
//   q, columns j0 = 32 q ..) holds two kinds of workgroups of 256 lanes, which touch disjoint entries:
//     panel workgroups  one per (block of 64 rows below the panel) x (problem).  Each applies panel q - 1's update to the old
//                   values of its own rows of panel q and of panel q's diagonal block (the only update they still miss: the
//                   earlier panels' came from the trailing tiles of earlier launches), factors the diagonal block for itself
//                   in wave 0's registers, and solves its rows against it in place.  Nobody writes the diagonal block in A in
//                   this launch, every panel workgroup of the problem is reading it: row block 0 keeps the factored block in
//                   work[k][q & 1], and copies the PREVIOUS panel's from work[k][(q - 1) & 1] into A, which no workgroup of this
//                   launch reads.  When no rows lie below, row block 0 is the problem's only workgroup and writes the block
//                   into A.  Row block 0 also writes info[k]: 0 in the first launch, j + 1 on a bad pivot j.
//     trailing tiles  one per (64 x 64 tile of the lower triangle right of panel q) x (problem): A_ij -= sum_p L_ip L_jp over
//                   panel q - 1's columns, which this launch only reads.
//   Per entry the panels' contributions arrive in ascending order: panels .. q - 2 from earlier launches' tiles, q - 1 from this
//   launch (its tiles, or the panel workgroup that owns the entry).
//   A launch returns at once for a problem whose info[k] is set.  info[k] is read at the top of a launch and written in it only
//   by row block 0 on a bad pivot, which every panel workgroup of that problem finds for itself from the same old values and
//   then writes nothing; a trailing tile that misses the word updates entries of a failed problem, whose content is unspecified.
//
//   rato_chol_solve_grid_batch_f64   one workgroup per (problem, right-hand side) and the row operations of chol_solve in their
//     order.  A diagonal block's triangle is in wave 0's registers before its 32-step chain starts: it is requested one panel
//     ahead, together with the first 256 rows' slices of the current panel, and both are in flight while the current chain runs
//     (the barrier behind the chain waits for them), so no load sits inside a dependent chain.
//
// No atomics, no waiting between workgroups: two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.
#include "rato_chol.h"

namespace {

using namespace rato;

constexpr int GRID_ROWS = 64;                        // rows of a panel launch's workgroup (one lane per row)
constexpr int GRID_DIAG = CHOL_NB * CHOL_NB;         // a factored diagonal block, row-major: work holds two per problem

// lane `lane`'s v in every lane (v_readlane: no LDS round trip, which is what __shfl costs inside a dependent chain)
__device__ __forceinline__ double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// The 32 x 32 diagonal block, factored in the registers of one wave as chol_factor does it: lane r owns row r (from V, LDS,
// row stride CHOL_LD), rows and columns past nb act as the identity.  -> 0, or j + 1 for the first bad pivot j (wave-uniform);
// row[] is the lane's row of L in its columns c <= r.  The columns c > r of a lane are not part of the block: they take part in
// the same instructions unpredicated (three instructions per (column, later column) pair instead of seven) and hold whatever
// that leaves, which no entry c <= r of any lane ever reads.
__device__ __forceinline__ int diag_factor(const double* V, int j0, int nb, int r, double (&row)[CHOL_NB]) {
#pragma unroll
  for (int c = 0; c < CHOL_NB; ++c) row[c] = (r < nb && c <= r && c < nb) ? V[r * CHOL_LD + c] : ((r == c) ? 1.0 : 0.0);
  int fail = 0;
#pragma unroll
  for (int j = 0; j < CHOL_NB; ++j) {
    const double piv = lane_value(row[j], j);
    if (!fail && !(piv > 0.0 && piv <= 1.79769313486231570815e308)) fail = j0 + j + 1;
    const double dj = sqrt(piv);
    row[j] = (r == j) ? dj : row[j] / dj;
#pragma unroll
    for (int c = j + 1; c < CHOL_NB; ++c) row[c] = fma(-row[j], lane_value(row[j], c), row[c]);
  }
  return fail;
}

constexpr int GRID_VROWS = CHOL_NB + GRID_ROWS;      // a panel workgroup's rows: the diagonal block's 32, then its own 64
constexpr int GRID_LDS_DOUBLES = 2 * GRID_VROWS * CHOL_LD;
static_assert(GRID_LDS_DOUBLES >= 2 * CHOL_TILE * CHOL_LD, "the trailing tiles' two slices fit the panel workgroups' LDS");

// launch q = j0 / 32: grid (nrb panel workgroups, then the trailing tiles of panel q - 1) x (problem)
__global__ __launch_bounds__(CHOL_BLOCK, 3) void chol_grid_step_kernel(double* __restrict__ A_all, int32_t n, int64_t lda,
                                                                    int32_t* __restrict__ info, double* __restrict__ work,
                                                                    int32_t j0, int32_t nrb) {
  __shared__ double lds[GRID_LDS_DOUBLES];
  __shared__ int32_t word;
  const int k = blockIdx.y, tid = threadIdx.x;
  if (j0 > 0 && info[k] != 0) return;
  double* A = A_all + (int64_t)k * n * lda;
  const int jp = j0 - CHOL_NB;                       // the previous panel's first column
  const int i0 = j0 + CHOL_NB;                       // first row (and column) behind this panel
  if ((int)blockIdx.x >= nrb) {
    // ---- a trailing tile: panel q - 1's update right of panel q
    double* Li = lds;
    double* Lj = lds + CHOL_TILE * CHOL_LD;
    int bi = 0, bj = (int)blockIdx.x - nrb;          // tile number in the lower triangle, row by row
    while (bj > bi) {
      bj -= bi + 1;
      ++bi;
    }
    const int ti = i0 + bi * CHOL_TILE, tj = i0 + bj * CHOL_TILE;
    for (int e = tid; e < CHOL_TILE * CHOL_NB; e += CHOL_BLOCK) {
      const int r = e / CHOL_NB, c = e - r * CHOL_NB;
      Li[r * CHOL_LD + c] = (ti + r < n) ? A[(int64_t)(ti + r) * lda + jp + c] : 0.0;
      Lj[r * CHOL_LD + c] = (tj + r < n) ? A[(int64_t)(tj + r) * lda + jp + c] : 0.0;
    }
    __syncthreads();
    const int tx = tid & 15, ty = tid >> 4;
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
        for (int v = 0; v < 4; ++v) acc[u][v] = fma(li[u], lj[v], acc[u][v]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = ti + ty + 16 * u, j = tj + tx + 16 * v;
        if (i < n && j <= i) A[(int64_t)i * lda + j] -= acc[u][v];
      }
    return;
  }
  // ---- a panel workgroup
  double* P = lds;                                   // panel q - 1's columns of the rows below
  double* V = lds + GRID_VROWS * CHOL_LD;            // panel q's columns: rows 0 .. 31 the diagonal block's, then the workgroup's own
  double* Ld = P;                                    // the factored diagonal block, once P has been used
  const int rb = blockIdx.x;
  const int nb = min(CHOL_NB, n - j0);
  const bool below = i0 < n;
  const int r0 = i0 + rb * GRID_ROWS;                // this workgroup's first row
  const int nr = below ? min(GRID_ROWS, n - r0) : 0;
  constexpr int PER_LANE = GRID_VROWS * CHOL_NB / CHOL_BLOCK;   // 12 entries per lane: entry e = (row e / 32, column e % 32)
  if (tid == 0) word = 0;
  if (rb == 0 && j0 > 0) {                           // the previous panel's factored diagonal block, from the launch before
    const double* src = work + ((int64_t)k * 2 + ((jp / CHOL_NB) & 1)) * GRID_DIAG;
    for (int e = tid; e < GRID_DIAG; e += CHOL_BLOCK) {
      const int r = e / CHOL_NB, c = e - r * CHOL_NB;
      if (c <= r) A[(int64_t)(jp + r) * lda + jp + c] = src[e];
    }
  }
#pragma unroll
  for (int m = 0; m < PER_LANE; ++m) {
    const int e = tid + CHOL_BLOCK * m;
    const int r = e / CHOL_NB, c = e - r * CHOL_NB;
    const bool diag = r < CHOL_NB;
    const bool live = diag ? r < nb : r - CHOL_NB < nr;
    const int64_t g = diag ? j0 + r : r0 + r - CHOL_NB;          // the row in A
    V[r * CHOL_LD + c] = (live && (!diag || (c <= r && c < nb))) ? A[g * lda + j0 + c] : 0.0;
    P[r * CHOL_LD + c] = (live && j0 > 0) ? A[g * lda + jp + c] : 0.0;
  }
  __syncthreads();
  if (j0 > 0) {                                      // A_ij -= sum_p L_ip L_jp over panel q - 1, as its trailing tiles do it
    double acc[PER_LANE];
#pragma unroll
    for (int m = 0; m < PER_LANE; ++m) acc[m] = 0.0;
    const int c = tid & (CHOL_NB - 1), rq = tid >> 5;            // entry m of the lane: row rq + 8 m, column c
#pragma unroll 4
    for (int p = 0; p < CHOL_NB; ++p) {
      const double lj = P[c * CHOL_LD + p];
#pragma unroll
      for (int m = 0; m < PER_LANE; ++m) acc[m] = fma(P[(rq + 8 * m) * CHOL_LD + p], lj, acc[m]);
    }
#pragma unroll
    for (int m = 0; m < PER_LANE; ++m) V[(rq + 8 * m) * CHOL_LD + c] -= acc[m];
    __syncthreads();
  }
  if (tid < RATO_WAVE) {
    double row[CHOL_NB];
    const int fail = diag_factor(V, j0, nb, tid, row);
    if (fail) {
      if (tid == 0) {
        word = fail;
        if (rb == 0) info[k] = fail;
      }
    } else {
      if (j0 == 0 && rb == 0 && tid == 0) info[k] = 0;
      if (tid < CHOL_NB) {
#pragma unroll
        for (int c = 0; c < CHOL_NB; ++c) Ld[tid * CHOL_LD + c] = row[c];
        if (rb == 0 && tid < nb) {
          double* dst = below ? work + ((int64_t)k * 2 + ((j0 / CHOL_NB) & 1)) * GRID_DIAG + tid * CHOL_NB
                              : A + (int64_t)(j0 + tid) * lda + j0;
#pragma unroll
          for (int c = 0; c < CHOL_NB; ++c)
            if (c <= tid) dst[c] = row[c];
        }
      }
    }
  }
  __syncthreads();
  if (word != 0 || !below) return;
  if (tid < nr) {                                    // x L11' = a, one lane per row
    double* a = V + (CHOL_NB + tid) * CHOL_LD;
    double x[CHOL_NB];
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c) x[c] = a[c];
    // per entry what chol_factor does (a_c, then fma(-x_p, L_cp, .) for p ascending, then / L_cc), with the fmas of a finished
    // x_p issued for every later column at once: independent work between two divisions of the chain
#pragma unroll
    for (int p = 0; p < CHOL_NB; ++p) {
      x[p] = x[p] / Ld[p * CHOL_LD + p];
#pragma unroll
      for (int c = p + 1; c < CHOL_NB; ++c) x[c] = fma(-x[p], Ld[c * CHOL_LD + p], x[c]);
      __builtin_amdgcn_sched_barrier(0);             // the later columns' reads of Ld stay in their own steps (registers)
    }
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c) a[c] = x[c];
  }
  __syncthreads();
  for (int e = tid; e < GRID_ROWS * CHOL_NB; e += CHOL_BLOCK) {
    const int r = e / CHOL_NB, c = e - r * CHOL_NB;
    if (r < nr) A[(int64_t)(r0 + r) * lda + j0 + c] = V[(CHOL_NB + r) * CHOL_LD + c];
  }
}

// x lives in LDS (n doubles, dynamic), as in chol_solve_kernel
__global__ __launch_bounds__(CHOL_BLOCK) void chol_grid_solve_kernel(const double* __restrict__ L_all, int32_t n, int64_t lda,
                                                                     double* __restrict__ B_all, int32_t nrhs, int64_t ldb) {
  extern __shared__ double xs[];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double* L = L_all + (int64_t)k * n * lda;
  double* b = B_all + ((int64_t)k * nrhs + blockIdx.y) * ldb;
  for (int i = tid; i < n; i += CHOL_BLOCK) xs[i] = b[i];
  const bool w0 = tid < RATO_WAVE;
  const int r = tid;
  double tri[CHOL_NB];                               // wave 0: lane r's row (forward) or column (backward) of the next triangle
  // ---- L y = b
#pragma unroll
  for (int c = 0; c < CHOL_NB; ++c)
    tri[c] = (w0 && c <= r && r < min(CHOL_NB, n)) ? L[(int64_t)r * lda + c] : ((r == c) ? 1.0 : 0.0);
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += CHOL_NB) {
    const int nb = min(CHOL_NB, n - j0);
    const int i1 = j0 + CHOL_NB + tid;               // the lane's first row below, its slice of the panel requested now
    double l[CHOL_NB];
#pragma unroll
    for (int p = 0; p < CHOL_NB; ++p) l[p] = (i1 < n) ? L[(int64_t)i1 * lda + j0 + p] : 0.0;
    const int jn = j0 + CHOL_NB, nbn = min(CHOL_NB, n - jn);   // and the next triangle: both land while the chain runs
    double trn[CHOL_NB];
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c)
      trn[c] = (w0 && c <= r && r < nbn) ? L[(int64_t)(jn + r) * lda + jn + c] : ((r == c) ? 1.0 : 0.0);
    if (w0) {
      double x = (r < nb) ? xs[j0 + r] : 0.0;
#pragma unroll
      for (int c = 0; c < CHOL_NB; ++c) {
        if (c < nb) {
          if (r == c) x = x / tri[c];
          const double xc = lane_value(x, c);
          if (r > c && r < nb) x = fma(-tri[c], xc, x);
        }
      }
      if (r < nb) xs[j0 + r] = x;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c) tri[c] = trn[c];
    for (int i = i1; i < n; i += CHOL_BLOCK) {
      if (i != i1) {
#pragma unroll
        for (int p = 0; p < CHOL_NB; ++p) l[p] = L[(int64_t)i * lda + j0 + p];
      }
      double s = xs[i];
#pragma unroll
      for (int p = 0; p < CHOL_NB; ++p) s = fma(-l[p], xs[j0 + p], s);
      xs[i] = s;
    }
    __syncthreads();
  }
  // ---- L' x = y, blocks from the end
  const int jl = ((n - 1) / CHOL_NB) * CHOL_NB;
  {
    const int nb = n - jl;
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c)
      tri[c] = (w0 && c >= r && c < nb) ? L[(int64_t)(jl + c) * lda + jl + r] : ((r == c) ? 1.0 : 0.0);
  }
  for (int j0 = jl; j0 >= 0; j0 -= CHOL_NB) {
    const int nb = min(CHOL_NB, n - j0);
    double l[CHOL_NB];                               // rows above: column tid of the block's rows
#pragma unroll
    for (int p = 0; p < CHOL_NB; ++p) l[p] = (tid < j0 && p < nb) ? L[(int64_t)(j0 + p) * lda + tid] : 0.0;
    const int jn = j0 - CHOL_NB;                     // the block before this one is full
    double trn[CHOL_NB];
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c)
      trn[c] = (w0 && jn >= 0 && c >= r && r < CHOL_NB) ? L[(int64_t)(jn + c) * lda + jn + r] : ((r == c) ? 1.0 : 0.0);
    if (w0) {
      double x = (r < nb) ? xs[j0 + r] : 0.0;
#pragma unroll
      for (int c = CHOL_NB - 1; c >= 0; --c) {
        if (c < nb) {
          if (r == c) x = x / tri[c];
          const double xc = lane_value(x, c);
          if (r < c) x = fma(-tri[c], xc, x);
        }
      }
      if (r < nb) xs[j0 + r] = x;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CHOL_NB; ++c) tri[c] = trn[c];
    for (int i = tid; i < j0; i += CHOL_BLOCK) {
      if (i != tid) {
#pragma unroll
        for (int p = 0; p < CHOL_NB; ++p) l[p] = (p < nb) ? L[(int64_t)(j0 + p) * lda + i] : 0.0;
      }
      double s = xs[i];
#pragma unroll
      for (int p = 0; p < CHOL_NB; ++p)
        if (p < nb) s = fma(-l[p], xs[j0 + p], s);
      xs[i] = s;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += CHOL_BLOCK) b[i] = xs[i];
}

}  // namespace

extern "C" int64_t rato_chol_grid_work_doubles(int32_t n) { return n > CHOL_NB ? 2 * GRID_DIAG : 0; }

extern "C" int rato_chol_factor_grid_batch_f64(double* A, int32_t n, int64_t lda, int32_t K, int32_t* info, double* work,
                                               void* stream) {
  if (!A || !info || n < 1 || lda < n || K < 1 || K > 65535) return RATO_EINVAL;
  if (!work && rato_chol_grid_work_doubles(n) > 0) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  for (int32_t j0 = 0; j0 < n; j0 += CHOL_NB) {
    const int32_t left = n - j0 - CHOL_NB;           // rows below the panel
    const int32_t nrb = left > 0 ? (left + GRID_ROWS - 1) / GRID_ROWS : 1;
    const int64_t T = (left > 0 && j0 > 0) ? (left + CHOL_TILE - 1) / CHOL_TILE : 0;   // the previous panel's trailing tiles
    hipLaunchKernelGGL(chol_grid_step_kernel, dim3((unsigned)(nrb + T * (T + 1) / 2), (unsigned)K), dim3(CHOL_BLOCK), 0,
                       (hipStream_t)stream, A, n, lda, info, work, j0, nrb);
    RATO_LAUNCH_CHECK();
  }
  return RATO_OK;
}

extern "C" int rato_chol_solve_grid_batch_f64(const double* L, int32_t n, int64_t lda, int32_t K, double* B, int32_t nrhs,
                                              int64_t ldb, void* stream) {
  if (!L || !B || n < 1 || n > 8000 || lda < n || K < 1 || K > 65535 || nrhs < 1 || nrhs > 65535 || ldb < n) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(chol_grid_solve_kernel, dim3((unsigned)K, (unsigned)nrhs), dim3(CHOL_BLOCK), (size_t)n * sizeof(double),
                     (hipStream_t)stream, L, n, lda, B, nrhs, ldb);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
