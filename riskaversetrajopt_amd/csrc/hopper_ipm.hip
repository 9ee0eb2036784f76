// Newton step of the hopper's interior-point solver (riskaversetrajopt_amd/hopper_ipm.py), fp64, K problems per launch.
//
//   rato_normal_matrix_f64      Kc = J' diag(d) J + W + diag(diag) on the fixed pattern of jac_g, through a product map the
//                               host builds once; the lower triangle of a dense n x n array, zero outside the structure
//   rato_chol_factor_batch_f64  in-place blocked Cholesky, one workgroup per problem; doubles as the inertia test
//   rato_chol_solve_batch_f64   forward and back substitution on the factor
//   rato_csc_matvec_f64 / rato_csc_tmatvec_f64   J v and J' w on the same pattern through a row / column list
//
// No floating-point atomics anywhere: every output entry has one owner that sums in a fixed order, so two calls are bitwise
// equal and problem k of a batch is bitwise its K = 1 call (nothing a lane computes depends on K).
//
// The Cholesky.  Row-major, lower triangle: L[i][j] = A[i * lda + j], j <= i.  Right-looking over panels of CH_NB = 32
// columns:
//   1. the 32 x 32 diagonal block is factored by wave 0 in registers (lane r owns row r; the pivot column travels by
//      __shfl), which needs no barrier; a non-positive or non-finite pivot j sets info = j + 1 and the workgroup leaves;
//   2. the rows below are solved against it, one lane per row, the block read from LDS (broadcast reads);
//   3. the trailing matrix is updated in 64 x 64 tiles; the two 64 x 32 slices of the panel a tile needs are staged in LDS
//      (the matrix itself stays in global memory: 1.28 MB at n = 400, L2 resident), each lane owns a 4 x 4 micro-tile whose
//      columns are consecutive across lanes (coalesced rows).
// Only entries with j <= i < n are ever read or written: the strict upper triangle and the padding may hold anything.
#include "rato_common.h"

#include <math.h>

namespace {

constexpr int CH_BLOCK = 256;
constexpr int CH_NB = 32;            // panel width
constexpr int CH_TILE = 64;          // trailing-update tile
constexpr int CH_LD = CH_NB + 1;     // LDS row stride of a staged slice (odd: no two rows of a column share a bank pair)
constexpr int IPM_BLOCK = 256;

// ---- normal matrix ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double jac_value(const double* v0, const double* v1, int64_t n0, int32_t i) {
  return i < n0 ? v0[i] : v1[i - n0];
}

__global__ __launch_bounds__(IPM_BLOCK) void normal_matrix_kernel(
    int32_t n, int64_t lda, const double* __restrict__ vals0, int64_t ld0, int64_t n0, const double* __restrict__ vals1,
    int64_t ld1, const double* __restrict__ d, int64_t ncon, const double* __restrict__ hess, int64_t n_hess,
    const double* __restrict__ diag, const int32_t* __restrict__ ent_of, const int64_t* __restrict__ ptr,
    const int32_t* __restrict__ tri_a, const int32_t* __restrict__ tri_b, const int32_t* __restrict__ tri_r,
    const int32_t* __restrict__ hess_src, double* __restrict__ Kc) {
  const int64_t e = (int64_t)blockIdx.x * IPM_BLOCK + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int32_t a = (int32_t)(e / n), b = (int32_t)(e - (int64_t)a * n);
  if (b > a) return;
  const int k = blockIdx.y;
  const int32_t id = ent_of[e];
  double acc = 0.0;
  if (id >= 0) {
    const double* v0 = vals0 + (int64_t)k * ld0;
    const double* v1 = vals1 ? vals1 + (int64_t)k * ld1 : nullptr;
    const double* dk = d + (int64_t)k * ncon;
    for (int64_t t = ptr[id]; t < ptr[id + 1]; ++t)
      acc += (jac_value(v0, v1, n0, tri_a[t]) * dk[tri_r[t]]) * jac_value(v0, v1, n0, tri_b[t]);
    const int32_t h = hess_src[id];
    if (hess && h >= 0) acc += hess[(int64_t)k * n_hess + h];
    if (diag && a == b) acc += diag[(int64_t)k * n + a];
  }
  Kc[(int64_t)k * n * lda + (int64_t)a * lda + b] = acc;
}

// y[i] = sum over the list segment of i of vals[idx] * x[other], in list order: J v through the row list, J' w through the
// column list
__global__ __launch_bounds__(IPM_BLOCK) void list_matvec_kernel(
    int64_t n_out, const double* __restrict__ vals0, int64_t ld0, int64_t n0, const double* __restrict__ vals1, int64_t ld1,
    const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const int32_t* __restrict__ other,
    const double* __restrict__ x, int64_t ldx, double* __restrict__ y, int64_t ldy) {
  const int64_t i = (int64_t)blockIdx.x * IPM_BLOCK + threadIdx.x;
  if (i >= n_out) return;
  const int k = blockIdx.y;
  const double* v0 = vals0 + (int64_t)k * ld0;
  const double* v1 = vals1 ? vals1 + (int64_t)k * ld1 : nullptr;
  const double* xk = x + (int64_t)k * ldx;
  double acc = 0.0;
  for (int64_t t = ptr[i]; t < ptr[i + 1]; ++t) acc += jac_value(v0, v1, n0, idx[t]) * xk[other[t]];
  y[(int64_t)k * ldy + i] = acc;
}

// ---- Cholesky ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CH_BLOCK) void chol_factor_kernel(double* __restrict__ A_all, int32_t n, int64_t lda,
                                                               int32_t* __restrict__ info) {
  __shared__ double Ld[CH_NB * CH_LD];            // the factored diagonal block
  __shared__ double Li[CH_TILE * CH_LD];          // panel slices of a trailing tile: its rows ...
  __shared__ double Lj[CH_TILE * CH_LD];          // ... and its columns
  __shared__ int32_t bad;
  const int k = blockIdx.x, tid = threadIdx.x;
  double* A = A_all + (int64_t)k * n * lda;
  if (tid == 0) bad = 0;
  __syncthreads();
  for (int j0 = 0; j0 < n; j0 += CH_NB) {
    const int nb = min(CH_NB, n - j0);
    // 1. the diagonal block, wave 0, registers; rows and columns past n act as the identity
    if (tid < RATO_WAVE) {
      const int r = tid;
      double row[CH_NB];
#pragma unroll
      for (int c = 0; c < CH_NB; ++c)
        row[c] = (r < nb && c <= r && c < nb) ? A[(int64_t)(j0 + r) * lda + j0 + c] : ((r == c) ? 1.0 : 0.0);
      int fail = 0;
#pragma unroll
      for (int j = 0; j < CH_NB; ++j) {
        const double piv = __shfl(row[j], j, RATO_WAVE);
        if (!fail && !(piv > 0.0 && piv <= 1.79769313486231570815e308)) fail = j0 + j + 1;   // wave-uniform
        const double dj = sqrt(piv);
        if (r == j) row[j] = dj;
        else if (r > j) row[j] = row[j] / dj;
#pragma unroll
        for (int c = j + 1; c < CH_NB; ++c) {
          const double lcj = __shfl(row[j], c, RATO_WAVE);
          if (r >= c) row[c] -= row[j] * lcj;
        }
        __builtin_amdgcn_sched_barrier(0);   // keeps the next column's shuffles from being hoisted (no scratch)
      }
      if (fail) {
        if (tid == 0) {
          bad = 1;
          info[k] = fail;
        }
      } else if (r < CH_NB) {
#pragma unroll
        for (int c = 0; c < CH_NB; ++c) {
          Ld[r * CH_LD + c] = row[c];
          if (r < nb && c <= r) A[(int64_t)(j0 + r) * lda + j0 + c] = row[c];
        }
      }
    }
    __syncthreads();
    if (bad) return;                               // every lane reads the same word after the barrier
    const int i0 = j0 + CH_NB;                     // first row below the block
    if (i0 >= n) break;
    // 2. rows below: x L11' = a, one lane per row
    for (int i = i0 + tid; i < n; i += CH_BLOCK) {
      double* a = A + (int64_t)i * lda + j0;
      double x[CH_NB];
#pragma unroll
      for (int c = 0; c < CH_NB; ++c) x[c] = a[c];
#pragma unroll
      for (int c = 0; c < CH_NB; ++c) {
        double s = x[c];
#pragma unroll
        for (int p = 0; p < c; ++p) s -= x[p] * Ld[c * CH_LD + p];
        x[c] = s / Ld[c * CH_LD + c];
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int c = 0; c < CH_NB; ++c) a[c] = x[c];
    }
    __syncthreads();
    // 3. trailing update, 64 x 64 tiles of the lower triangle
    const int tx = tid & 15, ty = tid >> 4;
    for (int ti = i0; ti < n; ti += CH_TILE) {
      for (int tj = i0; tj <= ti; tj += CH_TILE) {
        for (int e = tid; e < CH_TILE * CH_NB; e += CH_BLOCK) {
          const int r = e / CH_NB, c = e - r * CH_NB;
          Li[r * CH_LD + c] = (ti + r < n) ? A[(int64_t)(ti + r) * lda + j0 + c] : 0.0;
          Lj[r * CH_LD + c] = (tj + r < n) ? A[(int64_t)(tj + r) * lda + j0 + c] : 0.0;
        }
        __syncthreads();
        double acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
#pragma unroll 4
        for (int p = 0; p < CH_NB; ++p) {
          double li[4], lj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            li[u] = Li[(ty + 16 * u) * CH_LD + p];
            lj[u] = Lj[(tx + 16 * u) * CH_LD + p];
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
  if (tid == 0) info[k] = 0;
}

// one workgroup per (problem, right-hand side); x lives in LDS (n doubles, dynamic)
__global__ __launch_bounds__(CH_BLOCK) void chol_solve_kernel(const double* __restrict__ L_all, int32_t n, int64_t lda,
                                                              double* __restrict__ B_all, int32_t nrhs, int64_t ldb) {
  extern __shared__ double xs[];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double* L = L_all + (int64_t)k * n * lda;
  double* b = B_all + ((int64_t)k * nrhs + blockIdx.y) * ldb;
  for (int i = tid; i < n; i += CH_BLOCK) xs[i] = b[i];
  __syncthreads();
  // L y = b
  for (int j0 = 0; j0 < n; j0 += CH_NB) {
    const int nb = min(CH_NB, n - j0);
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
    for (int i = j0 + CH_NB + tid; i < n; i += CH_BLOCK) {   // rows below: contiguous reads of their own row
      const double* l = L + (int64_t)i * lda + j0;
      double s = xs[i];
      for (int p = 0; p < CH_NB; ++p) s -= l[p] * xs[j0 + p];
      xs[i] = s;
    }
    __syncthreads();
  }
  // L' x = y, blocks from the end
  for (int j0 = ((n - 1) / CH_NB) * CH_NB; j0 >= 0; j0 -= CH_NB) {
    const int nb = min(CH_NB, n - j0);
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
    for (int i = tid; i < j0; i += CH_BLOCK) {     // rows above: column i of the block's rows, consecutive across lanes
      double s = xs[i];
      for (int p = 0; p < nb; ++p) s -= L[(int64_t)(j0 + p) * lda + i] * xs[j0 + p];
      xs[i] = s;
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += CH_BLOCK) b[i] = xs[i];
}

unsigned blocks_of(int64_t n) {
  const int64_t nb = (n + IPM_BLOCK - 1) / IPM_BLOCK;
  return (nb < 1 || nb > 0x7fffffffLL) ? 0u : (unsigned)nb;
}

}  // namespace

extern "C" int rato_normal_matrix_f64(int32_t K, int32_t n, int64_t lda, const double* vals0, int64_t ld0, int64_t n0,
                                      const double* vals1, int64_t ld1, int64_t n1, const double* d, int64_t ncon,
                                      const double* hess, int64_t n_hess, const double* diag, const int32_t* ent_of,
                                      const int64_t* ptr, const int32_t* tri_a, const int32_t* tri_b, const int32_t* tri_r,
                                      const int32_t* hess_src, double* Kc, void* stream) {
  if (K < 1 || K > 65535 || n < 1 || n > 32768 || lda < n || !vals0 || n0 < 1 || ld0 < n0 || n1 < 0 || (n1 > 0 && (!vals1 || ld1 < n1)) ||
      !d || ncon < 1 || (hess && n_hess < 1) || !ent_of || !ptr || !tri_a || !tri_b || !tri_r || !hess_src || !Kc)
    return RATO_EINVAL;
  const unsigned nb = blocks_of((int64_t)n * n);
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(normal_matrix_kernel, dim3(nb, (unsigned)K), dim3(IPM_BLOCK), 0, (hipStream_t)stream, n, lda, vals0, ld0,
                     n0, n1 > 0 ? vals1 : nullptr, ld1, d, ncon, hess, n_hess, diag, ent_of, ptr, tri_a, tri_b, tri_r,
                     hess_src, Kc);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

static int list_matvec(int32_t K, int64_t n_out, int64_t n_in, const double* vals0, int64_t ld0, int64_t n0, const double* vals1,
                       int64_t ld1, int64_t n1, const int64_t* ptr, const int32_t* idx, const int32_t* other, const double* x,
                       int64_t ldx, double* y, int64_t ldy, void* stream) {
  if (K < 1 || K > 65535 || n_out < 1 || n_in < 1 || !vals0 || n0 < 1 || ld0 < n0 || n1 < 0 || (n1 > 0 && (!vals1 || ld1 < n1)) ||
      !ptr || !idx || !other || !x || !y || ldx < n_in || ldy < n_out)
    return RATO_EINVAL;
  const unsigned nb = blocks_of(n_out);
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(list_matvec_kernel, dim3(nb, (unsigned)K), dim3(IPM_BLOCK), 0, (hipStream_t)stream, n_out, vals0, ld0, n0,
                     n1 > 0 ? vals1 : nullptr, ld1, ptr, idx, other, x, ldx, y, ldy);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_csc_matvec_f64(int32_t K, int64_t ncon, int64_t n, const double* vals0, int64_t ld0, int64_t n0,
                                   const double* vals1, int64_t ld1, int64_t n1, const int64_t* row_ptr, const int32_t* row_idx,
                                   const int32_t* row_col, const double* v, int64_t ldv, double* out, int64_t ldo, void* stream) {
  return list_matvec(K, ncon, n, vals0, ld0, n0, vals1, ld1, n1, row_ptr, row_idx, row_col, v, ldv, out, ldo, stream);
}

extern "C" int rato_csc_tmatvec_f64(int32_t K, int64_t ncon, int64_t n, const double* vals0, int64_t ld0, int64_t n0,
                                    const double* vals1, int64_t ld1, int64_t n1, const int64_t* col_ptr, const int32_t* col_idx,
                                    const int32_t* col_row, const double* w, int64_t ldw, double* out, int64_t ldo, void* stream) {
  return list_matvec(K, n, ncon, vals0, ld0, n0, vals1, ld1, n1, col_ptr, col_idx, col_row, w, ldw, out, ldo, stream);
}

extern "C" int rato_chol_panel_width(void) { return CH_NB; }

extern "C" int rato_chol_factor_batch_f64(double* A, int32_t n, int64_t lda, int32_t K, int32_t* info, void* stream) {
  if (!A || !info || n < 1 || lda < n || K < 1 || K > 65535) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(chol_factor_kernel, dim3((unsigned)K), dim3(CH_BLOCK), 0, (hipStream_t)stream, A, n, lda, info);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_chol_solve_batch_f64(const double* L, int32_t n, int64_t lda, int32_t K, double* B, int32_t nrhs, int64_t ldb,
                                         void* stream) {
  if (!L || !B || n < 1 || n > 8000 || lda < n || K < 1 || K > 65535 || nrhs < 1 || nrhs > 65535 || ldb < n) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(chol_solve_kernel, dim3((unsigned)K, (unsigned)nrhs), dim3(CH_BLOCK), (size_t)n * sizeof(double),
                     (hipStream_t)stream, L, n, lda, B, nrhs, ldb);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
