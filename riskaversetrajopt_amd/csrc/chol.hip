// Batched Cholesky, fp64: the workgroup functions of csrc/rato_chol.h as kernels of their own, K problems per launch.
//
//   rato_chol_factor_batch_f64  in-place blocked Cholesky, one workgroup per problem; doubles as the inertia test of the
//                               interior-point solvers (riskaversetrajopt_amd/ipm.py)
//   rato_chol_solve_batch_f64   forward and back substitution on the factor, one workgroup per (problem, right-hand side)
//
// No atomics: two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.
#include "rato_chol.h"

namespace {

using namespace rato;

__global__ __launch_bounds__(CHOL_BLOCK) void chol_factor_kernel(double* __restrict__ A_all, int32_t n, int64_t lda,
                                                                 int32_t* __restrict__ info) {
  __shared__ double Ld[CHOL_NB * CHOL_LD];
  __shared__ double Li[CHOL_TILE * CHOL_LD];
  __shared__ double Lj[CHOL_TILE * CHOL_LD];
  __shared__ int32_t word;
  const int k = blockIdx.x;
  const int fail = chol_factor(A_all + (int64_t)k * n * lda, n, lda, Ld, Li, Lj, &word);
  if (threadIdx.x == 0) info[k] = fail;
}

// x lives in LDS (n doubles, dynamic)
__global__ __launch_bounds__(CHOL_BLOCK) void chol_solve_kernel(const double* __restrict__ L_all, int32_t n, int64_t lda,
                                                                double* __restrict__ B_all, int32_t nrhs, int64_t ldb) {
  extern __shared__ double xs[];
  const int k = blockIdx.x, tid = threadIdx.x;
  double* b = B_all + ((int64_t)k * nrhs + blockIdx.y) * ldb;
  for (int i = tid; i < n; i += CHOL_BLOCK) xs[i] = b[i];
  chol_solve(L_all + (int64_t)k * n * lda, n, lda, xs);
  for (int i = tid; i < n; i += CHOL_BLOCK) b[i] = xs[i];
}

}  // namespace

extern "C" int rato_chol_panel_width(void) { return CHOL_NB; }

extern "C" int rato_chol_factor_batch_f64(double* A, int32_t n, int64_t lda, int32_t K, int32_t* info, void* stream) {
  if (!A || !info || n < 1 || lda < n || K < 1 || K > 65535) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(chol_factor_kernel, dim3((unsigned)K), dim3(CHOL_BLOCK), 0, (hipStream_t)stream, A, n, lda, info);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_chol_solve_batch_f64(const double* L, int32_t n, int64_t lda, int32_t K, double* B, int32_t nrhs, int64_t ldb,
                                         void* stream) {
  if (!L || !B || n < 1 || n > 8000 || lda < n || K < 1 || K > 65535 || nrhs < 1 || nrhs > 65535 || ldb < n) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(chol_solve_kernel, dim3((unsigned)K, (unsigned)nrhs), dim3(CHOL_BLOCK), (size_t)n * sizeof(double),
                     (hipStream_t)stream, L, n, lda, B, nrhs, ldb);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
