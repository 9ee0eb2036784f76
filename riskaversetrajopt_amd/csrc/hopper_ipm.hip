// Newton step of the hopper's interior-point solver (riskaversetrajopt_amd/hopper_ipm.py), fp64, K problems per launch.
//
//   rato_normal_matrix_f64      Kc = J' diag(d) J + W + diag(diag) on the fixed pattern of jac_g, through a product map the
//                               host builds once; the lower triangle of a dense n x n array, zero outside the structure
//   rato_csc_matvec_f64 / rato_csc_tmatvec_f64   J v and J' w on the same pattern through a row / column list
//
// Kc is factored, and systems with it solved, by csrc/chol.hip (rato_chol_factor_batch_f64 / rato_chol_solve_batch_f64).
//
// No floating-point atomics anywhere: every output entry has one owner that sums in a fixed order, so two calls are bitwise
// equal and problem k of a batch is bitwise its K = 1 call (nothing a lane computes depends on K).
#include "rato_common.h"

namespace {

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
