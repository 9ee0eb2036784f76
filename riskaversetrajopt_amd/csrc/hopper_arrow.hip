// Arrowhead Newton step of the hopper's interior-point solver at large M (riskaversetrajopt_amd/hopper_arrow.py, newton='arrow';
// DESIGN §7.af), fp64, K problems per launch.
//
// The M variables ys enter the condensed matrix Kc only through E = diag(e) + d_0 1 1', so they are eliminated exactly and what
// is factored is the core's Schur complement S^ (n_c = 8(S+1) + 4S + 2).  Everything here is the work over the sample axis:
//
//   rato_hopper_arrow_reduce_f64    e, and G = B_s' diag(1/e) B_s, w = B_s' (1/e), a = B_s' 1, s = 1' (1/e) and the slip rows' own
//                                   5 x 5 blocks P_c over the q = 5C + 2 touched columns, b_i built on the fly from the partials
//   rato_hopper_arrow_assemble_f64  adds the sample terms into the lower triangle rato_normal_matrix_f64 left for the core
//   rato_hopper_arrow_cols_f64      sum_i omega_ic grad_c h_ic: J_risk' w (omega = w) and B_s' t (omega = -t_i d_ic)
//   rato_hopper_arrow_rows_f64      J_risk v on the risk rows, and B_s x
//   rato_hopper_arrow_edot_f64 / rato_hopper_arrow_eapply_f64   (1/e)' v and (1/e) o (v - kappa): E^-1 by Sherman-Morrison
//   rato_hopper_arrow_scale_f64 / _tfix_f64 / _kkbeta_f64 / _einv_f64 / _rhsfix_f64   the O(q + M) fix-ups between those launches
//                                   on device arrays, for the driver on the device
//
// Samples are cut into chunks of AR_CHUNK; a chunk sums its samples ascending into the caller's partials buffer
// [nchunks][K][n_part], a second launch sums the chunks ascending.  No floating-point atomics, every output has one owner and
// nothing a lane computes depends on K: two calls are bitwise equal and problem k of a batch is bitwise its K = 1 call.
// Partials: dh_dx [K][C][3][M] and dh_dfz [K][C][M] as rato_hopper_slip_f64 leaves them; grad_c h_ic = (dh/dx0, dh/dx2, dh/dx3,
// 1 on fx, dh/dfz, -1 on slack, -1 on t_risk); d is read in place at the risk rows (slip row of sample i, contact c at
// r0 + i C + c, the row -y_i at r0 - M + i, the sum row at r0 - M - 1).
#include "rato_common.h"

#include <math.h>

namespace {

constexpr int AR_CHUNK = 32;
constexpr int AR_BLOCK = 256;
constexpr int AR_MAX_C = 50;         // AR_CHUNK (5C + 2 + 1) doubles of LDS <= 64 KiB

__device__ __forceinline__ int tri_row(int e) {
  int p = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
  while ((p + 1) * (p + 2) / 2 <= e) ++p;
  while (p * (p + 1) / 2 > e) --p;
  return p;
}

// component j of (dh/dx0, dh/dx2, dh/dx3, 1, dh/dfz) of sample i, contact c
__device__ __forceinline__ double grad5(const double* __restrict__ dx, const double* __restrict__ dfz, int64_t M, int c, int j,
                                        int64_t i) {
  if (j < 3) return dx[((int64_t)c * 3 + j) * M + i];
  return j == 3 ? 1.0 : dfz[(int64_t)c * M + i];
}

__global__ __launch_bounds__(AR_BLOCK) void arrow_reduce_kernel(
    int32_t K, int64_t M, int32_t C, int32_t saa, const double* __restrict__ dh_dx, const double* __restrict__ dh_dfz,
    const double* __restrict__ d, int64_t ldd, int64_t r0, const double* __restrict__ ydiag, double* __restrict__ e_out,
    double* __restrict__ part) {
  extern __shared__ double lds[];
  const int q = 5 * C + 2, tid = threadIdx.x, k = blockIdx.y;
  double* b = lds;                       // [AR_CHUNK][q]
  double* us = lds + AR_CHUNK * q;       // [AR_CHUNK]
  const int64_t i0 = (int64_t)blockIdx.x * AR_CHUNK;
  const int ns = (int)min((int64_t)AR_CHUNK, M - i0);
  const double* dx = dh_dx + (int64_t)k * C * 3 * M;
  const double* dfz = dh_dfz + (int64_t)k * C * M;
  const double* dk = d + (int64_t)k * ldd;
  for (int idx = tid; idx < ns * C; idx += AR_BLOCK) {
    const int c = idx / ns, i = idx - c * ns;
    const double dic = dk[r0 + (i0 + i) * C + c];
    double* bi = b + i * q + 5 * c;
    bi[0] = -(dic * dx[((int64_t)c * 3 + 0) * M + i0 + i]);
    bi[1] = -(dic * dx[((int64_t)c * 3 + 1) * M + i0 + i]);
    bi[2] = -(dic * dx[((int64_t)c * 3 + 2) * M + i0 + i]);
    bi[3] = -dic;
    bi[4] = -(dic * dfz[(int64_t)c * M + i0 + i]);
  }
  __syncthreads();
  if (tid < ns) {
    double dsum = 0.0;
    for (int c = 0; c < C; ++c) dsum -= b[tid * q + 5 * c + 3];
    b[tid * q + 5 * C] = dsum;
    b[tid * q + 5 * C + 1] = saa ? dsum : 0.0;
    double e = ydiag[(int64_t)k * M + i0 + tid];
    if (saa) e = (e + dk[r0 - M + i0 + tid]) + dsum;
    e_out[(int64_t)k * M + i0 + tid] = e;
    us[tid] = 1.0 / e;
  }
  __syncthreads();
  const int nent = q * (q + 1) / 2;
  const int np = nent + 2 * q + 1 + 15 * C;
  double* out = part + ((int64_t)blockIdx.x * K + k) * np;
  for (int x = tid; x < np; x += AR_BLOCK) {
    double acc = 0.0;
    if (x < nent) {
      const int p = tri_row(x), r = x - p * (p + 1) / 2;
      for (int i = 0; i < ns; ++i) acc += (b[i * q + p] * us[i]) * b[i * q + r];
    } else if (x < nent + q) {
      const int p = x - nent;
      for (int i = 0; i < ns; ++i) acc += b[i * q + p] * us[i];
    } else if (x < nent + 2 * q) {
      const int p = x - nent - q;
      for (int i = 0; i < ns; ++i) acc += b[i * q + p];
    } else if (x == nent + 2 * q) {
      for (int i = 0; i < ns; ++i) acc += us[i];
    } else {
      const int y = x - (nent + 2 * q + 1), c = y / 15, f = y - 15 * c;
      const int j = tri_row(f), l = f - j * (j + 1) / 2;
      for (int i = 0; i < ns; ++i)
        acc += (dk[r0 + (i0 + i) * C + c] * grad5(dx, dfz, M, c, j, i0 + i)) * grad5(dx, dfz, M, c, l, i0 + i);
    }
    out[x] = acc;
  }
}

// red[k][x] = sum over the chunks, ascending
__global__ __launch_bounds__(AR_BLOCK) void arrow_sum_chunks_kernel(int32_t K, int32_t nch, int64_t np,
                                                                    const double* __restrict__ part, double* __restrict__ red) {
  const int64_t x = (int64_t)blockIdx.x * AR_BLOCK + threadIdx.x;
  if (x >= np) return;
  const int k = blockIdx.y;
  double acc = 0.0;
  for (int ch = 0; ch < nch; ++ch) acc += part[((int64_t)ch * K + k) * np + x];
  red[(int64_t)k * np + x] = acc;
}

__global__ __launch_bounds__(AR_BLOCK) void arrow_assemble_kernel(
    int64_t M, int32_t C, int32_t saa, int32_t nc, int64_t lda, const int32_t* __restrict__ qcol, const double* __restrict__ red,
    const double* __restrict__ d, int64_t ldd, int64_t r0, const double* __restrict__ malpha, double* __restrict__ Sh) {
  const int q = 5 * C + 2, nent = q * (q + 1) / 2;
  const int x = blockIdx.x * AR_BLOCK + threadIdx.x;
  if (x >= nent) return;
  const int k = blockIdx.y;
  const int p = tri_row(x), r = x - p * (p + 1) / 2;        // r <= p
  const int slack = 5 * C, tq = 5 * C + 1;
  if (!saa && p == tq) return;                              // the baseline has no t_risk entry in a slip row
  const double* R = red + (int64_t)k * (nent + 2 * q + 1 + 15 * C);
  const double* w = R + nent;
  const double* a = R + nent + q;
  double A;                                                 // the slip rows' own share sum_ic d_ic grad h grad h'
  if (p < slack) {
    const int cp = p / 5, cr = r / 5;
    A = (cp == cr) ? R[nent + 2 * q + 1 + 15 * cp + (p - 5 * cp) * (p - 5 * cp + 1) / 2 + (r - 5 * cr)] : 0.0;
  } else {
    A = (r < slack) ? a[r] : a[slack];
  }
  double T = A;
  if (saa) {
    const double d0 = d[(int64_t)k * ldd + r0 - M - 1], ma = malpha[k];
    const double beta = d0 * ma, s = R[nent + 2 * q], kk = d0 / (1.0 + d0 * s);
    const double etp = (p == tq) ? 1.0 : 0.0, etr = (r == tq) ? 1.0 : 0.0;
    const double vp = w[p] + (beta * s) * etp, vr = w[r] + (beta * s) * etr;
    const double sub = (R[x] + beta * (w[p] * etr + etp * w[r])) + ((beta * beta) * s) * (etp * etr);
    T = (A - sub) + (kk * vp) * vr;
    if (p == tq && r == tq) T += (d0 * ma) * ma;
  }
  const int gp = qcol[p], gr = qcol[r];
  const int hi = max(gp, gr), lo = min(gp, gr);
  Sh[(int64_t)k * nc * lda + (int64_t)hi * lda + lo] += T;
}

// mode 0: omega_ic = wv[r0 + i C + c] (J_risk' w; yout_i = w_0 - w_(1+i) - sum_c omega_ic with saa, 0 without)
// mode 1: omega_ic = -tv_i d_ic       (B_s' t; slot 5C takes sum_i tv_i)
__global__ __launch_bounds__(AR_BLOCK) void arrow_cols_kernel(
    int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* __restrict__ dh_dx, const double* __restrict__ dh_dfz,
    const double* __restrict__ wv, int64_t ldw, int64_t r0, const double* __restrict__ tv, double* __restrict__ yout,
    double* __restrict__ part) {
  const int k = blockIdx.y, tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * AR_CHUNK;
  const int ns = (int)min((int64_t)AR_CHUNK, M - i0);
  const double* dx = dh_dx + (int64_t)k * C * 3 * M;
  const double* dfz = dh_dfz + (int64_t)k * C * M;
  const double* wk = wv + (int64_t)k * ldw;
  const double* tk = mode ? tv + (int64_t)k * M : nullptr;
  const int np = 5 * C + 1;
  double* out = part + ((int64_t)blockIdx.x * K + k) * np;
  for (int x = tid; x < np; x += AR_BLOCK) {
    double acc = 0.0;
    if (x < 5 * C) {
      const int c = x / 5, j = x - 5 * c;
      for (int i = 0; i < ns; ++i) {
        const double wic = wk[r0 + (i0 + i) * C + c];
        const double om = mode ? -(tk[i0 + i] * wic) : wic;
        acc += om * grad5(dx, dfz, M, c, j, i0 + i);
      }
    } else if (mode) {
      for (int i = 0; i < ns; ++i) acc += tk[i0 + i];
    }
    out[x] = acc;
  }
  if (!mode && yout && tid < ns) {
    double y = 0.0;
    if (saa) {
      y = wk[r0 - M - 1] - wk[r0 - M + i0 + tid];
      for (int c = 0; c < C; ++c) y -= wk[r0 + (i0 + tid) * C + c];
    }
    yout[(int64_t)k * M + i0 + tid] = y;
  }
}

// mode 0: out[r0 + i C + c] = grad5 . xq_c - x_slack - x_t - xy_i, out[r0 - M + i] = -xy_i (saa), part[chunk][k] = sum_i xy_i
// mode 1: out[k][i] = bx_i = sum_c -d_ic (grad5 . xq_c - x_slack - x_t) + addc[k]  (B x_c), or xy_i - bx_i when xy is given
__global__ __launch_bounds__(AR_BLOCK) void arrow_rows_kernel(
    int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* __restrict__ dh_dx, const double* __restrict__ dh_dfz,
    const double* __restrict__ xq, const double* __restrict__ xy, const double* __restrict__ d, int64_t ldd, int64_t r0,
    const double* __restrict__ addc, double* __restrict__ out, int64_t ldo, double* __restrict__ part) {
  const int k = blockIdx.y, tid = threadIdx.x, q = 5 * C + 2;
  const int64_t i0 = (int64_t)blockIdx.x * AR_CHUNK;
  const int ns = (int)min((int64_t)AR_CHUNK, M - i0);
  const double* dx = dh_dx + (int64_t)k * C * 3 * M;
  const double* dfz = dh_dfz + (int64_t)k * C * M;
  const double* x = xq + (int64_t)k * q;
  const double xs = x[5 * C], xt = saa ? x[5 * C + 1] : 0.0;
  if (mode == 0) {
    double* o = out + (int64_t)k * ldo;
    for (int idx = tid; idx < ns * C; idx += AR_BLOCK) {
      const int c = idx / ns, i = idx - c * ns;
      double acc = 0.0;
      for (int j = 0; j < 5; ++j) acc += grad5(dx, dfz, M, c, j, i0 + i) * x[5 * c + j];
      acc = (acc - xs) - xt;
      if (saa) acc -= xy[(int64_t)k * M + i0 + i];
      o[r0 + (i0 + i) * C + c] = acc;
    }
    if (saa && tid < ns) o[r0 - M + i0 + tid] = -xy[(int64_t)k * M + i0 + tid];
    if (saa && tid == 0) {
      double acc = 0.0;
      for (int i = 0; i < ns; ++i) acc += xy[(int64_t)k * M + i0 + i];
      part[(int64_t)blockIdx.x * K + k] = acc;
    }
  } else if (tid < ns) {
    const double* dk = d + (int64_t)k * ldd;
    double tot = 0.0;
    for (int c = 0; c < C; ++c) {
      double acc = 0.0;
      for (int j = 0; j < 5; ++j) acc += grad5(dx, dfz, M, c, j, i0 + tid) * x[5 * c + j];
      acc = (acc - xs) - xt;
      tot -= dk[r0 + (i0 + tid) * C + c] * acc;
    }
    const double bx = tot + addc[k];
    out[(int64_t)k * ldo + i0 + tid] = xy ? xy[(int64_t)k * M + i0 + tid] - bx : bx;
  }
}

__global__ __launch_bounds__(AR_BLOCK) void arrow_edot_kernel(int32_t K, int64_t M, const double* __restrict__ e,
                                                              const double* __restrict__ v, double* __restrict__ part) {
  if (threadIdx.x != 0) return;
  const int k = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * AR_CHUNK;
  const int ns = (int)min((int64_t)AR_CHUNK, M - i0);
  double acc = 0.0;
  for (int i = 0; i < ns; ++i) acc += (1.0 / e[(int64_t)k * M + i0 + i]) * v[(int64_t)k * M + i0 + i];
  part[(int64_t)blockIdx.x * K + k] = acc;
}

__global__ __launch_bounds__(AR_BLOCK) void arrow_eapply_kernel(int64_t M, const double* __restrict__ e,
                                                                const double* __restrict__ v, const double* __restrict__ kappa,
                                                                double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * AR_BLOCK + threadIdx.x;
  if (i >= M) return;
  const int k = blockIdx.y;
  out[(int64_t)k * M + i] = (1.0 / e[(int64_t)k * M + i]) * (v[(int64_t)k * M + i] - kappa[k]);
}

// ---- the sample-axis fix-ups of the step under the driver on the device (ipm.solve_group_device): what ArrowDeviceBackend's list
// methods do on the host between the launches above, operation by operation in the host's order (__dmul_rn / __dadd_rn /
// __ddiv_rn wherever a product feeds a sum: the library is built with contraction on).  One lane per output.

// -ffp-contract=fast lets the back end fuse an inlined __dmul_rn into the add that follows it: a product that must stay a
// product goes through an empty asm statement, which hides where it came from (``unfused`` of driving.hip)
__device__ __forceinline__ double product(double a, double b) {
  double x = __dmul_rn(a, b);
  asm volatile("" : "+v"(x));
  return x;
}

// -sum_c of the fx column sums, contacts ascending
__device__ __forceinline__ double minus_fx_total(const double* __restrict__ R, int C) {
  double tot = 0.0;
  for (int c = 0; c < C; ++c) tot -= R[5 * c + 3];
  return tot;
}

// out[k][ocol] = a[k] x[k][col] (+ add[k])
__global__ __launch_bounds__(AR_BLOCK) void arrow_scale_kernel(int32_t K, const double* __restrict__ a, const double* __restrict__ x,
                                                               int64_t ldx, int64_t col, const double* __restrict__ add,
                                                               double* __restrict__ out, int64_t ldo, int64_t ocol) {
  const int k = blockIdx.x * AR_BLOCK + threadIdx.x;
  if (k >= K) return;
  const double prod = product(a[k], x[(int64_t)k * ldx + col]);
  out[(int64_t)k * ldo + ocol] = add ? __dadd_rn(prod, add[k]) : prod;
}

// J' w in z numbering after cols mode 0: the touched columns, slack, t_risk and (saa) the y block
__global__ __launch_bounds__(AR_BLOCK) void arrow_tfix_kernel(int64_t M, int32_t C, int32_t saa, int64_t n,
                                                              const int32_t* __restrict__ qz, const double* __restrict__ red,
                                                              int64_t ldr, const double* __restrict__ malpha,
                                                              const double* __restrict__ w, int64_t ldw, int64_t rr,
                                                              const double* __restrict__ yout, double* __restrict__ out,
                                                              int64_t ldo) {
  const int64_t x = (int64_t)blockIdx.x * AR_BLOCK + threadIdx.x;
  const int k = blockIdx.y;
  const int64_t y0 = n - 2 - M;
  const double* R = red + (int64_t)k * ldr;
  double* o = out + (int64_t)k * ldo;
  if (x < 5 * C) {
    const int64_t z = qz[x];
    if (z >= 0 && z < y0) o[z] += R[x];
  } else if (x == 5 * C) {
    o[n - 2] += minus_fx_total(R, C);
  } else if (x == 5 * C + 1 && saa) {
    o[n - 1] += __dadd_rn(product(malpha[k], w[(int64_t)k * ldw + rr]), minus_fx_total(R, C));
  }
  if (saa && x < M) o[y0 + x] = yout[(int64_t)k * M + x];
}

__global__ __launch_bounds__(AR_BLOCK) void arrow_kkbeta_kernel(int32_t K, int32_t C, const double* __restrict__ d, int64_t ldd,
                                                                int64_t rr, const double* __restrict__ red, int64_t ldr,
                                                                const double* __restrict__ malpha, double* __restrict__ kk,
                                                                double* __restrict__ beta) {
  const int k = blockIdx.x * AR_BLOCK + threadIdx.x;
  if (k >= K) return;
  const int q = 5 * C + 2;
  const double d0 = d[(int64_t)k * ldd + rr], s = red[(int64_t)k * ldr + q * (q + 1) / 2 + 2 * q];
  kk[k] = __ddiv_rn(d0, __dadd_rn(1.0, product(d0, s)));
  beta[k] = __dmul_rn(d0, malpha[k]);
}

// out_i = (1 / e_i) (v_i - kk[k] red[k]); kk NULL: (1 / e_i) v_i
__global__ __launch_bounds__(AR_BLOCK) void arrow_einv_kernel(int64_t M, const double* __restrict__ e, const double* __restrict__ v,
                                                              int64_t ldv, const double* __restrict__ kk,
                                                              const double* __restrict__ red, double* __restrict__ out,
                                                              int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * AR_BLOCK + threadIdx.x;
  if (i >= M) return;
  const int k = blockIdx.y;
  const double kappa = kk ? product(kk[k], red[k]) : 0.0;
  out[(int64_t)k * ldo + i] = __dmul_rn(__ddiv_rn(1.0, e[(int64_t)k * M + i]), v[(int64_t)k * ldv + i] - kappa);
}

// r_c -= B' t after cols mode 1 (core numbering); one workgroup per problem, q <= AR_BLOCK
static_assert(5 * AR_MAX_C + 2 <= AR_BLOCK, "one lane per touched column");
__global__ __launch_bounds__(AR_BLOCK) void arrow_rhsfix_kernel(int32_t C, int32_t nc, const int32_t* __restrict__ qcol,
                                                                const double* __restrict__ red, int64_t ldr,
                                                                const double* __restrict__ beta, double* __restrict__ rc,
                                                                int64_t ldrc) {
  const int x = threadIdx.x, k = blockIdx.x;
  const double* R = red + (int64_t)k * ldr;
  double* r = rc + (int64_t)k * ldrc;
  if (x < 5 * C) {
    const int col = qcol[x];
    if (col >= 0 && col < nc - 2) r[col] -= R[x];
  } else if (x == 5 * C) {
    r[nc - 2] -= minus_fx_total(R, C);
  } else if (x == 5 * C + 1) {
    r[nc - 1] -= __dadd_rn(minus_fx_total(R, C), product(beta[k], R[5 * C]));
  }
}

int64_t chunks_of(int64_t M) { return (M + AR_CHUNK - 1) / AR_CHUNK; }

bool shape_ok(int32_t K, int64_t M, int32_t C) {
  return K >= 1 && K <= 65535 && M >= 1 && C >= 1 && C <= AR_MAX_C && chunks_of(M) <= 0x7fffffffLL &&
         M <= (int64_t)0x7fffffff * AR_BLOCK;
}

int sum_chunks(int32_t K, int64_t M, int64_t np, const double* part, double* red, hipStream_t stream) {
  hipLaunchKernelGGL(arrow_sum_chunks_kernel, dim3((unsigned)((np + AR_BLOCK - 1) / AR_BLOCK), (unsigned)K), dim3(AR_BLOCK), 0,
                     stream, K, (int32_t)chunks_of(M), np, part, red);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

}  // namespace

extern "C" int rato_hopper_arrow_nchunks(int64_t M) {
  return (M < 1 || chunks_of(M) > 0x7fffffffLL) ? 0 : (int)chunks_of(M);
}

extern "C" int rato_hopper_arrow_chunk(void) { return AR_CHUNK; }

extern "C" int64_t rato_hopper_arrow_npart(int32_t C) {
  if (C < 1 || C > AR_MAX_C) return 0;
  const int64_t q = 5 * (int64_t)C + 2;
  return q * (q + 1) / 2 + 2 * q + 1 + 15 * (int64_t)C;
}

extern "C" int rato_hopper_arrow_reduce_f64(int32_t K, int64_t M, int32_t C, int32_t saa, const double* dh_dx,
                                            const double* dh_dfz, const double* d, int64_t ldd, int64_t r0, const double* ydiag,
                                            double* e, double* part, double* red, void* stream) {
  if (!shape_ok(K, M, C) || !dh_dx || !dh_dfz || !d || !ydiag || !e || !part || !red || r0 < (saa ? M + 1 : 0) ||
      ldd < r0 + M * C)
    return RATO_EINVAL;
  const int q = 5 * C + 2;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_reduce_kernel, dim3((unsigned)chunks_of(M), (unsigned)K), dim3(AR_BLOCK),
                     (size_t)AR_CHUNK * (q + 1) * sizeof(double), (hipStream_t)stream, K, M, C, saa ? 1 : 0, dh_dx, dh_dfz, d, ldd,
                     r0, ydiag, e, part);
  RATO_LAUNCH_CHECK();
  return sum_chunks(K, M, rato_hopper_arrow_npart(C), part, red, (hipStream_t)stream);
}

extern "C" int rato_hopper_arrow_assemble_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t nc, int64_t lda,
                                              const int32_t* qcol, const double* red, const double* d, int64_t ldd, int64_t r0,
                                              const double* malpha, double* Sh, void* stream) {
  if (!shape_ok(K, M, C) || nc < 5 * C + 2 || lda < nc || !qcol || !red || !d || !Sh || (saa && !malpha) ||
      r0 < (saa ? M + 1 : 0) || ldd < r0 + M * C)
    return RATO_EINVAL;
  const int q = 5 * C + 2, nent = q * (q + 1) / 2;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_assemble_kernel, dim3((unsigned)((nent + AR_BLOCK - 1) / AR_BLOCK), (unsigned)K), dim3(AR_BLOCK), 0,
                     (hipStream_t)stream, M, C, saa ? 1 : 0, nc, lda, qcol, red, d, ldd, r0, malpha, Sh);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_cols_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* dh_dx,
                                          const double* dh_dfz, const double* w, int64_t ldw, int64_t r0, const double* t,
                                          double* yout, double* part, double* red, void* stream) {
  if (!shape_ok(K, M, C) || (mode != 0 && mode != 1) || !dh_dx || !dh_dfz || !w || !part || !red || (mode == 1 && !t) ||
      r0 < (saa ? M + 1 : 0) || ldw < r0 + M * C)
    return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_cols_kernel, dim3((unsigned)chunks_of(M), (unsigned)K), dim3(AR_BLOCK), 0, (hipStream_t)stream, K, M, C,
                     saa ? 1 : 0, mode, dh_dx, dh_dfz, w, ldw, r0, t, yout, part);
  RATO_LAUNCH_CHECK();
  return sum_chunks(K, M, 5 * (int64_t)C + 1, part, red, (hipStream_t)stream);
}

extern "C" int rato_hopper_arrow_rows_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int32_t mode, const double* dh_dx,
                                          const double* dh_dfz, const double* xq, const double* xy, const double* d, int64_t ldd,
                                          int64_t r0, const double* addc, double* out, int64_t ldo, double* part, double* red,
                                          void* stream) {
  if (!shape_ok(K, M, C) || (mode != 0 && mode != 1) || !dh_dx || !dh_dfz || !xq || !out || r0 < (saa ? M + 1 : 0))
    return RATO_EINVAL;
  if (mode == 0 && (ldo < r0 + M * C || (saa && (!xy || !part || !red)))) return RATO_EINVAL;
  if (mode == 1 && (!d || !addc || ldd < r0 + M * C || ldo < M)) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_rows_kernel, dim3((unsigned)chunks_of(M), (unsigned)K), dim3(AR_BLOCK), 0, (hipStream_t)stream, K, M, C,
                     saa ? 1 : 0, mode, dh_dx, dh_dfz, xq, xy, d, ldd, r0, addc, out, ldo, part);
  RATO_LAUNCH_CHECK();
  if (mode == 0 && saa) return sum_chunks(K, M, 1, part, red, (hipStream_t)stream);
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_edot_f64(int32_t K, int64_t M, const double* e, const double* v, double* part, double* red,
                                          void* stream) {
  if (!shape_ok(K, M, 1) || !e || !v || !part || !red) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_edot_kernel, dim3((unsigned)chunks_of(M), (unsigned)K), dim3(AR_BLOCK), 0, (hipStream_t)stream, K, M, e,
                     v, part);
  RATO_LAUNCH_CHECK();
  return sum_chunks(K, M, 1, part, red, (hipStream_t)stream);
}

extern "C" int rato_hopper_arrow_eapply_f64(int32_t K, int64_t M, const double* e, const double* v, const double* kappa,
                                            double* out, void* stream) {
  if (!shape_ok(K, M, 1) || !e || !v || !kappa || !out) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_eapply_kernel, dim3((unsigned)((M + AR_BLOCK - 1) / AR_BLOCK), (unsigned)K), dim3(AR_BLOCK), 0,
                     (hipStream_t)stream, M, e, v, kappa, out);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_scale_f64(int32_t K, const double* a, const double* x, int64_t ldx, int64_t col, const double* add,
                                           double* out, int64_t ldo, int64_t ocol, void* stream) {
  if (K < 1 || K > 65535 || !a || !x || !out || col < 0 || col >= ldx || ocol < 0 || ocol >= ldo) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_scale_kernel, dim3((unsigned)((K + AR_BLOCK - 1) / AR_BLOCK)), dim3(AR_BLOCK), 0, (hipStream_t)stream, K, a,
                     x, ldx, col, add, out, ldo, ocol);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_tfix_f64(int32_t K, int64_t M, int32_t C, int32_t saa, int64_t n, const int32_t* qz,
                                          const double* red, int64_t ldr, const double* malpha, const double* w, int64_t ldw,
                                          int64_t rr, const double* yout, double* out, int64_t ldo, void* stream) {
  if (!shape_ok(K, M, C) || n < M + 2 || ldo < n || !qz || !red || ldr < 5 * (int64_t)C + 1 || !out) return RATO_EINVAL;
  if (saa && (!malpha || !w || !yout || rr < 0 || rr >= ldw)) return RATO_EINVAL;
  const int64_t work = max((int64_t)5 * C + 2, saa ? M : (int64_t)0);
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_tfix_kernel, dim3((unsigned)((work + AR_BLOCK - 1) / AR_BLOCK), (unsigned)K), dim3(AR_BLOCK), 0,
                     (hipStream_t)stream, M, C, saa ? 1 : 0, n, qz, red, ldr, malpha, w, ldw, rr, yout, out, ldo);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_kkbeta_f64(int32_t K, int32_t C, const double* d, int64_t ldd, int64_t rr, const double* red,
                                            int64_t ldr, const double* malpha, double* kk, double* beta, void* stream) {
  if (!shape_ok(K, 1, C) || !d || rr < 0 || rr >= ldd || !red || ldr < rato_hopper_arrow_npart(C) || !malpha || !kk || !beta)
    return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_kkbeta_kernel, dim3((unsigned)((K + AR_BLOCK - 1) / AR_BLOCK)), dim3(AR_BLOCK), 0, (hipStream_t)stream, K,
                     C, d, ldd, rr, red, ldr, malpha, kk, beta);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_einv_f64(int32_t K, int64_t M, const double* e, const double* v, int64_t ldv, const double* kk,
                                          const double* red, double* out, int64_t ldo, void* stream) {
  if (!shape_ok(K, M, 1) || !e || !v || ldv < M || (kk && !red) || !out || ldo < M) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_einv_kernel, dim3((unsigned)((M + AR_BLOCK - 1) / AR_BLOCK), (unsigned)K), dim3(AR_BLOCK), 0,
                     (hipStream_t)stream, M, e, v, ldv, kk, red, out, ldo);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_arrow_rhsfix_f64(int32_t K, int32_t C, int32_t nc, const int32_t* qcol, const double* red, int64_t ldr,
                                            const double* beta, double* rc, int64_t ldrc, void* stream) {
  if (!shape_ok(K, 1, C) || nc < 5 * C + 2 || !qcol || !red || ldr < 5 * (int64_t)C + 1 || !beta || !rc || ldrc < nc)
    return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(arrow_rhsfix_kernel, dim3((unsigned)K), dim3(AR_BLOCK), 0, (hipStream_t)stream, C, nc, qcol, red, ldr, beta, rc,
                     ldrc);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
