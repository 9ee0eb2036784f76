// Hopper slip rows in fp64 for K problems per call (hopper/hopper.py:68-81, :300-367, :569-580): h_ic = fx_c - mu_i(p_c) fz_c,
// its first derivatives with the end-effector chain applied, the per-sample maximum, and the three lambda-weighted sample
// sums per contact that hess(lam . g) needs -- computed from Z on the device.  The fp32 kernel of hopper.hip stays the
// Monte-Carlo / large-M throughput path; this one is what an NLP solver's callbacks read.  The per-lane arithmetic is in
// rato_hopper_slip64.h (shared with the host program of tests/host/).
//
// Launch shape of the slip kernel.  A workgroup of 256 lanes is a tile of TI samples x TC = 256 / TI contacts, TI the smallest
// power of two >= M (at most 256).  grid = (sample tiles, contact groups, K).  At the reference's size (M = 30, 20 contacts)
// a wave holds 2 contacts x 32 sample lanes, 60 of 64 busy, and the 20 contacts spread over 3 workgroups per problem; at
// M >= 256 a workgroup is 256 samples of one contact.  When the per-sample maximum is asked for, grid.y is 1 and the
// workgroup walks the contact groups itself (the maximum over contacts then needs no second pass).
//
// Sums.  Each workgroup reduces its lanes' terms over the samples of a contact row with a fixed-order tree in LDS and writes
// one partial per (sample tile, problem, contact): part[nblk][K][C][3].  rato_sum_partials_f64 adds the tiles in a fixed order.
// No atomics: two calls are bitwise equal, and column (k, c) of a K-problem call sees the additions of the K = 1 call.
//
// Fields.  rato_hopper_slip_f64 reads one a / theta / tau [30][M] for the K problems; rato_hopper_slip_f64_fields takes ldf, the
// doubles between the fields of problem k and k + 1 (0: shared).  The offset k ldf is applied in rato_slip64_run_lane, so the
// launch shape and the order of every sum are those of the shared call, and row k is bitwise the K = 1 call on its own fields.
#include "rato_common.h"
#include "rato_hopper_slip64.h"

namespace {

constexpr int HS_BLOCK = RATO_S64_BLOCK;

using Phases = rato_slip64_phases;

__global__ void __launch_bounds__(HS_BLOCK)
hopper_slip64_kernel(const rato_slip64_args A, double* __restrict__ Zmax, double* __restrict__ part) {
  __shared__ double red[3][HS_BLOCK];
  const int tid = threadIdx.x;
  const int ti = 1 << A.log2ti, mask = ti - 1, tc = HS_BLOCK >> A.log2ti;
  const int li = tid & mask, lc = tid >> A.log2ti;
  const int64_t i = (int64_t)blockIdx.x * ti + li;
  const int64_t k = blockIdx.z, K = gridDim.z;
  const int C = A.P.C;
  const int ncg = (C + tc - 1) / tc;
  double zmax = -INFINITY;
  for (int cg = blockIdx.y; cg < ncg; cg += gridDim.y) {   // uniform over the workgroup
    const int c = cg * tc + lc;
    double t[3];
    rato_slip64_run_lane(A, k, i, c, t, zmax);
    if (part) {                                            // a kernel argument: uniform
      red[0][tid] = t[0];
      red[1][tid] = t[1];
      red[2][tid] = t[2];
      __syncthreads();
      for (int half = ti >> 1; half > 0; half >>= 1) {
        rato_slip64_tree_step(red[0], tid, mask, half);
        rato_slip64_tree_step(red[1], tid, mask, half);
        rato_slip64_tree_step(red[2], tid, mask, half);
        __syncthreads();
      }
      if (li == 0 && c < C) {
        double* o = part + (((int64_t)blockIdx.x * K + k) * C + c) * 3;
        o[0] = red[0][tid];
        o[1] = red[1][tid];
        o[2] = red[2][tid];
      }
      __syncthreads();                                     // red is rewritten by the next contact group
    }
  }
  if (Zmax) {                                              // grid.y == 1: this workgroup saw every contact of its samples
    red[0][tid] = zmax;
    __syncthreads();
    for (int half = tc >> 1; half > 0; half >>= 1) {
      if (lc < half) red[0][tid] = fmax(red[0][tid], red[0][tid + half * ti]);
      __syncthreads();
    }
    if (lc == 0 && i < A.M) Zmax[k * A.M + i] = red[0][tid];
  }
}

// one lane per (problem, contact, entry): add[k][t_c][pos] += the contact's share; contacts sit on distinct steps
__global__ void __launch_bounds__(HS_BLOCK)
hopper_slip64_hess_kernel(const Phases P, const int64_t n_lanes, const double* __restrict__ Z, const int64_t ldz,
                          const double* __restrict__ D, double* __restrict__ add) {
  const int64_t idx = (int64_t)blockIdx.x * HS_BLOCK + threadIdx.x;
  if (idx >= n_lanes) return;              // no barrier below
  rato_slip64_hess_lane(P, idx, Z, ldz, D, add);
}

bool valid(const rato_hopper_nlp_params* p, int32_t K, int64_t ldz, Phases* P) {
  if (!p || K < 1 || K > 65535 || p->S < 1) return false;
  if (p->time_jump < 0 || p->time_jump > p->time_land || p->time_land > p->S) return false;
  if (ldz < (int64_t)RATO_S64_NX * (p->S + 1) + (int64_t)RATO_S64_NU * p->S) return false;
  *P = {p->S, p->time_jump, p->time_land, p->time_jump + (p->S - p->time_land)};
  return true;
}

}  // namespace

extern "C" int rato_hopper_slip_f64_nblocks(int32_t M) { return M < 1 ? 0 : (int)rato_slip64_nblocks(M); }

extern "C" int rato_hopper_slip_f64_fields(const rato_hopper_nlp_params* p, double mu_nom, int32_t K, int32_t M, const double* Z,
                                           int64_t ldz, const double* a, const double* theta, const double* tau, int64_t ldf,
                                           const double* lam, int64_t ldlam, int64_t lam_r0, double* h, double* dh_dfz,
                                           double* dh_dx, double* Zmax, double* part, double* D, void* stream) {
  Phases P;
  if (!valid(p, K, ldz, &P) || M < 1 || !Z || !a || !theta || !tau) return RATO_EINVAL;
  if (ldf != 0 && ldf < (int64_t)RATO_S64_NFEAT * M) return RATO_EINVAL;   // 0: one set of fields for the K problems
  if (P.C == 0) return RATO_OK;            // no contact step: nothing to write (the outputs are empty)
  const int64_t ncols = (int64_t)K * P.C * 3;
  if (lam && (!part || !D || lam_r0 < 0 || ldlam < lam_r0 + (int64_t)M * P.C || ncols > 0x7fffffff)) return RATO_EINVAL;
  if (!lam && !h && !dh_dfz && !dh_dx && !Zmax) return RATO_OK;
  const int log2ti = rato_slip64_log2_ti(M);
  const int64_t nblk = rato_slip64_nblocks(M);
  const int tc = HS_BLOCK >> log2ti;
  const int ncg = (P.C + tc - 1) / tc;
  const unsigned gy = Zmax ? 1u : (unsigned)(ncg < 65535 ? ncg : 65535);
  RATO_CLEAR_ERROR();
  const rato_slip64_args A = {P, mu_nom, (int64_t)M, log2ti, Z, ldz, a, theta, tau, lam, ldlam, lam_r0, h, dh_dfz, dh_dx, ldf};
  hipLaunchKernelGGL(hopper_slip64_kernel, dim3((unsigned)nblk, gy, (unsigned)K), dim3(HS_BLOCK), 0, (hipStream_t)stream, A,
                     Zmax, lam ? part : nullptr);
  RATO_LAUNCH_CHECK();
  if (lam) return rato_sum_partials_f64(part, (int32_t)nblk, (int32_t)ncols, 1.0, D, stream);
  return RATO_OK;
}

extern "C" int rato_hopper_slip_f64(const rato_hopper_nlp_params* p, double mu_nom, int32_t K, int32_t M, const double* Z,
                                    int64_t ldz, const double* a, const double* theta, const double* tau, const double* lam,
                                    int64_t ldlam, int64_t lam_r0, double* h, double* dh_dfz, double* dh_dx, double* Zmax,
                                    double* part, double* D, void* stream) {
  return rato_hopper_slip_f64_fields(p, mu_nom, K, M, Z, ldz, a, theta, tau, 0, lam, ldlam, lam_r0, h, dh_dfz, dh_dx, Zmax, part,
                                     D, stream);
}

extern "C" int rato_hopper_slip_hess_blocks_f64(const rato_hopper_nlp_params* p, int32_t K, const double* Z, int64_t ldz,
                                                const double* D, double* add, void* stream) {
  Phases P;
  if (!valid(p, K, ldz, &P) || !Z || !add) return RATO_EINVAL;
  if (P.C == 0) return RATO_OK;            // D is empty
  if (!D) return RATO_EINVAL;
  const int64_t n = (int64_t)K * P.C * RATO_S64_ENTRIES;
  const int64_t nb = (n + HS_BLOCK - 1) / HS_BLOCK;
  if (nb > 0x7fffffff) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(hopper_slip64_hess_kernel, dim3((unsigned)nb), dim3(HS_BLOCK), 0, (hipStream_t)stream, P, n, Z, ldz, D,
                     add);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
