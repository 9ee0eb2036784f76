// The interior-point driver's O(n + m) algebra on a state that stays on the device (riskaversetrajopt_amd/ipm.py:
// DeviceState, solve_group_device), fp64, K problems per launch.  Nothing here knows a model: the objective
// is sf (1/2 sum curv z^2 + sum lin z), the constraints arrive as values (g, J'y, J dz, W dz, ...) that other kernels leave on
// the device.  lin enters the gradient (gradf, hence rz, dual, E0 and Dbar) and the two objective values (the record of the step
// setup, phi_t); the second-order places (diag, phase R, quad) know curv alone.
//
// Each kernel restates one piece of the host driver (ipm.Problem, ipm.newton_steps, ipm.solve_group) and nothing else:
//   ipm_residuals_kernel   Problem.residuals, error, the status and mu logic, prepare_step
//   ipm_newton_kernel      the vector algebra between the launches of newton_steps, by phase
//   ipm_setup_kernel       the step setup: dzl, dzu, fraction to the boundary, c1, Dbar, quad, the nu rule, Dphi, phi
//   ipm_trial_kernel       vt = v + alpha dv
//   ipm_accept_kernel      phi_t, the Armijo test, the accepted step with the kappa_Sigma clip -- or alpha / 2
//   ipm_g_rows_kernel      g = (g0, J1 z): the linear rows of g behind the non-linear ones
//
// One workgroup of 256 lanes per problem, grid = K.  Every loop is lane-strided over ascending indices.  A max is exact (NaN
// propagates as in np.max); a sum takes the per-lane partials in ascending order, rato::wave_sum_dpp's fixed tree, then the
// four waves in order through LDS.  No atomics, no scratch, no workspace: two calls are bitwise equal and problem k of a
// batch is bitwise its K = 1 call.  A problem whose status is not RATO_IPM_RUNNING leaves every kernel at once (the whole
// workgroup: the barriers below are never divergent), so what it holds stops changing.
//
// Python's max(a, b) / min(a, b) keep a unless b compares greater / less: with a NaN the result depends on the order.  The
// scalar combinations that decide a branch on the host (E_mu, dual, the step lengths) are restated with that rule (pymax /
// pymin), and the expressions of the nu rule and the Armijo test are rounded operation by operation as the host rounds them
// (__dmul_rn / __dadd_rn: the library is built with contraction on).
// The arithmetic itself -- the row formulas, the accumulate expressions, the scalar epilogues -- is csrc/rato_ipm_rows.h, which
// the grid form (csrc/ipm_driver_grid.hip) compiles too: the kernels below are the loops, the reductions and the barriers.
#include "rato_ipm_rows.h"

namespace {

using namespace rato_ipm;

// comp(mu) of Problem.error: max |zl dL - mu| over the lower bounds, max |zu dU - mu| over the upper ones
__device__ __forceinline__ double complementarity(const rato_ipm_state& st, const View& w, double mu, double (*sh)[ID_WAVES]) {
  double mx[2] = {-INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < w.nv; i += ID_BLOCK) {
    const Dist b = dist(st.v[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
    if (b.hasL) mx[0] = nanmax(mx[0], comp_term(st.zl[w.ov + i], b.dL, mu));
    if (b.hasU) mx[1] = nanmax(mx[1], comp_term(st.zu[w.ov + i], b.dU, mu));
  }
  block_extreme<0>(mx, sh);
  return pymax(pymax(0.0, mx[0]), mx[1]);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_residuals_kernel(rato_ipm_state st, const double* __restrict__ g, int64_t ldg,
                                                                 const double* __restrict__ JTy, int64_t ldj, int last) {
  __shared__ double sh[3][ID_WAVES];
  const View w = view(st, blockIdx.x);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double sf = w.rec[RATO_IPM_SF], tol = w.rec[RATO_IPM_TOL];
  double mu = w.rec[RATO_IPM_MU], nu = w.rec[RATO_IPM_NU];
  const double* gk = g + (int64_t)blockIdx.x * ldg;
  const double* jk = JTy + (int64_t)blockIdx.x * ldj;
  double mx[3] = {-INFINITY, -INFINITY, -INFINITY};             // |c|, |rs|, |rz|
  for (int r = t; r < w.m; r += ID_BLOCK) residual_m_row(st, w, gk, r, mx);
  for (int j = t; j < n; j += ID_BLOCK) residual_z_row(st, w, jk, sf, j, mx);
  block_extreme<0>(mx, sh);
  const double prim = mx[0], dual = pymax(mx[2], st.nI > 0 ? mx[1] : 0.0);
  const double E0 = pymax(pymax(dual, prim), complementarity(st, w, 0.0, sh));
  const int status = residual_status(E0, tol, last);
  int passes = 0;
  if (status != RATO_IPM_RUNNING) {
    if (t == 0) residual_write_ended(w.rec, E0, prim, dual, status);
    return;
  }
  // the whole workgroup takes each pass
  mu_loop(mu, nu, passes, tol, dual, prim, [&](double m_) { return complementarity(st, w, m_, sh); });
  const double dc = dc_of(mu);
  for (int i = t; i < w.nv; i += ID_BLOCK) prepare_v_row(st, w, jk, mu, sf, i);    // gradf[i]: this lane's own store above
  for (int r = t; r < w.m; r += ID_BLOCK) prepare_m_row(st, w, dc, mu, r);        // c[r]: this lane's own store above
  if (t == 0) residual_write_running(w.rec, E0, prim, dual, mu, nu, dc, passes);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_newton_kernel(rato_ipm_state st, int phase, const double* __restrict__ a,
                                                              int64_t lda, const double* __restrict__ b, int64_t ldb,
                                                              const int32_t* __restrict__ info, int flag) {
  const View w = view(st, blockIdx.x);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double* ak = a ? a + (int64_t)blockIdx.x * lda : nullptr;
  const double* bk = b ? b + (int64_t)blockIdx.x * ldb : nullptr;
  const double dc = w.rec[RATO_IPM_DC], sf = w.rec[RATO_IPM_SF];
  double dw = w.rec[RATO_IPM_DW];
  switch (phase) {
    case RATO_IPM_PHASE_RHS:
      for (int j = t; j < n; j += ID_BLOCK) newton_rhs_row(st, w, ak, j);
      break;
    case RATO_IPM_PHASE_LADDER: {
      if (info[blockIdx.x] == 0) return;
      __syncthreads();                                           // every lane holds dw before lane 0 replaces it
      if (flag >= 60) {
        if (t == 0) w.rec[RATO_IPM_STATUS] = 2.0;
        return;
      }
      dw = ladder_dw(dw);
      for (int j = t; j < n; j += ID_BLOCK) newton_ladder_row(st, w, dw, sf, j);
      if (t == 0) w.rec[RATO_IPM_DW] = dw;
      break;
    }
    case RATO_IPM_PHASE_Q:
      for (int r = t; r < w.m; r += ID_BLOCK) newton_q_row(st, w, ak, dc, flag, r);
      break;
    case RATO_IPM_PHASE_R:
      for (int j = t; j < n; j += ID_BLOCK) newton_r_row(st, w, ak, bk, sf, dw, j);
      break;
    case RATO_IPM_PHASE_UPDATE:
      for (int j = t; j < n; j += ID_BLOCK) newton_update_z_row(st, w, j);
      for (int r = t; r < w.m; r += ID_BLOCK) newton_update_m_row(st, w, ak, dc, r);
      break;
    default:                                                     // RATO_IPM_PHASE_FINISH
      for (int j = t; j < n; j += ID_BLOCK) newton_finish_z_row(st, w, j);
      for (int r = t; r < w.m; r += ID_BLOCK) newton_finish_m_row(st, w, ak, r);
  }
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_setup_kernel(rato_ipm_state st, const double* __restrict__ Hdv, int64_t ldh) {
  __shared__ double sh[SETUP_SUMS][ID_WAVES];
  const View w = view(st, blockIdx.x);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double mu = w.rec[RATO_IPM_MU], dw = w.rec[RATO_IPM_DW], sf = w.rec[RATO_IPM_SF];
  const double nu = w.rec[RATO_IPM_NU];
  const double tau = pymax(0.99, 1.0 - mu);
  const double* hk = Hdv + (int64_t)blockIdx.x * ldh;
  double s[SETUP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mn[2] = {INFINITY, INFINITY};                           // the primal and the dual step to the boundary
  for (int i = t; i < w.nv; i += ID_BLOCK) {
    const double vi = st.v[w.ov + i], dvi = st.dv[w.ov + i];
    const Dist b = setup_row(st, w, mu, tau, i, vi, dvi, mn);
    acc_dot(s[1], st.gbar[w.ov + i], dvi);
    acc_sigma(s[3], st.Sigma[w.ov + i], dvi);
    acc_log(s[5], b.hasL, b.dL);
    acc_log(s[6], b.hasU, b.dU);
    if (i < n) {
      const double cv = st.curv[w.ov + i];
      acc_dot(s[0], st.gradf[w.ov + i], dvi);
      acc_hess(s[2], dvi, hk[i], sf, cv);
      acc_square(s[4], dvi);
      acc_curv(s[7], cv, vi);
      acc_dot(s[9], st.lin[w.ov + i], vi);
    }
  }
  for (int r = t; r < w.m; r += ID_BLOCK) acc_abs(s[8], st.c[w.om + r]);
  block_sum(s, sh);
  block_extreme<1>(mn, sh);
  const SetupScalars o = setup_scalars(s, mn, mu, dw, sf, nu);
  if (t == 0) setup_write(w.rec, o);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_trial_kernel(rato_ipm_state st) {
  const View w = view(st, blockIdx.x);
  if (!searching(w.rec)) return;
  const double alpha = w.rec[RATO_IPM_ALPHA];
  for (int i = threadIdx.x; i < w.nv; i += ID_BLOCK) trial_row(st, w, alpha, i);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_accept_kernel(rato_ipm_state st, const double* __restrict__ gt, int64_t ldg) {
  __shared__ double sh[ACCEPT_SUMS][ID_WAVES];
  const View w = view(st, blockIdx.x);
  if (!searching(w.rec)) return;
  const int t = threadIdx.x, n = w.n;
  const AcceptIn in = accept_in(w.rec);
  const double* gk = gt + (int64_t)blockIdx.x * ldg;
  double s[ACCEPT_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};             // the two barrier sums, sum curv z^2, sum |c|, sum lin z
  for (int i = t; i < w.nv; i += ID_BLOCK) {
    const double vi = st.vt[w.ov + i];
    const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
    acc_log(s[0], b.hasL, b.dL);
    acc_log(s[1], b.hasU, b.dU);
    if (i < n) {
      acc_curv(s[2], st.curv[w.ov + i], vi);
      acc_dot(s[4], st.lin[w.ov + i], vi);
    }
  }
  for (int r = t; r < w.m; r += ID_BLOCK) acc_abs(s[3], trial_c(st, w, gk, r));
  block_sum(s, sh);
  bool accept;
  const double phi_t = accept_scalars(s, in, &accept);
  if (accept) {
    for (int i = t; i < w.nv; i += ID_BLOCK) accept_v_row(st, w, in.mu, in.a_dual, i);
    for (int r = t; r < w.m; r += ID_BLOCK) accept_m_row(st, w, in.alpha, r);
  }
  if (t == 0) accept_write(w.rec, in, phi_t, accept);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_g_rows_kernel(int32_t n, const double* __restrict__ g0, int32_t m0, int64_t ldg0,
                                                              const double* __restrict__ J1, int32_t m1, int64_t ld1,
                                                              const double* __restrict__ z, int64_t ldz, double* __restrict__ g,
                                                              int64_t ldg) {
  __shared__ double sh[1][ID_WAVES];
  const int t = threadIdx.x;
  const double* zk = z + (int64_t)blockIdx.x * ldz;
  double* gk = g + (int64_t)blockIdx.x * ldg;
  for (int r = t; r < m0; r += ID_BLOCK) gk[r] = g0[(int64_t)blockIdx.x * ldg0 + r];
  for (int r = 0; r < m1; ++r) {
    double s[1] = {0.0};
    for (int c = t; c < n; c += ID_BLOCK) s[0] += J1[(int64_t)r * ld1 + c] * zk[c];
    block_sum(s, sh);
    if (t == 0) gk[m0 + r] = s[0];
  }
}

}  // namespace

extern "C" size_t rato_ipm_state_bytes(void) { return sizeof(rato_ipm_state); }

extern "C" int rato_ipm_g_rows_f64(int32_t K, int32_t n, const double* g0, int32_t m0, int64_t ldg0, const double* J1, int32_t m1,
                                   int64_t ld1, const double* z, int64_t ldz, double* g, int64_t ldg, void* stream) {
  if (K < 1 || K > 65535 || n < 1 || m0 < 0 || m1 < 0 || m0 + (int64_t)m1 < 1 || (m0 > 0 && (!g0 || ldg0 < m0)) ||
      (m1 > 0 && (!J1 || ld1 < n)) || !z || ldz < n || !g || ldg < (int64_t)m0 + m1)
    return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_g_rows_kernel, dim3((unsigned)K), dim3(ID_BLOCK), 0, (hipStream_t)stream, n, g0, m0, ldg0, J1, m1, ld1, z,
                     ldz, g, ldg);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_residuals_f64(const rato_ipm_state* st, const double* g, int64_t ldg, const double* JTy, int64_t ldj,
                                      int32_t last, void* stream) {
  if (!state_ok(st) || !g || !JTy || ldg < st->m || ldj < st->n) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_residuals_kernel, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st, g, ldg, JTy, ldj,
                     (int)last);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_newton_f64(const rato_ipm_state* st, int32_t phase, const double* a, int64_t lda, const double* b,
                                   int64_t ldb, const int32_t* info, int32_t flag, void* stream) {
  if (!state_ok(st) || !newton_args_ok(st, phase, a, lda, b, ldb, info, flag)) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_newton_kernel, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st, (int)phase, a, lda, b,
                     ldb, info, (int)flag);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_step_setup_f64(const rato_ipm_state* st, const double* Hdv, int64_t ldh, void* stream) {
  if (!state_ok(st) || !Hdv || ldh < st->n) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_setup_kernel, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st, Hdv, ldh);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_trial_f64(const rato_ipm_state* st, void* stream) {
  if (!state_ok(st)) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_trial_kernel, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_accept_f64(const rato_ipm_state* st, const double* gt, int64_t ldg, void* stream) {
  if (!state_ok(st) || !gt || ldg < st->m) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(ipm_accept_kernel, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st, gt, ldg);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
