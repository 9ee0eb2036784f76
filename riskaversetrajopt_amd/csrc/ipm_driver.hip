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
#include "rato_common.h"

#include <math.h>

namespace {

constexpr int ID_BLOCK = 256;
constexpr int ID_WAVES = ID_BLOCK / RATO_WAVE;
static_assert(ID_WAVES == 4, "the block reductions combine four waves");

__device__ __forceinline__ double nanmax(double a, double b) { return (a != a || b != b) ? (double)NAN : fmax(a, b); }
__device__ __forceinline__ double pymax(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double pymin(double a, double b) { return b < a ? b : a; }

template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*sh)[ID_WAVES]) {
  const int lane = threadIdx.x & (RATO_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double s = rato::wave_sum_dpp(v[i]);
    if (lane == 0) sh[i][wave] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((sh[i][0] + sh[i][1]) + sh[i][2]) + sh[i][3];
  __syncthreads();
}

// MODE 0: the maximum, NaN if any entry is NaN; MODE 1: the minimum, NaNs dropped
template <int MODE, int N>
__device__ __forceinline__ void block_extreme(double (&v)[N], double (*sh)[ID_WAVES]) {
  const int lane = threadIdx.x & (RATO_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = v[i];
#pragma unroll
    for (int off = RATO_WAVE / 2; off > 0; off >>= 1) {
      const double o = __shfl_xor(x, off, RATO_WAVE);
      x = MODE == 0 ? nanmax(x, o) : fmin(x, o);
    }
    if (lane == 0) sh[i][wave] = x;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = sh[i][0];
#pragma unroll
    for (int w = 1; w < ID_WAVES; ++w) x = MODE == 0 ? nanmax(x, sh[i][w]) : fmin(x, sh[i][w]);
    v[i] = x;
  }
  __syncthreads();
}

// distances to the bounds and their reciprocals: 1 / where(has, d, inf)
struct Dist {
  bool hasL, hasU;
  double dL, dU, iL, iU;
};
__device__ __forceinline__ Dist dist(double v, double vL, double vU) {
  Dist b;
  b.hasL = isfinite(vL);
  b.hasU = isfinite(vU);
  b.dL = v - vL;
  b.dU = vU - v;
  b.iL = b.hasL ? 1.0 / b.dL : 0.0;
  b.iU = b.hasU ? 1.0 / b.dU : 0.0;
  return b;
}

struct View {   // problem k's rows
  int n, nv, m;
  double* rec;
  int64_t ov, om;
};
__device__ __forceinline__ View view(const rato_ipm_state& st) {
  View w;
  w.n = st.n;
  w.nv = st.n + st.nI;
  w.m = st.m;
  w.rec = st.rec + (int64_t)blockIdx.x * RATO_IPM_REC;
  w.ov = (int64_t)blockIdx.x * st.ldv;
  w.om = (int64_t)blockIdx.x * st.ldm;
  return w;
}

// comp(mu) of Problem.error: max |zl dL - mu| over the lower bounds, max |zu dU - mu| over the upper ones
__device__ __forceinline__ double complementarity(const rato_ipm_state& st, const View& w, double mu, double (*sh)[ID_WAVES]) {
  double mx[2] = {-INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < w.nv; i += ID_BLOCK) {
    const Dist b = dist(st.v[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
    if (b.hasL) mx[0] = nanmax(mx[0], fabs(__dmul_rn(st.zl[w.ov + i], b.dL) - mu));
    if (b.hasU) mx[1] = nanmax(mx[1], fabs(__dmul_rn(st.zu[w.ov + i], b.dU) - mu));
  }
  block_extreme<0>(mx, sh);
  return pymax(pymax(0.0, mx[0]), mx[1]);
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_residuals_kernel(rato_ipm_state st, const double* __restrict__ g, int64_t ldg,
                                                                 const double* __restrict__ JTy, int64_t ldj, int last) {
  __shared__ double sh[3][ID_WAVES];
  const View w = view(st);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double sf = w.rec[RATO_IPM_SF], tol = w.rec[RATO_IPM_TOL];
  double mu = w.rec[RATO_IPM_MU], nu = w.rec[RATO_IPM_NU];
  const double* gk = g + (int64_t)blockIdx.x * ldg;
  const double* jk = JTy + (int64_t)blockIdx.x * ldj;
  double mx[3] = {-INFINITY, -INFINITY, -INFINITY};             // |c|, |rs|, |rz|
  for (int r = t; r < w.m; r += ID_BLOCK) {
    const int sl = st.row_slack[r];
    double cr;
    if (sl < 0) {
      cr = gk[r] - st.gL[w.om + r];
    } else {
      const int64_t i = w.ov + n + sl;
      cr = gk[r] - st.v[i];
      mx[1] = nanmax(mx[1], fabs(-st.y[w.om + r] - st.zl[i] + st.zu[i]));
    }
    st.c[w.om + r] = cr;
    mx[0] = nanmax(mx[0], fabs(cr));
  }
  for (int j = t; j < n; j += ID_BLOCK) {
    const double gf = sf * (st.curv[w.ov + j] * st.v[w.ov + j] + st.lin[w.ov + j]);
    st.gradf[w.ov + j] = gf;
    mx[2] = nanmax(mx[2], fabs(gf + jk[j] - st.zl[w.ov + j] + st.zu[w.ov + j]));
  }
  block_extreme<0>(mx, sh);
  const double prim = mx[0], dual = pymax(mx[2], st.nI > 0 ? mx[1] : 0.0);
  const double E0 = pymax(pymax(dual, prim), complementarity(st, w, 0.0, sh));
  int status = RATO_IPM_RUNNING, passes = 0;
  if (!isfinite(E0)) status = 2;
  else if (E0 <= tol) status = 0;
  else if (last) status = 1;
  if (status != RATO_IPM_RUNNING) {
    if (t == 0) {
      w.rec[RATO_IPM_E0] = E0;
      w.rec[RATO_IPM_PRIM] = prim;
      w.rec[RATO_IPM_DUAL] = dual;
      w.rec[RATO_IPM_STATUS] = (double)status;
    }
    return;
  }
  const double floor_mu = tol / 10.0;
  while (mu > floor_mu) {                                        // the whole workgroup takes each pass
    const double Emu = pymax(pymax(dual, prim), complementarity(st, w, mu, sh));
    if (!(Emu <= 10.0 * mu)) break;
    mu = pymax(floor_mu, pymin(0.2 * mu, __dmul_rn(mu, sqrt(mu))));
    nu = 0.0;
    ++passes;
  }
  const double dc = 1e-8 * sqrt(sqrt(mu));
  for (int i = t; i < w.nv; i += ID_BLOCK) {
    const Dist b = dist(st.v[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
    const double Sig = st.zl[w.ov + i] * b.iL + st.zu[w.ov + i] * b.iU, gb = -mu * b.iL + mu * b.iU;
    st.Sigma[w.ov + i] = Sig;
    st.gbar[w.ov + i] = gb;
    if (i < n) {
      st.rz[w.ov + i] = st.gradf[w.ov + i] + jk[i] + gb;         // gradf[i]: this lane's own store above
      st.diag[(int64_t)blockIdx.x * n + i] = (Sig + 0.0) + sf * st.curv[w.ov + i];
    }
  }
  for (int r = t; r < w.m; r += ID_BLOCK) {
    const int sl = st.row_slack[r];
    const double cr = st.c[w.om + r];                            // this lane's own store above
    if (sl < 0) {
      const double d = 1.0 / dc;
      st.d[w.om + r] = d;
      st.w[w.om + r] = d * cr;
    } else {
      const int64_t i = w.ov + n + sl;                           // Sigma and gbar of the slack again: no wait for their owner
      const Dist b = dist(st.v[i], st.vL[i], st.vU[i]);
      const double Sig = st.zl[i] * b.iL + st.zu[i] * b.iU, gb = -mu * b.iL + mu * b.iU;
      const double rs = -st.y[w.om + r] + gb;
      st.rs[w.om + r] = rs;
      st.d[w.om + r] = Sig;
      st.w[w.om + r] = Sig * cr + rs;
    }
  }
  if (t == 0) {
    w.rec[RATO_IPM_E0] = E0;
    w.rec[RATO_IPM_PRIM] = prim;
    w.rec[RATO_IPM_DUAL] = dual;
    w.rec[RATO_IPM_MU] = mu;
    w.rec[RATO_IPM_NU] = nu;
    w.rec[RATO_IPM_DW] = 0.0;
    w.rec[RATO_IPM_DC] = dc;
    w.rec[RATO_IPM_MU_PASSES] = (double)passes;
    w.rec[RATO_IPM_SEARCHING] = 0.0;
  }
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_newton_kernel(rato_ipm_state st, int phase, const double* __restrict__ a,
                                                              int64_t lda, const double* __restrict__ b, int64_t ldb,
                                                              const int32_t* __restrict__ info, int flag) {
  const View w = view(st);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double* ak = a ? a + (int64_t)blockIdx.x * lda : nullptr;
  const double* bk = b ? b + (int64_t)blockIdx.x * ldb : nullptr;
  const double dc = w.rec[RATO_IPM_DC], sf = w.rec[RATO_IPM_SF];
  double dw = w.rec[RATO_IPM_DW];
  switch (phase) {
    case RATO_IPM_PHASE_RHS:
      for (int j = t; j < n; j += ID_BLOCK) st.dz[w.ov + j] = -(st.rz[w.ov + j] + ak[j]);
      break;
    case RATO_IPM_PHASE_LADDER: {
      if (info[blockIdx.x] == 0) return;
      __syncthreads();                                           // every lane holds dw before lane 0 replaces it
      if (flag >= 60) {
        if (t == 0) w.rec[RATO_IPM_STATUS] = 2.0;
        return;
      }
      dw = dw == 0.0 ? 1e-4 : 8.0 * dw;
      for (int j = t; j < n; j += ID_BLOCK)
        st.diag[(int64_t)blockIdx.x * n + j] = (st.Sigma[w.ov + j] + dw) + sf * st.curv[w.ov + j];
      if (t == 0) w.rec[RATO_IPM_DW] = dw;
      break;
    }
    case RATO_IPM_PHASE_Q:
      for (int r = t; r < w.m; r += ID_BLOCK) {
        const int sl = st.row_slack[r];
        const double lin = ak[r] + st.c[w.om + r];
        if (sl < 0) {
          double dyE = st.dyE[w.om + r];
          if (flag) st.dyE[w.om + r] = dyE = lin / dc;
          const double r2 = -lin + dc * dyE;
          st.r2[w.om + r] = r2;
          st.q[w.om + r] = dyE - r2 / dc;
        } else {
          st.q[w.om + r] = st.Sigma[w.ov + n + sl] * lin + st.rs[w.om + r];
        }
      }
      break;
    case RATO_IPM_PHASE_R:
      for (int j = t; j < n; j += ID_BLOCK) {
        const double x = st.dz[w.ov + j], h = ak[j] + (sf * st.curv[w.ov + j]) * x;
        st.ez[w.ov + j] = -(st.rz[w.ov + j] + h + (st.Sigma[w.ov + j] + dw) * x + bk[j]);
      }
      break;
    case RATO_IPM_PHASE_UPDATE:
      for (int j = t; j < n; j += ID_BLOCK) st.dz[w.ov + j] += st.ez[w.ov + j];
      for (int r = t; r < w.m; r += ID_BLOCK)
        if (st.row_slack[r] < 0) st.dyE[w.om + r] += (ak[r] - st.r2[w.om + r]) / dc;
      break;
    default:                                                     // RATO_IPM_PHASE_FINISH
      for (int j = t; j < n; j += ID_BLOCK) st.dv[w.ov + j] = st.dz[w.ov + j];
      for (int r = t; r < w.m; r += ID_BLOCK) {
        const int sl = st.row_slack[r];
        if (sl < 0) {
          st.dy[w.om + r] = st.dyE[w.om + r];
        } else {
          const double ds = ak[r] + st.c[w.om + r];
          st.dv[w.ov + n + sl] = ds;
          st.dy[w.om + r] = st.Sigma[w.ov + n + sl] * ds + st.rs[w.om + r];
        }
      }
  }
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_setup_kernel(rato_ipm_state st, const double* __restrict__ Hdv, int64_t ldh) {
  __shared__ double sh[10][ID_WAVES];
  const View w = view(st);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int t = threadIdx.x, n = w.n;
  const double mu = w.rec[RATO_IPM_MU], dw = w.rec[RATO_IPM_DW], sf = w.rec[RATO_IPM_SF];
  double nu = w.rec[RATO_IPM_NU];
  const double tau = pymax(0.99, 1.0 - mu);
  const double* hk = Hdv + (int64_t)blockIdx.x * ldh;
  // sums: gradf . dv_z, gbar . dv, dv_z . W dv_z, sum Sigma dv^2, dv_z . dv_z, the two barrier sums, sum curv z^2, sum |c|,
  // sum lin z
  double s[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mn[2] = {INFINITY, INFINITY};                           // the primal and the dual step to the boundary
  for (int i = t; i < w.nv; i += ID_BLOCK) {
    const double vi = st.v[w.ov + i], dvi = st.dv[w.ov + i], zl = st.zl[w.ov + i], zu = st.zu[w.ov + i];
    const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
    const double dzl = b.hasL ? mu * b.iL - zl - zl * b.iL * dvi : 0.0;
    const double dzu = b.hasU ? mu * b.iU - zu + zu * b.iU * dvi : 0.0;
    st.dzl[w.ov + i] = dzl;
    st.dzu[w.ov + i] = dzu;
    if (b.hasL && dvi < 0.0) mn[0] = fmin(mn[0], -tau * b.dL / dvi);
    if (b.hasU && -dvi < 0.0) mn[0] = fmin(mn[0], -tau * b.dU / -dvi);
    if (b.hasL && dzl < 0.0) mn[1] = fmin(mn[1], -tau * zl / dzl);
    if (b.hasU && dzu < 0.0) mn[1] = fmin(mn[1], -tau * zu / dzu);
    s[1] += st.gbar[w.ov + i] * dvi;
    s[3] += st.Sigma[w.ov + i] * dvi * dvi;
    if (b.hasL) s[5] += log(b.dL);
    if (b.hasU) s[6] += log(b.dU);
    if (i < n) {
      const double cv = st.curv[w.ov + i];
      s[0] += st.gradf[w.ov + i] * dvi;
      s[2] += dvi * (hk[i] + (sf * cv) * dvi);
      s[4] += dvi * dvi;
      s[7] += cv * vi * vi;
      s[9] += st.lin[w.ov + i] * vi;
    }
  }
  for (int r = t; r < w.m; r += ID_BLOCK) s[8] += fabs(st.c[w.om + r]);
  block_sum(s, sh);
  block_extreme<1>(mn, sh);
  const double a_max = fmin(1.0, mn[0]), a_dual = fmin(1.0, mn[1]);
  const double c1 = s[8], Dbar = s[0] + s[1], quad = __dadd_rn(__dadd_rn(s[2], s[3]), __dmul_rn(dw, s[4]));
  if (c1 > 0.0) {
    const double nu_trial = __dadd_rn(Dbar, __dmul_rn(0.5, pymax(quad, 0.0))) / __dmul_rn(0.9, c1);
    if (nu < nu_trial) nu = __dadd_rn(nu_trial, 1.0);
  }
  const double Dphi = pymin(__dadd_rn(Dbar, -__dmul_rn(nu, c1)), 0.0);
  const double objective = 0.5 * s[7] + s[9], barrier = -mu * (s[5] + s[6]);
  const double phi = __dadd_rn(__dadd_rn(__dmul_rn(sf, objective), barrier), __dmul_rn(nu, c1));
  if (t == 0) {
    w.rec[RATO_IPM_A_MAX] = a_max;
    w.rec[RATO_IPM_A_DUAL] = a_dual;
    w.rec[RATO_IPM_C1] = c1;
    w.rec[RATO_IPM_DBAR] = Dbar;
    w.rec[RATO_IPM_QUAD] = quad;
    w.rec[RATO_IPM_NU] = nu;
    w.rec[RATO_IPM_DPHI] = Dphi;
    w.rec[RATO_IPM_PHI] = phi;
    w.rec[RATO_IPM_BARRIER] = barrier;
    w.rec[RATO_IPM_OBJECTIVE] = objective;
    w.rec[RATO_IPM_ALPHA] = a_max;
    w.rec[RATO_IPM_TRIALS] = 0.0;
    w.rec[RATO_IPM_SEARCHING] = 1.0;
    w.rec[RATO_IPM_ACCEPTED] = 0.0;
  }
}

__device__ __forceinline__ bool searching(const double* rec) {
  return rec[RATO_IPM_STATUS] == (double)RATO_IPM_RUNNING && rec[RATO_IPM_SEARCHING] == 1.0;
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_trial_kernel(rato_ipm_state st) {
  const View w = view(st);
  if (!searching(w.rec)) return;
  const double alpha = w.rec[RATO_IPM_ALPHA];
  for (int i = threadIdx.x; i < w.nv; i += ID_BLOCK) st.vt[w.ov + i] = st.v[w.ov + i] + alpha * st.dv[w.ov + i];
}

__global__ __launch_bounds__(ID_BLOCK) void ipm_accept_kernel(rato_ipm_state st, const double* __restrict__ gt, int64_t ldg) {
  __shared__ double sh[5][ID_WAVES];
  const View w = view(st);
  if (!searching(w.rec)) return;
  const int t = threadIdx.x, n = w.n;
  const double mu = w.rec[RATO_IPM_MU], nu = w.rec[RATO_IPM_NU], sf = w.rec[RATO_IPM_SF], phi = w.rec[RATO_IPM_PHI];
  const double Dphi = w.rec[RATO_IPM_DPHI], alpha = w.rec[RATO_IPM_ALPHA], a_dual = w.rec[RATO_IPM_A_DUAL];
  const int trials = (int)w.rec[RATO_IPM_TRIALS] + 1, iterations = (int)w.rec[RATO_IPM_ITERATIONS];
  const double* gk = gt + (int64_t)blockIdx.x * ldg;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                       // the two barrier sums, sum curv z^2, sum |c|, sum lin z
  for (int i = t; i < w.nv; i += ID_BLOCK) {
    const double vi = st.vt[w.ov + i];
    const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
    if (b.hasL) s[0] += log(b.dL);
    if (b.hasU) s[1] += log(b.dU);
    if (i < n) {
      s[2] += st.curv[w.ov + i] * vi * vi;
      s[4] += st.lin[w.ov + i] * vi;
    }
  }
  for (int r = t; r < w.m; r += ID_BLOCK) {
    const int sl = st.row_slack[r];
    s[3] += fabs(sl < 0 ? gk[r] - st.gL[w.om + r] : gk[r] - st.vt[w.ov + n + sl]);
  }
  block_sum(s, sh);
  const double phi_t = __dadd_rn(__dadd_rn(__dmul_rn(sf, 0.5 * s[2] + s[4]), -mu * (s[0] + s[1])), __dmul_rn(nu, s[3]));
  const double bound = __dadd_rn(__dadd_rn(phi, __dmul_rn(__dmul_rn(1e-8, alpha), Dphi)),
                                 __dmul_rn(10.0 * 2.220446049250313e-16, fabs(phi)));
  const bool accept = isfinite(phi_t) && phi_t <= bound;
  if (accept) {
    for (int i = t; i < w.nv; i += ID_BLOCK) {
      const double vi = st.vt[w.ov + i];
      const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
      const double dL = b.hasL ? b.dL : 1.0, dU = b.hasU ? b.dU : 1.0;
      const double zl = st.zl[w.ov + i] + a_dual * st.dzl[w.ov + i], zu = st.zu[w.ov + i] + a_dual * st.dzu[w.ov + i];
      st.v[w.ov + i] = vi;
      st.zl[w.ov + i] = b.hasL ? fmin(fmax(zl, mu / dL / 1e10), 1e10 * mu / dL) : 0.0;      // kappa_Sigma
      st.zu[w.ov + i] = b.hasU ? fmin(fmax(zu, mu / dU / 1e10), 1e10 * mu / dU) : 0.0;
    }
    for (int r = t; r < w.m; r += ID_BLOCK) st.y[w.om + r] += alpha * st.dy[w.om + r];
  }
  if (t == 0) {
    w.rec[RATO_IPM_PHI_T] = phi_t;
    w.rec[RATO_IPM_TRIALS] = (double)trials;
    if (accept) {
      w.rec[RATO_IPM_ITERATIONS] = (double)(iterations + 1);
      w.rec[RATO_IPM_SEARCHING] = 0.0;
      w.rec[RATO_IPM_ACCEPTED] = 1.0;
    } else if (trials >= 40) {
      w.rec[RATO_IPM_STATUS] = 2.0;
      w.rec[RATO_IPM_SEARCHING] = 0.0;
    } else {
      w.rec[RATO_IPM_ALPHA] = alpha * 0.5;
    }
  }
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

bool state_ok(const rato_ipm_state* st) {
  if (!st || st->K < 1 || st->K > 65535 || st->n < 1 || st->nI < 0 || st->m < 1 || st->nI > st->m ||
      st->ldv < (int64_t)st->n + st->nI || st->ldm < st->m)
    return false;
  const void* p[] = {st->row_slack, st->v, st->zl, st->zu, st->vL, st->vU, st->curv, st->lin, st->y, st->gL, st->rec, st->Sigma, st->gbar,
                     st->dv, st->dzl, st->dzu, st->vt, st->gradf, st->rz, st->dz, st->ez, st->diag, st->c, st->d, st->w, st->rs,
                     st->dyE, st->r2, st->q, st->dy};
  for (const void* q : p)
    if (!q) return false;
  return true;
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
  if (!state_ok(st)) return RATO_EINVAL;
  const bool rows = phase == RATO_IPM_PHASE_Q || phase == RATO_IPM_PHASE_UPDATE || phase == RATO_IPM_PHASE_FINISH;
  if (phase == RATO_IPM_PHASE_LADDER) {
    if (!info || flag < 1) return RATO_EINVAL;
  } else if (phase == RATO_IPM_PHASE_RHS || phase == RATO_IPM_PHASE_R || rows) {
    if (!a || lda < (rows ? st->m : st->n)) return RATO_EINVAL;
    if (phase == RATO_IPM_PHASE_R && (!b || ldb < st->n)) return RATO_EINVAL;
  } else {
    return RATO_EINVAL;
  }
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
