// The interior-point driver's arithmetic, once: what one row of each phase computes, the expressions the sums accumulate, and
// the scalar epilogues (status and mu logic, the nu rule, the Armijo test).  csrc/ipm_driver.hip (one workgroup per problem)
// and csrc/ipm_driver_grid.hip (a grid over the rows) compile these functions and nothing else for their
// arithmetic, so that contraction (the library is built with -ffp-contract=fast) decides the same way in both forms and the
// grid form's results are BITWISE the workgroup form's.  Every function is __forceinline__: it costs nothing and a kernel's
// loop is what it was when the expressions stood in it.
//
// A function that takes `k` serves problem k (ipm_driver.hip: k = blockIdx.x).
#pragma once
#include "rato_common.h"

#include <math.h>

namespace rato_ipm {

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
  int64_t ov, om, od;   // of the [K][ldv], [K][ldm] and [K][n] arrays
};
__device__ __forceinline__ View view(const rato_ipm_state& st, unsigned k) {
  View w;
  w.n = st.n;
  w.nv = st.n + st.nI;
  w.m = st.m;
  w.rec = st.rec + (int64_t)k * RATO_IPM_REC;
  w.ov = (int64_t)k * st.ldv;
  w.om = (int64_t)k * st.ldm;
  w.od = (int64_t)k * st.n;
  return w;
}

__device__ __forceinline__ bool searching(const double* rec) {
  return rec[RATO_IPM_STATUS] == (double)RATO_IPM_RUNNING && rec[RATO_IPM_SEARCHING] == 1.0;
}

// ---- the residual phase -------------------------------------------------------------------------------------------------------
// One term of comp(mu) of Problem.error, |z d - mu|.  ONE rounding: this toolchain's __dmul_rn is a plain multiplication,
// which contraction fused with the subtraction in the workgroup kernel; the fused form is written out so that neither form
// depends on where the compiler finds the product (the grid form's finishing launch holds it outside the mu loop).  At
// mu = 0 it is |fl(z d)|.
__device__ __forceinline__ double comp_term(double z, double d, double mu) { return fabs(__builtin_fma(z, d, -mu)); }

// constraint row r: c, and |c| and |rs| into mx[0], mx[1]
__device__ __forceinline__ void residual_m_row(const rato_ipm_state& st, const View& w, const double* gk, int r, double (&mx)[3]) {
  const int sl = st.row_slack[r];
  double cr;
  if (sl < 0) {
    cr = gk[r] - st.gL[w.om + r];
  } else {
    const int64_t i = w.ov + w.n + sl;
    cr = gk[r] - st.v[i];
    mx[1] = nanmax(mx[1], fabs(-st.y[w.om + r] - st.zl[i] + st.zu[i]));
  }
  st.c[w.om + r] = cr;
  mx[0] = nanmax(mx[0], fabs(cr));
}

// variable j < n: gradf, and |rz| into mx[2]
__device__ __forceinline__ void residual_z_row(const rato_ipm_state& st, const View& w, const double* jk, double sf, int j,
                                               double (&mx)[3]) {
  const double gf = sf * (st.curv[w.ov + j] * st.v[w.ov + j] + st.lin[w.ov + j]);
  st.gradf[w.ov + j] = gf;
  mx[2] = nanmax(mx[2], fabs(gf + jk[j] - st.zl[w.ov + j] + st.zu[w.ov + j]));
}

// -> RATO_IPM_RUNNING or the status E0 ends the problem with
__device__ __forceinline__ int residual_status(double E0, double tol, int last) {
  int status = RATO_IPM_RUNNING;
  if (!isfinite(E0)) status = 2;
  else if (E0 <= tol) status = 0;
  else if (last) status = 1;
  return status;
}

__device__ __forceinline__ void residual_write_ended(double* rec, double E0, double prim, double dual, int status) {
  rec[RATO_IPM_E0] = E0;
  rec[RATO_IPM_PRIM] = prim;
  rec[RATO_IPM_DUAL] = dual;
  rec[RATO_IPM_STATUS] = (double)status;
}

// the mu loop of solve_group; comp(mu) is Problem.error's complementarity part
template <class Comp>
__device__ __forceinline__ void mu_loop(double& mu, double& nu, int& passes, double tol, double dual, double prim, Comp comp) {
  const double floor_mu = tol / 10.0;
  while (mu > floor_mu) {
    const double Emu = pymax(pymax(dual, prim), comp(mu));
    if (!(Emu <= 10.0 * mu)) break;
    mu = pymax(floor_mu, pymin(0.2 * mu, __dmul_rn(mu, sqrt(mu))));
    nu = 0.0;
    ++passes;
  }
}

__device__ __forceinline__ double dc_of(double mu) { return 1e-8 * sqrt(sqrt(mu)); }

__device__ __forceinline__ void residual_write_running(double* rec, double E0, double prim, double dual, double mu, double nu,
                                                       double dc, int passes) {
  rec[RATO_IPM_E0] = E0;
  rec[RATO_IPM_PRIM] = prim;
  rec[RATO_IPM_DUAL] = dual;
  rec[RATO_IPM_MU] = mu;
  rec[RATO_IPM_NU] = nu;
  rec[RATO_IPM_DW] = 0.0;
  rec[RATO_IPM_DC] = dc;
  rec[RATO_IPM_MU_PASSES] = (double)passes;
  rec[RATO_IPM_SEARCHING] = 0.0;
}

// prepare_step, entry i < nv: Sigma, gbar, and rz, diag where i < n (gradf: what residual_z_row left)
__device__ __forceinline__ void prepare_v_row(const rato_ipm_state& st, const View& w, const double* jk, double mu, double sf, int i) {
  const Dist b = dist(st.v[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
  const double Sig = st.zl[w.ov + i] * b.iL + st.zu[w.ov + i] * b.iU, gb = -mu * b.iL + mu * b.iU;
  st.Sigma[w.ov + i] = Sig;
  st.gbar[w.ov + i] = gb;
  if (i < w.n) {
    st.rz[w.ov + i] = st.gradf[w.ov + i] + jk[i] + gb;
    st.diag[w.od + i] = (Sig + 0.0) + sf * st.curv[w.ov + i];
  }
}

// prepare_step, constraint row r: d, w, rs (c: what residual_m_row left; Sigma and gbar of the slack again: no wait for
// their owner)
__device__ __forceinline__ void prepare_m_row(const rato_ipm_state& st, const View& w, double dc, double mu, int r) {
  const int sl = st.row_slack[r];
  const double cr = st.c[w.om + r];
  if (sl < 0) {
    const double d = 1.0 / dc;
    st.d[w.om + r] = d;
    st.w[w.om + r] = d * cr;
  } else {
    const int64_t i = w.ov + w.n + sl;
    const Dist b = dist(st.v[i], st.vL[i], st.vU[i]);
    const double Sig = st.zl[i] * b.iL + st.zu[i] * b.iU, gb = -mu * b.iL + mu * b.iU;
    const double rs = -st.y[w.om + r] + gb;
    st.rs[w.om + r] = rs;
    st.d[w.om + r] = Sig;
    st.w[w.om + r] = Sig * cr + rs;
  }
}

// ---- the Newton phases ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void newton_rhs_row(const rato_ipm_state& st, const View& w, const double* ak, int j) {
  st.dz[w.ov + j] = -(st.rz[w.ov + j] + ak[j]);
}
__device__ __forceinline__ double ladder_dw(double dw) { return dw == 0.0 ? 1e-4 : 8.0 * dw; }
__device__ __forceinline__ void newton_ladder_row(const rato_ipm_state& st, const View& w, double dw, double sf, int j) {
  st.diag[w.od + j] = (st.Sigma[w.ov + j] + dw) + sf * st.curv[w.ov + j];
}
__device__ __forceinline__ void newton_q_row(const rato_ipm_state& st, const View& w, const double* ak, double dc, int flag, int r) {
  const int sl = st.row_slack[r];
  const double lin = ak[r] + st.c[w.om + r];
  if (sl < 0) {
    double dyE = st.dyE[w.om + r];
    if (flag) st.dyE[w.om + r] = dyE = lin / dc;
    const double r2 = -lin + dc * dyE;
    st.r2[w.om + r] = r2;
    st.q[w.om + r] = dyE - r2 / dc;
  } else {
    st.q[w.om + r] = st.Sigma[w.ov + w.n + sl] * lin + st.rs[w.om + r];
  }
}
__device__ __forceinline__ void newton_r_row(const rato_ipm_state& st, const View& w, const double* ak, const double* bk, double sf,
                                             double dw, int j) {
  const double x = st.dz[w.ov + j], h = ak[j] + (sf * st.curv[w.ov + j]) * x;
  st.ez[w.ov + j] = -(st.rz[w.ov + j] + h + (st.Sigma[w.ov + j] + dw) * x + bk[j]);
}
__device__ __forceinline__ void newton_update_z_row(const rato_ipm_state& st, const View& w, int j) {
  st.dz[w.ov + j] += st.ez[w.ov + j];
}
__device__ __forceinline__ void newton_update_m_row(const rato_ipm_state& st, const View& w, const double* ak, double dc, int r) {
  if (st.row_slack[r] < 0) st.dyE[w.om + r] += (ak[r] - st.r2[w.om + r]) / dc;
}
__device__ __forceinline__ void newton_finish_z_row(const rato_ipm_state& st, const View& w, int j) {
  st.dv[w.ov + j] = st.dz[w.ov + j];
}
__device__ __forceinline__ void newton_finish_m_row(const rato_ipm_state& st, const View& w, const double* ak, int r) {
  const int sl = st.row_slack[r];
  if (sl < 0) {
    st.dy[w.om + r] = st.dyE[w.om + r];
  } else {
    const double ds = ak[r] + st.c[w.om + r];
    st.dv[w.ov + w.n + sl] = ds;
    st.dy[w.om + r] = st.Sigma[w.ov + w.n + sl] * ds + st.rs[w.om + r];
  }
}

// ---- the step setup --------------------------------------------------------------------------------------------------------------
// entry i < nv: dzl, dzu and the steps to the boundary into mn (primal, dual); -> the distances, for the barrier terms
__device__ __forceinline__ Dist setup_row(const rato_ipm_state& st, const View& w, double mu, double tau, int i, double vi, double dvi,
                                          double (&mn)[2]) {
  const double zl = st.zl[w.ov + i], zu = st.zu[w.ov + i];
  const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
  const double dzl = b.hasL ? mu * b.iL - zl - zl * b.iL * dvi : 0.0;
  const double dzu = b.hasU ? mu * b.iU - zu + zu * b.iU * dvi : 0.0;
  st.dzl[w.ov + i] = dzl;
  st.dzu[w.ov + i] = dzu;
  if (b.hasL && dvi < 0.0) mn[0] = fmin(mn[0], -tau * b.dL / dvi);
  if (b.hasU && -dvi < 0.0) mn[0] = fmin(mn[0], -tau * b.dU / -dvi);
  if (b.hasL && dzl < 0.0) mn[1] = fmin(mn[1], -tau * zl / dzl);
  if (b.hasU && dzu < 0.0) mn[1] = fmin(mn[1], -tau * zu / dzu);
  return b;
}

// what the sums accumulate, one entry at a time
__device__ __forceinline__ void acc_dot(double& s, double a, double b) { s += a * b; }                 // gradf . dv, gbar . dv, lin . z
__device__ __forceinline__ void acc_sigma(double& s, double Sig, double dvi) { s += Sig * dvi * dvi; }
__device__ __forceinline__ void acc_hess(double& s, double dvi, double h, double sf, double cv) { s += dvi * (h + (sf * cv) * dvi); }
__device__ __forceinline__ void acc_square(double& s, double dvi) { s += dvi * dvi; }
__device__ __forceinline__ void acc_curv(double& s, double cv, double vi) { s += cv * vi * vi; }
__device__ __forceinline__ void acc_log(double& s, bool has, double d) {
  if (has) s += log(d);
}
__device__ __forceinline__ void acc_abs(double& s, double c) { s += fabs(c); }
// The grid form's barrier sums add stored terms, has ? log(d) : +0.0, where acc_log skips an absent bound.  The bits are the
// same: an accumulator starts at +0.0 and x + (+0.0) == x bitwise for every x but -0.0, which a sum that started at +0.0 can
// never hold (round to nearest gives -0.0 only from (-0.0) + (-0.0)); a NaN stays the NaN it is.
__device__ __forceinline__ double log_term(bool has, double d) { return has ? log(d) : 0.0; }
__device__ __forceinline__ void acc_term(double& s, double t) { s += t; }
// c at the trial point of constraint row r
__device__ __forceinline__ double trial_c(const rato_ipm_state& st, const View& w, const double* gk, int r) {
  const int sl = st.row_slack[r];
  return sl < 0 ? gk[r] - st.gL[w.om + r] : gk[r] - st.vt[w.ov + w.n + sl];
}

// the sums of the step setup: gradf . dv_z, gbar . dv, dv_z . W dv_z, sum Sigma dv^2, dv_z . dv_z, the two barrier sums, sum
// curv z^2, sum |c|, sum lin z
enum { SETUP_SUMS = 10, ACCEPT_SUMS = 5 };

struct SetupScalars {
  double a_max, a_dual, c1, Dbar, quad, nu, Dphi, phi, barrier, objective;
};
__device__ __forceinline__ SetupScalars setup_scalars(const double (&s)[SETUP_SUMS], const double (&mn)[2], double mu, double dw,
                                                      double sf, double nu) {
  SetupScalars o;
  o.a_max = fmin(1.0, mn[0]);
  o.a_dual = fmin(1.0, mn[1]);
  o.c1 = s[8];
  o.Dbar = s[0] + s[1];
  o.quad = __dadd_rn(__dadd_rn(s[2], s[3]), __dmul_rn(dw, s[4]));
  if (o.c1 > 0.0) {
    const double nu_trial = __dadd_rn(o.Dbar, __dmul_rn(0.5, pymax(o.quad, 0.0))) / __dmul_rn(0.9, o.c1);
    if (nu < nu_trial) nu = __dadd_rn(nu_trial, 1.0);
  }
  o.nu = nu;
  o.Dphi = pymin(__dadd_rn(o.Dbar, -__dmul_rn(nu, o.c1)), 0.0);
  o.objective = 0.5 * s[7] + s[9];
  o.barrier = -mu * (s[5] + s[6]);
  o.phi = __dadd_rn(__dadd_rn(__dmul_rn(sf, o.objective), o.barrier), __dmul_rn(nu, o.c1));
  return o;
}
__device__ __forceinline__ void setup_write(double* rec, const SetupScalars& o) {
  rec[RATO_IPM_A_MAX] = o.a_max;
  rec[RATO_IPM_A_DUAL] = o.a_dual;
  rec[RATO_IPM_C1] = o.c1;
  rec[RATO_IPM_DBAR] = o.Dbar;
  rec[RATO_IPM_QUAD] = o.quad;
  rec[RATO_IPM_NU] = o.nu;
  rec[RATO_IPM_DPHI] = o.Dphi;
  rec[RATO_IPM_PHI] = o.phi;
  rec[RATO_IPM_BARRIER] = o.barrier;
  rec[RATO_IPM_OBJECTIVE] = o.objective;
  rec[RATO_IPM_ALPHA] = o.a_max;
  rec[RATO_IPM_TRIALS] = 0.0;
  rec[RATO_IPM_SEARCHING] = 1.0;
  rec[RATO_IPM_ACCEPTED] = 0.0;
}

// ---- trial and accept ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void trial_row(const rato_ipm_state& st, const View& w, double alpha, int i) {
  st.vt[w.ov + i] = st.v[w.ov + i] + alpha * st.dv[w.ov + i];
}

// what the accept phase reads of the record before anything replaces it
struct AcceptIn {
  double mu, nu, sf, phi, Dphi, alpha, a_dual;
  int trials, iterations;
};
__device__ __forceinline__ AcceptIn accept_in(const double* rec) {
  AcceptIn a;
  a.mu = rec[RATO_IPM_MU];
  a.nu = rec[RATO_IPM_NU];
  a.sf = rec[RATO_IPM_SF];
  a.phi = rec[RATO_IPM_PHI];
  a.Dphi = rec[RATO_IPM_DPHI];
  a.alpha = rec[RATO_IPM_ALPHA];
  a.a_dual = rec[RATO_IPM_A_DUAL];
  a.trials = (int)rec[RATO_IPM_TRIALS] + 1;
  a.iterations = (int)rec[RATO_IPM_ITERATIONS];
  return a;
}
// the sums: the two barrier sums, sum curv z^2, sum |c|, sum lin z at the trial point -> phi_t; *accept: the Armijo test
__device__ __forceinline__ double accept_scalars(const double (&s)[ACCEPT_SUMS], const AcceptIn& a, bool* accept) {
  const double phi_t = __dadd_rn(__dadd_rn(__dmul_rn(a.sf, 0.5 * s[2] + s[4]), -a.mu * (s[0] + s[1])), __dmul_rn(a.nu, s[3]));
  const double bound = __dadd_rn(__dadd_rn(a.phi, __dmul_rn(__dmul_rn(1e-8, a.alpha), a.Dphi)),
                                 __dmul_rn(10.0 * 2.220446049250313e-16, fabs(a.phi)));
  *accept = isfinite(phi_t) && phi_t <= bound;
  return phi_t;
}
// the accepted step of entry i < nv, with the kappa_Sigma clip
__device__ __forceinline__ void accept_v_row(const rato_ipm_state& st, const View& w, double mu, double a_dual, int i) {
  const double vi = st.vt[w.ov + i];
  const Dist b = dist(vi, st.vL[w.ov + i], st.vU[w.ov + i]);
  const double dL = b.hasL ? b.dL : 1.0, dU = b.hasU ? b.dU : 1.0;
  const double zl = st.zl[w.ov + i] + a_dual * st.dzl[w.ov + i], zu = st.zu[w.ov + i] + a_dual * st.dzu[w.ov + i];
  st.v[w.ov + i] = vi;
  st.zl[w.ov + i] = b.hasL ? fmin(fmax(zl, mu / dL / 1e10), 1e10 * mu / dL) : 0.0;
  st.zu[w.ov + i] = b.hasU ? fmin(fmax(zu, mu / dU / 1e10), 1e10 * mu / dU) : 0.0;
}
__device__ __forceinline__ void accept_m_row(const rato_ipm_state& st, const View& w, double alpha, int r) {
  st.y[w.om + r] += alpha * st.dy[w.om + r];
}
__device__ __forceinline__ void accept_write(double* rec, const AcceptIn& a, double phi_t, bool accept) {
  rec[RATO_IPM_PHI_T] = phi_t;
  rec[RATO_IPM_TRIALS] = (double)a.trials;
  if (accept) {
    rec[RATO_IPM_ITERATIONS] = (double)(a.iterations + 1);
    rec[RATO_IPM_SEARCHING] = 0.0;
    rec[RATO_IPM_ACCEPTED] = 1.0;
  } else if (a.trials >= 40) {
    rec[RATO_IPM_STATUS] = 2.0;
    rec[RATO_IPM_SEARCHING] = 0.0;
  } else {
    rec[RATO_IPM_ALPHA] = a.alpha * 0.5;
  }
}

// the argument checks both forms share (host)
inline bool state_ok(const rato_ipm_state* st) {
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
// what rato_ipm_newton_f64 refuses beyond state_ok
inline bool newton_args_ok(const rato_ipm_state* st, int32_t phase, const double* a, int64_t lda, const double* b, int64_t ldb,
                           const int32_t* info, int32_t flag) {
  const bool rows = phase == RATO_IPM_PHASE_Q || phase == RATO_IPM_PHASE_UPDATE || phase == RATO_IPM_PHASE_FINISH;
  if (phase == RATO_IPM_PHASE_LADDER) return info && flag >= 1;
  if (phase == RATO_IPM_PHASE_RHS || phase == RATO_IPM_PHASE_R || rows) {
    if (!a || lda < (rows ? st->m : st->n)) return false;
    return !(phase == RATO_IPM_PHASE_R && (!b || ldb < st->n));
  }
  return false;
}

}  // namespace rato_ipm
