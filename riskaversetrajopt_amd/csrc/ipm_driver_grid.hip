// The interior-point driver's vector kernels spread over the rows (riskaversetrajopt_amd/ipm.py: DeviceState(vec='grid'),
// driver='device_grid'): a second form of the phases of csrc/ipm_driver.hip whose results -- every array of the
// state, the padding, every field of rec, after every phase, for running and for ended problems, in a batch and alone -- are
// BITWISE those of the one-workgroup-per-problem kernels.  Both forms compile their arithmetic from csrc/rato_ipm_rows.h.
//
// Launches.  Elementwise work runs on a grid of (block of ROWS rows) x (problem); block b serves entry b ROWS + lane of
// every vector of the phase, whatever its length.  A scalar that needs every row is made by stream-ordered launches:
//   residuals   rows (c, gradf, per-block extremes -> work)  |  finish, one workgroup per problem (status and mu logic ->
//               rec)  |  rows (Sigma, gbar, rz, diag, d, w, rs with the final mu)
//   newton      one rows launch per phase; LADDER: rows (diag from the old dw)  |  finish (dw or the status -> rec)
//   step_setup  rows (dzl, dzu, the barrier terms and per-block steps to the boundary -> work)  |  sums, one workgroup per
//               (group of sums, problem)  |  finish (the nu rule, ... -> rec)
//   trial       rows
//   accept      rows (barrier terms at vt -> work)  |  sums  |  finish (Armijo -> rec, and a token -> work)  |  apply, rows
// No workgroup waits for another, none reads what another one of the same launch writes (rec is written by the finishing
// launches alone, and they hold one workgroup per problem), no atomics, no private memory, no device state of the
// library's: what one launch makes and another needs lies in `work`, the caller's.  A problem that has ended (or is not
// searching: trial, accept) is left by every workgroup of every launch at once.
//
// Sums.  A sum is NOT split over the rows: one workgroup walks the full length with the workgroup form's lane-strided
// chain, wave_sum_dpp's tree and the four waves in order, through the same acc_* functions -- the association and the
// contraction are the workgroup form's.  What the split buys is one to three arrays per walk instead of fifteen, and five
// (three) walks side by side.  The barrier terms are not products: the rows launch stores has ? log(d) : +0.0 and the sum adds
// the stored terms (rato_ipm_rows.h: log_term says why the bits agree).
//
// Extremes are order free: nanmax and fmin are exact, so per-block partials are combined in the finishing launch.
//
// The mu loop evaluates comp(mu) = max_i |fl(z_i d_i - mu)| (comp_term: ONE rounding of the exact product minus mu) a
// data-dependent number of times.  It does not walk the rows again.  Rounding to nearest is monotone: x <= x' implies
// fl(x - mu) <= fl(x' - mu) for reals x, x' and any mu.  So with x_i = z_i d_i exact, every fl(x_i - mu) lies between
// fl(x_min - mu) and fl(x_max - mu), its magnitude is at most the larger of the two ends' magnitudes, and both ends are terms:
//     max_i |fl(x_i - mu)| = max(|fl(x_max - mu)|, |fl(x_min - mu)|).
// The rows launch therefore finds, per side, the entries with the largest and the smallest EXACT product and hands on their
// factors (z, d); the finishing launch evaluates comp_term on them for each mu.  Exact products are compared as (p, e), p =
// fl(z d), e = fma(z, d, -p) = z d - p (exact unless it underflows, which needs |z d| < 2^-968: far below half an ulp of any
// mu the loop can hold for a tolerance above 1e-290, so all such terms are the same number); ties are the same real and give
// the same term.  A product that rounds to +-inf gives the same term whichever factors made it (mu is finite).  nanmax
// propagates a NaN: a side with a NaN product is flagged and its maximum is NaN; a side without a bound is flagged empty
// and yields the -inf the workgroup form starts from, which pymax(0, .) turns into 0.  At mu = 0 (E0) the same formula
// holds with |fl(x)|.  tests/test_ipm_driver_grid_cpu.py checks the identity in exact rational arithmetic.
#include "rato_ipm_rows.h"

namespace {

using namespace rato_ipm;

constexpr int ROWS = ID_BLOCK;            // rows per workgroup: one per lane
constexpr int HEAD = 32;                  // per problem: [0, 10) the sums of the phase, [TOKEN] accept's token
constexpr int TOKEN = 16;
constexpr int PART = 32;                  // per (problem, block): the partials below
enum { P_C = 0, P_RS, P_RZ, P_NAN_L, P_NAN_U, P_PICK = 8 };   // then 4 picks of 5: L max, L min, U max, U min
constexpr int SETUP_GROUPS = 5, ACCEPT_GROUPS = 3;

__host__ __device__ inline int64_t blocks_for(int64_t len) { return (len + ROWS - 1) / ROWS; }
__host__ __device__ inline int64_t blocks_max(int64_t nv, int64_t m) { return blocks_for(nv > m ? nv : m); }
__host__ __device__ inline int64_t work_per_problem(int64_t nv, int64_t m) { return HEAD + 2 * nv + PART * blocks_max(nv, m); }

struct Work {   // problem k's part of the caller's scratch
  double *head, *tL, *tU, *part;
};
__device__ __forceinline__ Work work_of(double* work, const View& w, unsigned k) {
  Work x;
  x.head = work + (int64_t)k * work_per_problem(w.nv, w.m);
  x.tL = x.head + HEAD;
  x.tU = x.tL + w.nv;
  x.part = x.tU + w.nv;
  return x;
}

// an entry's exact product z d = p + e, with its factors
struct Pick {
  double has, p, e, z, d;
};
template <int MAX>
__device__ __forceinline__ bool better(const Pick& o, const Pick& x) {
  if (o.has == 0.0) return false;
  if (x.has == 0.0) return true;
  return MAX ? (o.p > x.p || (o.p == x.p && o.e > x.e)) : (o.p < x.p || (o.p == x.p && o.e < x.e));
}
__device__ __forceinline__ Pick shuffled(const Pick& x, int off) {
  Pick o;
  o.has = __shfl_xor(x.has, off, RATO_WAVE);
  o.p = __shfl_xor(x.p, off, RATO_WAVE);
  o.e = __shfl_xor(x.e, off, RATO_WAVE);
  o.z = __shfl_xor(x.z, off, RATO_WAVE);
  o.d = __shfl_xor(x.d, off, RATO_WAVE);
  return o;
}
// the best of the workgroup's picks in every lane; sh [5][ID_WAVES]
template <int MAX>
__device__ __forceinline__ void block_pick(Pick& x, double (*sh)[ID_WAVES]) {
  const int lane = threadIdx.x & (RATO_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = RATO_WAVE / 2; off > 0; off >>= 1) {
    const Pick o = shuffled(x, off);
    if (better<MAX>(o, x)) x = o;
  }
  if (lane == 0) {
    sh[0][wave] = x.has;
    sh[1][wave] = x.p;
    sh[2][wave] = x.e;
    sh[3][wave] = x.z;
    sh[4][wave] = x.d;
  }
  __syncthreads();
  x = Pick{sh[0][0], sh[1][0], sh[2][0], sh[3][0], sh[4][0]};
#pragma unroll
  for (int v = 1; v < ID_WAVES; ++v) {
    const Pick o{sh[0][v], sh[1][v], sh[2][v], sh[3][v], sh[4][v]};
    if (better<MAX>(o, x)) x = o;
  }
  __syncthreads();
}
__device__ __forceinline__ void store_pick(double* p, const Pick& x) {
  p[0] = x.has;
  p[1] = x.p;
  p[2] = x.e;
  p[3] = x.z;
  p[4] = x.d;
}
__device__ __forceinline__ Pick load_pick(const double* p) { return Pick{p[0], p[1], p[2], p[3], p[4]}; }

// one side of an entry into the side's picks and NaN flag
__device__ __forceinline__ void offer(double z, double d, Pick& hi, Pick& lo, double& nan) {
  const double p = __dmul_rn(z, d);
  if (p != p) {
    nan = 1.0;
    return;
  }
  const Pick o{1.0, p, __builtin_fma(z, d, -p), z, d};
  if (better<1>(o, hi)) hi = o;
  if (better<0>(o, lo)) lo = o;
}
// max |z d - mu| over a side from its picks: NaN with a NaN product, -inf without a bound
__device__ __forceinline__ double side_comp(const Pick& hi, const Pick& lo, double nan, double mu) {
  if (nan != 0.0) return (double)NAN;
  if (hi.has == 0.0) return -INFINITY;
  return nanmax(comp_term(hi.z, hi.d, mu), comp_term(lo.z, lo.d, mu));
}

// ---- residuals -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ID_BLOCK) void grid_residual_rows(rato_ipm_state st, const double* __restrict__ g, int64_t ldg,
                                                               const double* __restrict__ JTy, int64_t ldj, double* work) {
  __shared__ double sh[5][ID_WAVES];
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const Work x = work_of(work, w, k);
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  const double sf = w.rec[RATO_IPM_SF];
  const double* gk = g + (int64_t)k * ldg;
  const double* jk = JTy + (int64_t)k * ldj;
  double mx[3] = {-INFINITY, -INFINITY, -INFINITY};             // |c|, |rs|, |rz|
  double nan[2] = {0.0, 0.0};
  Pick pk[4] = {};                                              // L max, L min, U max, U min: has = 0
  if (i < w.m) residual_m_row(st, w, gk, i, mx);
  if (i < w.n) residual_z_row(st, w, jk, sf, i, mx);
  if (i < w.nv) {
    const Dist b = dist(st.v[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
    if (b.hasL) offer(st.zl[w.ov + i], b.dL, pk[0], pk[1], nan[0]);
    if (b.hasU) offer(st.zu[w.ov + i], b.dU, pk[2], pk[3], nan[1]);
  }
  block_extreme<0>(mx, sh);
  block_extreme<0>(nan, sh);
  block_pick<1>(pk[0], sh);
  block_pick<0>(pk[1], sh);
  block_pick<1>(pk[2], sh);
  block_pick<0>(pk[3], sh);
  if (threadIdx.x == 0) {
    double* p = x.part + (int64_t)blockIdx.x * PART;
    p[P_C] = mx[0];
    p[P_RS] = mx[1];
    p[P_RZ] = mx[2];
    p[P_NAN_L] = nan[0];
    p[P_NAN_U] = nan[1];
#pragma unroll
    for (int q = 0; q < 4; ++q) store_pick(p + P_PICK + 5 * q, pk[q]);
  }
}

__global__ __launch_bounds__(ID_BLOCK) void grid_residual_finish(rato_ipm_state st, int last, double* work) {
  __shared__ double sh[5][ID_WAVES];
  const unsigned k = blockIdx.x;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const Work x = work_of(work, w, k);
  const int nb = (int)blocks_max(w.nv, w.m);
  const double tol = w.rec[RATO_IPM_TOL];
  double mu = w.rec[RATO_IPM_MU], nu = w.rec[RATO_IPM_NU];
  double mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  double nan[2] = {0.0, 0.0};
  Pick pk[4] = {};
  for (int b = threadIdx.x; b < nb; b += ID_BLOCK) {
    const double* p = x.part + (int64_t)b * PART;
    mx[0] = nanmax(mx[0], p[P_C]);
    mx[1] = nanmax(mx[1], p[P_RS]);
    mx[2] = nanmax(mx[2], p[P_RZ]);
    nan[0] = fmax(nan[0], p[P_NAN_L]);
    nan[1] = fmax(nan[1], p[P_NAN_U]);
    const Pick o0 = load_pick(p + P_PICK), o1 = load_pick(p + P_PICK + 5), o2 = load_pick(p + P_PICK + 10),
               o3 = load_pick(p + P_PICK + 15);
    if (better<1>(o0, pk[0])) pk[0] = o0;
    if (better<0>(o1, pk[1])) pk[1] = o1;
    if (better<1>(o2, pk[2])) pk[2] = o2;
    if (better<0>(o3, pk[3])) pk[3] = o3;
  }
  block_extreme<0>(mx, sh);
  block_extreme<0>(nan, sh);
  block_pick<1>(pk[0], sh);
  block_pick<0>(pk[1], sh);
  block_pick<1>(pk[2], sh);
  block_pick<0>(pk[3], sh);
  // from here on every lane holds the same values: the scalar part of ipm_residuals_kernel
  auto comp = [&](double m_) {
    return pymax(pymax(0.0, side_comp(pk[0], pk[1], nan[0], m_)), side_comp(pk[2], pk[3], nan[1], m_));
  };
  const double prim = mx[0], dual = pymax(mx[2], st.nI > 0 ? mx[1] : 0.0);
  const double E0 = pymax(pymax(dual, prim), comp(0.0));
  const int status = residual_status(E0, tol, last);
  int passes = 0;
  if (status != RATO_IPM_RUNNING) {
    if (threadIdx.x == 0) residual_write_ended(w.rec, E0, prim, dual, status);
    return;
  }
  mu_loop(mu, nu, passes, tol, dual, prim, comp);
  if (threadIdx.x == 0) residual_write_running(w.rec, E0, prim, dual, mu, nu, dc_of(mu), passes);
}

__global__ __launch_bounds__(ID_BLOCK) void grid_prepare_rows(rato_ipm_state st, const double* __restrict__ JTy, int64_t ldj) {
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;   // ended before, or by the finishing launch just now
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  const double mu = w.rec[RATO_IPM_MU], dc = w.rec[RATO_IPM_DC], sf = w.rec[RATO_IPM_SF];
  const double* jk = JTy + (int64_t)k * ldj;
  if (i < w.nv) prepare_v_row(st, w, jk, mu, sf, i);
  if (i < w.m) prepare_m_row(st, w, dc, mu, i);
}

// ---- newton --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ID_BLOCK) void grid_newton_rows(rato_ipm_state st, int phase, const double* __restrict__ a, int64_t lda,
                                                             const double* __restrict__ b, int64_t ldb,
                                                             const int32_t* __restrict__ info, int flag) {
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x, n = w.n;
  const double* ak = a ? a + (int64_t)k * lda : nullptr;
  const double* bk = b ? b + (int64_t)k * ldb : nullptr;
  const double dc = w.rec[RATO_IPM_DC], sf = w.rec[RATO_IPM_SF], dw = w.rec[RATO_IPM_DW];
  switch (phase) {
    case RATO_IPM_PHASE_RHS:
      if (i < n) newton_rhs_row(st, w, ak, i);
      break;
    case RATO_IPM_PHASE_LADDER:                                  // rec keeps the old dw until grid_ladder_finish
      if (info[k] == 0) return;
      if (i < n) newton_ladder_row(st, w, ladder_dw(dw), sf, i);
      break;
    case RATO_IPM_PHASE_Q:
      if (i < w.m) newton_q_row(st, w, ak, dc, flag, i);
      break;
    case RATO_IPM_PHASE_R:
      if (i < n) newton_r_row(st, w, ak, bk, sf, dw, i);
      break;
    case RATO_IPM_PHASE_UPDATE:
      if (i < n) newton_update_z_row(st, w, i);
      if (i < w.m) newton_update_m_row(st, w, ak, dc, i);
      break;
    default:                                                     // RATO_IPM_PHASE_FINISH
      if (i < n) newton_finish_z_row(st, w, i);
      if (i < w.m) newton_finish_m_row(st, w, ak, i);
  }
}

__global__ __launch_bounds__(RATO_WAVE) void grid_ladder_finish(rato_ipm_state st, const int32_t* __restrict__ info, int flag) {
  const View w = view(st, blockIdx.x);
  if (threadIdx.x != 0 || w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING || info[blockIdx.x] == 0) return;
  if (flag >= 60) w.rec[RATO_IPM_STATUS] = 2.0;
  else w.rec[RATO_IPM_DW] = ladder_dw(w.rec[RATO_IPM_DW]);
}

// ---- step setup ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ID_BLOCK) void grid_setup_rows(rato_ipm_state st, double* work) {
  __shared__ double sh[2][ID_WAVES];
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const Work x = work_of(work, w, k);
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  const double mu = w.rec[RATO_IPM_MU];
  const double tau = pymax(0.99, 1.0 - mu);
  double mn[2] = {INFINITY, INFINITY};
  if (i < w.nv) {
    const Dist b = setup_row(st, w, mu, tau, i, st.v[w.ov + i], st.dv[w.ov + i], mn);
    x.tL[i] = log_term(b.hasL, b.dL);
    x.tU[i] = log_term(b.hasU, b.dU);
  }
  block_extreme<1>(mn, sh);
  if (threadIdx.x == 0) {
    x.part[(int64_t)blockIdx.x * PART] = mn[0];
    x.part[(int64_t)blockIdx.x * PART + 1] = mn[1];
  }
}

// one workgroup per (group of sums, problem): the workgroup form's chains over the full length
__global__ __launch_bounds__(ID_BLOCK) void grid_setup_sums(rato_ipm_state st, const double* __restrict__ Hdv, int64_t ldh,
                                                            double* work) {
  __shared__ double sh[3][ID_WAVES];
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const Work x = work_of(work, w, k);
  const int t = threadIdx.x, n = w.n;
  const double sf = w.rec[RATO_IPM_SF];
  const double* hk = Hdv + (int64_t)k * ldh;
  double s[3] = {0.0, 0.0, 0.0};
  int slot[3] = {-1, -1, -1};
  switch (blockIdx.x) {
    case 0:                                                      // gradf . dv_z, gbar . dv
      slot[0] = 0, slot[1] = 1;
#pragma unroll 4
      for (int i = t; i < n; i += ID_BLOCK) acc_dot(s[0], st.gradf[w.ov + i], st.dv[w.ov + i]);
#pragma unroll 4
      for (int i = t; i < w.nv; i += ID_BLOCK) acc_dot(s[1], st.gbar[w.ov + i], st.dv[w.ov + i]);
      break;
    case 1:                                                      // dv_z . W dv_z, dv_z . dv_z
      slot[0] = 2, slot[1] = 4;
#pragma unroll 4
      for (int i = t; i < n; i += ID_BLOCK) {
        const double dvi = st.dv[w.ov + i];
        acc_hess(s[0], dvi, hk[i], sf, st.curv[w.ov + i]);
        acc_square(s[1], dvi);
      }
      break;
    case 2:                                                      // sum Sigma dv^2
      slot[0] = 3;
#pragma unroll 4
      for (int i = t; i < w.nv; i += ID_BLOCK) acc_sigma(s[0], st.Sigma[w.ov + i], st.dv[w.ov + i]);
      break;
    case 3:                                                      // the two barrier sums, from the rows launch's terms
      slot[0] = 5, slot[1] = 6;
#pragma unroll 4
      for (int i = t; i < w.nv; i += ID_BLOCK) {
        acc_term(s[0], x.tL[i]);
        acc_term(s[1], x.tU[i]);
      }
      break;
    default:                                                     // sum curv z^2, sum lin z, sum |c|
      slot[0] = 7, slot[1] = 9, slot[2] = 8;
#pragma unroll 4
      for (int i = t; i < n; i += ID_BLOCK) {
        const double vi = st.v[w.ov + i];
        acc_curv(s[0], st.curv[w.ov + i], vi);
        acc_dot(s[1], st.lin[w.ov + i], vi);
      }
#pragma unroll 4
      for (int r = t; r < w.m; r += ID_BLOCK) acc_abs(s[2], st.c[w.om + r]);
  }
  block_sum(s, sh);
  if (t == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (slot[q] >= 0) x.head[slot[q]] = s[q];
  }
}

__global__ __launch_bounds__(ID_BLOCK) void grid_setup_finish(rato_ipm_state st, double* work) {
  __shared__ double sh[2][ID_WAVES];
  const unsigned k = blockIdx.x;
  const View w = view(st, k);
  if (w.rec[RATO_IPM_STATUS] != (double)RATO_IPM_RUNNING) return;
  const Work x = work_of(work, w, k);
  const int nb = (int)blocks_for(w.nv);
  double mn[2] = {INFINITY, INFINITY};
  for (int b = threadIdx.x; b < nb; b += ID_BLOCK) {
    mn[0] = fmin(mn[0], x.part[(int64_t)b * PART]);
    mn[1] = fmin(mn[1], x.part[(int64_t)b * PART + 1]);
  }
  block_extreme<1>(mn, sh);
  double s[SETUP_SUMS];
#pragma unroll
  for (int q = 0; q < SETUP_SUMS; ++q) s[q] = x.head[q];
  const SetupScalars o =
      setup_scalars(s, mn, w.rec[RATO_IPM_MU], w.rec[RATO_IPM_DW], w.rec[RATO_IPM_SF], w.rec[RATO_IPM_NU]);
  __syncthreads();                                               // every lane has read rec before lane 0 replaces nu
  if (threadIdx.x == 0) setup_write(w.rec, o);
}

// ---- trial and accept --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ID_BLOCK) void grid_trial_rows(rato_ipm_state st) {
  const View w = view(st, blockIdx.y);
  if (!searching(w.rec)) return;
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  if (i < w.nv) trial_row(st, w, w.rec[RATO_IPM_ALPHA], i);
}

__global__ __launch_bounds__(ID_BLOCK) void grid_accept_rows(rato_ipm_state st, double* work) {
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (!searching(w.rec)) return;
  const Work x = work_of(work, w, k);
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  if (i < w.nv) {
    const Dist b = dist(st.vt[w.ov + i], st.vL[w.ov + i], st.vU[w.ov + i]);
    x.tL[i] = log_term(b.hasL, b.dL);
    x.tU[i] = log_term(b.hasU, b.dU);
  }
}

__global__ __launch_bounds__(ID_BLOCK) void grid_accept_sums(rato_ipm_state st, const double* __restrict__ gt, int64_t ldg,
                                                             double* work) {
  __shared__ double sh[2][ID_WAVES];
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (!searching(w.rec)) return;
  const Work x = work_of(work, w, k);
  const int t = threadIdx.x;
  const double* gk = gt + (int64_t)k * ldg;
  double s[2] = {0.0, 0.0};
  int slot[2] = {-1, -1};
  switch (blockIdx.x) {
    case 0:                                                      // the two barrier sums
      slot[0] = 0, slot[1] = 1;
#pragma unroll 4
      for (int i = t; i < w.nv; i += ID_BLOCK) {
        acc_term(s[0], x.tL[i]);
        acc_term(s[1], x.tU[i]);
      }
      break;
    case 1:                                                      // sum curv z^2, sum lin z
      slot[0] = 2, slot[1] = 4;
#pragma unroll 4
      for (int i = t; i < w.n; i += ID_BLOCK) {
        const double vi = st.vt[w.ov + i];
        acc_curv(s[0], st.curv[w.ov + i], vi);
        acc_dot(s[1], st.lin[w.ov + i], vi);
      }
      break;
    default:                                                     // sum |c|
      slot[0] = 3;
#pragma unroll 4
      for (int r = t; r < w.m; r += ID_BLOCK) acc_abs(s[0], trial_c(st, w, gk, r));
  }
  block_sum(s, sh);
  if (t == 0) {
    x.head[slot[0]] = s[0];
    if (slot[1] >= 0) x.head[slot[1]] = s[1];
  }
}

// The Armijo test.  The token says whether THIS accept call accepted problem k: the line search of another problem of the
// batch keeps accept calls coming, and the accepted step (zl += a_dual dzl, y += alpha dy) must be applied once.  It is
// written for every problem, searching or not -- work is scratch, not state.
__global__ __launch_bounds__(RATO_WAVE) void grid_accept_finish(rato_ipm_state st, double* work) {
  const unsigned k = blockIdx.x;
  const View w = view(st, k);
  if (threadIdx.x != 0) return;
  const Work x = work_of(work, w, k);
  x.head[TOKEN] = 0.0;
  if (!searching(w.rec)) return;
  const AcceptIn in = accept_in(w.rec);
  double s[ACCEPT_SUMS];
#pragma unroll
  for (int q = 0; q < ACCEPT_SUMS; ++q) s[q] = x.head[q];
  bool accept;
  const double phi_t = accept_scalars(s, in, &accept);
  accept_write(w.rec, in, phi_t, accept);
  if (accept) x.head[TOKEN] = 1.0;
}

__global__ __launch_bounds__(ID_BLOCK) void grid_accept_apply(rato_ipm_state st, const double* work) {
  const unsigned k = blockIdx.y;
  const View w = view(st, k);
  if (work[(int64_t)k * work_per_problem(w.nv, w.m) + TOKEN] != 1.0) return;
  const int i = (int)blockIdx.x * ROWS + (int)threadIdx.x;
  // mu, a_dual and alpha are what the test read: an accepting grid_accept_finish replaces none of them
  if (i < w.nv) accept_v_row(st, w, w.rec[RATO_IPM_MU], w.rec[RATO_IPM_A_DUAL], i);
  if (i < w.m) accept_m_row(st, w, w.rec[RATO_IPM_ALPHA], i);
}

bool work_ok(const rato_ipm_state* st, const double* work, int64_t work_len) {
  return work && work_len >= rato_ipm_grid_work_doubles(st->n, st->nI, st->m, st->K);
}
dim3 rows_grid(const rato_ipm_state* st, int64_t len) { return dim3((unsigned)blocks_for(len), (unsigned)st->K); }
int64_t longest(const rato_ipm_state* st) { return (int64_t)st->n + st->nI > st->m ? (int64_t)st->n + st->nI : st->m; }

}  // namespace

extern "C" int32_t rato_ipm_grid_rows(void) { return ROWS; }

extern "C" int64_t rato_ipm_grid_work_doubles(int32_t n, int32_t nI, int32_t m, int32_t K) {
  if (n < 1 || nI < 0 || m < 1 || K < 1) return 0;
  return (int64_t)K * work_per_problem((int64_t)n + nI, m);
}

extern "C" int rato_ipm_residuals_grid_f64(const rato_ipm_state* st, const double* g, int64_t ldg, const double* JTy, int64_t ldj,
                                           int32_t last, double* work, int64_t work_len, void* stream) {
  if (!state_ok(st) || !g || !JTy || ldg < st->m || ldj < st->n || !work_ok(st, work, work_len)) return RATO_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(grid_residual_rows, rows_grid(st, longest(st)), dim3(ID_BLOCK), 0, s, *st, g, ldg, JTy, ldj, work);
  hipLaunchKernelGGL(grid_residual_finish, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, s, *st, (int)last, work);
  hipLaunchKernelGGL(grid_prepare_rows, rows_grid(st, longest(st)), dim3(ID_BLOCK), 0, s, *st, JTy, ldj);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_newton_grid_f64(const rato_ipm_state* st, int32_t phase, const double* a, int64_t lda, const double* b,
                                        int64_t ldb, const int32_t* info, int32_t flag, double* work, int64_t work_len,
                                        void* stream) {
  if (!state_ok(st) || !newton_args_ok(st, phase, a, lda, b, ldb, info, flag) || !work_ok(st, work, work_len)) return RATO_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  const bool z_only = phase == RATO_IPM_PHASE_RHS || phase == RATO_IPM_PHASE_LADDER || phase == RATO_IPM_PHASE_R;
  const int64_t len = z_only ? st->n : phase == RATO_IPM_PHASE_Q ? st->m : (st->n > st->m ? st->n : st->m);
  RATO_CLEAR_ERROR();
  if (phase != RATO_IPM_PHASE_LADDER || flag < 60)               // the sixtieth failure writes no diag
    hipLaunchKernelGGL(grid_newton_rows, rows_grid(st, len), dim3(ID_BLOCK), 0, s, *st, (int)phase, a, lda, b, ldb, info, (int)flag);
  if (phase == RATO_IPM_PHASE_LADDER)
    hipLaunchKernelGGL(grid_ladder_finish, dim3((unsigned)st->K), dim3(RATO_WAVE), 0, s, *st, info, (int)flag);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_step_setup_grid_f64(const rato_ipm_state* st, const double* Hdv, int64_t ldh, double* work, int64_t work_len,
                                            void* stream) {
  if (!state_ok(st) || !Hdv || ldh < st->n || !work_ok(st, work, work_len)) return RATO_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(grid_setup_rows, rows_grid(st, (int64_t)st->n + st->nI), dim3(ID_BLOCK), 0, s, *st, work);
  hipLaunchKernelGGL(grid_setup_sums, dim3(SETUP_GROUPS, (unsigned)st->K), dim3(ID_BLOCK), 0, s, *st, Hdv, ldh, work);
  hipLaunchKernelGGL(grid_setup_finish, dim3((unsigned)st->K), dim3(ID_BLOCK), 0, s, *st, work);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_trial_grid_f64(const rato_ipm_state* st, double* work, int64_t work_len, void* stream) {
  if (!state_ok(st) || !work_ok(st, work, work_len)) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(grid_trial_rows, rows_grid(st, (int64_t)st->n + st->nI), dim3(ID_BLOCK), 0, (hipStream_t)stream, *st);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_ipm_accept_grid_f64(const rato_ipm_state* st, const double* gt, int64_t ldg, double* work, int64_t work_len,
                                        void* stream) {
  if (!state_ok(st) || !gt || ldg < st->m || !work_ok(st, work, work_len)) return RATO_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(grid_accept_rows, rows_grid(st, (int64_t)st->n + st->nI), dim3(ID_BLOCK), 0, s, *st, work);
  hipLaunchKernelGGL(grid_accept_sums, dim3(ACCEPT_GROUPS, (unsigned)st->K), dim3(ID_BLOCK), 0, s, *st, gt, ldg, work);
  hipLaunchKernelGGL(grid_accept_finish, dim3((unsigned)st->K), dim3(RATO_WAVE), 0, s, *st, work);
  hipLaunchKernelGGL(grid_accept_apply, rows_grid(st, longest(st)), dim3(ID_BLOCK), 0, s, *st, work);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
