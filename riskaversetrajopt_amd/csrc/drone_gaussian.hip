// Drone Gaussian baseline (drone/drone_gaussian.py:135-486): the callbacks of its NLP in z = (u (3S), state allocations
// (S n_obs), obstacle allocations (n_obs)) -- g, jacfwd(g) and the Hessian of lam . g -- in fp64, for K problems per call.
//
// The recursion.  Per axis j the mean is (p_j, v_j)+ = (p_j + dt v_j, v_j + dt acc_j), acc_j = (u_j + kp p_j + kd v_j -
// c_d |v_j| v_j) / m.  A = I + dt db/dx is block diagonal over the axes, A_j = [[1, dt], [dt kp / m, c_j]] with
// c_j = 1 + dt (kd - 2 c_d |v_j|) / m, so each 2x2 block B = Sigma[(p_j, v_j), (p_k, v_k)] evolves on its own:
//   B+ = A_j B A_k^T + s 1 1^T (+ dt (beta / m)^2 on the velocity entry of a diagonal block),
// where s = var_m |b_dm|^2 = (var_m / m^2) sum_j (dt acc_j)^2 is the reference's scalar mass term (b_dm is 1-D there, so
// `b_dm @ b_dm.T` is an inner product that `Sig_next +=` adds to all 36 entries).  The rows read the position entries of the
// blocks (x,x), (x,y), (y,y) only; the z axis enters through s.
//
// One generic step, written once over a number type: double (the trajectory), D1 (value and one tangent: a lane per control
// direction, as car_gaussian.hip) and D2 (value, two tangents and the mixed second derivative: a lane per pair of control
// directions).  Every array is compile-time indexed and fully unrolled, so the state lives in registers: no LDS, no barrier,
// no scratch (DESIGN 7.aa holds the resource report).  |v| follows the AD convention sign(0) = 0.
#include "rato_common.h"
#include "rato_ppnd16.h"

#include <math.h>

namespace {

constexpr int DG_MAX_S = 64;
constexpr int DG_NOBS = 3;
constexpr int DG_DIR_BLOCK = 3 * DG_MAX_S;   // one lane per control direction
constexpr int DG_PAIR_BLOCK = 256;           // lanes of a pair-kernel workgroup
constexpr double SQRT_2PI = 2.5066282746310002;

// ---- number types --------------------------------------------------------------------------------------------------------
struct D1 {
  double v, d;
};
struct D2 {
  double v, a, b, ab;
};

__device__ __forceinline__ D1 operator+(D1 x, D1 y) { return {x.v + y.v, x.d + y.d}; }
__device__ __forceinline__ D1 operator-(D1 x, D1 y) { return {x.v - y.v, x.d - y.d}; }
__device__ __forceinline__ D1 operator*(D1 x, D1 y) { return {x.v * y.v, x.v * y.d + x.d * y.v}; }
__device__ __forceinline__ D1 operator*(double c, D1 x) { return {c * x.v, c * x.d}; }
__device__ __forceinline__ D1 operator+(D1 x, double c) { return {x.v + c, x.d}; }
__device__ __forceinline__ D1 recip(D1 x) {
  const double r = 1.0 / x.v;
  return {r, -r * r * x.d};
}
__device__ __forceinline__ D1 sqrtd(D1 x) {
  const double y = sqrt(x.v);
  return {y, x.d / (2.0 * y)};
}
__device__ __forceinline__ D1 absd(D1 x) {
  const double s = (double)((x.v > 0.0) - (x.v < 0.0));
  return {fabs(x.v), s * x.d};
}

__device__ __forceinline__ D2 operator+(D2 x, D2 y) { return {x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab}; }
__device__ __forceinline__ D2 operator-(D2 x, D2 y) { return {x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab}; }
__device__ __forceinline__ D2 operator*(D2 x, D2 y) {
  return {x.v * y.v, x.v * y.a + x.a * y.v, x.v * y.b + x.b * y.v, x.v * y.ab + x.ab * y.v + x.a * y.b + x.b * y.a};
}
__device__ __forceinline__ D2 operator*(double c, D2 x) { return {c * x.v, c * x.a, c * x.b, c * x.ab}; }
__device__ __forceinline__ D2 operator+(D2 x, double c) { return {x.v + c, x.a, x.b, x.ab}; }
__device__ __forceinline__ D2 recip(D2 x) {
  const double r = 1.0 / x.v, r2 = r * r;
  return {r, -r2 * x.a, -r2 * x.b, -r2 * x.ab + 2.0 * r2 * r * x.a * x.b};
}
__device__ __forceinline__ D2 sqrtd(D2 x) {
  const double y = sqrt(x.v), h = 0.5 / y;
  return {y, h * x.a, h * x.b, h * x.ab - x.a * x.b / (4.0 * y * y * y)};
}
__device__ __forceinline__ D2 absd(D2 x) {
  const double s = (double)((x.v > 0.0) - (x.v < 0.0));
  return {fabs(x.v), s * x.a, s * x.b, s * x.ab};
}

__device__ __forceinline__ double absd(double x) { return fabs(x); }

// ---- the recursion ------------------------------------------------------------------------------------------------------
struct Cst {
  double dt, inv_m, kp, kd, cd, dtm, gA, kappa, sig_w;
};

__device__ __forceinline__ Cst constants(const rato_drone_gauss_params& P) {
  Cst c;
  c.dt = P.dt;
  c.inv_m = 1.0 / P.mass_nom;
  c.kp = P.feedback_kp;
  c.kd = P.feedback_kd;
  c.cd = P.drag;
  c.dtm = P.dt / P.mass_nom;
  c.gA = P.dt * P.feedback_kp / P.mass_nom;
  c.kappa = P.mass_var / (P.mass_nom * P.mass_nom);
  c.sig_w = P.dt * (P.beta / P.mass_nom) * (P.beta / P.mass_nom);   // dt sigma sigma^T (:205-206)
  return c;
}

// block b of the covariance is Sigma[(p_j, v_j), (p_k, v_k)] = [P, Q, R, W] = [pp, pv, vp, vv]; the first three blocks are
// the ones the rows read
__host__ __device__ constexpr int blk_j(int b) { return b == 2 || b == 4 ? 1 : (b == 5 ? 2 : 0); }
__host__ __device__ constexpr int blk_k(int b) { return b == 0 ? 0 : (b <= 2 ? 1 : 2); }

// one step (:168-173, :202-216) of the mean (p, v) and of the first NB blocks, at the controls u of this step
template <class T, int NB>
__device__ __forceinline__ void gstep(const Cst& c, T (&p)[3], T (&v)[3], T (&B)[NB][4], const T (&u)[3]) {
  T cj[3], dv[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const T av = absd(v[j]);
    const T num = u[j] + c.kp * p[j] + c.kd * v[j] - c.cd * (av * v[j]);
    dv[j] = (c.dt * c.inv_m) * num;
    cj[j] = (-2.0 * c.cd * c.dtm) * av + (1.0 + c.dtm * c.kd);
  }
  const T s = c.kappa * (dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int j = blk_j(b), k = blk_k(b);
    const T t00 = B[b][0] + c.dt * B[b][2], t01 = B[b][1] + c.dt * B[b][3];                      // T = A_j B
    const T t10 = c.gA * B[b][0] + cj[j] * B[b][2], t11 = c.gA * B[b][1] + cj[j] * B[b][3];
    B[b][0] = t00 + c.dt * t01 + s;                                                              // B+ = T A_k^T + s
    B[b][1] = c.gA * t00 + t01 * cj[k] + s;
    B[b][2] = t10 + c.dt * t11 + s;
    B[b][3] = c.gA * t10 + t11 * cj[k] + s + (j == k ? c.sig_w : 0.0);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = p[j] + c.dt * v[j];
    v[j] = v[j] + dv[j];
  }
}

// |d| and sqrt(n^T Sigma[:2,:2] n) of obstacle i at the state (p, B) (:246-263)
template <class T>
__device__ __forceinline__ void obstacle(const rato_drone_gauss_params& P, int i, const T (&p)[3], const T (&B)[3][4], T& dist,
                                         T& sw) {
  const T d0 = p[0] + (-P.obs_positions[i][0]), d1 = p[1] + (-P.obs_positions[i][1]);
  const T d00 = d0 * d0, d11 = d1 * d1;
  const T r2 = d00 + d11;
  dist = sqrtd(r2);
  sw = sqrtd((d00 * B[0][0] + 2.0 * ((d0 * d1) * B[1][0]) + d11 * B[2][0]) * recip(r2));
}

struct Sizes {
  int D, na, nvar, n_nl, r_high, r_low;
};
__host__ __device__ inline Sizes sizes(int S) {
  Sizes z;
  z.D = 3 * S;
  z.na = S * DG_NOBS + DG_NOBS;
  z.nvar = z.D + z.na;
  z.r_high = 6 + DG_NOBS * S;
  z.r_low = z.r_high + 2 * (S + 1);
  z.n_nl = z.r_low + 2 * (S + 1);
  return z;
}

// ---- the trajectory: one lane per problem ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(RATO_WAVE)
drone_gaussian_trajectory_kernel(const rato_drone_gauss_params P, int K, const double* __restrict__ Z, double* __restrict__ mus,
                                 double* __restrict__ Sigmas) {
  const int k = blockIdx.x * RATO_WAVE + threadIdx.x;
  if (k >= K) return;
  const int S = P.S;
  const Sizes z = sizes(S);
  const Cst c = constants(P);
  Z += (size_t)k * z.nvar;
  if (mus) mus += (size_t)k * (S + 1) * 6;
  if (Sigmas) Sigmas += (size_t)k * (S + 1) * 36;
  double p[3], v[3], B[6][4];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = P.x_init[j];
    v[j] = P.x_init[3 + j];
  }
#pragma unroll
  for (int b = 0; b < 6; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) B[b][e] = 0.0;
  for (int t = 0; t <= S; ++t) {
    if (mus) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        mus[(size_t)t * 6 + j] = p[j];
        mus[(size_t)t * 6 + 3 + j] = v[j];
      }
    }
    if (Sigmas) {
      double* Sg = Sigmas + (size_t)t * 36;
#pragma unroll
      for (int b = 0; b < 6; ++b) {
        const int j = blk_j(b), q = blk_k(b);
        Sg[j * 6 + q] = Sg[q * 6 + j] = B[b][0];
        Sg[j * 6 + 3 + q] = Sg[(3 + q) * 6 + j] = B[b][1];
        Sg[(3 + j) * 6 + q] = Sg[q * 6 + 3 + j] = B[b][2];
        Sg[(3 + j) * 6 + 3 + q] = Sg[(3 + q) * 6 + 3 + j] = B[b][3];
      }
    }
    if (t == S) break;
    const double u[3] = {Z[3 * t], Z[3 * t + 1], Z[3 * t + 2]};
    gstep<double, 6>(c, p, v, B, u);
  }
}

// ---- values and Jacobian: one workgroup per problem, one lane per control direction ----------------------------------------
__global__ void __launch_bounds__(DG_DIR_BLOCK)
drone_gaussian_linearize_kernel(const rato_drone_gauss_params P, const double* __restrict__ Z, double* __restrict__ g_nl,
                                double* __restrict__ jac_nl) {
  const int S = P.S;
  const Sizes z = sizes(S);
  const Cst c = constants(P);
  const size_t k = blockIdx.x;
  const int lane = threadIdx.x, nl = blockDim.x;
  const bool live = lane < z.D;             // lanes past 3S carry a zero tangent and store no control column
  const bool lead = lane == 0;
  const int tp = lane / 3, ti = lane - 3 * tp;
  Z += k * (size_t)z.nvar;
  g_nl += k * (size_t)z.n_nl;
  jac_nl += k * (size_t)z.n_nl * z.nvar;
  const double* a_state = Z + z.D;
  const double* a_obs = Z + z.D + S * DG_NOBS;

  D1 p[3], v[3], B[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = {P.x_init[j], 0.0};
    v[j] = {P.x_init[3 + j], 0.0};
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) B[b][e] = {0.0, 0.0};

  // a mean row of state t: its control column (0.0 at steps t' >= t and across axes) and its allocation columns (all 0.0)
  auto mean_row = [&](int row, int t, int axis, double value, double dvalue) {
    double* J = jac_nl + (size_t)row * z.nvar;
    if (live) J[lane] = (tp >= t || ti != axis) ? 0.0 : dvalue;
    for (int col = lane; col < z.na; col += nl) J[z.D + col] = 0.0;
    if (lead) g_nl[row] = value;
  };

  for (int t = 0; t <= S; ++t) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {          // xs[:, :2] - high and -xs[:, :2] + low (:368-369), state 0 included
      mean_row(z.r_high + t * 2 + j, t, j, p[j].v - P.bound_high[j], p[j].d);
      mean_row(z.r_low + t * 2 + j, t, j, P.bound_low[j] - p[j].v, 0.0 - p[j].d);
    }
    if (t == S) break;
    D1 u[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = {Z[3 * t + j], (live && t == tp && j == ti) ? 1.0 : 0.0};
    gstep<D1, 3>(c, p, v, B, u);
#pragma unroll
    for (int i = 0; i < DG_NOBS; ++i) {    // -(|d| - ppf(1 - a) sqrt(n^T Sigma n) - r_i) at state t + 1 (:246-264)
      D1 dist, sw;
      obstacle(P, i, p, B, dist, sw);
      const double q = ppnd16(1.0 - a_state[t * DG_NOBS + i]);
      const double ipdf = SQRT_2PI * exp(0.5 * q * q);       // 1 / pdf(q)
      const int row = 6 + i * S + t;
      double* J = jac_nl + (size_t)row * z.nvar;
      if (live) J[lane] = tp > t ? 0.0 : q * sw.d - dist.d;
      for (int col = lane; col < z.na; col += nl)
        J[z.D + col] = col == t * DG_NOBS + i ? -sw.v * ipdf : (col == S * DG_NOBS + i ? -2.0 * P.obs_radii_delta / 3.0 : 0.0);
      if (lead) {
        const double rad = (P.obs_radii[i] + P.obs_radii_delta) - (a_obs[i] / 3.0) * (2.0 * P.obs_radii_delta);
        g_nl[row] = -(dist.v - q * sw.v - rad);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {            // x_S - x_final (:235-236)
    mean_row(j, S, j, p[j].v - P.x_final[j], p[j].d);
    mean_row(3 + j, S, j, v[j].v - P.x_final[3 + j], v[j].d);
  }
}

// ---- Hessian of lam . g, the (u,u) block: one lane per pair (a >= b) of control directions -------------------------------
// entry e of the block is entry e of np.tril_indices(nvar) as well: the control rows come first
__global__ void __launch_bounds__(DG_PAIR_BLOCK)
drone_gaussian_hessian_pairs_kernel(const rato_drone_gauss_params P, const double* __restrict__ Z, const double* __restrict__ lam,
                                    double* __restrict__ hess) {
  const int S = P.S;
  const Sizes z = sizes(S);
  const int npairs = z.D * (z.D + 1) / 2;
  const int e = blockIdx.x * DG_PAIR_BLOCK + threadIdx.x;
  if (e >= npairs) return;                 // no barrier below
  const Cst c = constants(P);
  const size_t k = blockIdx.y;
  Z += k * (size_t)z.nvar;
  lam += k * (size_t)z.n_nl;
  hess += k * ((size_t)z.nvar * (z.nvar + 1) / 2);
  const double* a_state = Z + z.D;

  int ra = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);   // the row of e in the lower triangle, exact after the fix-up
  while ((ra + 1) * (ra + 2) / 2 <= e) ++ra;
  while (ra * (ra + 1) / 2 > e) --ra;
  const int rb = e - ra * (ra + 1) / 2;
  const int ta = ra / 3, ia = ra - 3 * ta, tb = rb / 3, ib = rb - 3 * tb;

  D2 p[3], v[3], B[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = {P.x_init[j], 0.0, 0.0, 0.0};
    v[j] = {P.x_init[3 + j], 0.0, 0.0, 0.0};
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) B[b][q] = {0.0, 0.0, 0.0, 0.0};

  double h = 0.0;
  for (int t = 0; t < S; ++t) {
    D2 u[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      u[j] = {Z[3 * t + j], (t == ta && j == ia) ? 1.0 : 0.0, (t == tb && j == ib) ? 1.0 : 0.0, 0.0};
    gstep<D2, 3>(c, p, v, B, u);
    if (t < ta) continue;                  // ta >= tb: every mixed derivative is still zero
#pragma unroll
    for (int i = 0; i < DG_NOBS; ++i) {
      D2 dist, sw;
      obstacle(P, i, p, B, dist, sw);
      const double q = ppnd16(1.0 - a_state[t * DG_NOBS + i]);
      h += lam[6 + i * S + t] * (q * sw.ab - dist.ab);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) h += (lam[z.r_high + (t + 1) * 2 + j] - lam[z.r_low + (t + 1) * 2 + j]) * p[j].ab;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) h += lam[j] * p[j].ab + lam[3 + j] * v[j].ab;
  hess[e] = h;
}

// ---- Hessian of lam . g, the allocation rows: (u, a_{t,i}), the diagonal of (a,a) and the zeros around them ----------------
__global__ void __launch_bounds__(DG_DIR_BLOCK)
drone_gaussian_hessian_alloc_kernel(const rato_drone_gauss_params P, const double* __restrict__ Z, const double* __restrict__ lam,
                                    double* __restrict__ hess) {
  const int S = P.S;
  const Sizes z = sizes(S);
  const Cst c = constants(P);
  const size_t k = blockIdx.x;
  const int lane = threadIdx.x, nl = blockDim.x;
  const bool live = lane < z.D;
  const int tp = lane / 3, ti = lane - 3 * tp;
  Z += k * (size_t)z.nvar;
  lam += k * (size_t)z.n_nl;
  hess += k * ((size_t)z.nvar * (z.nvar + 1) / 2);
  const double* a_state = Z + z.D;

  D1 p[3], v[3], B[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p[j] = {P.x_init[j], 0.0};
    v[j] = {P.x_init[3 + j], 0.0};
  }
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) B[b][e] = {0.0, 0.0};

  for (int t = 0; t < S; ++t) {
    D1 u[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = {Z[3 * t + j], (live && t == tp && j == ti) ? 1.0 : 0.0};
    gstep<D1, 3>(c, p, v, B, u);
#pragma unroll
    for (int i = 0; i < DG_NOBS; ++i) {
      D1 dist, sw;
      obstacle(P, i, p, B, dist, sw);
      const double q = ppnd16(1.0 - a_state[t * DG_NOBS + i]);
      const double ipdf = SQRT_2PI * exp(0.5 * q * q);
      const double l = lam[6 + i * S + t];
      const int row = z.D + t * DG_NOBS + i;                 // the variable a_{t,i}
      double* H = hess + (size_t)row * (row + 1) / 2;
      if (live) H[lane] = tp > t ? 0.0 : l * (-ipdf) * sw.d;
      for (int col = z.D + lane; col < row; col += nl) H[col] = 0.0;
      if (lane == 0) H[row] = l * q * ipdf * ipdf * sw.v;
    }
  }
  for (int i = 0; i < DG_NOBS; ++i) {                        // everything involving a_obs is 0
    const int row = z.D + S * DG_NOBS + i;
    double* H = hess + (size_t)row * (row + 1) / 2;
    for (int col = lane; col <= row; col += nl) H[col] = 0.0;
  }
}

bool valid(const rato_drone_gauss_params* p, int32_t K) { return p && K >= 1 && p->S >= 1 && p->S <= DG_MAX_S; }

}  // namespace

extern "C" size_t rato_drone_gauss_params_bytes(void) { return sizeof(rato_drone_gauss_params); }

extern "C" int rato_drone_gaussian_linearize(const rato_drone_gauss_params* p, int32_t K, const double* Z, double* mus,
                                             double* Sigmas, double* g_nl, double* jac_nl, void* stream) {
  if (!valid(p, K) || !Z || !g_nl || !jac_nl) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  const int block = 3 * p->S <= RATO_WAVE ? RATO_WAVE : DG_DIR_BLOCK;
  hipLaunchKernelGGL(drone_gaussian_linearize_kernel, dim3((unsigned)K), dim3(block), 0, (hipStream_t)stream, *p, Z, g_nl,
                     jac_nl);
  if (mus || Sigmas)
    hipLaunchKernelGGL(drone_gaussian_trajectory_kernel, dim3((unsigned)((K + RATO_WAVE - 1) / RATO_WAVE)), dim3(RATO_WAVE), 0,
                       (hipStream_t)stream, *p, (int)K, Z, mus, Sigmas);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

// Every kernel keeps its state in registers: no workspace is needed at any S, K.
extern "C" size_t rato_drone_gaussian_hessian_workspace_bytes(int32_t S, int32_t K) {
  (void)S;
  (void)K;
  return 0;
}

extern "C" int rato_drone_gaussian_hessian(const rato_drone_gauss_params* p, int32_t K, const double* Z, const double* lam,
                                           double* hess_tril, void* workspace, size_t workspace_bytes, void* stream) {
  if (!valid(p, K) || !Z || !lam || !hess_tril) return RATO_EINVAL;
  const size_t need = rato_drone_gaussian_hessian_workspace_bytes(p->S, K);
  if (workspace_bytes < need || (need > 0 && !workspace)) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  const int D = 3 * p->S, npairs = D * (D + 1) / 2;
  hipLaunchKernelGGL(drone_gaussian_hessian_pairs_kernel, dim3((unsigned)((npairs + DG_PAIR_BLOCK - 1) / DG_PAIR_BLOCK), (unsigned)K),
                     dim3(DG_PAIR_BLOCK), 0, (hipStream_t)stream, *p, Z, lam, hess_tril);
  const int block = D <= RATO_WAVE ? RATO_WAVE : DG_DIR_BLOCK;
  hipLaunchKernelGGL(drone_gaussian_hessian_alloc_kernel, dim3((unsigned)K), dim3(block), 0, (hipStream_t)stream, *p, Z, lam,
                     hess_tril);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
