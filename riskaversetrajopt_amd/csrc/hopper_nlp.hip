// Hopper NLP (hopper/hopper.py:239-298, :491-514, :569-580): the sample-independent rows of g -- the RK4 defect of the 8-state
// leg, the no-slip row J_T q_dot and the end-effector height -- with their first derivatives, and the Hessian of lam . g as
// one 12 x 12 block per step, in fp64, for K problems per call.  The slip rows (the sample axis) stay in hopper.hip.
//
// The recursion.  b(x, u) = (q_dot, M^-1 (-C + B(x2) u_robot + J(x2, x3)^T f)) (:218-231) reads the state through
// s = sin x2, c = cos x2 and x3 only, and is affine in u:
//   qdd0 = (fx - s u1) / mt,  qdd1 = (c u1 + fz - mt g) / mt,  qdd2 = (u0 + x3 (c fx + s fz)) / It,  qdd3 = (u1 + s fx - c fz) / ml.
// The defect of step t is x_{t+1} - (x_t + dt/6 (k1 + 2 k2 + 2 k3 + k4)) with the four RK4 stages of :243-246.  One generic
// routine, written once over a number type, carries it: D1 (value and one tangent: a lane per direction of (x_t, u_t)) for the
// Jacobian, D2 (value, two tangents and the mixed second derivative: a lane per pair of directions) for the Hessian.  Every
// array is compile-time indexed and fully unrolled, so the state lives in registers: no LDS, no barrier.
//
// Structure used.  The defect of step t reads (x_t, u_t) and, linearly with coefficient 1, x_{t+1}; the two state rows read one
// state.  So the Hessian of lam . g is block diagonal over the steps, block t on (x_t (8), u_t (4)), the last block on x_S
// alone.  Inside a block the defect and the rows are affine in x0, x1, x4, x5 with constant coefficients: a pair that holds one
// of those directions has no second derivative and its lane only forwards `add` (the slip part reaches x0 that way).
//
// The kernels are phase-agnostic: they produce per-step local quantities, and the caller owns the contact / flight masks (it
// folds them into lam_rows) and the constant unit coefficients.
#include "rato_common.h"

#include <math.h>

namespace {

constexpr int HN_BLOCK = 256;
constexpr int HN_NX = 8, HN_NU = 4, HN_NL = HN_NX + HN_NU;   // local variables of a step block: (x_t, u_t)
constexpr int HN_PAIRS = HN_NL * (HN_NL + 1) / 2;            // 78 = lower triangle of 12 x 12

// ---- number types (the D1 / D2 of drone_gaussian.hip, with sin and cos) ---------------------------------------------------
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
__device__ __forceinline__ void sincosd(D1 x, D1& s, D1& c) {
  double sv, cv;
  sincos(x.v, &sv, &cv);
  s = {sv, cv * x.d};
  c = {cv, -sv * x.d};
}

__device__ __forceinline__ D2 operator+(D2 x, D2 y) { return {x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab}; }
__device__ __forceinline__ D2 operator-(D2 x, D2 y) { return {x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab}; }
__device__ __forceinline__ D2 operator*(D2 x, D2 y) {
  return {x.v * y.v, x.v * y.a + x.a * y.v, x.v * y.b + x.b * y.v, x.v * y.ab + x.ab * y.v + x.a * y.b + x.b * y.a};
}
__device__ __forceinline__ D2 operator*(double c, D2 x) { return {c * x.v, c * x.a, c * x.b, c * x.ab}; }
__device__ __forceinline__ D2 operator+(D2 x, double c) { return {x.v + c, x.a, x.b, x.ab}; }
__device__ __forceinline__ void sincosd(D2 x, D2& s, D2& c) {
  double sv, cv;
  sincos(x.v, &sv, &cv);
  const double aa = x.a * x.b;
  s = {sv, cv * x.a, cv * x.b, cv * x.ab - sv * aa};
  c = {cv, -sv * x.a, -sv * x.b, -sv * x.ab - cv * aa};
}

// ---- the recursion ------------------------------------------------------------------------------------------------------
struct Cst {
  double dt, inv_mt, inv_it, inv_ml, weight;   // weight = (mass_body + mass_leg) gravity
};

__device__ __forceinline__ Cst constants(const rato_hopper_nlp_params& P) {
  Cst c;
  c.dt = P.dt;
  c.inv_mt = 1.0 / (P.mass_body + P.mass_leg);
  c.inv_it = 1.0 / (P.inertia_body + P.inertia_leg);
  c.inv_ml = 1.0 / P.mass_leg;
  c.weight = (P.mass_body + P.mass_leg) * P.gravity;
  return c;
}

// b(x, u) (:218-231); x[0], x[1] are not read
template <class T>
__device__ __forceinline__ void dyn(const Cst& c, const T (&x)[HN_NX], const T (&u)[HN_NU], T (&k)[HN_NX]) {
  T s, cs;
  sincosd(x[2], s, cs);
#pragma unroll
  for (int i = 0; i < 4; ++i) k[i] = x[4 + i];
  k[4] = c.inv_mt * (u[2] - s * u[1]);
  k[5] = c.inv_mt * ((cs * u[1] + u[3]) + (-c.weight));
  k[6] = c.inv_it * (u[0] + x[3] * (cs * u[2] + s * u[3]));
  k[7] = c.inv_ml * ((u[1] + s * u[2]) - cs * u[3]);
}

// x + dt/6 (k1 + 2 k2 + 2 k3 + k4) (:243-247)
template <class T>
__device__ __forceinline__ void rk4(const Cst& c, const T (&x)[HN_NX], const T (&u)[HN_NU], T (&xn)[HN_NX]) {
  T k[HN_NX], y[HN_NX], acc[HN_NX];
  dyn(c, x, u, k);
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) {
    acc[i] = k[i];
    y[i] = x[i] + (0.5 * c.dt) * k[i];
  }
  dyn(c, y, u, k);
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) {
    acc[i] = acc[i] + 2.0 * k[i];
    y[i] = x[i] + (0.5 * c.dt) * k[i];
  }
  dyn(c, y, u, k);
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) {
    acc[i] = acc[i] + 2.0 * k[i];
    y[i] = x[i] + c.dt * k[i];
  }
  dyn(c, y, u, k);
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) xn[i] = x[i] + (c.dt * (1.0 / 6.0)) * (acc[i] + k[i]);
}

__host__ __device__ inline int64_t nvar_min(int S) { return (int64_t)HN_NX * (S + 1) + (int64_t)HN_NU * S; }

// ---- values and first derivatives: one lane per (problem, state, direction of (x_t, u_t)) ----------------------------------
__global__ void __launch_bounds__(HN_BLOCK)
hopper_nlp_linearize_kernel(const rato_hopper_nlp_params P, int64_t n_lanes, const double* __restrict__ Z, int64_t ldz,
                            double* __restrict__ defect, double* __restrict__ d_defect, double* __restrict__ rows,
                            double* __restrict__ d_rows) {
  const int64_t idx = (int64_t)blockIdx.x * HN_BLOCK + threadIdx.x;
  if (idx >= n_lanes) return;              // no barrier below
  const int S = P.S;
  const int d = (int)(idx % HN_NL);
  const int64_t kt = idx / HN_NL;
  const int t = (int)(kt % (S + 1));
  const int64_t k = kt / (S + 1);
  const double* z = Z + k * ldz;
  const double* xt = z + (int64_t)HN_NX * t;

  if (d < 2 && (rows || d_rows)) {         // row d of state t: 0 = J_T q_dot (:288-293), 1 = end-effector height (:166-171)
    const double x2 = xt[2], x3 = xt[3], x6 = xt[6], x7 = xt[7];
    double s, c;
    sincos(x2, &s, &c);
    const int64_t r = (k * (S + 1) + t) * 2 + d;
    if (d == 0) {
      if (rows) rows[r] = xt[4] + (x3 * c) * x6 + s * x7;
      if (d_rows) {
        d_rows[r * 4 + 0] = c * x7 - (x3 * s) * x6;
        d_rows[r * 4 + 1] = c * x6;
        d_rows[r * 4 + 2] = x3 * c;
        d_rows[r * 4 + 3] = s;
      }
    } else {
      if (rows) rows[r] = xt[1] - x3 * c;
      if (d_rows) {
        d_rows[r * 4 + 0] = x3 * s;
        d_rows[r * 4 + 1] = -c;
        d_rows[r * 4 + 2] = 0.0;
        d_rows[r * 4 + 3] = 0.0;
      }
    }
  }
  if (t == S || !(defect || d_defect)) return;

  const Cst c = constants(P);
  const double* ut = z + (int64_t)HN_NX * (S + 1) + (int64_t)HN_NU * t;
  D1 x[HN_NX], u[HN_NU], xn[HN_NX];
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) x[i] = {xt[i], d == i ? 1.0 : 0.0};
#pragma unroll
  for (int i = 0; i < HN_NU; ++i) u[i] = {ut[i], d == HN_NX + i ? 1.0 : 0.0};
  rk4(c, x, u, xn);
  const int64_t row = (k * S + t) * HN_NX;
#pragma unroll
  for (int i = 0; i < HN_NX; ++i) {
    if (d_defect) d_defect[(row + i) * HN_NL + d] = -xn[i].d;
    if (defect && d == 0) defect[row + i] = xt[HN_NX + i] - xn[i].v;
  }
}

// ---- Hessian of lam . g: one lane per (problem, block, pair a >= b of local directions) ------------------------------------
__global__ void __launch_bounds__(HN_BLOCK)
hopper_nlp_hessian_kernel(const rato_hopper_nlp_params P, int64_t n_lanes, const double* __restrict__ Z, int64_t ldz,
                          const double* __restrict__ lam_dyn, const double* __restrict__ lam_rows,
                          const double* __restrict__ add, double* __restrict__ hess_blocks) {
  const int64_t idx = (int64_t)blockIdx.x * HN_BLOCK + threadIdx.x;
  if (idx >= n_lanes) return;              // no barrier below
  const int S = P.S;
  const int e = (int)(idx % HN_PAIRS);
  const int64_t kt = idx / HN_PAIRS;
  const int t = (int)(kt % (S + 1));
  const int64_t k = kt / (S + 1);
  int ra = 0;                              // the row of e in np.tril_indices(12)
  while ((ra + 1) * (ra + 2) / 2 <= e) ++ra;
  const int rb = e - ra * (ra + 1) / 2;    // ra >= rb

  // x0, x1, x4, x5 enter the defect and both rows affinely: no second derivative on a pair that holds one of them
  const unsigned active = 0xfccu;          // bits 2, 3, 6, 7 and the four controls 8..11
  double h = 0.0;
  if (((active >> ra) & 1u) && ((active >> rb) & 1u)) {
    const double* z = Z + k * ldz;
    const double* xt = z + (int64_t)HN_NX * t;
    if (ra < HN_NX) {                      // both directions in x_t: the two state rows (closed forms of :166-171, :288-293)
      const double x3 = xt[3], x6 = xt[6], x7 = xt[7];
      double s, c;
      sincos(xt[2], &s, &c);
      const double* lr = lam_rows + (k * (S + 1) + t) * 2;
      double slip = 0.0, height = 0.0;     // d2 (x4 + x3 c x6 + s x7), d2 (x1 - x3 c) on (ra, rb)
      if (ra == 2 && rb == 2) {
        slip = -(x3 * c) * x6 - s * x7;
        height = x3 * c;
      } else if (ra == 3 && rb == 2) {
        slip = -s * x6;
        height = s;
      } else if (ra == 6 && rb == 2) {
        slip = -x3 * s;
      } else if (ra == 7 && rb == 2) {
        slip = c;
      } else if (ra == 6 && rb == 3) {
        slip = c;
      }
      h = lr[0] * slip + lr[1] * height;
    }
    if (t < S) {                           // the defect of step t
      const Cst c = constants(P);
      const double* ut = z + (int64_t)HN_NX * (S + 1) + (int64_t)HN_NU * t;
      D2 x[HN_NX], u[HN_NU], xn[HN_NX];
#pragma unroll
      for (int i = 0; i < HN_NX; ++i) x[i] = {xt[i], ra == i ? 1.0 : 0.0, rb == i ? 1.0 : 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < HN_NU; ++i) u[i] = {ut[i], ra == HN_NX + i ? 1.0 : 0.0, rb == HN_NX + i ? 1.0 : 0.0, 0.0};
      rk4(c, x, u, xn);
      const double* ld = lam_dyn + (k * S + t) * HN_NX;
      double hd = 0.0;
#pragma unroll
      for (int i = 0; i < HN_NX; ++i) hd += ld[i] * xn[i].ab;
      h -= hd;
    }
  }
  if (add) h += add[idx];
  hess_blocks[idx] = h;
}

// ---- emission: dst[k][map[n]] = scale[n] src[k][n] ---------------------------------------------------------------------------
__global__ void __launch_bounds__(HN_BLOCK)
scatter_f64_kernel(int64_t n, const double* __restrict__ src, int64_t ld_src, const int64_t* __restrict__ map,
                   const double* __restrict__ scale, double* __restrict__ dst, int64_t ld_dst, int64_t n_dst) {
  const int64_t i = (int64_t)blockIdx.x * HN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t m = map[i];
  if (m < 0 || m >= n_dst) return;         // an entry that is not emitted
  const int64_t k = blockIdx.y;
  const double v = src[k * ld_src + i];
  dst[k * ld_dst + m] = scale ? scale[i] * v : v;
}

bool valid(const rato_hopper_nlp_params* p, int32_t K, int64_t ldz) {
  if (!p || K < 1 || p->S < 1) return false;
  if (p->time_jump < 0 || p->time_jump > p->time_land || p->time_land > p->S) return false;
  return ldz >= nvar_min(p->S);
}

// blocks of HN_BLOCK lanes for n lanes, or 0 when the grid would leave the index range
unsigned blocks_for(int64_t n) {
  const int64_t nb = (n + HN_BLOCK - 1) / HN_BLOCK;
  return nb >= 1 && nb <= 0x7fffffff ? (unsigned)nb : 0u;
}

}  // namespace

extern "C" size_t rato_hopper_nlp_params_bytes(void) { return sizeof(rato_hopper_nlp_params); }

extern "C" int rato_hopper_nlp_linearize(const rato_hopper_nlp_params* p, int32_t K, const double* Z, int64_t ldz,
                                         double* defect, double* d_defect, double* rows, double* d_rows, void* stream) {
  if (!valid(p, K, ldz) || !Z) return RATO_EINVAL;
  const int64_t n = (int64_t)K * (p->S + 1) * HN_NL;
  const unsigned nb = blocks_for(n);
  if (!nb) return RATO_EINVAL;
  if (!defect && !d_defect && !rows && !d_rows) return RATO_OK;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(hopper_nlp_linearize_kernel, dim3(nb), dim3(HN_BLOCK), 0, (hipStream_t)stream, *p, n, Z, ldz, defect,
                     d_defect, rows, d_rows);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_nlp_hessian(const rato_hopper_nlp_params* p, int32_t K, const double* Z, int64_t ldz,
                                       const double* lam_dyn, const double* lam_rows, const double* add, double* hess_blocks,
                                       void* stream) {
  if (!valid(p, K, ldz) || !Z || !lam_dyn || !lam_rows || !hess_blocks) return RATO_EINVAL;
  const int64_t n = (int64_t)K * (p->S + 1) * HN_PAIRS;
  const unsigned nb = blocks_for(n);
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(hopper_nlp_hessian_kernel, dim3(nb), dim3(HN_BLOCK), 0, (hipStream_t)stream, *p, n, Z, ldz, lam_dyn,
                     lam_rows, add, hess_blocks);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_scatter_f64(int32_t K, int64_t n, const double* src, int64_t ld_src, const int64_t* map,
                                const double* scale, double* dst, int64_t ld_dst, int64_t n_dst, void* stream) {
  if (K < 1 || K > 65535 || n < 1 || ld_src < n || n_dst < 1 || ld_dst < n_dst || !src || !map || !dst) return RATO_EINVAL;
  const unsigned nb = blocks_for(n);
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(scatter_f64_kernel, dim3(nb, (unsigned)K), dim3(HN_BLOCK), 0, (hipStream_t)stream, n, src, ld_src, map,
                     scale, dst, ld_dst, n_dst);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
