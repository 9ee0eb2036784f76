// Driving Gaussian baseline (car/driving_gaussian.py:115-354): the linearization of the S-step mean / 8x8-covariance
// recursion with respect to the 2S controls and the S risk allocations, in fp64, for K problems in one launch.
//
// Layout: one workgroup per problem, one lane per tangent direction (t', i) = column t'*2+i of the reference's jacfwd
// (:315, reshaped 'C' at :330).  Every lane carries the primal (mean 8, symmetric Sigma 36) AND its own tangent (8 + 36)
// through the sequential recursion in registers: the primal is recomputed by every lane rather than shared, so the kernel
// has no LDS, no barrier and no cross-lane traffic (the fp64 work of the primal is a third of a lane's step, and the lanes
// of a wave run it in lockstep anyway).  All derivatives are closed form; the tangent of A = I + dt db/dx needs the second
// derivatives of b (v cos phi, v sin phi, d/|d|).
//
// The reference's quirks are reproduced on the default path (outer_product = 0), see rato_saa.h.
#include "rato_common.h"
#include "rato_ppnd16.h"

#include <math.h>

namespace {

constexpr int NX = 8;
constexpr int NSYM = NX * (NX + 1) / 2;
constexpr int GAUSS_MAX_S = 64;
constexpr int GAUSS_BLOCK = 2 * GAUSS_MAX_S;

// upper-triangle index of a symmetric 8x8
__host__ __device__ constexpr int sidx(int i, int j) {
  return i <= j ? i * NX - (i * (i - 1)) / 2 + (j - i) : j * NX - (j * (j - 1)) / 2 + (i - j);
}

// The non-constant entries of J = db/dx (:150-153) at one state, and of its directional derivative.
//   rows 0,1:  J02 = cos phi, J03 = -v sin phi, J12 = sin phi, J13 = v cos phi
//   rows 6,7:  J[6:8,0:2] = -G, J[6:8,4:6] = +G with G = omega_r (I - n n^T)/|d| (symmetric), J67 = J77 = -omega_s
//   rows 4,5:  J46 = J57 = 1;  rows 2,3: zero
struct Jac {
  double c, s, mvs, vc;
  double g00, g01, g11;
};

// y = (I + dt J) x
__device__ __forceinline__ void amul(const Jac& J, double ws, double dt, const double (&x)[NX], double (&y)[NX]) {
  const double e0 = x[4] - x[0], e1 = x[5] - x[1];
  y[0] = x[0] + dt * (J.c * x[2] + J.mvs * x[3]);
  y[1] = x[1] + dt * (J.s * x[2] + J.vc * x[3]);
  y[2] = x[2];
  y[3] = x[3];
  y[4] = x[4] + dt * x[6];
  y[5] = x[5] + dt * x[7];
  y[6] = x[6] + dt * (J.g00 * e0 + J.g01 * e1 - ws * x[7]);
  y[7] = x[7] + dt * (J.g01 * e0 + J.g11 * e1 - ws * x[7]);
}

// rows 0, 1, 6, 7 of dt Jdot x (the other rows of Jdot are zero, and so is its omega_s column)
__device__ __forceinline__ void jdmul(const Jac& D, double dt, const double (&x)[NX], double (&y)[4]) {
  const double e0 = x[4] - x[0], e1 = x[5] - x[1];
  y[0] = dt * (D.c * x[2] + D.mvs * x[3]);
  y[1] = dt * (D.s * x[2] + D.vc * x[3]);
  y[2] = dt * (D.g00 * e0 + D.g01 * e1);
  y[3] = dt * (D.g01 * e0 + D.g11 * e1);
}

__global__ void __launch_bounds__(GAUSS_BLOCK)
car_gaussian_linearize_kernel(const rato_car_gauss_params P, const double* __restrict__ us, const double* __restrict__ alphas,
                              double* __restrict__ mus, double* __restrict__ Sigmas, double* __restrict__ g_obs,
                              double* __restrict__ g_obs_du, double* __restrict__ g_obs_dalpha, double* __restrict__ v_final,
                              double* __restrict__ v_final_du) {
  const int S = P.S;
  const int ncol = 2 * S;
  const size_t k = blockIdx.x;
  const int lane = threadIdx.x;
  const bool live = lane < ncol;            // lanes past 2S carry a zero tangent and store nothing
  const bool lead = lane == 0;              // the primal outputs are written once, by lane 0
  const int tp = lane >> 1, ti = lane & 1;  // this lane's tangent direction: d / d u[tp][ti]
  const double dt = P.dt, wsn = P.omega_speed_nom, wrn = P.omega_repulsive_nom;
  const double dt2 = dt * dt;
  const double sig_w = dt * P.beta * P.beta;   // dt sigma sigma^T on the pedestrian velocity block (:204-205)

  us += k * (size_t)S * 2;
  alphas += k * (size_t)S;
  if (mus) mus += k * (size_t)(S + 1) * NX;
  if (Sigmas) Sigmas += k * (size_t)(S + 1) * NX * NX;
  g_obs += k * (size_t)S;
  g_obs_du += k * (size_t)S * ncol;
  g_obs_dalpha += k * (size_t)S;
  v_final += k * 4;
  v_final_du += k * (size_t)4 * ncol;

  double x[NX], xd[NX], sg[NSYM], sd[NSYM];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = P.mean_init[i];
    xd[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < NSYM; ++i) sg[i] = sd[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) sg[sidx(4 + i, 4 + i)] = P.ped_var_init[i];

  if (lead) {
    if (mus) {
#pragma unroll
      for (int i = 0; i < NX; ++i) mus[i] = x[i];
    }
    if (Sigmas) {
#pragma unroll
      for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < NX; ++j) Sigmas[i * NX + j] = sg[sidx(i, j)];
    }
  }

  for (int t = 0; t < S; ++t) {
    const double u0 = us[2 * t], u1 = us[2 * t + 1];

    // ---- the Jacobian of b at (x_t) and its derivative along this lane's tangent --------------------------------
    const double v = x[2], vdot = xd[2], phd = xd[3];
    double sn, cs;
    sincos(x[3], &sn, &cs);
    const double d0 = x[0] - x[4], d1 = x[1] - x[5];
    const double r = sqrt(d0 * d0 + d1 * d1);
    const double ir = 1.0 / r;
    const double n0 = d0 * ir, n1 = d1 * ir;
    const double dd0 = xd[0] - xd[4], dd1 = xd[1] - xd[5];
    const double rdot = n0 * dd0 + n1 * dd1;
    const double nd0 = (dd0 - n0 * rdot) * ir, nd1 = (dd1 - n1 * rdot) * ir;

    Jac J, D;
    J.c = cs;
    J.s = sn;
    J.mvs = -v * sn;
    J.vc = v * cs;
    const double p00 = 1.0 - n0 * n0, p01 = -n0 * n1, p11 = 1.0 - n1 * n1;
    const double wr_r = wrn * ir;
    J.g00 = wr_r * p00;
    J.g01 = wr_r * p01;
    J.g11 = wr_r * p11;
    D.c = -sn * phd;
    D.s = cs * phd;
    D.mvs = -vdot * sn - v * cs * phd;
    D.vc = vdot * cs - v * sn * phd;
    const double rr = rdot * ir;
    D.g00 = -wr_r * (2.0 * nd0 * n0 + p00 * rr);
    D.g01 = -wr_r * (nd0 * n1 + n0 * nd1 + p01 * rr);
    D.g11 = -wr_r * (2.0 * nd1 * n1 + p11 * rr);

    // ---- the term of the uncertain omegas (:207-211) --------------------------------------------------------------
    // b_ds = dt (0,..,0, s, s) with s = speed_des - x7 and b_dr = -dt (0,..,0, n0, n1) are 1-D in the reference, so
    // `b_ds @ b_ds.T` is an inner product and the sum below is ONE scalar, added to all 64 entries (outer_product = 0).
    const double sp = P.speed_ped_des - x[7], spd = -xd[7];
    const double vs2 = P.omega_speed_var * dt2, vr2 = P.omega_repulsive_var * dt2;
    double m66, m67, m77, m66d, m67d, m77d, c_om = 0.0, c_omd = 0.0;
    if (P.outer_product) {
      m66 = vs2 * sp * sp + vr2 * n0 * n0;
      m67 = vs2 * sp * sp + vr2 * n0 * n1;
      m77 = vs2 * sp * sp + vr2 * n1 * n1;
      m66d = 2.0 * vs2 * sp * spd + 2.0 * vr2 * n0 * nd0;
      m67d = 2.0 * vs2 * sp * spd + vr2 * (nd0 * n1 + n0 * nd1);
      m77d = 2.0 * vs2 * sp * spd + 2.0 * vr2 * n1 * nd1;
    } else {
      c_om = 2.0 * vs2 * sp * sp + vr2 * (n0 * n0 + n1 * n1);
      c_omd = 4.0 * vs2 * sp * spd;          // d(n.n) = 0
      m66 = m67 = m77 = c_om;
      m66d = m67d = m77d = c_omd;
    }

    // ---- Sigma+ = A Sigma A^T + dt sigma sigma^T + Sigma_omega and its tangent ------------------------------------
    // T = A Sigma (column j = A Sigma[:, j]); V = Adot T^T has rows 0, 1, 6, 7 only; then
    // Sigma+ = T A^T,  Sigmadot+ = (A Sigmadot) A^T + V + V^T.
    double T[NX][NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double col[NX], y[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = sg[sidx(i, j)];
      amul(J, wsn, dt, col, y);
#pragma unroll
      for (int i = 0; i < NX; ++i) T[i][j] = y[i];
    }
    double V[4][NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double y[4];
      jdmul(D, dt, T[j], y);
#pragma unroll
      for (int a = 0; a < 4; ++a) V[a][j] = y[a];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double y[NX];
      amul(J, wsn, dt, T[i], y);
#pragma unroll
      for (int j = i; j < NX; ++j) {
        double a = y[j];
        if (i == 6 && j == 6) a += sig_w + m66;
        else if (i == 6 && j == 7) a += m67;
        else if (i == 7 && j == 7) a += sig_w + m77;
        else if (!P.outer_product) a += c_om;
        sg[sidx(i, j)] = a;
      }
    }
    // (T is dead from here: U reuses its registers)
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      double col[NX], y[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = sd[sidx(i, j)];
      amul(J, wsn, dt, col, y);
#pragma unroll
      for (int i = 0; i < NX; ++i) T[i][j] = y[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      double y[NX];
      amul(J, wsn, dt, T[i], y);
#pragma unroll
      for (int j = i; j < NX; ++j) {
        double a = y[j];
        // V[row][col] with row in {0,1,6,7} -> slot {0,1,2,3}
        if (i < 2) a += V[i][j];
        else if (i >= 6) a += V[i - 4][j];
        if (j < 2) a += V[j][i];
        else if (j >= 6) a += V[j - 4][i];
        if (i == 6 && j == 6) a += m66d;
        else if (i == 6 && j == 7) a += m67d;
        else if (i == 7 && j == 7) a += m77d;
        else if (!P.outer_product) a += c_omd;
        sd[sidx(i, j)] = a;
      }
    }

    // ---- the mean (Euler, :179-185) and its tangent: xdot+ = A xdot + dt e_{2+i} at t == t' ------------------------
    {
      double y[NX];
      amul(J, wsn, dt, xd, y);
#pragma unroll
      for (int i = 0; i < NX; ++i) xd[i] = y[i];
      const bool mine = live && t == tp;
      xd[2] += (mine && ti == 0) ? dt : 0.0;
      xd[3] += (mine && ti == 1) ? dt : 0.0;
    }
    {
      const double f = wsn * sp;   // the scalar omega_s (speed_des - x7), added to BOTH force components (:126-127)
      const double x6 = x[6], x7 = x[7];
      x[0] += dt * (v * cs);
      x[1] += dt * (v * sn);
      x[2] += dt * u0;
      x[3] += dt * u1;
      x[4] += dt * x6;
      x[5] += dt * x7;
      x[6] += dt * (-wrn * n0 + f);
      x[7] += dt * (-wrn * n1 + f);
    }

    // ---- the chance-constraint row of step t+1 (:238-258) ------------------------------------------------------------
    const double e0 = x[0] - x[4], e1 = x[1] - x[5];
    const double er = sqrt(e0 * e0 + e1 * e1);
    const double ier = 1.0 / er;
    const double m0 = e0 * ier, m1 = e1 * ier;
    const double s44 = sg[sidx(4, 4)], s45 = sg[sidx(4, 5)], s55 = sg[sidx(5, 5)];
    const double a0 = s44 * m0 + s45 * m1, a1 = s45 * m0 + s55 * m1;
    const double w = m0 * a0 + m1 * a1;
    const double sw = sqrt(w);
    const double q = ppnd16(1.0 - alphas[t]);
    const double ed0 = xd[0] - xd[4], ed1 = xd[1] - xd[5];
    const double erd = m0 * ed0 + m1 * ed1;
    const double md0 = (ed0 - m0 * erd) * ier, md1 = (ed1 - m1 * erd) * ier;
    const double wd = 2.0 * (md0 * a0 + md1 * a1) +
                      m0 * m0 * sd[sidx(4, 4)] + 2.0 * m0 * m1 * sd[sidx(4, 5)] + m1 * m1 * sd[sidx(5, 5)];
    if (live) g_obs_du[(size_t)t * ncol + lane] = tp > t ? 0.0 : -erd + q * wd / (2.0 * sw);
    if (lead) {
      g_obs[t] = -(er - q * sw - P.min_separation_distance);
      g_obs_dalpha[t] = -sw * 2.5066282746310002 * exp(0.5 * q * q);   // -sqrt(w) / pdf(q), sqrt(2 pi)
      if (mus) {
#pragma unroll
        for (int i = 0; i < NX; ++i) mus[(size_t)(t + 1) * NX + i] = x[i];
      }
      if (Sigmas) {
#pragma unroll
        for (int i = 0; i < NX; ++i)
#pragma unroll
          for (int j = 0; j < NX; ++j) Sigmas[(size_t)(t + 1) * NX * NX + i * NX + j] = sg[sidx(i, j)];
      }
    }
  }

  if (live) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v_final_du[(size_t)i * ncol + lane] = xd[i];
  }
  if (lead) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v_final[i] = x[i] - P.ego_goal[i];
  }
}

}  // namespace

extern "C" size_t rato_car_gauss_params_bytes(void) { return sizeof(rato_car_gauss_params); }

extern "C" int rato_car_gaussian_linearize(const rato_car_gauss_params* p, int32_t K, const double* us,
                                           const double* alphas_risk, double* mus, double* Sigmas, double* g_obs,
                                           double* g_obs_du, double* g_obs_dalpha, double* v_final, double* v_final_du,
                                           void* stream) {
  if (!p || K < 1 || p->S < 1 || p->S > GAUSS_MAX_S || !us || !alphas_risk || !g_obs || !g_obs_du || !g_obs_dalpha ||
      !v_final || !v_final_du)
    return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  const int block = 2 * p->S <= RATO_WAVE ? RATO_WAVE : GAUSS_BLOCK;
  hipLaunchKernelGGL(car_gaussian_linearize_kernel, dim3((unsigned)K), dim3(block), 0, (hipStream_t)stream, *p, us,
                     alphas_risk, mus, Sigmas, g_obs, g_obs_du, g_obs_dalpha, v_final, v_final_du);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
