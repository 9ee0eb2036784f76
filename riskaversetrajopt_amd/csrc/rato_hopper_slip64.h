// Hopper slip rows in fp64 (hopper/hopper.py:68-81, :300-367, :569-580): the per-lane arithmetic of csrc/hopper_slip64.hip as
// __host__ __device__ functions, so that a host program can execute every lane of both grids (tests/host/hopper_slip64_host.hip).
// Nothing here touches the HIP runtime, LDS or a barrier; the kernels own the launch shape and the order of the sums, and the
// helpers below that fix that order (tile geometry, tree step) are shared with the host program for the same reason.
//
// z = (x_0 .. x_S (8 each), u_0 .. u_{S-1} (4 each), ...) (:105-132).  Contact c sits on step t_c of [0, time_jump) U
// [time_land, S) (:306-311).  h_ic = fx_c - mu_i(p_c) fz_c with p = x0 + x3 sin x2 (:166-171) and
// mu_i(p) = mu_nom + sum_k a_ik cos(theta_ik p + tau_ik) (:75-81).
#ifndef RATO_HOPPER_SLIP64_H
#define RATO_HOPPER_SLIP64_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RATO_S64_HD __host__ __device__ inline
#else
#define RATO_S64_HD inline
#endif

#define RATO_S64_NFEAT 30   /* == RATO_HOPPER_NFEAT */
#define RATO_S64_BLOCK 256  /* lanes of a workgroup of the slip kernel: TI samples x (256 / TI) contacts */
#define RATO_S64_NX 8
#define RATO_S64_NU 4
#define RATO_S64_ENTRIES 9  /* tril entries of a contact's Hessian share: local (x0, x2, x3) and fz */

// ---- launch geometry (host only arithmetic, no device state) ---------------------------------------------------------------
// The workgroup is a TI x TC tile of (sample, contact) pairs, TI = 2^log2 the smallest power of two >= M (at most 256):
// at M = 30 a wave holds 2 contacts x 32 sample lanes (60 of 64 busy), at M >= 256 a workgroup is 256 samples of one contact.
RATO_S64_HD int rato_slip64_log2_ti(int64_t M) {
  int l = 0;
  while (l < 8 && ((int64_t)1 << l) < M) ++l;
  return l;
}
// sample tiles = per-workgroup partial sums per contact
RATO_S64_HD int64_t rato_slip64_nblocks(int64_t M) {
  const int l = rato_slip64_log2_ti(M);
  return (M + ((int64_t)1 << l) - 1) >> l;
}
RATO_S64_HD int rato_slip64_contact_step(int c, int time_jump, int time_land) {
  return c < time_jump ? c : time_land + (c - time_jump);
}

// ---- the sample-independent part of a contact ---------------------------------------------------------------------------------
struct rato_slip64_contact {
  double p;         // end-effector x position x0 + x3 sin x2
  double J[3];      // dp / d(x0, x2, x3) = (1, x3 cos x2, sin x2)
  double s, c, x3;  // sin x2, cos x2 (the curvature of p: H11 = -x3 s, H12 = H21 = c)
  double fx, fz;
};

RATO_S64_HD void rato_slip64_sincos(double x, double& s, double& c) {
  // locals of an inlined function, as in hopper_nlp.hip: the out-pointers are promoted to registers (no private memory)
  double sv, cv;
  sincos(x, &sv, &cv);
  s = sv;
  c = cv;
}

RATO_S64_HD rato_slip64_contact rato_slip64_load_contact(const double* z, int S, int t) {
  const double* x = z + (int64_t)RATO_S64_NX * t;
  const double* u = z + (int64_t)RATO_S64_NX * (S + 1) + (int64_t)RATO_S64_NU * t;
  rato_slip64_contact q;
  q.x3 = x[3];
  rato_slip64_sincos(x[2], q.s, q.c);
  q.p = x[0] + q.x3 * q.s;
  q.J[0] = 1.0;
  q.J[1] = q.x3 * q.c;
  q.J[2] = q.s;
  q.fx = u[2];
  q.fz = u[3];
  return q;
}

// ---- one (sample, contact) lane -----------------------------------------------------------------------------------------------
struct rato_slip64_lane {
  double h, dh_dfz, dh_dp;   // fx - mu fz, -mu, -mu' fz
  double d2h_dpdfz, d2h_dp2; // -mu', -mu'' fz
};

// fields [30][M] (sample i of feature k at k M + i), summed over the features in index order
RATO_S64_HD rato_slip64_lane rato_slip64_eval(const double* a, const double* theta, const double* tau, int64_t M, int64_t i,
                                              double mu_nom, double p, double fx, double fz) {
  double mu = mu_nom, dmu = 0.0, d2mu = 0.0;
  for (int k = 0; k < RATO_S64_NFEAT; ++k) {
    const double ak = a[(int64_t)k * M + i], th = theta[(int64_t)k * M + i], ta = tau[(int64_t)k * M + i];
    double s, c;
    rato_slip64_sincos(th * p + ta, s, c);
    const double ath = ak * th;
    mu += ak * c;
    dmu -= ath * s;
    d2mu -= (ath * th) * c;
  }
  rato_slip64_lane r;
  r.h = fx - mu * fz;
  r.dh_dfz = -mu;
  r.dh_dp = -dmu * fz;
  r.d2h_dpdfz = -dmu;
  r.d2h_dp2 = -d2mu * fz;
  return r;
}

struct rato_slip64_phases {
  int S, time_jump, time_land, C;   // C = time_jump + S - time_land contacts
};

struct rato_slip64_args {
  rato_slip64_phases P;
  double mu_nom;
  int64_t M;
  int log2ti;
  const double* Z;                  // [K][ldz]
  int64_t ldz;
  const double *a, *theta, *tau;    // [30][M], problem k's at + k ldf
  const double* lam;                // [K][ldlam] or NULL, read at lam_r0 + i C + c
  int64_t ldlam, lam_r0;
  double *h, *dh_dfz, *dh_dx;       // [K][C][M], [K][C][M], [K][C][3][M] or NULL
  int64_t ldf;                      // doubles between the fields of problem k and k + 1; 0 (an aggregate's default): shared
};

// The lane (sample i, contact c) of problem k: its stores, its lambda-weighted terms t = (D1, D2, D0 shares; 0 for a lane outside
// the problem) and the running maximum of h.  No barrier, no shared memory.
RATO_S64_HD void rato_slip64_run_lane(const rato_slip64_args& A, int64_t k, int64_t i, int c, double (&t)[3], double& zmax) {
  t[0] = t[1] = t[2] = 0.0;
  const int C = A.P.C;
  if (c >= C || i >= A.M) return;
  const int64_t M = A.M;
  const int step = rato_slip64_contact_step(c, A.P.time_jump, A.P.time_land);
  const rato_slip64_contact q = rato_slip64_load_contact(A.Z + k * A.ldz, A.P.S, step);
  const int64_t fo = k * A.ldf;     // uniform over the workgroup: one problem per blockIdx.z
  const rato_slip64_lane r = rato_slip64_eval(A.a + fo, A.theta + fo, A.tau + fo, M, i, A.mu_nom, q.p, q.fx, q.fz);
  const int64_t row = k * C + c;
  if (A.h) A.h[row * M + i] = r.h;
  if (A.dh_dfz) A.dh_dfz[row * M + i] = r.dh_dfz;
  if (A.dh_dx) {
    double* o = A.dh_dx + row * 3 * M + i;
    o[0] = r.dh_dp * q.J[0];
    o[M] = r.dh_dp * q.J[1];
    o[2 * M] = r.dh_dp * q.J[2];
  }
  zmax = fmax(zmax, r.h);
  if (A.lam) {
    const double l = A.lam[k * A.ldlam + A.lam_r0 + i * C + c];
    t[0] = l * r.d2h_dpdfz;
    t[1] = l * r.d2h_dp2;
    t[2] = l * r.dh_dp;
  }
}

// One step of the workgroup's fixed-order tree over the sample lanes of a contact row: v[tid] += v[tid + half] for the lanes
// whose sample index inside the tile is below half.  The kernel runs it for its own lane between barriers, the host program
// for every lane of the workgroup in turn (a lane below half reads a lane at or above half, which this step does not write).
RATO_S64_HD void rato_slip64_tree_step(double* v, int tid, int ti_mask, int half) {
  if ((tid & ti_mask) < half) v[tid] += v[tid + half];
}

// ---- the contact's share of hess(lam . g): entry e of 9 ----------------------------------------------------------------------
// D = (D1, D2, D0) = sum_i lam (d2h/(dp dfz), d2h/dp2, dh/dp).  Block on (x0, x2, x3): D2 J J' + D0 H; mixed with fz: D1 J.
// -> the value; *pos = its position in np.tril_indices(12) order (local indices 0, 2, 3 of x_t and 11 = fz of u_t)
RATO_S64_HD double rato_slip64_hess_entry(const rato_slip64_contact& q, double D1, double D2, double D0, int e, int* pos) {
  // (row, column) in local (x0, x2, x3) numbering 0..2, row 3 = fz
  const int ra = e < 1 ? 0 : e < 3 ? 1 : e < 6 ? 2 : 3;
  const int rb = e - (e < 1 ? 0 : e < 3 ? 1 : e < 6 ? 3 : 6);
  const int loc_a = ra == 0 ? 0 : ra == 1 ? 2 : ra == 2 ? 3 : 11;
  const int loc_b = rb == 0 ? 0 : rb == 1 ? 2 : 3;
  *pos = loc_a * (loc_a + 1) / 2 + loc_b;
  const double Jb = rb == 0 ? q.J[0] : rb == 1 ? q.J[1] : q.J[2];
  if (ra == 3) return D1 * Jb;
  const double Ja = ra == 0 ? q.J[0] : ra == 1 ? q.J[1] : q.J[2];
  double H = 0.0;
  if (ra == 1 && rb == 1) H = -q.x3 * q.s;
  if (ra == 2 && rb == 1) H = q.c;
  return D2 * (Ja * Jb) + D0 * H;
}

// lane idx of the Hessian-block grid: (problem, contact, entry) = (idx / (9 C), (idx / 9) % C, idx % 9); one writer per entry
RATO_S64_HD void rato_slip64_hess_lane(const rato_slip64_phases& P, int64_t idx, const double* Z, int64_t ldz, const double* D,
                                       double* add) {
  const int e = (int)(idx % RATO_S64_ENTRIES);
  const int64_t kc = idx / RATO_S64_ENTRIES;
  const int c = (int)(kc % P.C);
  const int64_t k = kc / P.C;
  const int t = rato_slip64_contact_step(c, P.time_jump, P.time_land);
  const rato_slip64_contact q = rato_slip64_load_contact(Z + k * ldz, P.S, t);
  const double* d = D + kc * 3;
  int pos;
  const double v = rato_slip64_hess_entry(q, d[0], d[1], d[2], e, &pos);
  add[(k * (P.S + 1) + t) * 78 + pos] += v;
}

#endif /* RATO_HOPPER_SLIP64_H */
