// Batched dense convex QP solver (riskaversetrajopt_amd/qp_ipm.py), fp64: a Mehrotra predictor-corrector interior-point method
// that solves K small QPs  min 1/2 z'P z + q'z, l <= A z <= u  TO COMPLETION in one launch -- one workgroup per problem carries
// the whole loop, no host round trip inside a solve.  It serves the QPs of the driving Gaussian baseline
// (car/driving_gaussian.py:428-456: n = 3S + 1, m = 4S + 5).  The method, its constants and the reasons are in qp_ipm.py and
// DESIGN 7.z; qp_ipm.solve_numpy is the same algorithm on the host.
//
// Storage.  The problem's data (P, q, A) is read where the caller left it (L2 resident: 403 KB of A at the largest size).  The
// condensed matrix Kc (n x n, row-major, leading dimension n) lives in the caller's workspace: its lower triangle is factored in
// place, its strict upper triangle and a diagonal vector in LDS keep the UN-factored, un-regularised matrix -- the retry ladder
// restores the lower triangle from there and the refinement steps multiply by it.  Every vector of the iteration (16 of length
// m, 8 of length n) and the Cholesky's staging tiles live in dynamic LDS.
//
// Termination is structural: the iteration loop and the retry ladder have compile-time caps, every exit decision is read by all
// lanes from one LDS word that one lane wrote before a barrier, and no lane leaves a loop that holds a barrier on its own.
// Determinism: no atomics; every sum has one owner and a fixed order (a lane's own rows in ascending order, then the xor
// butterfly of its wave, then the four waves in order), and nothing a workgroup computes depends on K or on its neighbours, so
// problem k of a batch is bitwise its K = 1 run.
//
// The Cholesky and the triangular solves are the workgroup functions of csrc/rato_chol.h, the ones csrc/chol.hip launches on
// their own: called here because a solve must not leave the workgroup.
#include "rato_chol.h"

#include <math.h>

namespace {

constexpr int QP_BLOCK = 256;
constexpr int QP_MAX_N = 256, QP_MAX_M = 384;
constexpr int QP_HARD_CAP = 200;      // iterations, whatever max_iter says
constexpr int QP_MAX_RETRIES = 12;    // of one factorization
constexpr double QP_DELTA_C = 1e-10, QP_DELTA_W0 = 1e-12, QP_DELTA_W_GROWTH = 100.0;
constexpr double QP_MU_FLOOR = 1e-2;   // the corrector's target is max(sigma mu, QP_MU_FLOOR tol)
constexpr int QP_M_VECS = 16, QP_N_VECS = 8;
constexpr int QP_INFO_WORDS = 8;
constexpr double QP_INF = __builtin_huge_val();
enum { ST_SOLVED = 0, ST_MAX_ITER = 1, ST_NUMERICAL = 2, ST_INVALID = 3 };
enum { HAS_L = 1, HAS_U = 2, IS_EQ = 4 };

__host__ __device__ constexpr int even(int x) { return (x + 1) & ~1; }
// doubles of dynamic LDS: the Cholesky's three staging tiles, the vectors, 8 words of reduction scratch; then 4 int32
__host__ __device__ constexpr size_t lds_bytes(int n, int m) {
  return sizeof(double) * ((size_t)rato::CHOL_LDS_DOUBLES + (size_t)QP_M_VECS * even(m) + (size_t)QP_N_VECS * even(n) + 8) + 16;
}
static_assert((rato::CHOL_NB * rato::CHOL_LD) % 2 == 0 && (rato::CHOL_TILE * rato::CHOL_LD) % 2 == 0,
              "every carve offset is a multiple of 16 bytes");
static_assert(QP_BLOCK == rato::CHOL_BLOCK, "the Cholesky's workgroup");
static_assert(lds_bytes(QP_MAX_N, QP_MAX_M) <= 160 * 1024, "one workgroup's LDS");

__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN

struct Ctx {
  int tid, n, m;
  double* red;       // [8]
  int32_t* word;     // [4]: 0 the loop's control word, 1 the Cholesky's
};

// ---- reductions: the same value in every lane; two barriers each ----------------------------------------------------------
template <int OP>   // 0 sum, 1 max, 2 min
__device__ __forceinline__ double combine(double a, double b) {
  return OP == 0 ? a + b : (OP == 1 ? fmax(a, b) : fmin(a, b));
}
template <int OP>
__device__ __forceinline__ double block_reduce(const Ctx& c, double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = combine<OP>(v, __shfl_xor(v, off, RATO_WAVE));
  if ((c.tid & (RATO_WAVE - 1)) == 0) c.red[c.tid / RATO_WAVE] = v;
  __syncthreads();
  const double r = combine<OP>(combine<OP>(c.red[0], c.red[1]), combine<OP>(c.red[2], c.red[3]));
  __syncthreads();
  return r;
}
// max that keeps a NaN (fmax drops it): a non-finite entry must reach the decision
__device__ __forceinline__ double nanmax(double acc, double v) { return finite(v) ? fmax(acc, fabs(v)) : QP_INF; }

__device__ __forceinline__ int row_kind(double lo, double up) {
  const bool hl = lo > -QP_INF, hu = up < QP_INF;
  if (hl && hu && lo == up) return IS_EQ;
  return (hl ? HAS_L : 0) | (hu ? HAS_U : 0);
}

// ---- matrix-vector products; the caller places the barrier ----------------------------------------------------------------
// out[i] = sum_j A[i][j] x[j], one lane per row, j ascending
__device__ __forceinline__ void rows_matvec(const Ctx& c, const double* __restrict__ A, int64_t lda, const double* x, double* out) {
  for (int i = c.tid; i < c.m; i += QP_BLOCK) {
    const double* a = A + (int64_t)i * lda;
    double s = 0.0;
#pragma unroll 4
    for (int j = 0; j < c.n; ++j) s += a[j] * x[j];
    out[i] = s;
  }
}

struct Vecs {
  double *lo, *up, *sl, *su, *ll, *lu, *rl, *ru, *D, *t, *dsl, *dsu, *dll, *dlu, *cl, *cu;   // m
  double *z, *dz, *rhs, *rd, *diag, *tv;                                                      // n
};

// One Newton step for the complementarity targets in cl / cu: dz, then ds and dlam (dlu carries dy_E on equality rows).
// rl / ru hold r_l and r_u (r_E on equality rows, in ru).  Ends behind a barrier.
__device__ __forceinline__ void newton_step(const Ctx& c, const Vecs& v, const double* __restrict__ A, int64_t lda, const double* Kc) {
  const int tid = c.tid, n = c.n, m = c.m;
  for (int i = tid; i < m; i += QP_BLOCK) {
    const int kind = row_kind(v.lo[i], v.up[i]);
    double g = (kind & IS_EQ) ? v.ru[i] / QP_DELTA_C : 0.0;
    if (kind & HAS_U) g += (v.cu[i] - v.lu[i] * v.ru[i]) / v.su[i];
    if (kind & HAS_L) g -= (v.cl[i] - v.ll[i] * v.rl[i]) / v.sl[i];
    v.t[i] = g;
  }
  __syncthreads();
  for (int j = tid; j < n; j += QP_BLOCK) {        // rhs = -r_d - A'g: one lane per column, rows ascending (coalesced)
    double s = 0.0;
    for (int i = 0; i < m; ++i) s += A[(int64_t)i * lda + j] * v.t[i];
    const double r = -v.rd[j] - s;
    v.rhs[j] = r;
  }
  __syncthreads();
  for (int rep = 0; rep < 3; ++rep) {              // the solve, then two refinement steps against the matrix without delta_w
    for (int a = tid; a < n; a += QP_BLOCK) {      // (its strict upper triangle + diag): tv = rhs - Kc0 dz
      double s = v.rhs[a];
      if (rep > 0) {
        for (int b = 0; b < a; ++b) s -= Kc[(int64_t)b * n + a] * v.dz[b];
        s -= v.diag[a] * v.dz[a];
        for (int b = a + 1; b < n; ++b) s -= Kc[(int64_t)a * n + b] * v.dz[b];
      }
      v.tv[a] = s;
    }
    rato::chol_solve(Kc, n, n, v.tv);
    for (int a = tid; a < n; a += QP_BLOCK) v.dz[a] = rep > 0 ? v.dz[a] + v.tv[a] : v.tv[a];
    __syncthreads();
  }
  rows_matvec(c, A, lda, v.dz, v.t);               // t = A dz (a lane reads back only its own rows below)
  for (int i = tid; i < m; i += QP_BLOCK) {
    const int kind = row_kind(v.lo[i], v.up[i]);
    const double dAz = v.t[i];
    double dsl = 0.0, dsu = 0.0, dll = 0.0, dlu = 0.0;
    if (kind & HAS_L) {
      dsl = dAz + v.rl[i];
      dll = (v.cl[i] - v.ll[i] * dsl) / v.sl[i];
    }
    if (kind & HAS_U) {
      dsu = -dAz + v.ru[i];
      dlu = (v.cu[i] - v.lu[i] * dsu) / v.su[i];
    }
    if (kind & IS_EQ) dlu = (dAz + v.ru[i]) / QP_DELTA_C;
    v.dsl[i] = dsl, v.dsu[i] = dsu, v.dll[i] = dll, v.dlu[i] = dlu;
  }
  __syncthreads();
}

// the largest steps that keep s and lam non-negative (inf when nothing shrinks), and whether every step entry is finite
__device__ __forceinline__ void step_lengths(const Ctx& c, const Vecs& v, double* ap, double* ad, double* nonfinite) {
  double p = QP_INF, d = QP_INF, bad = 0.0;
  for (int i = c.tid; i < c.m; i += QP_BLOCK) {
    const int kind = row_kind(v.lo[i], v.up[i]);
    if (kind & HAS_L) {
      if (v.dsl[i] < 0.0) p = fmin(p, -v.sl[i] / v.dsl[i]);
      if (v.dll[i] < 0.0) d = fmin(d, -v.ll[i] / v.dll[i]);
    }
    if (kind & HAS_U) {
      if (v.dsu[i] < 0.0) p = fmin(p, -v.su[i] / v.dsu[i]);
      if (v.dlu[i] < 0.0) d = fmin(d, -v.lu[i] / v.dlu[i]);
    }
    if (!(finite(v.dsl[i]) && finite(v.dsu[i]) && finite(v.dll[i]) && finite(v.dlu[i]))) bad = 1.0;
  }
  for (int j = c.tid; j < c.n; j += QP_BLOCK)
    if (!finite(v.dz[j])) bad = 1.0;
  *ap = block_reduce<2>(c, p);
  *ad = block_reduce<2>(c, d);
  *nonfinite = block_reduce<1>(c, bad);
}

__global__ __launch_bounds__(QP_BLOCK) void qp_ipm_kernel(
    int32_t n, int32_t m, const double* __restrict__ P_all, int64_t strideP, const double* __restrict__ q_all, int64_t strideq,
    const double* __restrict__ A_all, int64_t lda, int64_t strideA, const double* __restrict__ l_all,
    const double* __restrict__ u_all, int64_t stridelu, double tol, int32_t max_iter, double* __restrict__ z_all, int64_t stridez,
    double* __restrict__ y_all, int64_t stridey, double* __restrict__ info_all, double* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = blockIdx.x, tid = threadIdx.x;
  const double* P = P_all + (int64_t)k * strideP;
  const double* q = q_all + (int64_t)k * strideq;
  const double* A = A_all + (int64_t)k * strideA;
  const double* lg = l_all + (int64_t)k * stridelu;
  const double* ug = u_all + (int64_t)k * stridelu;
  double* zo = z_all + (int64_t)k * stridez;
  double* yo = y_all + (int64_t)k * stridey;
  double* info = info_all + (int64_t)k * QP_INFO_WORDS;
  double* Kc = work + (int64_t)k * n * n;

  double* base = reinterpret_cast<double*>(smem);
  double* Ld = base;
  double* Li = Ld + rato::CHOL_NB * rato::CHOL_LD;
  double* Lj = Li + rato::CHOL_TILE * rato::CHOL_LD;
  double* mv = Ld + rato::CHOL_LDS_DOUBLES;
  const int mp = even(m), np = even(n);
  Vecs v;
  v.lo = mv, v.up = mv + mp, v.sl = mv + 2 * mp, v.su = mv + 3 * mp, v.ll = mv + 4 * mp, v.lu = mv + 5 * mp, v.rl = mv + 6 * mp;
  v.ru = mv + 7 * mp, v.D = mv + 8 * mp, v.t = mv + 9 * mp, v.dsl = mv + 10 * mp, v.dsu = mv + 11 * mp, v.dll = mv + 12 * mp;
  v.dlu = mv + 13 * mp, v.cl = mv + 14 * mp, v.cu = mv + 15 * mp;
  double* nv = mv + QP_M_VECS * mp;
  v.z = nv, v.dz = nv + np, v.rhs = nv + 2 * np, v.rd = nv + 3 * np, v.diag = nv + 4 * np, v.tv = nv + 5 * np;
  double* aI = nv + 6 * np;                         // A_I'y_I, for the stop rule's scale
  Ctx c;
  c.tid = tid, c.n = n, c.m = m;
  c.red = nv + QP_N_VECS * np;
  c.word = reinterpret_cast<int32_t*>(c.red + 8);

  // ---- the data: finite P, q, A; bounds that are no NaN and leave a side to stand on --------------------------------------
  double bad = 0.0, qinf = 0.0;
  for (int e = tid; e < n * n; e += QP_BLOCK)
    if (!finite(P[e])) bad = 1.0;
  for (int j = tid; j < n; j += QP_BLOCK) {
    if (!finite(q[j])) bad = 1.0;
    qinf = fmax(qinf, fabs(q[j]));
  }
  for (int e = tid; e < m * n; e += QP_BLOCK) {
    const int i = e / n, j = e - i * n;
    if (!finite(A[(int64_t)i * lda + j])) bad = 1.0;
  }
  int my_sides = 0;
  for (int i = tid; i < m; i += QP_BLOCK) {
    const double lo = lg[i], up = ug[i];
    if (!(lo <= up) || lo == QP_INF || up == -QP_INF) bad = 1.0;   // (a NaN fails lo <= up)
    v.lo[i] = lo, v.up[i] = up;
    const int kind = row_kind(lo, up);
    my_sides += ((kind & HAS_L) ? 1 : 0) + ((kind & HAS_U) ? 1 : 0);
  }
  bad = block_reduce<1>(c, bad);
  qinf = block_reduce<1>(c, qinf);
  const double nsides = block_reduce<0>(c, (double)my_sides);    // (integers below 2^53: exact in any order)
  if (tid == 0) c.word[0] = bad != 0.0;
  __syncthreads();
  const int invalid = c.word[0];
  __syncthreads();
  const double qnan = __builtin_nan("");
  if (invalid) {                                    // the same word in every lane
    for (int j = tid; j < n; j += QP_BLOCK) zo[j] = qnan;
    for (int i = tid; i < m; i += QP_BLOCK) yo[i] = qnan;
    if (tid == 0) {
      info[0] = ST_INVALID, info[1] = 0.0, info[2] = 0.0, info[3] = qnan, info[4] = qnan, info[5] = qnan, info[6] = 0.0;
      info[7] = qnan;
    }
    return;
  }
  if (tol <= 0.0) tol = 1e-8;
  if (max_iter <= 0) max_iter = 100;
  if (max_iter > QP_HARD_CAP) max_iter = QP_HARD_CAP;

  // ---- start: z = 0, w = A z = 0 moved inside its bounds, slacks from that w, lam = 1 / s clipped, y_E = 0 ----------------
  for (int j = tid; j < n; j += QP_BLOCK) v.z[j] = 0.0;
  for (int i = tid; i < m; i += QP_BLOCK) {
    const double lo = v.lo[i], up = v.up[i];
    const int kind = row_kind(lo, up);
    double sl = 1.0, su = 1.0, ll = 0.0, lu = 0.0, w0 = 0.0;
    const double one_l = 1e-2 * fmax(1.0, fabs(lo)), one_u = 1e-2 * fmax(1.0, fabs(up));
    const bool two = (kind & HAS_L) && (kind & HAS_U);
    const double mar_l = two ? fmin(0.1 * (up - lo), one_l) : one_l, mar_u = two ? mar_l : one_u;
    if (kind & HAS_L) w0 = fmax(w0, lo + mar_l);
    if (kind & HAS_U) w0 = fmin(w0, up - mar_u);
    if (kind & HAS_L) {
      sl = w0 - lo;
      ll = fmin(fmax(1.0 / sl, 1e-2), 1e4);
    }
    if (kind & HAS_U) {
      su = up - w0;
      lu = fmin(fmax(1.0 / su, 1e-2), 1e4);
    }
    v.sl[i] = sl, v.su[i] = su, v.ll[i] = ll, v.lu[i] = lu;
  }
  __syncthreads();

  int status = ST_MAX_ITER, iters = 0, nfact = 0;
  double pres = qnan, dres = qnan, mu = qnan, comp = qnan, dw_last = 0.0;
  for (int it = 0; it <= QP_HARD_CAP; ++it) {
    // ---- residuals ---------------------------------------------------------------------------------------------------------
    rows_matvec(c, A, lda, v.z, v.t);               // t = A z
    double p_loc = 0.0, az_loc = 0.0, mu_loc = 0.0, c_loc = 0.0;
    for (int i = tid; i < m; i += QP_BLOCK) {
      const int kind = row_kind(v.lo[i], v.up[i]);
      const double Az = v.t[i];
      double rl = 0.0, ru = 0.0, sum = 0.0;
      if (kind & HAS_L) {
        rl = (Az - v.lo[i]) - v.sl[i];
        sum += v.sl[i] * v.ll[i];
        c_loc = nanmax(c_loc, v.ll[i] * fabs(Az - v.lo[i]));
      }
      if (kind & HAS_U) {
        ru = (v.up[i] - Az) - v.su[i];
        sum += v.su[i] * v.lu[i];
        c_loc = nanmax(c_loc, v.lu[i] * fabs(v.up[i] - Az));
      }
      if (kind & IS_EQ) ru = Az - v.lo[i];
      v.rl[i] = rl, v.ru[i] = ru;
      mu_loc += sum;
      p_loc = nanmax(nanmax(p_loc, rl), ru);
      az_loc = nanmax(az_loc, Az);
    }
    __syncthreads();
    double d_loc = 0.0, pz_loc = 0.0, ai_loc = 0.0;
    for (int j = tid; j < n; j += QP_BLOCK) {       // one lane per column: P z (P symmetric: column reads), A_I'y_I, A_E'y_E
      double pz = 0.0, sI = 0.0, sE = 0.0;
      for (int b = 0; b < n; ++b) pz += P[(int64_t)b * n + j] * v.z[b];
      for (int i = 0; i < m; ++i) {
        const int kind = row_kind(v.lo[i], v.up[i]);
        const double a = A[(int64_t)i * lda + j];
        if (kind & IS_EQ) sE += a * v.lu[i];
        else sI += a * (v.lu[i] - v.ll[i]);
      }
      const double rd = pz + q[j] + (sI + sE);
      v.rd[j] = rd;
      aI[j] = sI;
      d_loc = nanmax(d_loc, rd);
      pz_loc = nanmax(pz_loc, pz);
      ai_loc = nanmax(ai_loc, sI);
    }
    pres = block_reduce<1>(c, p_loc);
    dres = block_reduce<1>(c, d_loc);
    const double az_inf = block_reduce<1>(c, az_loc), pz_inf = block_reduce<1>(c, pz_loc), ai_inf = block_reduce<1>(c, ai_loc);
    const double mu_sum = block_reduce<0>(c, mu_loc);
    comp = block_reduce<1>(c, c_loc);
    mu = nsides > 0.0 ? mu_sum / nsides : 0.0;
    if (tid == 0) {
      int w = 0;
      if (!(finite(pres) && finite(dres) && finite(mu) && finite(comp))) w = 1 + ST_NUMERICAL;
      else if (pres <= tol * (1.0 + az_inf) && mu <= tol && comp <= tol && dres <= tol * (1.0 + fmax(fmax(pz_inf, qinf), ai_inf))) w = 1 + ST_SOLVED;
      else if (it >= max_iter) w = 1 + ST_MAX_ITER;
      c.word[0] = w;
    }
    __syncthreads();
    const int w = c.word[0];
    if (w) {
      status = w - 1;
      break;
    }
    // ---- Kc0 = P + A' D A (D = lam_l / s_l + lam_u / s_u, 1 / delta_c on equalities): lower and mirrored upper triangle ------
    for (int i = tid; i < m; i += QP_BLOCK) {
      const int kind = row_kind(v.lo[i], v.up[i]);
      double d = (kind & IS_EQ) ? 1.0 / QP_DELTA_C : 0.0;
      if (kind & HAS_L) d += v.ll[i] / v.sl[i];
      if (kind & HAS_U) d += v.lu[i] / v.su[i];
      v.D[i] = d;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += QP_BLOCK) {
      const int a = e / n, b = e - a * n;
      if (b > a) continue;
      double acc = P[(int64_t)a * n + b];
      for (int r = 0; r < m; ++r) {
        const double ara = A[(int64_t)r * lda + a];
        if (ara != 0.0) acc += (ara * v.D[r]) * A[(int64_t)r * lda + b];   // (a zero term adds nothing: bound rows are unit rows)
      }
      if (a == b) v.diag[a] = acc;
      else Kc[(int64_t)b * n + a] = acc;
    }
    __syncthreads();
    // ---- factor Kc0 + delta_w I, delta_w x 100 while a pivot fails ---------------------------------------------------------------
    double dw = QP_DELTA_W0;
    int ok = 0;
    for (int attempt = 0; attempt <= QP_MAX_RETRIES; ++attempt) {
      for (int e = tid; e < n * n; e += QP_BLOCK) {
        const int a = e / n, b = e - a * n;
        if (b < a) Kc[(int64_t)a * n + b] = Kc[(int64_t)b * n + a];
        else if (b == a) Kc[(int64_t)a * n + a] = v.diag[a] + dw;
      }
      __syncthreads();
      ok = rato::chol_factor(Kc, n, n, Ld, Li, Lj, c.word + 1) == 0;   // the same in every lane
      ++nfact;
      dw_last = dw;
      if (ok) break;
      dw *= QP_DELTA_W_GROWTH;
    }
    if (!ok) {
      status = ST_NUMERICAL;
      break;
    }
    // ---- affine step (pass 0: c = -s lam), then the corrector (pass 1: c = target - s lam - ds_aff dlam_aff) ----------------
    double ap = 0.0, ad = 0.0, nonfinite = 0.0, sigma = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int i = tid; i < m; i += QP_BLOCK) {
        double cl = -v.sl[i] * v.ll[i], cu = -v.su[i] * v.lu[i];
        if (pass) {
          const double target = fmax(sigma * mu, QP_MU_FLOOR * tol);   // (no use in shrinking mu far below tol: qp_ipm.py)
          cl = target + cl - v.dsl[i] * v.dll[i];
          cu = target + cu - v.dsu[i] * v.dlu[i];
        }
        v.cl[i] = cl, v.cu[i] = cu;
      }
      __syncthreads();
      newton_step(c, v, A, lda, Kc);
      step_lengths(c, v, &ap, &ad, &nonfinite);
      if (pass == 0) {
        ap = fmin(1.0, ap), ad = fmin(1.0, ad);
        double aff = 0.0;
        for (int i = tid; i < m; i += QP_BLOCK) {
          const int kind = row_kind(v.lo[i], v.up[i]);
          double sum = 0.0;
          if (kind & HAS_L) sum += (v.sl[i] + ap * v.dsl[i]) * (v.ll[i] + ad * v.dll[i]);
          if (kind & HAS_U) sum += (v.su[i] + ap * v.dsu[i]) * (v.lu[i] + ad * v.dlu[i]);
          aff += sum;
        }
        aff = block_reduce<0>(c, aff);
        if (nsides > 0.0 && mu > 0.0) {
          const double r = (aff / nsides) / mu;
          sigma = r * r * r;
        }
      }
    }
    const double tau = fmax(0.995, 1.0 - mu);
    ap = fmin(1.0, tau * ap), ad = fmin(1.0, tau * ad);
    if (tid == 0) c.word[0] = !(nonfinite == 0.0 && finite(ap) && finite(ad));
    __syncthreads();
    const int stop = c.word[0];
    __syncthreads();
    if (stop) {                                      // the iterate stays the last finite one
      status = ST_NUMERICAL;
      break;
    }
    for (int j = tid; j < n; j += QP_BLOCK) v.z[j] += ap * v.dz[j];
    for (int i = tid; i < m; i += QP_BLOCK) {
      const int kind = row_kind(v.lo[i], v.up[i]);
      if (kind & HAS_L) {
        v.sl[i] += ap * v.dsl[i];
        v.ll[i] += ad * v.dll[i];
      }
      if (kind & HAS_U) v.su[i] += ap * v.dsu[i];
      if (kind & (HAS_U | IS_EQ)) v.lu[i] += ad * v.dlu[i];
    }
    iters = it + 1;
    __syncthreads();
  }
  __syncthreads();
  for (int j = tid; j < n; j += QP_BLOCK) zo[j] = v.z[j];
  for (int i = tid; i < m; i += QP_BLOCK) {
    const int kind = row_kind(v.lo[i], v.up[i]);
    yo[i] = (kind & IS_EQ) ? v.lu[i] : v.lu[i] - v.ll[i];
  }
  if (tid == 0) {
    info[0] = status, info[1] = iters, info[2] = nfact, info[3] = pres, info[4] = dres, info[5] = mu, info[6] = dw_last;
    info[7] = comp;
  }
}

}  // namespace

extern "C" size_t rato_qp_ipm_workspace_bytes(int32_t K, int32_t n, int32_t m) {
  if (K < 1 || n < 1 || m < 0) return 0;
  return (size_t)K * (size_t)n * (size_t)n * sizeof(double);
}

extern "C" int rato_qp_ipm_batch_f64(int32_t K, int32_t n, int32_t m, const double* P, int64_t strideP, const double* q,
                                     int64_t strideq, const double* A, int64_t lda, int64_t strideA, const double* l,
                                     const double* u, int64_t stridelu, double tol, int32_t max_iter, double* z, int64_t stridez,
                                     double* y, int64_t stridey, double* info, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (K < 1 || K > 65535 || n < 1 || n > QP_MAX_N || m < 0 || m > QP_MAX_M || !P || !q || !z || !y || !info || !workspace ||
      (m > 0 && (!A || !l || !u)) || lda < n || (strideP != 0 && strideP < (int64_t)n * n) || (strideq != 0 && strideq < n) ||
      (m > 0 && (strideA < (int64_t)m * lda || stridelu < m)) || stridez < n || stridey < m || !(tol == tol) ||
      workspace_bytes < rato_qp_ipm_workspace_bytes(K, n, m))
    return RATO_EINVAL;
  static rato::DynamicLdsLimit limit;
  return rato::launch_dynamic_lds(qp_ipm_kernel, limit, lds_bytes(QP_MAX_N, QP_MAX_M), lds_bytes(n, m), dim3((unsigned)K),
                                  dim3(QP_BLOCK), (hipStream_t)stream, n, m, P, strideP, q, strideq, A, lda, strideA, l, u,
                                  stridelu, tol, max_iter, z, stridez, y, stridey, info, static_cast<double*>(workspace));
}
