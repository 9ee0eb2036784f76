// Hopper NLP pieces the interior-point driver on the device needs between the launches of csrc/hopper_nlp.hip and
// csrc/hopper_slip64.hip (riskaversetrajopt_amd/hopper_ipm.py: DeviceBackend.eval_full_t / eval_g_t / hess_apply_t; DESIGN
// §7.ah), fp64, K problems per launch:
//   hopper_g_kernel           g in the script's row order (hopper/hopper.py:491-514) from z and what rato_hopper_nlp_linearize
//                             and rato_hopper_slip_f64 left on the device: hopper_ipm.assemble_g without the four downloads
//   hopper_block_symv_kernel  W x with W given as its S + 1 step blocks: hopper_ipm._hess_apply
//
// g.  One lane per row.  Every row but the SAA group's sum row is a copy, a negation or a chain of at most three additions done
// in the host's order -- ((h - t) - y_i) - slack -- so it is bitwise what the host computes from the same pieces.  The sum row
// M alpha t + sum ys has ONE owner, a workgroup of its own behind the row blocks: per-lane partials over i = lane, lane + 256, ...
// ascending, rato::wave_sum_dpp's fixed tree, then the four waves in order (block_sum of ipm_driver.hip).  The order depends on
// M alone: not on K, not on the grid.  No atomics, no scratch, no workspace; the padding behind ncon is never written.
//
// W x.  The blocks hold disjoint variables, so one lane per (problem, block, local row) owns its output entry and sums the 12
// products of its row with the column ascending (the u part of block S does not exist: 8 rows of 8 products).  The entries of
// ys, slack and t_risk, which no block holds, are written +0.
#include "rato_common.h"

namespace {

constexpr int HG_BLOCK = 256;
constexpr int HG_WAVES = HG_BLOCK / RATO_WAVE;
constexpr int HG_NX = 8, HG_NU = 4, HG_NL = HG_NX + HG_NU;
constexpr int HG_PAIRS = HG_NL * (HG_NL + 1) / 2;
static_assert(HG_WAVES == 4, "the sum row combines four waves");

struct GShape {   // the ten groups' offsets (hopper.Model.nlp_layout()["off"]) by arithmetic
  int64_t S, M, C, tj, tl, n_state, nX, nU, nvar;
  int64_t x0, xf, slip, contact, over, risk, n_risk, control, slack, len, ncon;
};

__host__ __device__ inline GShape g_shape(int32_t S, int32_t tj, int32_t tl, int64_t M, int saa) {
  GShape s;
  s.S = S, s.M = M, s.tj = tj, s.tl = tl;
  s.C = tj + (S - tl);
  s.n_state = tj + (S + 1 - tl);
  s.nX = (int64_t)HG_NX * (S + 1), s.nU = (int64_t)HG_NU * S;
  s.nvar = s.nX + s.nU + M + 2;
  s.x0 = (int64_t)HG_NX * S;
  s.xf = s.x0 + HG_NX;
  s.slip = s.xf + 2;
  s.contact = s.slip + s.n_state;
  s.over = s.contact + s.n_state;
  s.risk = s.over + (tl - tj);
  s.n_risk = saa ? 1 + M + M * s.C + 1 : M * s.C;
  s.control = s.risk + s.n_risk;
  s.slack = s.control + s.nU;
  s.len = s.slack + 1;
  s.ncon = s.len + 3 * (int64_t)S;
  return s;
}

__global__ __launch_bounds__(HG_BLOCK) void hopper_g_kernel(rato_hopper_nlp_params p, GShape s, int saa, unsigned row_blocks,
                                                            const double* __restrict__ Z, int64_t ldz,
                                                            const double* __restrict__ defect, const double* __restrict__ rows,
                                                            const double* __restrict__ h, int64_t h_si, int64_t h_sc,
                                                            const double* __restrict__ malpha, double* __restrict__ g,
                                                            int64_t ldg) {
  __shared__ double sh[HG_WAVES];
  const int64_t k = blockIdx.y;
  const double* z = Z + k * ldz;
  double* gk = g + k * ldg;
  const double* ys = z + s.nX + s.nU;
  if (blockIdx.x == row_blocks) {                                  // the sum row's owner (saa only)
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < s.M; i += HG_BLOCK) v += ys[i];
    const int lane = threadIdx.x & (RATO_WAVE - 1), wave = threadIdx.x >> 6;
    v = rato::wave_sum_dpp(v);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) gk[s.risk] = malpha[k] * z[s.nvar - 1] + (((sh[0] + sh[1]) + sh[2]) + sh[3]);
    return;
  }
  const int64_t r = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
  if (r >= s.ncon) return;
  // a state row's state: the contact states [0, tj), then [tl, S]
  auto state_of = [&](int64_t i) { return i < s.tj ? i : s.tl + (i - s.tj); };
  double v;
  if (r < s.x0) {
    v = defect[k * s.x0 + r];
  } else if (r < s.xf) {
    v = z[r - s.x0] - p.state_initial[r - s.x0];
  } else if (r < s.slip) {
    const int64_t j = 4 + (r - s.xf);
    v = z[HG_NX * s.S + j] - p.state_final[j];
  } else if (r < s.contact) {
    v = rows[(k * (s.S + 1) + state_of(r - s.slip)) * 2 + 0];
  } else if (r < s.over) {
    v = rows[(k * (s.S + 1) + state_of(r - s.contact)) * 2 + 1];
  } else if (r < s.risk) {
    v = -rows[(k * (s.S + 1) + s.tj + (r - s.over)) * 2 + 1];
  } else if (r < s.control) {
    const int64_t q = r - s.risk;
    const double slack = z[s.nvar - 2], t_risk = z[s.nvar - 1];
    const double* hk = h + k * s.M * s.C;
    if (!saa) {
      v = hk[(q / s.C) * h_si + (q % s.C) * h_sc] - slack;
    } else if (q == 0) {
      return;                                                      // the sum row: its owner's
    } else if (q <= s.M) {
      v = -ys[q - 1];
    } else if (q < s.n_risk - 1) {
      const int64_t e = q - 1 - s.M, i = e / s.C, c = e % s.C;
      v = ((hk[i * h_si + c * h_sc] - t_risk) - ys[i]) - slack;
    } else {
      v = 0.0;
    }
  } else if (r < s.slack) {
    v = z[s.nX + (r - s.control)];
  } else if (r < s.len) {
    v = z[s.nvar - 2];
  } else {
    const int64_t e = r - s.len, j = e / s.S, t = e % s.S;
    v = z[HG_NX * (t + 1) + (j == 0 ? 3 : j == 1 ? 7 : 6)];
  }
  gk[r] = v;
}

__global__ __launch_bounds__(HG_BLOCK) void hopper_block_symv_kernel(int32_t S, int64_t n, const double* __restrict__ blocks,
                                                                     const double* __restrict__ x, int64_t ldx,
                                                                     double* __restrict__ out, int64_t ldo) {
  const int64_t k = blockIdx.y, nX = (int64_t)HG_NX * (S + 1), nU = (int64_t)HG_NU * S, in_blocks = (int64_t)(S + 1) * HG_NL;
  const int64_t e = (int64_t)blockIdx.x * HG_BLOCK + threadIdx.x;
  if (e >= in_blocks + (n - nX - nU)) return;
  double* ok = out + k * ldo;
  if (e >= in_blocks) {
    ok[nX + nU + (e - in_blocks)] = 0.0;                           // ys, slack, t_risk: in no block
    return;
  }
  const int t = (int)(e / HG_NL), a = (int)(e % HG_NL), width = t < S ? HG_NL : HG_NX;
  if (a >= width) return;                                          // the u part of block S does not exist
  const double* B = blocks + (k * (S + 1) + t) * HG_PAIRS;
  const double* xk = x + k * ldx;
  const double* xx = xk + (int64_t)HG_NX * t;
  const double* xu = xk + nX + (int64_t)HG_NU * t;
  double acc = 0.0;
  for (int b = 0; b < width; ++b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    acc += B[hi * (hi + 1) / 2 + lo] * (b < HG_NX ? xx[b] : xu[b - HG_NX]);
  }
  ok[a < HG_NX ? (int64_t)HG_NX * t + a : nX + (int64_t)HG_NU * t + (a - HG_NX)] = acc;
}

unsigned blocks_for(int64_t n) {
  const int64_t nb = (n + HG_BLOCK - 1) / HG_BLOCK;
  return nb >= 1 && nb < 0x7fffffff ? (unsigned)nb : 0u;
}

}  // namespace

extern "C" int rato_hopper_g_f64(const rato_hopper_nlp_params* p, int32_t K, int64_t M, int32_t saa, const double* Z, int64_t ldz,
                                 const double* defect, const double* rows, const double* h, int64_t h_stride_sample,
                                 int64_t h_stride_contact, const double* malpha, double* g, int64_t ldg, void* stream) {
  if (!p || K < 1 || K > 65535 || p->S < 1 || M < 1 || p->time_jump < 0 || p->time_jump > p->time_land || p->time_land > p->S ||
      !Z || !defect || !rows || !g)
    return RATO_EINVAL;
  const GShape s = g_shape(p->S, p->time_jump, p->time_land, M, saa != 0);
  if (ldz < s.nvar || ldg < s.ncon || (saa && !malpha)) return RATO_EINVAL;
  if (s.C > 0 && (!h || h_stride_sample < 1 || h_stride_contact < 1 ||
                  (M - 1) * h_stride_sample + (s.C - 1) * h_stride_contact > M * s.C - 1))
    return RATO_EINVAL;
  const unsigned nb = blocks_for(s.ncon);
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(hopper_g_kernel, dim3(nb + (saa ? 1u : 0u), (unsigned)K), dim3(HG_BLOCK), 0, (hipStream_t)stream, *p, s,
                     (int)(saa != 0), nb, Z, ldz, defect, rows, h, h_stride_sample, h_stride_contact, malpha, g, ldg);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}

extern "C" int rato_hopper_block_symv_f64(int32_t K, int32_t S, int64_t n, const double* blocks, const double* x, int64_t ldx,
                                          double* out, int64_t ldo, void* stream) {
  if (K < 1 || K > 65535 || S < 1 || !blocks || !x || !out) return RATO_EINVAL;
  const int64_t core = (int64_t)HG_NX * (S + 1) + (int64_t)HG_NU * S;
  if (n < core || ldx < n || ldo < n) return RATO_EINVAL;
  const unsigned nb = blocks_for((int64_t)(S + 1) * HG_NL + (n - core));
  if (!nb) return RATO_EINVAL;
  RATO_CLEAR_ERROR();
  hipLaunchKernelGGL(hopper_block_symv_kernel, dim3(nb, (unsigned)K), dim3(HG_BLOCK), 0, (hipStream_t)stream, S, n, blocks, x, ldx,
                     out, ldo);
  RATO_LAUNCH_CHECK();
  return RATO_OK;
}
