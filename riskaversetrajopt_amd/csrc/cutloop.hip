// Host side of the boundary, continued (nnls.hip, master.hip): the CUTTING-PLANE LOOP of one reduced SCP subproblem as
// ONE library call -- HOST code only; the device work it issues is the table-free cut oracle of cvar.hip.
//
// The reference hands every SCP subproblem to OSQP as one QP with M auxiliary variables (drone_risk.py:425-469,
// driving.py:423-456).  Here the subproblem is that QP reduced exactly to (u, slack) (riskaversetrajopt_amd/cvar_cuts.py
// has the derivation) and solved by Kelley cuts: master QP on the host (rato_master_*), oracle on the device
// (rato_cut_oracle_rollout: rowmax -> exact tail selection -> tail-row sums -> read-back, one round trip per cut).
// Round 3 drove that loop from Python (cvar_cuts.CvarCutSolver._solve): ~20 ms of interpreter time per 60 SCP iterations
// against ~35 ms of device time.  This file is the same loop, statement for statement -- lazy control bounds, the "last
// cut joins the master" rule, the keep rule for recycled cuts, the multipliers for the KKT certificate -- so that ONE
// ctypes call per subproblem remains (rato_cut_begin is its stream-ordered prologue).  The Python loop stays as the
// implementation for sharded batches and the table forms of the oracle, and as the checker: both produce BITWISE the
// same iterates (tests/test_gpu_scp.py), which is why every inner product that feeds the master is an exactly rounded
// sum here and there (fsum below == math.fsum).
#pragma clang fp contract(off)   // the exactly-rounded sums below must see individually rounded products

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "rato_common.h"
#include "rato_saa.h"
#include "rato_select.h"

namespace {

// Shewchuk's exact summation (the algorithm of CPython's math.fsum, Modules/mathmodule.c): the correctly rounded value
// of the exact sum of the inputs -- independent of their order, hence identical to math.fsum on the same numbers.
double fsum(const double* v, int n) {
  std::vector<double> p;
  p.reserve(32);
  for (int k = 0; k < n; ++k) {
    double x = v[k];
    size_t i = 0;
    for (size_t j = 0; j < p.size(); ++j) {
      double y = p[j];
      if (fabs(x) < fabs(y)) std::swap(x, y);
      const double hi = x + y;
      const double lo = y - (hi - x);
      if (lo != 0.0) p[i++] = lo;
      x = hi;
    }
    p.resize(i);
    p.push_back(x);
  }
  double hi = 0.0;
  size_t n_p = p.size();
  if (n_p > 0) {
    hi = p[--n_p];
    double lo = 0.0;
    while (n_p > 0) {
      const double x = hi;
      const double y = p[--n_p];
      hi = x + y;
      const double yr = hi - x;
      lo = y - yr;
      if (lo != 0.0) break;
    }
    // round half to even across the remaining partials
    if (n_p > 0 && ((lo < 0.0 && p[n_p - 1] < 0.0) || (lo > 0.0 && p[n_p - 1] > 0.0))) {
      const double y = lo * 2.0;
      const double x = hi + y;
      const double yr = x - hi;
      if (y == yr) hi = x;
    }
  }
  return hi;
}

double dot_exact(const double* a, const double* b, int n, std::vector<double>& prod) {
  prod.resize(n);
  for (int i = 0; i < n; ++i) prod[i] = a[i] * b[i];
  return fsum(prod.data(), n);
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

struct rato_cut_solver {
  rato_cut_config c;
  rato_drone_params drone = {};
  rato_car_params car = {};
  int nU = 0, n = 0, nc = 0, nres = 0, nblk = 0;
  std::vector<double> p_diag, q;
  hipEvent_t sums_ready = nullptr;   // rato_cut_define_drone: recorded behind the linearization's sample sums (lazily created)
  bool kept_armed = false;           // sums_b_host was pre-set before the kept cuts' launch in flight (readback_arm): the wait may watch it
  const void* params() const { return c.system == 0 ? (const void*)&drone : (const void*)&car; }
  ~rato_cut_solver() {
    if (sums_ready) (void)hipEventDestroy(sums_ready);
  }
};

extern "C" int rato_cut_solver_create(rato_cut_solver** out, const rato_cut_config* cfg) {
  if (!out || !cfg) return RATO_EINVAL;
  const rato_cut_config& c = *cfg;
  if ((c.system != 0 && c.system != 1) || !c.params || c.S < 1 || c.M < 1 || c.cap < 2 || c.keep_max < 0 ||
      c.keep_recent < 0 || c.keep_idle < 0 || !(c.alphaM > 0.0) || !c.s0 || !c.s1 || !c.s2 || (c.system == 1 && !c.s3) ||
      !c.uk_dev || !c.uk_host || !c.x_host || !c.x_dev || !c.ring_m || !c.ring_arg || !c.ring_res || !c.workspace ||
      !c.res_host || !c.p_diag || !c.q)
    return RATO_EINVAL;
  if (c.S > 1 && (!c.part || (c.keep_max > 0 && (!c.part_b || !c.sums_b_host || !c.slots_dev || !c.slots_host))))
    return RATO_EINVAL;
  rato_cut_solver* s = new rato_cut_solver;
  s->c = c;
  int n_u;
  if (c.system == 0) {
    s->drone = *static_cast<const rato_drone_params*>(c.params);
    if (s->drone.S != c.S || s->drone.M != c.M) { delete s; return RATO_EINVAL; }
    n_u = 3;
  } else {
    s->car = *static_cast<const rato_car_params*>(c.params);
    if (s->car.S != c.S || s->car.M != c.M) { delete s; return RATO_EINVAL; }
    n_u = 2;
  }
  s->nU = n_u * c.S;
  s->n = s->nU + 1;
  s->nres = rato::record_words(c.S);
  s->nc = s->nres - RATO_N_STATS;
  s->nblk = (int)((c.M + 255) / 256);
  s->p_diag.assign(c.p_diag, c.p_diag + s->n);
  s->q.assign(c.q, c.q + s->n);
  s->c.params = nullptr;   // (the copy above is what is used)
  *out = s;
  return RATO_OK;
}

extern "C" void rato_cut_solver_destroy(rato_cut_solver* s) { delete s; }

extern "C" size_t rato_cut_config_bytes(void) { return sizeof(rato_cut_config); }
extern "C" size_t rato_cut_result_bytes(void) { return sizeof(rato_cut_result); }

namespace {

int tail_rows_launch(rato_cut_solver* s, const float* m_base, const int32_t* arg_base, const double* res_base,
                     const int32_t* slots, int K, double* part, void* stream) {
  const rato_cut_config& c = s->c;
  return c.system == 0 ? rato_drone_tail_rows_rollout(&s->drone, c.uk_dev, c.s0, c.s1, c.s2, m_base, arg_base, res_base,
                                                      s->nres, slots, K, c.alphaM, part, stream)
                       : rato_car_tail_rows_rollout(&s->car, c.uk_dev, c.s0, c.s1, c.s2, c.s3, m_base, arg_base,
                                                    res_base, s->nres, slots, K, c.alphaM, part, stream);
}

// u_k, the controls and the kept slots reach the device IN THE ARGUMENTS of one small launch: an asynchronous copy of a
// kilobyte costs ~25 us of host time on this stack (the define issued three), a launch ~5.
constexpr int STAGE_MAX = 192, STAGE_SLOTS = 64;
struct StageArgs {
  double uk[STAGE_MAX];
  float us[STAGE_MAX];
  int32_t slots[STAGE_SLOTS];
};
__global__ void cut_stage_kernel(const StageArgs a, int n_uk, int n_us, int n_slots, double* __restrict__ uk_dev,
                                 float* __restrict__ us_dev, int32_t* __restrict__ slots_dev) {
  const int i = threadIdx.x;
  if (i < n_uk) uk_dev[i] = a.uk[i];
  if (i < n_us) us_dev[i] = a.us[i];
  if (i < n_slots) slots_dev[i] = a.slots[i];
}

// u_lin -> uk_dev (fp64), us (optional) -> us_dev (fp32), keep -> slots_dev: one launch when they fit its arguments
int stage_inputs(rato_cut_solver* s, const double* u_lin, const float* us_f32, float* us_dev, const int32_t* keep, int n_keep,
                 hipStream_t st) {
  const rato_cut_config& c = s->c;
  const int nU = s->nU;
  if (nU <= STAGE_MAX && n_keep <= STAGE_SLOTS) {
    StageArgs a;
    memcpy(a.uk, u_lin, sizeof(double) * (size_t)nU);
    if (us_f32) memcpy(a.us, us_f32, sizeof(float) * (size_t)nU);
    for (int k = 0; k < n_keep; ++k) a.slots[k] = keep[k];
    hipLaunchKernelGGL(cut_stage_kernel, dim3(1), dim3(STAGE_MAX), 0, st, a, nU, us_f32 ? nU : 0, n_keep, c.uk_dev, us_dev,
                       c.slots_dev);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RATO_OK : RATO_EHIP - (int)e;
  }
  memcpy(c.uk_host, u_lin, sizeof(double) * (size_t)nU);
  hipError_t e = hipMemcpyAsync(c.uk_dev, c.uk_host, sizeof(double) * (size_t)nU, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return RATO_EHIP - (int)e;
  if (us_f32) {   // (us_f32 is the caller's pinned buffer)
    e = hipMemcpyAsync(us_dev, us_f32, sizeof(float) * (size_t)nU, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
  }
  if (n_keep > 0) {
    for (int k = 0; k < n_keep; ++k) c.slots_host[k] = keep[k];
    e = hipMemcpyAsync(c.slots_dev, c.slots_host, sizeof(int32_t) * (size_t)n_keep, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
  }
  return RATO_OK;
}

// the kept cuts' tail-row sums under the linearization point staged last, reduced into pinned host memory
int kept_cuts_launch(rato_cut_solver* s, int n_keep, void* stream) {
  const rato_cut_config& c = s->c;
  if (n_keep == 0 || c.S < 2) return RATO_OK;
  int rc = tail_rows_launch(s, c.ring_m, c.ring_arg, c.ring_res, c.slots_dev, n_keep, c.part_b, stream);
  if (rc != RATO_OK) return rc;
  return rato_sum_partials_f64(c.part_b, s->nblk, n_keep * s->nc, 1.0, c.sums_b_host, stream);
}

// A kept-cuts launch is still marked in flight (define / begin followed by another define / begin without the solve that
// waits for it): let it finish before its pinned words are pre-set again -- a late write of the OLD launch would
// otherwise satisfy the NEW wait with stale sums.  Clears the mark whatever happens.
int settle_kept(rato_cut_solver* s, hipStream_t st) {
  if (!s->kept_armed) return RATO_OK;
  s->kept_armed = false;
  const hipError_t e = hipStreamSynchronize(st);
  return e == hipSuccess ? RATO_OK : RATO_EHIP - (int)e;
}

// the kept cuts as every entry takes them: a count within keep_max and ring slots below the scratch slot (cap - 1).  The
// slots are checked at S = 1 too, where nothing re-linearizes them: CutLoop::init indexes host tables with them regardless.
bool keep_args_ok(const rato_cut_solver* s, const int32_t* keep, int n_keep) {
  if (n_keep < 0 || n_keep > s->c.keep_max || (n_keep > 0 && !keep)) return false;
  for (int k = 0; k < n_keep; ++k)
    if (keep[k] < 0 || keep[k] >= s->c.cap - 1) return false;
  return true;
}

// are there kept cuts to re-linearize?  (no control enters the only row of S = 1: its cuts have no rows)
bool with_cuts(const rato_cut_solver* s, int n_keep) { return n_keep > 0 && s->c.S >= 2; }

}  // namespace

// Stream-ordered prologue of a subproblem: u_k -> device (fp64), and -- when cuts were kept from the previous
// subproblem -- their tail-row sums under the NEW linearization point, reduced straight into pinned host memory
// (sums_b_host).  Nothing is synchronised: the caller's own read-back of the linearization's sample sums waits for
// this work too (one device round trip per "define" instead of two).
extern "C" int rato_cut_begin(rato_cut_solver* s, const double* u_lin, const int32_t* keep, int32_t n_keep, void* stream) {
  if (!s || !u_lin || !keep_args_ok(s, keep, n_keep)) return RATO_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int n_cuts = with_cuts(s, n_keep) ? n_keep : 0;
  int rc = settle_kept(s, st);
  if (rc != RATO_OK) return rc;
  rc = stage_inputs(s, u_lin, nullptr, nullptr, keep, n_cuts, st);
  if (rc != RATO_OK) return rc;
  const bool arm_kept = n_cuts > 0 && rato::readback_poll_enabled();
  if (arm_kept) rato::readback_arm(s->c.sums_b_host, n_cuts * s->nc);
  rc = kept_cuts_launch(s, n_cuts, stream);
  s->kept_armed = arm_kept && rc == RATO_OK;   // armed words with nothing launched behind them are never waited for
  return rc;
}

// The "define" half of a reduced SCP iteration of the DRONE as one call (table-free oracle: no linearization table is
// kept): the controls to the device, the generators-only linearization at them (what is left of it here: the sample
// sums of the final rows and Z), the reduction of those sums straight into PINNED host memory, the count of
// non-finite outputs, rato_cut_begin (u_k in fp64 + the kept cuts against it) and ONE synchronisation.  Round 3 issued
// these from Python: ~0.15 ms of interpreter time per SCP iteration around 0.1 ms of device work.
//   us [S][3] doubles (host);  us_host (pinned) / us_dev: [S][3] floats;  A22 [S][3][ld] floats (the kernel's scratch);
//   Z [ld] or NULL (nothing downstream of this call reads it: without it no obstacle row is formed at all);
//   part [ceil(M/256)][6S+6] floats;  sums_host (pinned): 6S+6 doubles (sums, not means);
//   bad_dev / bad_host (pinned): one uint32 each, or both NULL (no non-finite check).
extern "C" int rato_cut_define_drone(rato_cut_solver* s, const double* us, float* us_host, float* us_dev, float* A22,
                                     float* Z, int64_t z_floats, float* part, double* sums_host, uint32_t* bad_dev,
                                     uint32_t* bad_host, const int32_t* keep, int32_t n_keep, void* stream) {
  if (!s || s->c.system != 0 || !us || !us_host || !us_dev || !A22 || !part || !sums_host || (!bad_dev != !bad_host) ||
      (bad_dev && !Z) || (Z && z_floats < s->c.M) || !keep_args_ok(s, keep, n_keep))
    return RATO_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nU = s->nU, S = s->c.S, ncols = 6 * S + 6;
  const int n_cuts = with_cuts(s, n_keep) ? n_keep : 0;
  for (int i = 0; i < nU; ++i) us_host[i] = (float)us[i];
  hipError_t e = hipSuccess;
  // the sample sums land in pinned memory and are watched for (rato_common.h: readback_*); with the non-finite count
  // (a copy node behind them) the event below is waited for instead
  const bool watch = rato::readback_poll_enabled() && !bad_dev;
  int rc = settle_kept(s, st);   // a kept-cuts launch nobody waited for must not write into words armed anew
  if (rc != RATO_OK) return rc;
  if (watch) rato::readback_arm(sums_host, ncols);
  const bool arm_kept = n_cuts > 0 && rato::readback_poll_enabled();
  if (arm_kept) rato::readback_arm(s->c.sums_b_host, n_cuts * s->nc);   // (kept_armed only once the launch is out)
  rc = stage_inputs(s, us, us_host, us_dev, keep, n_cuts, st);   // us, u_k (fp64) and the kept slots: one launch
  if (rc != RATO_OK) return rc;
  rc = rato_drone_linearize_generators(&s->drone, us_dev, s->c.s0, s->c.s1, s->c.s2, A22, nullptr, nullptr, Z, part,
                                           stream);
  if (rc != RATO_OK) return rc;
  if ((rc = rato_sum_partials(part, s->nblk, ncols, 1.0, sums_host, stream)) != RATO_OK) return rc;
  if (bad_dev) {
    if ((rc = rato_count_nonfinite(Z, z_floats, bad_dev, stream)) != RATO_OK) return rc;
    if ((rc = rato_count_nonfinite_acc(part, (int64_t)s->nblk * ncols, bad_dev, stream)) != RATO_OK) return rc;
    e = hipMemcpyAsync(bad_host, bad_dev, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
  }
  // The host continues (sample sums -> equality rows -> the master's factorisation) as soon as the SUMS are back; the kept
  // cuts' re-linearization behind them is waited for by rato_cut_solve(kept_in_flight = 1), after it has built the master.
  if (!watch) {
    if (!s->sums_ready) {
      e = hipEventCreateWithFlags(&s->sums_ready, hipEventDisableTiming);
      if (e != hipSuccess) return RATO_EHIP - (int)e;
    }
    e = hipEventRecord(s->sums_ready, st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
  }
  if ((rc = kept_cuts_launch(s, n_cuts, stream)) != RATO_OK) return rc;
  s->kept_armed = arm_kept;
  e = watch ? rato::readback_wait(sums_host, ncols, st) : hipEventSynchronize(s->sums_ready);
  if (e != hipSuccess) return RATO_EHIP - (int)e;
  if (bad_host && *bad_host) return RATO_ENONFINITE;
  return RATO_OK;
}

namespace {

// One subproblem's cutting-plane loop as a RESUMABLE state: what rato_cut_solve runs start to end with the oracle round trip
// in the middle, cut at the round trip so that a batch (rato_scp_batch_run_drone) can issue the round trips of many
// subproblems as one.  init: the equality rows (+ the slack row) into a fresh master;  add_kept: the rows of the cuts kept
// from the previous subproblem, from their sums under the new linearization point;  begin: the first master solve and the
// first query;  then, while !done: x (u - u_k) and ring (the slot the round trip writes) are the query, consume(record)
// takes the round trip's record and runs the master up to the next query;  finish: the keep rule and the outputs.  The
// statements are those of the loop as it was written in one piece -- same order, same arithmetic: the iterates of
// rato_cut_solve did not change bit for bit (tests/test_gpu_scp.py).  No state outside the object (and the solver's
// read-only configuration) is touched: the masters of a batch run on several host threads.
struct CutLoop {
  struct BoundRows {
    int r0;
    std::vector<int> idx;
    double sgn;
  };
  const rato_cut_solver* s = nullptr;
  const double* u_lin = nullptr;
  bool cvar = false, slack_row = false, check_finite = false, done = false, have_prev = false;
  double tol = 0.0, final_cut_above = 0.0, phi = NAN, tstar = NAN, oracle_s = 0.0, master_s = 0.0;
  int max_cuts = 0, nU = 0, n = 0, S = 0, nc = 0, n_u = 0, n_rows = 0, n_kept = 0, n_cuts = 0, status = 0, it = 0, slot = -1,
      ring = -1;
  int32_t *keep = nullptr, *keep_idle_count = nullptr, *n_keep_io = nullptr;
  rato_master* master = nullptr;
  std::vector<double> prod, row, g, x, z, lam, z_prev;
  std::vector<std::pair<int, int>> cut_rows;   // (row of the master, ring slot)
  std::vector<int> free_slots;                 // ascending; the loop takes from the back
  std::vector<uint8_t> in_master;
  std::vector<BoundRows> bound_rows;

  CutLoop() = default;
  CutLoop(const CutLoop&) = delete;
  CutLoop& operator=(const CutLoop&) = delete;
  ~CutLoop() { rato_master_destroy(master); }

  int init(const rato_cut_solver* sv, const double* final_du, const double* final_rhs, int n_c, const double* u_lin_,
           bool with_cvar, double tol_, int max_cuts_, double final_cut_above_, bool check_finite_, int32_t* keep_,
           int32_t* keep_idle_count_, int32_t* n_keep_io_) {
    s = sv;
    const rato_cut_config& c = s->c;
    u_lin = u_lin_;
    cvar = with_cvar;
    slack_row = cvar && c.mode_saa != 0;
    tol = tol_;
    max_cuts = max_cuts_;
    final_cut_above = final_cut_above_;
    check_finite = check_finite_;
    keep = keep_;
    keep_idle_count = keep_idle_count_;
    n_keep_io = n_keep_io_;
    nU = s->nU, n = s->n, S = c.S, nc = s->nc, n_u = nU / S;
    row.resize(n);
    g.resize(nU);
    x.resize(nU);
    z.resize(n);
    z_prev.resize(n);
    const auto t0 = std::chrono::steady_clock::now();
    // master: equalities [final_du | 0] z = final_rhs
    std::vector<double> F((size_t)n_c * n, 0.0);
    for (int r = 0; r < n_c; ++r) memcpy(&F[(size_t)r * n], final_du + (size_t)r * nU, sizeof(double) * nU);
    int rc = rato_master_create(&master, n, s->p_diag.data(), s->q.data(), n_c, F.data(), final_rhs);
    if (rc != RATO_OK) return RATO_ERANK;
    if (slack_row) {   // -slack <= 0
      std::fill(row.begin(), row.end(), 0.0);
      row[nU] = -1.0;
      const double zero = 0.0;
      if ((rc = rato_master_add_rows(master, 1, row.data(), &zero)) != RATO_OK) return rc;
      n_rows = 1;
    }
    // the kept slots index host tables below (is_kept, idle) whether or not their re-linearization is already in flight:
    // checked here too, not only inside rato_cut_begin / rato_cut_define_drone
    if (!keep_args_ok(s, keep, *n_keep_io)) return RATO_EINVAL;
    n_kept = (cvar && c.recycle) ? *n_keep_io : 0;
    master_s += seconds_since(t0);
    return RATO_OK;
  }

  bool wants_kept() const { return with_cuts(s, n_kept); }

  // sums [n_kept][nc]: the kept cuts' tail-row sums under the current linearization point
  int add_kept(const double* sums) {
    const rato_cut_config& c = s->c;
    const auto t0 = std::chrono::steady_clock::now();
    // cut k under the current linearization (delta form):  rows_k . (u - u_k) + c0_k - c_s s <= rhs0
    std::vector<double> rows((size_t)n_kept * n, 0.0), rhs(n_kept);
    for (int k = 0; k < n_kept; ++k) {
      const double* r = sums + (size_t)k * nc;
      double* rk = &rows[(size_t)k * n];
      for (int t = 0; t < S - 1; ++t) {
        rk[t * n_u + 0] = r[2 * t + 0] / c.alphaM;
        rk[t * n_u + 1] = r[2 * t + 1] / c.alphaM;
      }
      rk[nU] = -c.c_s;
      const double d = dot_exact(rk, u_lin, nU, prod);
      rhs[k] = (c.rhs0 + d) - 1.0 * (r[nc - 1] / c.alphaM);
      cut_rows.emplace_back(n_rows + k, keep[k]);
    }
    const int rc = rato_master_add_rows(master, n_kept, rows.data(), rhs.data());
    if (rc != RATO_OK) return rc;
    n_rows += n_kept;
    master_s += seconds_since(t0);
    return RATO_OK;
  }

  int begin() {
    const rato_cut_config& c = s->c;
    {
      std::vector<uint8_t> is_kept(c.cap, 0);
      for (int k = 0; k < n_kept; ++k) is_kept[keep[k]] = 1;
      for (int sl = 0; sl < c.cap - 1; ++sl)
        if (!is_kept[sl]) free_slots.push_back(sl);
    }
    in_master.assign(2 * (size_t)nU, 0);
    it = 0;
    return query();
  }

  int solve_master() {   // the master with the control bounds entering lazily: only the violated ones
    const rato_cut_config& c = s->c;
    for (;;) {
      lam.assign(n_rows, 0.0);
      const int r = rato_master_solve(master, z.data(), lam.data());
      if (r == RATO_EINFEASIBLE) return RATO_EINFEASIBLE;
      if (r != 1) return RATO_ENNLS;
      std::vector<int> hi, lo;
      for (int i = 0; i < nU; ++i) {
        if (z[i] > c.u_max + 1e-9 && !in_master[i]) hi.push_back(i);
        if (z[i] < c.u_min - 1e-9 && !in_master[nU + i]) lo.push_back(i);
      }
      if (hi.empty() && lo.empty()) return RATO_OK;
      for (int pass = 0; pass < 2; ++pass) {
        const std::vector<int>& idx = pass == 0 ? hi : lo;
        if (idx.empty()) continue;
        const double sgn = pass == 0 ? 1.0 : -1.0;
        std::vector<double> R((size_t)idx.size() * n, 0.0), b(idx.size(), pass == 0 ? c.u_max : -c.u_min);
        for (size_t k = 0; k < idx.size(); ++k) {
          R[k * n + idx[k]] = sgn;
          in_master[(pass == 0 ? 0 : nU) + idx[k]] = 1;
        }
        const int r2 = rato_master_add_rows(master, (int)idx.size(), R.data(), b.data());
        if (r2 != RATO_OK) return r2;
        bound_rows.push_back({n_rows, idx, sgn});
        n_rows += (int)idx.size();
      }
    }
  }

  // iteration `it` up to its oracle round trip: the master, then (CVaR rows on) the ring slot and x = z - u_k
  int query() {
    auto t0 = std::chrono::steady_clock::now();
    const int rc = solve_master();
    if (rc != RATO_OK) return rc;
    master_s += seconds_since(t0);
    if (!cvar) {
      done = true;
      return RATO_OK;
    }
    t0 = std::chrono::steady_clock::now();
    slot = -1;
    if (!free_slots.empty()) {
      slot = free_slots.back();
      free_slots.pop_back();
    }
    ring = slot >= 0 ? slot : s->c.cap - 1;   // (the last slot: scratch for calls beyond the ring)
    for (int i = 0; i < nU; ++i) x[i] = z[i] - u_lin[i];
    oracle_s += seconds_since(t0);
    return RATO_OK;
  }

  int add_cut() {   // phi(u) >= phi_k + g_k.(u - u_k)  =>  g_k.u - c_s s <= rhs0 + g_k.u_k - phi_k
    const rato_cut_config& c = s->c;
    memcpy(row.data(), g.data(), sizeof(double) * nU);
    row[nU] = -c.c_s;
    const double rhs = c.rhs0 + (dot_exact(g.data(), z.data(), nU, prod) - phi);
    const int r2 = rato_master_add_rows(master, 1, row.data(), &rhs);
    if (r2 != RATO_OK) return r2;
    if (slot >= 0) cut_rows.emplace_back(n_rows, slot);
    n_rows += 1;
    n_cuts += 1;
    return RATO_OK;
  }

  // the record of iteration `it`'s round trip: [RATO_N_STATS statistics | nc cut sums]
  int consume(const double* r) {
    const rato_cut_config& c = s->c;
    auto t0 = std::chrono::steady_clock::now();
    if (isnan(r[0])) return RATO_ESELECT;     // the one-launch selection gave up (or the m values hold NaN): the caller
    //                                           repeats the subproblem with the recovering Python loop
    if (check_finite && !(isfinite(r[3]) && isfinite(r[4]))) return RATO_ENONFINITE;
    std::fill(g.begin(), g.end(), 0.0);
    if (S > 1) {
      for (int t = 0; t < S - 1; ++t) {
        g[t * n_u + 0] = r[RATO_N_STATS + 2 * t + 0] / c.alphaM;
        g[t * n_u + 1] = r[RATO_N_STATS + 2 * t + 1] / c.alphaM;
      }
      phi = dot_exact(g.data(), x.data(), nU, prod) + 1.0 * (r[RATO_N_STATS + nc - 1] / c.alphaM);
    } else {
      phi = r[1];
    }
    tstar = r[0];
    oracle_s += seconds_since(t0);
    const double slack = z[nU];
    const double viol = phi - c.c_s * slack - c.rhs0;
    // stall: the cut added last moved nothing although it was violated -- the oracle returns cuts the master already
    // holds; what is left of the violation is the accuracy of the master's own NNLS (cvar_cuts.py: STALL_*)
    if (have_prev && viol > tol && viol <= 1e-7) {
      double step = 0.0;
      for (int i = 0; i < n; ++i) step = fmax(step, fabs(z[i] - z_prev[i]));
      if (step <= 1e-10) {
        status = 2;
        done = true;
        return RATO_OK;
      }
    }
    z_prev = z;
    have_prev = true;
    int rc;
    if (viol <= tol) {
      if (viol > final_cut_above && it < max_cuts) {   // the cut just evaluated is paid for: it joins the master
        t0 = std::chrono::steady_clock::now();
        if ((rc = add_cut()) != RATO_OK) return rc;
        if ((rc = solve_master()) != RATO_OK) return rc;
        master_s += seconds_since(t0);
      }
      done = true;
      return RATO_OK;
    }
    if (it == max_cuts) {
      status = 1;
      done = true;
      return RATO_OK;
    }
    if ((rc = add_cut()) != RATO_OK) return rc;
    ++it;
    return query();
  }

  void finish(rato_cut_result* out) {
    const rato_cut_config& c = s->c;
    // multipliers of the last master solve, for whoever certifies the solution against the full QP
    std::vector<double> lam_full(n_rows, 0.0);
    for (size_t i = 0; i < lam.size() && i < (size_t)n_rows; ++i) lam_full[i] = lam[i];
    if (cvar && c.recycle) {
      // keep rule: the cuts that carry a multiplier (newest first; keep_idle > 0: or did within the last keep_idle solves),
      // plus the newest keep_recent
      std::vector<int> idle(c.cap, -1);
      for (int k = 0; k < *n_keep_io; ++k) idle[keep[k]] = keep_idle_count[k];
      for (auto& cr : cut_rows) {
        const bool active = cr.first < (int)lam.size() && lam[cr.first] > 1e-12;
        idle[cr.second] = active ? 0 : (idle[cr.second] < 0 ? 0 : idle[cr.second]) + 1;
      }
      std::vector<int> new_keep;
      auto push = [&](int sl) {
        if (std::find(new_keep.begin(), new_keep.end(), sl) == new_keep.end()) new_keep.push_back(sl);
      };
      for (auto it2 = cut_rows.rbegin(); it2 != cut_rows.rend(); ++it2)
        if (idle[it2->second] <= c.keep_idle) push(it2->second);
      int cnt = 0;
      for (auto it2 = cut_rows.rbegin(); it2 != cut_rows.rend() && cnt < c.keep_recent; ++it2, ++cnt) push(it2->second);
      if ((int)new_keep.size() > c.keep_max) new_keep.resize(c.keep_max);
      for (size_t k = 0; k < new_keep.size(); ++k) {
        keep[k] = new_keep[k];
        keep_idle_count[k] = idle[new_keep[k]];
      }
      *n_keep_io = (int)new_keep.size();
    }
    memcpy(out->us, z.data(), sizeof(double) * nU);
    out->slack = z[nU];
    out->t_risk = slack_row ? tstar + z[nU] : 0.0;
    out->phi = phi;
    out->oracle_s = oracle_s;
    out->master_s = master_s;
    out->cuts = n_cuts;
    out->recycled = n_kept;
    out->status = status;
    out->lam_slack = slack_row ? lam_full[0] : 0.0;
    out->uncertified_cuts = n_cuts + n_kept - (int)cut_rows.size();
    out->n_cut_rows = 0;
    if (out->cut_slot && out->cut_lambda) {
      for (auto& cr : cut_rows) {
        if (out->n_cut_rows >= out->cut_capacity) break;
        out->cut_slot[out->n_cut_rows] = cr.second;
        out->cut_lambda[out->n_cut_rows] = lam_full[cr.first];
        ++out->n_cut_rows;
      }
    }
    out->n_bounds = 0;
    if (out->bound_var && out->bound_sign && out->bound_lambda) {
      for (auto& br : bound_rows)
        for (size_t k = 0; k < br.idx.size(); ++k) {
          if (out->n_bounds >= out->bound_capacity) break;
          out->bound_var[out->n_bounds] = br.idx[k];
          out->bound_sign[out->n_bounds] = br.sgn;
          out->bound_lambda[out->n_bounds] = lam_full[br.r0 + (int)k];
          ++out->n_bounds;
        }
    }
  }
};

}  // namespace

extern "C" int rato_cut_solve(rato_cut_solver* s, const double* final_du, const double* final_rhs, int32_t n_c,
                              const double* u_lin, int32_t with_cvar, double tol, int32_t max_cuts,
                              double final_cut_above, int32_t check_finite, int32_t* keep, int32_t* keep_idle_count,
                              int32_t* n_keep_io, int32_t kept_in_flight, rato_cut_result* out, void* stream) {
  if (!s || !final_du || !final_rhs || n_c < 0 || !u_lin || !out || !out->us || !keep || !keep_idle_count || !n_keep_io ||
      max_cuts < 0)
    return RATO_EINVAL;
  const rato_cut_config& c = s->c;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  CutLoop L;
  int rc = L.init(s, final_du, final_rhs, n_c, u_lin, with_cvar != 0, tol, max_cuts, final_cut_above, check_finite != 0, keep,
                  keep_idle_count, n_keep_io);
  if (rc != RATO_OK) return rc;
  if (L.wants_kept()) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!kept_in_flight) {
      if ((rc = rato_cut_begin(s, u_lin, keep, L.n_kept, stream)) != RATO_OK) return rc;
    }
    // (the kept cuts' sums were armed where they were launched: rato_cut_begin / rato_cut_define_drone)
    const bool armed = s->kept_armed;
    s->kept_armed = false;
    hipError_t e = armed ? rato::readback_wait(c.sums_b_host, L.n_kept * s->nc, st) : hipStreamSynchronize(st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
    // (not armed: the words were not watched -- a define that failed before its launch leaves them pre-set; never data)
    if (!armed && rato::readback_pending(c.sums_b_host, L.n_kept * s->nc)) return RATO_EHIP - (int)hipErrorNotReady;
    L.oracle_s += seconds_since(t0);
    if ((rc = L.add_kept(c.sums_b_host)) != RATO_OK) return rc;
  }
  if ((rc = L.begin()) != RATO_OK) return rc;
  const size_t M = (size_t)c.M;
  while (!L.done) {
    const auto t0 = std::chrono::steady_clock::now();
    memcpy(c.x_host, L.x.data(), sizeof(double) * (size_t)s->nU);
    const int ring = L.ring;
    rc = rato_cut_oracle_rollout(c.system, s->params(), c.uk_dev, c.s0, c.s1, c.s2, c.s3, c.x_host, c.x_dev,
                                 c.ring_m + (size_t)ring * M, c.ring_arg + (size_t)ring * M, c.alpha, c.thr, c.alphaM,
                                 c.workspace, c.workspace_bytes, c.ring_res + (size_t)ring * s->nres, c.part, c.res_host,
                                 stream);
    if (rc != RATO_OK) return rc;
    L.oracle_s += seconds_since(t0);
    if ((rc = L.consume(c.res_host)) != RATO_OK) return rc;
  }
  L.finish(out);
  return RATO_OK;
}


namespace {
// the record of one iteration of a native SCP loop: solve = oracle round trips + master, define = the rest of `total`
void scp_record(rato_scp_iter& r, const rato_cut_result& res, double total) {
  r.oracle_s = res.oracle_s;
  r.master_s = res.master_s;
  r.solve_s = res.oracle_s + res.master_s;
  r.define_s = total - r.solve_s;
  r.t_risk = res.t_risk;
  r.slack = res.slack;
  r.phi = res.phi;
  r.cuts = res.cuts;
  r.status = res.status;
  r.recycled = res.recycled;
  r.reserved = 0;
}

// where a subproblem's outputs land: the solution and the certificate's (slot, multiplier) pairs
struct ResultBuf {
  std::vector<double> sol, cut_lambda;
  std::vector<int32_t> cut_slot;
  explicit ResultBuf(const rato_cut_solver* s) : sol(s->nU), cut_lambda(s->c.cap + 8), cut_slot(s->c.cap + 8) {}
  rato_cut_result wired() {   // a zeroed result pointing into this storage
    rato_cut_result r = {};
    r.us = sol.data();
    r.cut_slot = cut_slot.data();
    r.cut_lambda = cut_lambda.data();
    r.cut_capacity = (int)cut_slot.size();
    return r;
  }
};

// The drone's equality rows from the sample sums [6S + 6] of its linearization: mean of the final-state Jacobian (axis a: row a
// = position, row 3 + a = velocity; the axes decouple) and of its right-hand side (drone_risk.py:271-273, :294-300).  The rows
// are sums * (1 / M), the right-hand side sums / M: the two roundings of the Python checker (expand_final_du(.., 1.0 / M),
// sums[6S:] / M), which the solo loop and the batch must both reproduce to the bit.  final_du [6][3S], final_rhs [6].
void drone_final_rows(const double* sums, int S, int64_t M, double* final_du, double* final_rhs) {
  const int nU = 3 * S;
  const double Md = (double)M, inv_M = 1.0 / Md;
  std::fill(final_du, final_du + (size_t)6 * nU, 0.0);
  for (int t = 0; t < S; ++t)
    for (int a = 0; a < 3; ++a) {
      final_du[(size_t)a * nU + t * 3 + a] = sums[t * 6 + a] * inv_M;
      final_du[(size_t)(3 + a) * nU + t * 3 + a] = sums[t * 6 + 3 + a] * inv_M;
    }
  for (int r = 0; r < 6; ++r) final_rhs[r] = sums[6 * S + r] / Md;
}

// The reduced SCP of one problem as ONE call: `iters` iterations of [define at the current controls -> rato_cut_solve], the
// reference's fixed-count protocol (drone_risk.py:519-532, drone_times.py:509-550; driving.py:486-513) with its per-iteration
// wall clocks taken here.  define(us, K, final_du, final_rhs) -> rc is the system's: it leaves the n_c equality rows on the
// host and u_k plus the K kept cuts' re-linearization on the stream.  Each iteration is timed from its first instruction to
// the moment its solution is on the host (the last oracle round trip has been read back: the device has nothing of this
// iteration left to do); the stream is synchronised ONCE, after the last iteration, inside that iteration's clock.
// Returns the first non-OK status of a define / solve (RATO_ERANK, RATO_ESELECT: repeat with the per-iteration calls, whose
// Python loop recovers), *done = iterations completed.
template <class Define>
int scp_run(rato_cut_solver* s, int n_c, const double* us0, int32_t iters, int32_t first_cvar, double tol, int32_t max_cuts,
            double final_cut_above, int32_t check_finite, int32_t* keep, int32_t* keep_idle_count, int32_t* n_keep_io,
            double* us_hist, rato_scp_iter* rec, int32_t* done, void* stream, Define&& define) {
  const int nU = s->nU;
  std::vector<double> us(us0, us0 + nU), final_du((size_t)n_c * nU), final_rhs(n_c);
  ResultBuf out(s);
  *done = 0;
  for (int it = 0; it < iters; ++it) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool cvar = it >= first_cvar;
    const int K = (cvar && s->c.recycle && s->c.S >= 2) ? *n_keep_io : 0;
    int rc = define(us.data(), K, final_du.data(), final_rhs.data());
    if (rc != RATO_OK) return rc;
    rato_cut_result res = out.wired();
    rc = rato_cut_solve(s, final_du.data(), final_rhs.data(), n_c, us.data(), cvar ? 1 : 0, tol, max_cuts, final_cut_above,
                        check_finite, keep, keep_idle_count, n_keep_io, K > 0 ? 1 : 0, &res, stream);
    if (rc != RATO_OK) return rc;
    if (it == iters - 1) {   // the protocol's closing synchronisation, once: inside the last iteration's clock
      const hipError_t e = hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
      if (e != hipSuccess) return RATO_EHIP - (int)e;
    }
    scp_record(rec[it], res, seconds_since(t0));
    memcpy(us_hist + (size_t)it * nU, out.sol.data(), sizeof(double) * nU);
    us = out.sol;
    *done = it + 1;
  }
  return RATO_OK;
}
}  // namespace

// The reduced SCP of the drone (scp_run above); its define: rato_cut_define_drone at the current controls -> the equality rows
// from the sample sums.  scp.run_drone_reduced's Python loop (one define + one solve call per iteration, a device
// synchronisation on both sides of each) stays as the checker: same iterates bit for bit (tests/test_gpu_scp.py).
//   us0 [S][3]: the initial guess;  first_cvar: the first iteration with the CVaR rows (2: drone_risk.py:413-417);
//   us_hist [iters][S][3] (host): the solution of every iteration;  rec [iters];
//   the define's buffers as for rato_cut_define_drone;  keep / keep_idle_count / n_keep_io: in and out as for rato_cut_solve.
extern "C" int rato_scp_run_drone(rato_cut_solver* s, const double* us0, int32_t iters, int32_t first_cvar, double tol,
                                  int32_t max_cuts, double final_cut_above, int32_t check_finite, float* us_host,
                                  float* us_dev, float* A22, float* part, double* sums_host, int32_t* keep,
                                  int32_t* keep_idle_count, int32_t* n_keep_io, double* us_hist, rato_scp_iter* rec,
                                  int32_t* done, void* stream) {
  if (!s || s->c.system != 0 || !us0 || iters < 0 || !us_host || !us_dev || !A22 || !part || !sums_host || !keep ||
      !keep_idle_count || !n_keep_io || !us_hist || !rec || !done)
    return RATO_EINVAL;
  const int S = s->c.S;
  return scp_run(s, 6, us0, iters, first_cvar, tol, max_cuts, final_cut_above, check_finite, keep, keep_idle_count, n_keep_io,
                 us_hist, rec, done, stream, [&](const double* us, int K, double* final_du, double* final_rhs) {
                   const int rc = rato_cut_define_drone(s, us, us_host, us_dev, A22, nullptr, 0, part, sums_host, nullptr,
                                                        nullptr, keep, K, stream);
                   if (rc != RATO_OK) return rc;
                   if (check_finite && !all_finite(sums_host, 6 * (size_t)S + 6)) return RATO_ENONFINITE;
                   drone_final_rows(sums_host, S, s->c.M, final_du, final_rhs);
                   return RATO_OK;
                 });
}

extern "C" size_t rato_scp_iter_bytes(void) { return sizeof(rato_scp_iter); }

// The final-state rows of the ego (driving.py:283-288) on the host, in fp64: the ego carries no noise, so x_S[0:4] and its
// control Jacobian are sample independent -- the car's "define" has no device linearization.  The formulas of
// driving.Model.ego_final_rows with plain sequential sums in ascending k and libm's sincos (this file is compiled with
// contraction off): the native SCP loops below and the per-iteration Python loop that checks them call THIS function, so
// their equality rows agree to the bit; against NumPy's cos / sin / pairwise sums they agree to rounding.
//   v_k = v_0 + dt sum_{j<k} u_j0,  phi_k alike;   x_S = (x_0 + dt sum_k v_k cos phi_k, y_0 + dt sum_k v_k sin phi_k, v_S, phi_S)
//   d x_S / d u_t0 = dt^2 sum_{k>t} cos phi_k,  d x_S / d u_t1 = -dt^2 sum_{k>t} v_k sin phi_k  (y alike);  rows 2, 3: dt
//   final_rhs = -(x_S - goal) + final_du . u
extern "C" int rato_car_ego_final_rows(const rato_car_params* p, const double* us, const double* goal, double* final_du,
                                       double* final_rhs) {
  if (!p || p->S < 1 || !(p->dt64 > 0.0) || !us || !goal || !final_du || !final_rhs) return RATO_EINVAL;
  const int S = p->S, nU = 2 * S;
  const double dt = p->dt64;
  std::vector<double> v(S + 1), cs(S), sn(S), vs(S), vc(S);
  double cu0 = 0.0, cu1 = 0.0, ph = 0.0;
  v[0] = p->ego_init64[2] + dt * 0.0;
  for (int k = 0; k < S; ++k) {
    ph = p->ego_init64[3] + dt * cu1;        // phi_k
    sincos(ph, &sn[k], &cs[k]);
    vc[k] = v[k] * cs[k];
    vs[k] = v[k] * sn[k];
    cu0 += us[2 * k + 0];
    cu1 += us[2 * k + 1];
    v[k + 1] = p->ego_init64[2] + dt * cu0;
  }
  ph = p->ego_init64[3] + dt * cu1;          // phi_S
  double sx = 0.0, sy = 0.0;
  for (int k = 0; k < S; ++k) {
    sx += vc[k];
    sy += vs[k];
  }
  const double xS[4] = {p->ego_init64[0] + dt * sx, p->ego_init64[1] + dt * sy, v[S], ph};
  std::fill(final_du, final_du + (size_t)4 * nU, 0.0);
  for (int t = 0; t < S; ++t) {
    double ac = 0.0, as = 0.0, avs = 0.0, avc = 0.0;
    for (int k = t + 1; k < S; ++k) {
      ac += cs[k];
      as += sn[k];
      avs += vs[k];
      avc += vc[k];
    }
    final_du[(size_t)0 * nU + 2 * t + 0] = dt * dt * ac;
    final_du[(size_t)0 * nU + 2 * t + 1] = -dt * dt * avs;
    final_du[(size_t)1 * nU + 2 * t + 0] = dt * dt * as;
    final_du[(size_t)1 * nU + 2 * t + 1] = dt * dt * avc;
    final_du[(size_t)2 * nU + 2 * t + 0] = dt;
    final_du[(size_t)3 * nU + 2 * t + 1] = dt;
  }
  for (int r = 0; r < 4; ++r) {
    double d = 0.0;
    for (int i = 0; i < nU; ++i) d += final_du[(size_t)r * nU + i] * us[i];
    final_rhs[r] = -(xS[r] - goal[r]) + d;
  }
  return RATO_OK;
}

// The reduced SCP of the DRIVING problem (scp_run above; driving.py:486-513); its define: rato_car_ego_final_rows at the
// current controls -> rato_cut_begin (u_k in fp64 + the kept cuts against it).
// scp.run_driving_reduced(native_loop=False, final_rows='native') is the per-iteration checker: same iterates bit for bit
// (tests/test_gpu_scp_car_native.py).
//   us0 [S][2];  goal [4]: the ego's goal state (position, speed, heading);  first_cvar: 1 (driving.py:411-415);
//   us_hist [iters][S][2];  rec [iters];  keep / keep_idle_count / n_keep_io: in and out as for rato_cut_solve.
extern "C" int rato_scp_run_car(rato_cut_solver* s, const double* us0, const double* goal, int32_t iters, int32_t first_cvar,
                                double tol, int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep,
                                int32_t* keep_idle_count, int32_t* n_keep_io, double* us_hist, rato_scp_iter* rec, int32_t* done,
                                void* stream) {
  if (!s || s->c.system != 1 || !us0 || !goal || iters < 0 || !keep || !keep_idle_count || !n_keep_io || !us_hist || !rec || !done)
    return RATO_EINVAL;
  const size_t nU = (size_t)s->nU;
  return scp_run(s, 4, us0, iters, first_cvar, tol, max_cuts, final_cut_above, check_finite, keep, keep_idle_count, n_keep_io,
                 us_hist, rec, done, stream, [&](const double* us, int K, double* final_du, double* final_rhs) {
                   const int rc = rato_car_ego_final_rows(&s->car, us, goal, final_du, final_rhs);
                   if (rc != RATO_OK) return rc;
                   if (check_finite && !(all_finite(final_du, 4 * nU) && all_finite(final_rhs, 4))) return RATO_ENONFINITE;
                   return rato_cut_begin(s, us, keep, K, stream);
                 });
}

// ---------------------------------------------------------------------------------------------------------------------
// The reduced SCP of MANY problems of one system in lockstep (the reference's alpha x repeat grids, drone_risk.py:495-539,
// driving.py:467-529): one problem = one rato_cut_solver (its own samples, alpha, rings and kept cuts) over one shared S, M
// and parameter struct.  Per SCP iteration: ONE batched define for every problem still running (drone: controls and u_k up,
// generators-only linearization, sample sums, the kept cuts' re-linearization, one wait;  driving: the sample-independent
// final rows on the host threads, u_k up, the kept cuts' re-linearization, one wait), the masters of all problems on up to
// n_threads host threads, and then ROUNDS: one batched oracle round trip (rowmax -> exact selection -> tail rows -> cut_finish, one
// wait) for every problem still cutting, whose records are fed back to their masters in parallel.  A round's launches do
// not grow with the batch: the table of its problems travels in one copy and every launch indexes it with blockIdx.y.  A
// problem that leaves its subproblem early waits for the others before the next define.  Each problem runs the statements
// of rato_scp_run_drone / rato_scp_run_car on the workgroup bodies of its single-problem kernels: its iterates are those of
// a solo run, bit for bit.  A problem that fails leaves the batch (status[p]); the others go on.
namespace {

constexpr size_t BATCH_ALIGN = 256;
size_t align_up(size_t v) { return (v + BATCH_ALIGN - 1) / BATCH_ALIGN * BATCH_ALIGN; }

// a small persistent pool: run(n, f) calls f(0 .. n-1) on the caller and up to n_threads - 1 workers
class TaskPool {
 public:
  explicit TaskPool(int n_threads) {
    for (int i = 1; i < n_threads; ++i) workers_.emplace_back([this] { work(); });
  }
  ~TaskPool() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      stop_ = true;
      ++gen_;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  template <class F>
  void run(int n, F&& f) {
    if (workers_.empty() || n < 2) {
      for (int i = 0; i < n; ++i) f(i);
      return;
    }
    {
      std::lock_guard<std::mutex> lk(mu_);
      fn_ = [&f](int i) { f(i); };
      total_ = n;
      next_.store(0);
      pending_ = (int)workers_.size();
      ++gen_;
    }
    cv_.notify_all();
    drain();
    std::unique_lock<std::mutex> lk(mu_);
    done_cv_.wait(lk, [this] { return pending_ == 0; });
    fn_ = nullptr;
  }

 private:
  void drain() {
    for (;;) {
      const int i = next_.fetch_add(1);
      if (i >= total_) return;
      fn_(i);
    }
  }
  void work() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
      }
      drain();
      std::lock_guard<std::mutex> lk(mu_);
      if (--pending_ == 0) done_cv_.notify_one();
    }
  }
  std::vector<std::thread> workers_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  std::function<void(int)> fn_;
  std::atomic<int> next_{0};
  int total_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// sizes of a batch of K problems (S, M, ld, keep_max shared).  The driving problem (system 1) has no device linearization:
// its fp32 controls, A22, gpart and sample-sum regions are empty.
struct BatchLayout {
  size_t d_tab, d_uk, d_us, d_slots, d_rows, d_size;   // define region (table + staged inputs + kept-cut rows)
  size_t r_tab, r_x, r_size;                           // round region (table + x)
  size_t a22, gpart, dev_bytes;                        // device: [define | round | A22 [K][S 3 ld] | gpart [K][nblk][6S+6]]
  size_t h_res, h_sums, h_ksums, host_bytes;           // pinned: [define | round | res [K][nres] | sums | kept sums]
  BatchLayout(int system, int K, int S, int64_t ld, int nblk, int keep_max, int nc, int nres) {
    const size_t nU = (system == 0 ? 3 : 2) * (size_t)S, Kz = (size_t)K, km = (size_t)std::max(keep_max, 1);
    const size_t lin = system == 0 ? 1 : 0;            // (the drone's define linearizes on the device)
    d_tab = 0;
    d_uk = align_up(Kz * sizeof(rato::BatchProb));
    d_us = d_uk + align_up(Kz * nU * sizeof(double));
    d_slots = d_us + align_up(lin * Kz * nU * sizeof(float));
    d_rows = d_slots + align_up(Kz * km * sizeof(int32_t));
    d_size = d_rows + align_up(Kz * km * sizeof(rato::BatchCut));
    r_tab = d_size;
    r_x = r_tab + align_up(Kz * sizeof(rato::BatchProb));
    r_size = r_x + align_up(Kz * nU * sizeof(double)) - r_tab;
    a22 = r_tab + r_size;
    gpart = a22 + align_up(lin * Kz * nU * (size_t)ld * sizeof(float));
    dev_bytes = gpart + align_up(lin * Kz * (size_t)nblk * (6 * (size_t)S + 6) * sizeof(float));
    h_res = r_tab + r_size;
    h_sums = h_res + align_up(Kz * (size_t)nres * sizeof(double));
    h_ksums = h_sums + align_up(lin * Kz * (6 * (size_t)S + 6) * sizeof(double));
    host_bytes = h_ksums + align_up(Kz * km * (size_t)nc * sizeof(double));
  }
};

int batch_check(rato_cut_solver* const* solvers, int32_t K) {
  if (!solvers || K < 1 || K > 65535) return RATO_EINVAL;
  const rato_cut_solver* s0 = solvers[0];
  for (int32_t p = 0; p < K; ++p) {
    const rato_cut_solver* s = solvers[p];
    if (!s || s->c.system != s0->c.system || s->c.mode_saa == 0 || s->c.S < 2 || s->c.S != s0->c.S || s->c.M != s0->c.M ||
        s->c.keep_max != s0->c.keep_max || s->c.cap != s0->c.cap || !s->c.part || (s->c.keep_max > 0 && !s->c.part_b) ||
        (s->c.system == 0 ? memcmp(&s->drone, &s0->drone, sizeof(rato_drone_params))
                          : memcmp(&s->car, &s0->car, sizeof(rato_car_params))) != 0)
      return RATO_EINVAL;
    for (int32_t q = 0; q < p; ++q)
      if (solvers[q] == s) return RATO_EINVAL;   // (one solver's rings cannot serve two problems)
  }
  return RATO_OK;
}

BatchLayout batch_layout(const rato_cut_solver* s, int K) {
  return BatchLayout(s->c.system, K, s->c.S, s->c.system == 0 ? s->drone.ld : s->c.M, s->nblk, s->c.keep_max, s->nc, s->nres);
}

}  // namespace

struct rato_scp_batch {
  std::vector<rato_cut_solver*> sv;
  int system = 0;
  rato_drone_params P;   // system 0
  rato_car_params C;     // system 1
  int K = 0, S = 0, nU = 0, nc = 0, nres = 0, nblk = 0, keep_max = 0, ncols = 0;
  int64_t M = 0, ld = 0;
  unsigned char *dev = nullptr, *host = nullptr;
  BatchLayout lay{0, 1, 2, 1, 1, 0, 1, 1};
  std::unique_ptr<TaskPool> pool;
};

extern "C" int rato_scp_batch_bytes(rato_cut_solver* const* solvers, int32_t K, size_t* device_bytes, size_t* host_bytes) {
  if (!device_bytes || !host_bytes) return RATO_EINVAL;
  const int rc = batch_check(solvers, K);
  if (rc != RATO_OK) return rc;
  const rato_cut_solver* s = solvers[0];
  const BatchLayout lay = batch_layout(s, K);
  *device_bytes = lay.dev_bytes;
  *host_bytes = lay.host_bytes;
  return RATO_OK;
}

extern "C" int rato_scp_batch_create(rato_scp_batch** out, rato_cut_solver* const* solvers, int32_t K, int32_t n_threads,
                                     void* device_buf, size_t device_bytes, void* host_buf, size_t host_bytes) {
  if (!out || n_threads < 1 || n_threads > 256 || !device_buf || !host_buf) return RATO_EINVAL;
  int rc = batch_check(solvers, K);
  if (rc != RATO_OK) return rc;
  const rato_cut_solver* s = solvers[0];
  const BatchLayout lay = batch_layout(s, K);
  if (device_bytes < lay.dev_bytes || host_bytes < lay.host_bytes || ((uintptr_t)device_buf % BATCH_ALIGN) != 0 ||
      ((uintptr_t)host_buf % 16) != 0)
    return RATO_EINVAL;
  rato_scp_batch* b = new rato_scp_batch;
  b->sv.assign(solvers, solvers + K);
  b->system = s->c.system;
  b->P = s->drone;
  b->C = s->car;
  b->K = K;
  b->S = s->c.S;
  b->nU = s->nU;
  b->nc = s->nc;
  b->nres = s->nres;
  b->nblk = s->nblk;
  b->keep_max = s->c.keep_max;
  b->ncols = b->system == 0 ? 6 * b->S + 6 : 0;   // the define's sample sums (drone only)
  b->M = s->c.M;
  b->ld = b->system == 0 ? s->drone.ld : s->c.M;
  b->dev = static_cast<unsigned char*>(device_buf);
  b->host = static_cast<unsigned char*>(host_buf);
  b->lay = lay;
  b->pool.reset(new TaskPool(std::min<int>(n_threads, K)));
  *out = b;
  return RATO_OK;
}

extern "C" void rato_scp_batch_destroy(rato_scp_batch* b) { delete b; }

extern "C" size_t rato_scp_batch_iter_bytes(void) { return sizeof(rato_scp_batch_iter); }

namespace {

// The lockstep run of both systems.  What differs between them sits behind `car`: the define (the drone linearizes on the
// device and reads its sample sums back; the car's equality rows come from rato_car_ego_final_rows on the host threads and
// only u_k and the kept cuts travel) and the two oracle launches of a round.  goal: the car's goal state [4] (drone: unused).
int batch_run(rato_scp_batch* b, const double* us0, const double* goal, int32_t iters, int32_t first_cvar, double tol,
              int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep, int32_t* keep_idle_count,
              int32_t* n_keep, double* us_hist, rato_scp_iter* rec, rato_scp_batch_iter* brec, int32_t* status, int32_t* done,
              int32_t* rounds, void* stream) {
  if (!b || !us0 || iters < 0 || max_cuts < 0 || !keep || !keep_idle_count || !n_keep || !us_hist || !rec || !brec ||
      !status || !done || !rounds)
    return RATO_EINVAL;
  const bool car = b->system == 1;
  if (car && !goal) return RATO_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int K = b->K, S = b->S, nU = b->nU, nc = b->nc, nres = b->nres, ncols = b->ncols, km = std::max(b->keep_max, 1);
  const int n_c = car ? 4 : 6;
  const size_t Mz = (size_t)b->M;
  const BatchLayout& L = b->lay;
  double* res_host = reinterpret_cast<double*>(b->host + L.h_res);
  double* sums_host = reinterpret_cast<double*>(b->host + L.h_sums);
  double* ksums_host = reinterpret_cast<double*>(b->host + L.h_ksums);
  auto dev_of = [&](const void* host_ptr) {   // the device address of a byte of the define / round mirrors
    return b->dev + (static_cast<const unsigned char*>(host_ptr) - b->host);
  };
  std::vector<std::vector<double>> us(K);
  std::vector<std::unique_ptr<CutLoop>> loop(K);
  std::vector<ResultBuf> out;
  out.reserve(K);
  std::vector<int> dpos(K, -1);
  std::vector<std::vector<double>> car_du(car ? K : 0), car_rhs(car ? K : 0);   // the car's equality rows of the iteration
  for (int p = 0; p < K; ++p) {
    us[p].assign(us0 + (size_t)p * nU, us0 + (size_t)(p + 1) * nU);
    out.emplace_back(b->sv[p]);
    if (car) {
      car_du[p].resize((size_t)n_c * nU);
      car_rhs[p].resize(n_c);
    }
    status[p] = RATO_OK;
    done[p] = 0;
    const int rc = settle_kept(b->sv[p], st);   // a kept-cuts launch of a solo define nobody waited for
    if (rc != RATO_OK) return rc;
  }
  *rounds = 0;
  // the problems' own device copies (only the pointers differ): the table's rows of a problem
  auto fill_common = [&](rato::BatchProb& t, int p) {
    const rato_cut_config& c = b->sv[p]->c;
    memset(&t, 0, sizeof(t));
    t.s0 = c.s0;
    t.s1 = c.s1;
    t.s2 = c.s2;
    t.s3 = c.s3;
    t.alpha = c.alpha;
    t.alphaM = c.alphaM;
    t.thr = c.thr;
    int vmax = 0;
    unsigned kr = 0;
    rato_sel::stats_rank(b->M, c.alpha, kr, vmax);
    t.k = kr;
    t.var_is_max = vmax;
    t.m_base = c.ring_m;
    t.arg_base = c.ring_arg;
    t.res_base = c.ring_res;
    t.part = c.part;
    t.part_b = c.part_b;
  };
  const bool select_batched = rato::risk_stats_batch_applies(b->M);
  for (int it = 0; it < iters; ++it) {
    const auto t_it = std::chrono::steady_clock::now();
    rato_scp_batch_iter& br = brec[it];
    memset(&br, 0, sizeof(br));
    const bool cvar = it >= first_cvar;
    std::vector<int> act;
    for (int p = 0; p < K; ++p)
      if (status[p] == RATO_OK) act.push_back(p);
    br.active = (int32_t)act.size();
    if (act.empty()) continue;
    if (car) {   // ---- the car's equality rows at the current controls (as rato_scp_run_car computes them), in parallel
      b->pool->run((int)act.size(), [&](int i) {
        const int p = act[i];
        const int r2 = rato_car_ego_final_rows(&b->C, us[p].data(), goal, car_du[p].data(), car_rhs[p].data());
        if (r2 != RATO_OK)
          status[p] = r2;
        else if (check_finite && !(all_finite(car_du[p].data(), car_du[p].size()) && all_finite(car_rhs[p].data(), n_c)))
          status[p] = RATO_ENONFINITE;
      });
      act.erase(std::remove_if(act.begin(), act.end(), [&](int p) { return status[p] != RATO_OK; }), act.end());
      if (act.empty()) continue;
    }
    // ---- define: every active problem's table row, staged inputs and kept-cut rows into the pinned mirror, ONE copy
    rato::BatchProb* tab = reinterpret_cast<rato::BatchProb*>(b->host + L.d_tab);
    double* uk_h = reinterpret_cast<double*>(b->host + L.d_uk);
    float* us_h = reinterpret_cast<float*>(b->host + L.d_us);
    int32_t* slots_h = reinterpret_cast<int32_t*>(b->host + L.d_slots);
    rato::BatchCut* rows_h = reinterpret_cast<rato::BatchCut*>(b->host + L.d_rows);
    std::vector<rato::BatchCut> plain, uni;
    int n = 0, kn_max = 0, keep_top = 0;
    for (int p : act) {
      rato_cut_solver* s = b->sv[p];
      int32_t* kp = keep + (size_t)p * km;
      if (!keep_args_ok(s, kp, n_keep[p])) {
        status[p] = RATO_EINVAL;
        continue;
      }
      const int Kp = (cvar && s->c.recycle) ? n_keep[p] : 0;   // (S >= 2 in a batch: every kept cut has rows)
      rato::BatchProb& t = tab[n];
      fill_common(t, p);
      double* uk = uk_h + (size_t)n * nU;
      float* usf = us_h + (size_t)n * nU;
      int32_t* sl = slots_h + (size_t)n * km;
      for (int i = 0; i < nU; ++i) uk[i] = us[p][i];
      for (int k = 0; k < Kp; ++k) sl[k] = kp[k];
      t.uk = reinterpret_cast<const double*>(dev_of(uk));
      t.slots = reinterpret_cast<const int32_t*>(dev_of(sl));
      t.n_keep = Kp;
      t.sums_b_host = ksums_host + (size_t)p * km * nc;
      if (!car) {   // the linearization's inputs, scratch and sample sums
        for (int i = 0; i < nU; ++i) usf[i] = (float)us[p][i];
        t.us = reinterpret_cast<const float*>(dev_of(usf));
        t.A22 = reinterpret_cast<float*>(b->dev + L.a22) + (size_t)n * nU * (size_t)b->ld;
        t.gpart = reinterpret_cast<float*>(b->dev + L.gpart) + (size_t)n * b->nblk * ncols;
        t.sums_host = sums_host + (size_t)p * ncols;
        if (rato::readback_poll_enabled()) rato::readback_arm(t.sums_host, ncols);
      }
      if (Kp > 0) {
        if (rato::readback_poll_enabled()) rato::readback_arm(t.sums_b_host, Kp * nc);
        keep_top = std::max(keep_top, Kp);
        if (!car && rato::drone_tail_union_form(S, Kp)) {
          for (int k0 = 0; k0 < Kp; k0 += 16) {   // (TRU_KMAX cuts per row: the single launcher's chunks)
            const int kn = std::min(16, Kp - k0);
            uni.push_back({n, k0, kn, Kp});
            kn_max = std::max(kn_max, kn);
          }
        } else {
          for (int k = 0; k < Kp; ++k) plain.push_back({n, k, 1, Kp});
        }
      }
      dpos[p] = n++;
    }
    act.erase(std::remove_if(act.begin(), act.end(), [&](int p) { return status[p] != RATO_OK; }), act.end());
    if (n == 0) continue;
    for (size_t i = 0; i < plain.size(); ++i) rows_h[i] = plain[i];
    for (size_t i = 0; i < uni.size(); ++i) rows_h[plain.size() + i] = uni[i];
    // (a car iteration without the CVaR rows has no device work at all: nothing reads its table)
    hipError_t e = (car && !cvar) ? hipSuccess
                                  : hipMemcpyAsync(b->dev + L.d_tab, b->host + L.d_tab, L.d_size, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return RATO_EHIP - (int)e;
    const rato::BatchProb* tab_d = reinterpret_cast<const rato::BatchProb*>(b->dev + L.d_tab);
    const rato::BatchCut* rows_d = reinterpret_cast<const rato::BatchCut*>(b->dev + L.d_rows);
    int rc = RATO_OK;
    if (car) {   // (no union form: every kept cut is one row)
      if (!plain.empty()) rc = rato::launch_car_tail_kept_batch(&b->C, tab_d, rows_d, (int)plain.size(), st);
    } else {
      rc = rato::launch_drone_linearize_generators_batch(&b->P, tab_d, n, st);
      if (rc == RATO_OK) rc = rato::launch_define_sums_batch(tab_d, n, b->nblk, ncols, st);
      if (rc == RATO_OK && !plain.empty())
        rc = rato::launch_drone_tail_kept_batch(&b->P, tab_d, rows_d, (int)plain.size(), false, 1, st);
      if (rc == RATO_OK && !uni.empty())
        rc = rato::launch_drone_tail_kept_batch(&b->P, tab_d, rows_d + plain.size(), (int)uni.size(), true, kn_max, st);
    }
    if (rc == RATO_OK && keep_top > 0) rc = rato::launch_kept_sums_batch(tab_d, n, b->nblk, nc, keep_top, st);
    if (rc != RATO_OK) return rc;
    for (int p : act) {
      const rato::BatchProb& t = tab[dpos[p]];
      e = car ? hipSuccess : rato::readback_wait(t.sums_host, ncols, st);
      if (e == hipSuccess && t.n_keep > 0) e = rato::readback_wait(t.sums_b_host, t.n_keep * nc, st);
      if (e != hipSuccess) return RATO_EHIP - (int)e;
    }
    br.define_s = seconds_since(t_it);
    // ---- the subproblems up to their first query (equality rows, kept cuts, first master), in parallel
    auto t0 = std::chrono::steady_clock::now();
    b->pool->run((int)act.size(), [&](int i) {
      const int p = act[i];
      rato_cut_solver* s = b->sv[p];
      std::vector<double> drone_du, drone_rhs;
      if (!car) {
        const double* sm = tab[dpos[p]].sums_host;
        if (check_finite && !all_finite(sm, ncols)) {
          status[p] = RATO_ENONFINITE;
          return;
        }
        drone_du.resize((size_t)n_c * nU);
        drone_rhs.resize(n_c);
        drone_final_rows(sm, S, b->M, drone_du.data(), drone_rhs.data());
      }
      const std::vector<double>&final_du = car ? car_du[p] : drone_du, &final_rhs = car ? car_rhs[p] : drone_rhs;
      loop[p].reset(new CutLoop);
      CutLoop& lp = *loop[p];
      int r2 = lp.init(s, final_du.data(), final_rhs.data(), n_c, us[p].data(), cvar, tol, max_cuts, final_cut_above,
                       check_finite != 0, keep + (size_t)p * km, keep_idle_count + (size_t)p * km, n_keep + p);
      if (r2 == RATO_OK && lp.wants_kept()) r2 = lp.add_kept(tab[dpos[p]].sums_b_host);
      if (r2 == RATO_OK) r2 = lp.begin();
      if (r2 != RATO_OK) status[p] = r2;
    });
    br.master_s += seconds_since(t0);
    // ---- rounds: one batched oracle round trip for every problem still cutting
    rato::BatchProb* rtab = reinterpret_cast<rato::BatchProb*>(b->host + L.r_tab);
    double* x_h = reinterpret_cast<double*>(b->host + L.r_x);
    for (;;) {
      std::vector<int> q;
      for (int p : act)
        if (status[p] == RATO_OK && !loop[p]->done) q.push_back(p);
      if (q.empty()) break;
      t0 = std::chrono::steady_clock::now();
      const int nq = (int)q.size();
      for (int i = 0; i < nq; ++i) {
        const int p = q[i];
        const rato_cut_config& c = b->sv[p]->c;
        const CutLoop& lp = *loop[p];
        rato::BatchProb& t = rtab[i];
        t = tab[dpos[p]];
        double* x = x_h + (size_t)i * nU;
        memcpy(x, lp.x.data(), sizeof(double) * nU);
        t.x = reinterpret_cast<const double*>(dev_of(x));
        t.m_out = c.ring_m + (size_t)lp.ring * Mz;
        t.arg_out = c.ring_arg + (size_t)lp.ring * Mz;
        t.res_dev = c.ring_res + (size_t)lp.ring * nres;
        t.res_host = res_host + (size_t)p * nres;
        if (rato::readback_poll_enabled()) rato::readback_arm(t.res_host, nres);
      }
      // (one copy: the rows, then x at a fixed offset -- only the rows' and x's used parts travel)
      e = hipMemcpyAsync(b->dev + L.r_tab, b->host + L.r_tab, (size_t)nq * sizeof(rato::BatchProb), hipMemcpyHostToDevice, st);
      if (e == hipSuccess)
        e = hipMemcpyAsync(b->dev + L.r_x, b->host + L.r_x, (size_t)nq * nU * sizeof(double), hipMemcpyHostToDevice, st);
      if (e != hipSuccess) return RATO_EHIP - (int)e;
      const rato::BatchProb* rtab_d = reinterpret_cast<const rato::BatchProb*>(b->dev + L.r_tab);
      rc = car ? rato::launch_car_rowmax_rollout_batch(&b->C, rtab_d, nq, st)
               : rato::launch_drone_rowmax_rollout_batch(&b->P, rtab_d, nq, st);
      if (rc == RATO_OK) {
        if (select_batched) {
          rc = rato::launch_risk_stats_batch(rtab_d, nq, b->M, st);
        } else {   // beyond the one-workgroup selection: each problem's own (on its own workspace), stream-ordered
          for (int i = 0; i < nq && rc == RATO_OK; ++i) {
            const rato_cut_config& c = b->sv[q[i]]->c;
            rc = rato_risk_stats(rtab[i].m_out, b->M, c.alpha, c.thr, c.workspace, c.workspace_bytes, rtab[i].res_dev, stream);
          }
        }
      }
      if (rc == RATO_OK)
        rc = car ? rato::launch_car_tail_rows_batch(&b->C, rtab_d, nq, st) : rato::launch_drone_tail_rows_batch(&b->P, rtab_d, nq, st);
      if (rc == RATO_OK) rc = rato::launch_cut_finish_batch(rtab_d, nq, b->nblk, nc, RATO_N_STATS, st);
      if (rc != RATO_OK) return rc;
      for (int i = 0; i < nq; ++i) {
        e = rato::readback_wait(rtab[i].res_host, nres, st);
        if (e != hipSuccess) return RATO_EHIP - (int)e;
      }
      br.oracle_s += seconds_since(t0);
      ++br.rounds;
      ++*rounds;
      t0 = std::chrono::steady_clock::now();
      b->pool->run(nq, [&](int i) {
        const int p = q[i];
        const int r2 = loop[p]->consume(rtab[i].res_host);
        if (r2 != RATO_OK) status[p] = r2;
      });
      br.master_s += seconds_since(t0);
    }
    // ---- the keep rule and the outputs of every problem that solved its subproblem
    for (int p : act) {
      if (status[p] != RATO_OK) {
        loop[p].reset();
        continue;
      }
      rato_cut_result r = out[p].wired();
      loop[p]->finish(&r);
      loop[p].reset();
      rato_scp_iter& ri = rec[(size_t)p * iters + it];
      scp_record(ri, r, 0.0);
      ri.define_s = ri.solve_s = ri.oracle_s = NAN;   // (per problem only the master's own time is known: brec has the clocks)
      memcpy(us_hist + ((size_t)p * iters + it) * nU, out[p].sol.data(), sizeof(double) * nU);
      us[p] = out[p].sol;
      done[p] = it + 1;
    }
    if (it == iters - 1) {
      e = hipStreamSynchronize(st);
      if (e != hipSuccess) return RATO_EHIP - (int)e;
    }
    br.total_s = seconds_since(t_it);
  }
  return RATO_OK;
}

}  // namespace

extern "C" int rato_scp_batch_run_drone(rato_scp_batch* b, const double* us0, int32_t iters, int32_t first_cvar, double tol,
                                        int32_t max_cuts, double final_cut_above, int32_t check_finite, int32_t* keep,
                                        int32_t* keep_idle_count, int32_t* n_keep, double* us_hist, rato_scp_iter* rec,
                                        rato_scp_batch_iter* brec, int32_t* status, int32_t* done, int32_t* rounds,
                                        void* stream) {
  if (!b || b->system != 0) return RATO_EINVAL;
  return batch_run(b, us0, nullptr, iters, first_cvar, tol, max_cuts, final_cut_above, check_finite, keep, keep_idle_count, n_keep,
                   us_hist, rec, brec, status, done, rounds, stream);
}

extern "C" int rato_scp_batch_run_car(rato_scp_batch* b, const double* us0, const double* goal, int32_t iters,
                                      int32_t first_cvar, double tol, int32_t max_cuts, double final_cut_above,
                                      int32_t check_finite, int32_t* keep, int32_t* keep_idle_count, int32_t* n_keep,
                                      double* us_hist, rato_scp_iter* rec, rato_scp_batch_iter* brec, int32_t* status,
                                      int32_t* done, int32_t* rounds, void* stream) {
  if (!b || b->system != 1) return RATO_EINVAL;
  return batch_run(b, us0, goal, iters, first_cvar, tol, max_cuts, final_cut_above, check_finite, keep, keep_idle_count, n_keep,
                   us_hist, rec, brec, status, done, rounds, stream);
}
