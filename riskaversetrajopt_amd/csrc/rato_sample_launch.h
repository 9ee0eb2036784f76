// The host-side launch policy the drone and driving sample kernels share (drone.hip, driving.hip): where the statistics
// of Z run, and how a row-parallel linearize launch gets its plan and its tile queue.  The rule that picks the launch
// geometry itself is rato_rows_plan.h's; the kernels, their argument lists and their LDS sizes stay with their files.
#pragma once
#include "rato_common.h"
#include "rato_rows_plan.h"
#include "rato_select.h"

namespace rato {

// params.stats_* of either params struct: the statistics of the Z a call produces (rato_saa.h)
struct StatsRequest {
  void* workspace;   // NULL: none asked for
  double* out;
  double alpha;
  float thr;
  int flags;
  bool ok(const float* Z) const { return !workspace || (Z && out && alpha > 0.0 && alpha <= 1.0); }
};
template <class Params>
StatsRequest stats_request(const Params* p) {
  return {p->stats_workspace, p->stats_out, p->stats_alpha, p->stats_thr, p->stats_flags};
}

// Where a request's statistics run: in extra workgroups at the end of the producer's own launch (tail.ws != NULL; grid and
// lds are then what to launch with), or as rato_risk_stats behind it (behind).  Neither without a request.
struct StatsPlacement {
  rato_sel::StatsTail tail;
  int grid;
  size_t lds;
  bool behind;
};
// `grid` producer workgroups of NT threads with `lds` bytes of their own; may_carry: the launch can take the statistics
// along (the caller's answer: every workgroup resident at once / asked for by the caller).  RATO_EINVAL: it may, but M is
// beyond the one-launch forms of the selection (use rato_risk_stats behind the kernel).
template <int NT>
int place_stats(const StatsRequest& rq, int64_t M, int grid, size_t lds, bool may_carry, StatsPlacement& sp) {
  sp = {{}, grid, lds, rq.workspace && !may_carry};
  if (!rq.workspace || !may_carry) return RATO_OK;
  const int extra = rato_sel::stats_tail_workgroups<NT>(M, sp.tail.G);
  if (extra < 0) return RATO_EINVAL;
  sp.tail.ws = static_cast<rato_sel::Workspace*>(rq.workspace);
  sp.tail.out = rq.out;
  sp.tail.alpha = rq.alpha;
  sp.tail.thr = rq.thr;
  sp.tail.n_prod = grid;
  rato_sel::stats_rank(M, rq.alpha, sp.tail.k, sp.tail.var_is_max);
  sp.grid = grid + extra;
  if (sp.lds < rato_sel::rs_body_lds_bytes<NT>()) sp.lds = rato_sel::rs_body_lds_bytes<NT>();
  return RATO_OK;
}
// the call that ends a launch site: rato_risk_stats on the producer's stream when the statistics were placed behind it
inline int stats_behind(const StatsRequest& rq, bool behind, const float* Z, int64_t M, void* stream) {
  if (!behind) return RATO_OK;
  return rato_risk_stats(Z, M, rq.alpha, rq.thr, rq.workspace, rato_risk_stats_workspace_bytes(M), rq.out, stream);
}

// A row-parallel linearize launch before its kernel-specific parts.  plan_with(queue_available) -> rato_rows_plan is the
// file's call of rato_rows_plan.h.  A queue is taken only for a shape that wants one (a captured launch consumes an entry
// of the pool for good; launches that overlap on different streams get different queues, and each launch leaves its queue
// zeroed); when the pool has none left the shape falls back to the static form.  The statistics ride in the launch only
// while the whole grid is resident at once -- no queue; otherwise behind it.
struct RowsLaunch {
  rato_rows_plan plan;
  unsigned* queue;   // NULL: static form
  StatsPlacement stats;
};
template <int NT, class PlanWith>
int prepare_rows_launch(PlanWith&& plan_with, TileQueuePool& pool, unsigned* (*resolve)(), hipStream_t st,
                        const StatsRequest& rq, int64_t M, size_t lds, RowsLaunch& rl) {
  rl.plan = plan_with(true);
  rl.queue = rl.plan.wants_queue ? pool.take(st, resolve) : nullptr;
  if (rl.plan.wants_queue && !rl.queue) rl.plan = plan_with(false);
  return place_stats<NT>(rq, M, rl.plan.workgroups, lds, !rl.queue, rl.stats);
}

}  // namespace rato
