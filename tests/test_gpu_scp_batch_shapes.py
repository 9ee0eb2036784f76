"""GPU: the lockstep SCP batch (rato_scp_batch_run_drone / rato_scp_batch_run_car, csrc/cutloop.hip) at the launch shapes its
table-driven kernels had never run at -- generators-batch, define-sums-batch, tail-kept-batch (plain and union),
kept-sums-batch, rowmax-rollout-batch, rs_small_tab, tail-rows-batch and cut-finish-batch have no C entry point of their own,
so they are reached through the batch run.

Method: tests/test_gpu_scp_batch.py's and tests/test_gpu_scp_car_batch.py's, with their helpers -- the batch against each
problem solved alone by the native solo loop on an identically built Model, bit for bit (iterates, cut counts, t_risk, kept cuts
and idle counts, the follow-up subproblem).  The solo kernels are held to the fp64 oracle at every horizon edge by
tests/test_gpu_cut_producers.py and tests/test_gpu_cut_tails.py; one case per system ties the batch to the oracle directly
(``test_large_batch_equals_the_fp64_oracle``).

Every case asserts that the branch it exists for was taken (``recycled``: the kept cuts a problem entered an iteration with;
``cuts`` per problem and iteration; ``rounds_per_iter``); inputs that do not produce the condition fail the test.  Seeds were
chosen here, on the MI355X, as the first ones tried that produce the condition in the fewest iterations.

Wall time on the MI355X: 5.7 s for the 20 cases; the two oracle cases 1.2 s and 0.8 s (the fp64 oracle on 12289 samples),
test_sample_block_edges[drone-255] 0.7 s (it pays the first launches of the process), every other case <= 0.1 s.  The oracle
cases sit at 0.98 (drone) and 0.995 (driving) of the bound on m -- the final rounding to fp32, as in
tests/test_gpu_cut_producers.py -- and at <= 0.012 of the bounds on the cut sums.

Mutation check (scratch builds of the library, one in-bounds mistake each; this file and the two older batch files once per
build):
  per-problem selection reads rtab[0].m_out for every problem   test_large_batch_equals_the_fp64_oracle[drone | driving],
                                                                test_per_problem_selection_forced_at_a_small_size[drone |
                                                                driving]; the older files pass
  kept-cut chunks of 15 cuts instead of 16                      test_more_than_sixteen_kept_cuts_drone,
                                                                test_union_plain_switch[175]; the older files pass
  define sums over nblk - 1 blocks when nblk > 1                five drone cases here (sample_block_edges[257], both M = 12288 /
                                                                12289 cases, smallest_horizon, the rounds case) -- and
                                                                test_batch_multi_block_samples and
                                                                test_batch_long_horizon_x_beyond_the_argument_limit of
                                                                tests/test_gpu_scp_batch.py: that mistake was covered before"""
import math

import numpy as np
import pytest

import test_gpu_scp_batch as D
import test_gpu_scp_car_batch as Cb
from tests import _cut_designs as cd
from tests import _tail_patterns as tp

pytestmark = pytest.mark.gpu

RS_SMALL_MAX = 12 * 1024        # csrc/rato_select.h: the largest one-workgroup selection
TRU_KMAX, WAVE = 16, 64         # csrc/cvar.hip: cuts per chunk of the union form; RATO_WAVE


class _System:
    def __init__(self, name, mod, n_u, first_cvar):
        self.name, self.mod, self.n_u, self.first_cvar = name, mod, n_u, first_cvar

    def model(self, M, S, alpha, seed):
        return self.mod._model(M, S, alpha, seed)

    def batch(self, models, iters):
        from riskaversetrajopt_amd import scp
        run = scp.run_drone_reduced_batch if self.name == "drone" else scp.run_driving_reduced_batch
        return run(models, num_scp_iters_max=iters)

    def solo(self, model, iters):
        from riskaversetrajopt_amd import scp
        if self.name == "drone":
            return scp.run_drone_reduced(model, num_scp_iters_max=iters)
        return Cb._solo(model, iters)

    def follow_up(self, model, us, iters):
        kw = {} if self.name == "drone" else {"final_rows": "native"}
        return model.solve_reduced(us, iters, **kw)


DRONE = _System("drone", D, 3, 2)       # (first_cvar: the first iteration with the CVaR rows, i.e. with oracle rounds)
CAR = _System("driving", Cb, 2, 1)
SYSTEMS = {"drone": DRONE, "driving": CAR}


def run_and_compare(system, M, S, grid, iters):
    """the batch and the solo runs of ``grid`` = [(alpha, seed)], compared bit for bit -> (batch results, batch Models)"""
    mb = [system.model(M, S, a, s) for a, s in grid]
    ms = [system.model(M, S, a, s) for a, s in grid]
    rb = system.batch(mb, iters)
    rs = [system.solo(m, iters) for m in ms]
    for k in range(len(grid)):
        system.mod._assert_bitwise(rb[k], mb[k], rs[k], ms[k], k)
        assert rb[k]["loop"].startswith("native batch"), rb[k]["loop"]
        ub, tb, ib = system.follow_up(mb[k], rb[k]["us"], iters)
        us_, ts, is_ = system.follow_up(ms[k], rs[k]["us"], iters)
        assert np.array_equal(ub, us_) and tb == ts and ib["cuts"] == is_["cuts"], k
        assert mb[k]._cut_solver.keep == ms[k]._cut_solver.keep, k
    assert sum(int(np.sum(r["cuts"])) for r in rb) > 0 and rb[0]["rounds"] > 0     # the oracle ran
    return rb, mb


def _recycled(rb):
    return np.stack([r["recycled"] for r in rb])      # (problem, iteration)


# ---- sample-block edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [255, 256, 257])
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_sample_block_edges(system, M):
    """M = 255 / 256 / 257 at S = 20, K = 3: one block short of full, exactly full, and a second block of one sample.  The last
    iteration starts with kept cuts (tail-kept-batch and kept-sums-batch run over the same blocks)."""
    s = SYSTEMS[system]
    grid = [(0.05, 91), (0.1, 92), (0.3, 93)] if system == "drone" else [(0.02, 91), (0.05, 92), (0.1, 93)]
    rb, _ = run_and_compare(s, M, 20, grid, s.first_cvar + 2)
    assert (_recycled(rb)[:, -1] >= 1).all()


# ---- the selection: the largest one-workgroup size, the first size beyond it, and the forced per-problem form ----------------
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_largest_one_workgroup_selection(system):
    """M = 12288 = RS_SMALL_MAX: rs_small_tab with every key slot of its one workgroup per problem in use; K = 2, the first
    iteration with oracle rounds"""
    from riskaversetrajopt_amd import _lib
    s = SYSTEMS[system]
    assert _lib.load() is not None and RS_SMALL_MAX == 12288
    grid = [(0.05, 101), (0.2, 102)] if system == "drone" else [(0.02, 101), (0.1, 102)]
    rb, _ = run_and_compare(s, RS_SMALL_MAX, 20, grid, s.first_cvar + 1)
    assert all(r["cuts"][-1] >= 3 for r in rb)


def _last_evaluation(model, r):
    """the ring slot of the problem's last oracle evaluation: the one whose VaR is t_risk - slack"""
    cs = model._cut_solver
    rec = cs.ring_res.cpu().numpy()
    slot = int(np.argmin(np.abs(rec[:cs.cap - 1, 0] - (r["t_risk"] - r["slack"][-1]))))
    assert rec[slot, 0] + r["slack"][-1] == r["t_risk"], "no ring slot holds the VaR of the returned t_risk"
    return slot, cs.ring_m[slot].cpu().numpy(), cs.ring_arg[slot].cpu().numpy(), rec[slot]


def _samples(system, M, S, seed):
    if system == "drone":
        from riskaversetrajopt_amd import drone_params as P
        from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
        return sample_uncertain_parameters('saa', M=M, S=S, dt=P.T / S, rng=np.random.RandomState(seed))
    from riskaversetrajopt_amd import driving
    return driving.sample_uncertain_parameters(M, 'saa', S, np.random.RandomState(seed))


def _model_on(system, S, samples, alpha):
    if system == "drone":
        from riskaversetrajopt_amd import drone_risk
        return drone_risk.Model(S, *samples, 'saa', alpha)
    from riskaversetrajopt_amd import driving
    return driving.Model(samples[0].shape[0], 'saa', alpha, S=S, samples=samples)


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_large_batch_equals_the_fp64_oracle(system):
    """M = 12289 = RS_SMALL_MAX + 1, K = 2: ``select_batched`` is false, every problem's selection is its own rato_risk_stats on its
    own workspace between the batched rowmax and tail launches.  Bitwise against the solo runs, and directly against oracle/:
    for the problem with the most rounds in the last iteration (its last evaluation is AT the returned controls: cuts ==
    rounds - 1, asserted) the m values, the returned t_risk = VaR + slack and the cut sums of that evaluation equal the fp64
    oracle's at the returned controls, within the bounds the solo kernels are held to (tests/_cut_designs.m_limit,
    tests/_tail_patterns.rollout_tolerance)."""
    from riskaversetrajopt_amd import stats
    from test_gpu_cut_producers import _check_against_rows, _reference
    s = SYSTEMS[system]
    M, S = RS_SMALL_MAX + 1, 20
    grid = [(0.05, 101), (0.2, 102)] if system == "drone" else [(0.02, 101), (0.1, 102)]
    iters = s.first_cvar + 1
    # (no follow-up subproblem before the rings are read: it would reuse their slots)
    drawn = [_samples(system, M, S, sd) for a, sd in grid]
    mb = [_model_on(system, S, smp, a) for smp, (a, sd) in zip(drawn, grid)]
    ms = [_model_on(system, S, smp, a) for smp, (a, sd) in zip(drawn, grid)]
    rb = s.batch(mb, iters)
    rs = [s.solo(m, iters) for m in ms]
    for k in range(len(grid)):
        s.mod._assert_bitwise(rb[k], mb[k], rs[k], ms[k], k)
    last = [int(r["cuts"][-1]) for r in rb]
    k = int(np.argmax(last))
    assert last[k] == rb[k]["rounds_per_iter"][-1] - 1 and last[k] >= 3, (last, rb[k]["rounds_per_iter"])
    alpha, seed = grid[k]
    r = rb[k]
    slot, m32, arg, rec = _last_evaluation(mb[k], r)
    u_lin, us = r["us_hist"][-2], r["us"]
    x = us - u_lin
    const = cd.drone_const(S) if system == "drone" else cd.car_const(S)
    samples = [cd.r32(a) for a in drawn[k]]          # (rounded to fp32, as the device holds them)
    rows, spread = _reference("drone" if system == "drone" else "driving", const, samples, u_lin, x)
    worst = []
    _check_against_rows(f"batch {system} M={M}", m32, arg, rows, spread, worst)
    # the selection: the documented rule on the device's own m values, and t_risk is its VaR plus the master's slack
    w, thr, n_gt, n_eq, lam = tp.weights(m32, alpha, M)
    td = np.float32(rec[10])
    lam_d = min(max((alpha * M - rec[8]) / rec[9], 0.0), 1.0) if rec[9] > 0 else 0.0
    assert np.array_equal((m32 > td) * 1.0 + (m32 == td) * lam_d, w)
    # ... and the VaR of the oracle's own m values, to the bound on m
    m_o = rows.max(axis=1)
    scale = max(1.0, np.abs(rows).max())
    k_th = np.sort(m_o)[::-1][min(max(int(math.ceil(alpha * M - 1e-12)), 1), M) - 1]
    assert abs((r["t_risk"] - r["slack"][-1]) - k_th) <= float(np.max(cd.m_limit(m_o, scale, spread)))
    # the cut of that evaluation
    dense = (cd.drone_dense if system == "drone" else cd.car_dense)(const, samples, u_lin, x, arg=arg.astype(np.int64))
    nw = 2 * (S - 1)
    cols = dense["G_arg"].reshape(M, S, s.n_u)[:, :S - 1, :2].reshape(M, nw)
    ref = tp.cut_sums(cols[:, None, :], dense["g_arg"][:, None], w, np.zeros(M, dtype=np.int64), m32 == np.float32(thr), lam)
    tol_grad, tol_off = tp.rollout_tolerance(ref)
    sums = rec[stats.N_STATS:]
    e_grad, e_off = np.abs(sums[:nw] - ref["grad"]), abs(sums[nw] - ref["off"])
    print(f"{system}: m err/limit {max(worst):.3f}, cut gradient err/bound {float(np.max(e_grad / tol_grad)):.3f}, "
          f"offset {e_off / tol_off:.3f}")
    assert np.all(e_grad <= tol_grad) and e_off <= tol_off, (float(np.max(e_grad / tol_grad)), e_off / tol_off)


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_per_problem_selection_forced_at_a_small_size(system, monkeypatch):
    """RATO_RS_PATH=m at M = 50: the batch reads the variable on every call and takes the per-problem branch (one
    rato_risk_stats per problem and round); batch and solo both run under it (results of different selection forms are not
    compared: their fp64 sums are ordered differently)"""
    s = SYSTEMS[system]
    grid = [(0.05, 111), (0.1, 112), (0.3, 113)] if system == "drone" else [(0.02, 111), (0.05, 112), (0.1, 113)]
    # rato_risk_stats itself reads the variable once per process, for its own launch form: one selection before it is set
    # pins that form, so that this test leaves every later test of the process what it was
    s.solo(s.model(50, 20, grid[0][0], 110), s.first_cvar + 1)
    monkeypatch.setenv("RATO_RS_PATH", "m")
    rb, _ = run_and_compare(s, 50, 20, grid, s.first_cvar + 2)
    assert (_recycled(rb)[:, -1] >= 1).all()


# ---- the smallest horizon ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_smallest_horizon(system):
    """S = 2 at M = 300 (two sample blocks): one control step enters the rows, nc = 3.  A kept cut is re-linearized in the last
    iteration.  S = 1 is refused by the batch before any device work."""
    s = SYSTEMS[system]
    grid = [(0.05, 81), (0.1, 82), (0.3, 83)] if system == "drone" else [(0.02, 81), (0.05, 82), (0.1, 83)]
    rb, _ = run_and_compare(s, 300, 2, grid, s.first_cvar + 2)
    assert _recycled(rb)[:, -1].max() >= 1
    one = [s.model(300, 1, a, sd) for a, sd in grid[:2]]
    with pytest.raises(ValueError, match="S >= 2"):
        s.batch(one, 3)
    for m in one:    # nothing ran: no cut solver was even built
        assert getattr(m, "_cut_solver", None) is None


# ---- more than 16 kept cuts --------------------------------------------------------------------------------------------
def test_more_than_sixteen_kept_cuts_drone(monkeypatch):
    """RATO_KEEP_RECENT=28 (read when the cut solver is built, inside the runs), M = 50, S = 20: the last iteration starts with
    14, 21 and 19 kept cuts -- in ONE tail-kept-batch launch of the union form a single partial chunk (14), and twice a full
    chunk of 16 followed by a partial one (5, 3): kn_max = 16 beside smaller chunks, k0 = 16 as a chunk's first cut"""
    monkeypatch.setenv("RATO_KEEP_RECENT", "28")
    rb, _ = run_and_compare(DRONE, 50, 20, [(0.05, 111), (0.1, 112), (0.3, 113)], 4)
    n_keep = _recycled(rb)[:, -1]
    assert ((n_keep > TRU_KMAX) & (n_keep < 2 * TRU_KMAX)).any() and ((n_keep >= 2) & (n_keep <= TRU_KMAX)).any(), n_keep
    assert ((n_keep > TRU_KMAX) & (n_keep % TRU_KMAX != 0)).any(), n_keep


def test_more_than_sixteen_kept_cuts_driving(monkeypatch):
    """the driving batch has no union form: every kept cut is a row of tail-kept-batch, and kept-sums-batch sums max(n_keep) nc
    columns.  RATO_KEEP_RECENT=28, M = 257: the last iteration starts with 18, 15 and 11 kept cuts"""
    monkeypatch.setenv("RATO_KEEP_RECENT", "28")
    rb, _ = run_and_compare(CAR, 257, 20, [(0.01, 72), (0.02, 71), (0.05, 72)], 5)
    n_keep = _recycled(rb)[:, -1]
    assert (n_keep > TRU_KMAX).any() and ((n_keep >= 2) & (n_keep <= TRU_KMAX)).any(), n_keep


# ---- the union / plain switch of the kept cuts -----------------------------------------------------------------------------
def tail_union_lds_bytes(S, K):
    """csrc/cvar.hip"""
    nc = 2 * (S - 1) + 1
    return 8 * (K * nc + K * 2 * WAVE) + 4 * S * 2 * WAVE + (4 + 4) * K * WAVE + 4 * S


def union_form(S, K):
    """rato::drone_tail_union_form"""
    return K > 1 and tail_union_lds_bytes(S, min(K, TRU_KMAX)) + 4096 <= 160 * 1024


S_UNION = max(S for S in range(2, 400) if union_form(S, TRU_KMAX))      # the largest S at which 16 or more cuts are a union
assert S_UNION == 175 and not union_form(S_UNION + 1, TRU_KMAX) and union_form(S_UNION + 1, TRU_KMAX - 1)


@pytest.mark.parametrize("S", [S_UNION, S_UNION + 1])
def test_union_plain_switch(S, monkeypatch):
    """tail_union_lds_bytes(S, min(K, 16)) + 4096 <= 160 KiB holds for K >= 16 up to S = 175 and fails from S = 176.  With
    RATO_KEEP_RECENT=24 both problems enter the last iteration with >= 16 kept cuts: at S = 175 they are union rows (a full
    chunk of 16 and a partial one), at S = 176 plain rows, one per cut"""
    monkeypatch.setenv("RATO_KEEP_RECENT", "24")
    rb, _ = run_and_compare(DRONE, 50, S, [(0.1, 121), (0.3, 122)], 4)
    n_keep = _recycled(rb)[:, -1]
    assert (n_keep >= TRU_KMAX).all(), n_keep
    assert all(union_form(S, int(k)) == (S == S_UNION) for k in n_keep)


# ---- problems that leave the rounds at different times ---------------------------------------------------------------------
# drone: iteration 7 is the first of the ten (alpha, seed) tried in which a problem needs no cut (0 / 11 / 13 cuts);
# driving: iteration 4 (0 / 3 / 3 cuts)
ROUNDS = {"drone": ([(0.1, 72), (0.3, 72), (0.6, 71)], 8), "driving": ([(0.3, 71), (0.02, 71), (0.05, 72)], 5)}


@pytest.mark.parametrize("system", ["drone", "driving"])
def test_a_problem_finishes_in_the_first_round_while_another_takes_three(system):
    """M = 257: in the last iteration one problem's first evaluation already satisfies the stopping test (0 cuts: it leaves
    after round 1) while another adds >= 3 cuts (>= 3 rounds): the round tables shrink while they are being indexed"""
    s = SYSTEMS[system]
    grid, iters = ROUNDS[system]
    rb, _ = run_and_compare(s, 257, 20, grid, iters)
    cuts = np.stack([r["cuts"] for r in rb])[:, s.first_cvar:]
    both = (cuts.min(axis=0) == 0) & (cuts.max(axis=0) >= 3)
    assert both.any(), cuts
    assert rb[0]["rounds_per_iter"][s.first_cvar:][both].min() >= 3
