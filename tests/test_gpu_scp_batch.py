"""GPU: the reduced SCP of many drone problems in ONE lockstep batch (scp.run_drone_reduced_batch ->
rato_scp_batch_run_drone) against each problem solved alone by the native loop (scp.run_drone_reduced) on a separate,
identically built Model: the same iterates, cut counts, t_risk and kept cuts, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _model(M, S, alpha, seed, method='saa'):
    from riskaversetrajopt_amd import drone_risk
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    DWs, masses, Q = sample_uncertain_parameters(method, M=M, S=S, dt=P.T / S, rng=np.random.RandomState(seed))
    return drone_risk.Model(S, DWs, masses, Q, method, alpha)


def _grid(M, S, alphas, seeds):
    return [(a, s) for a in alphas for s in seeds]


def _assert_bitwise(rb, mb, rs, ms, k):
    assert rb["loop"].startswith("native batch"), (k, rb["loop"])
    assert rs["loop"].startswith("native"), (k, rs["loop"])
    assert rb["us_hist"].shape == rs["us_hist"].shape, k
    for i in range(rs["us_hist"].shape[0]):
        assert np.array_equal(rb["us_hist"][i], rs["us_hist"][i]), (k, i, np.abs(rb["us_hist"][i] - rs["us_hist"][i]).max())
    assert np.array_equal(rb["cuts"], rs["cuts"]), (k, rb["cuts"], rs["cuts"])
    assert rb["t_risk"] == rs["t_risk"], k
    assert np.array_equal(rb["us"], rs["us"]) and np.array_equal(rb["L2_error"], rs["L2_error"]), k
    assert mb._cut_solver.keep == ms._cut_solver.keep and mb._cut_solver.idle == ms._cut_solver.idle, k


def _run_and_compare(M, S, alphas, seeds, iters, follow_up=True, n_threads=None):
    from riskaversetrajopt_amd import scp
    grid = _grid(M, S, alphas, seeds)
    mb = [_model(M, S, a, s) for a, s in grid]
    ms = [_model(M, S, a, s) for a, s in grid]
    rb = scp.run_drone_reduced_batch(mb, num_scp_iters_max=iters, n_threads=n_threads)
    rs = [scp.run_drone_reduced(m, num_scp_iters_max=iters) for m in ms]
    for k in range(len(grid)):
        _assert_bitwise(rb[k], mb[k], rs[k], ms[k], k)
        if follow_up:   # the solvers were left as a solo run leaves them: the next subproblem agrees too
            ub, tb, ib = mb[k].solve_reduced(rb[k]["us"], iters)
            us_, ts, is_ = ms[k].solve_reduced(rs[k]["us"], iters)
            assert np.array_equal(ub, us_) and tb == ts and ib["cuts"] == is_["cuts"], k
    total_trips = sum(int(np.sum(r["cuts"])) for r in rs)
    assert 0 < rb[0]["rounds"] <= total_trips + len(grid) * iters
    assert len(rb[0]["define_s"]) == iters and (rb[0]["cumulative_s"] > 0).all()
    return rb, rs


def test_batch_equals_solo_runs_at_the_reference_size():
    """K = 8 (2 sample batches x alphas 0.05 / 0.1 / 0.2 / 0.3), M = 50, S = 20, 60 iterations: bitwise against solo runs,
    and the problems leave their subproblems at different rounds (lockstep with early finishers is exercised)"""
    rb, rs = _run_and_compare(50, 20, (0.05, 0.1, 0.2, 0.3), (11, 12), 60, n_threads=4)
    cuts = np.stack([r["cuts"] for r in rb])
    assert (cuts.max(axis=0) != cuts.min(axis=0)).any()
    # fewer batched round trips than the problems' round trips together
    trips = sum(int(np.sum(r["cuts"])) for r in rs)
    assert rb[0]["rounds"] < trips


def test_batch_multi_block_samples():
    """M = 1000 (four sample blocks, the last one partial), K = 3, 20 iterations"""
    _run_and_compare(1000, 20, (0.05, 0.1, 0.2), (21,), 20)


def test_batch_long_horizon_x_beyond_the_argument_limit():
    """S = 70: 3 S > XARG_MAX, the solo oracle takes x through device memory as the batch always does"""
    _run_and_compare(300, 70, (0.1, 0.2), (31, 32), 4)


def test_single_threaded_batch_is_the_same():
    _run_and_compare(50, 20, (0.1, 0.3), (41,), 12, follow_up=False, n_threads=1)


def test_failure_is_isolated():
    """a NaN in one problem's noise: that problem fails (RatoNonFiniteError / its status), the others are bitwise their
    solo runs"""
    from riskaversetrajopt_amd import _lib, drone_risk, scp
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    M, S, iters = 50, 20, 12
    DWs, masses, Q = sample_uncertain_parameters('saa', M=M, S=S, dt=P.T / S, rng=np.random.RandomState(51))
    bad = DWs.copy()
    bad[3, 5, 3] = np.nan      # (a velocity-noise column: rows 3..5 of DWs drive the dynamics)
    grid = [(0.1, 52), (0.2, 53)]
    for on_error in ("return", "raise"):
        mb = [_model(M, S, a, s) for a, s in grid[:1]] + [drone_risk.Model(S, bad, masses, Q, 'saa', 0.1)] + \
             [_model(M, S, a, s) for a, s in grid[1:]]
        if on_error == "raise":
            with pytest.raises(_lib.RatoNonFiniteError, match="problem 1"):
                scp.run_drone_reduced_batch(mb, num_scp_iters_max=iters, on_error="raise")
            continue
        rb = scp.run_drone_reduced_batch(mb, num_scp_iters_max=iters, on_error="return")
        assert rb[1]["status"] == _lib.RATO_ENONFINITE and isinstance(rb[1]["error"], _lib.RatoNonFiniteError)
        assert rb[1]["done"] == 0
        with pytest.raises(_lib.RatoNonFiniteError):     # (what the solo path does with that Model)
            scp.run_drone_reduced(drone_risk.Model(S, bad, masses, Q, 'saa', 0.1), num_scp_iters_max=iters)
        for k, (a, s) in zip((0, 2), grid):
            ms = _model(M, S, a, s)
            _assert_bitwise(rb[k], mb[k], scp.run_drone_reduced(ms, num_scp_iters_max=iters), ms, k)


def test_reference_experiment_grid():
    """the reference's whole drone experiment: 4 alphas x 30 repeats = 120 problems at M = 50, S = 20, 60 iterations in ONE
    batch, then the Monte-Carlo report per alpha at M = 10000; six problems spread over the grid are bitwise their solo runs"""
    from riskaversetrajopt_amd import drone_risk, scp
    from riskaversetrajopt_amd import drone_params as P
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    S = 20
    DWs, masses, Q = sample_uncertain_parameters('saa', M=10000, S=S, dt=P.T / S, rng=np.random.RandomState(99))
    mc = drone_risk.Model(S, DWs, masses, Q, 'saa', 0.1)
    alphas, R = (0.05, 0.1, 0.2, 0.3), 30
    out = scp.drone_saa_experiment(alphas=alphas, num_repeats=R, M=50, S=S, iters=60, seed=0, mc_model=mc)
    assert out["us"].shape == (4, R, S, 3) and np.isfinite(out["us"]).all()
    batches = scp.draw_saa_batches(R, 50, S, 0)
    trips = 0
    for i, r in ((0, 0), (0, 29), (1, 7), (2, 13), (3, 21), (3, 29)):
        ms = drone_risk.Model(S, *batches[r], 'saa', alphas[i])
        rs = scp.run_drone_reduced(ms, num_scp_iters_max=60)
        _assert_bitwise(out["results"][i][r], out["models"][i * R + r], rs, ms, (i, r))
    trips = sum(int(np.sum(out["results"][i][r]["cuts"])) for i in range(4) for r in range(R))
    assert out["rounds"] < trips
    for a in alphas:
        rep = out["reports"][a]
        for key in ("frac_satisfied_mean", "avar_mean", "cost_mean", "frac_satisfied_median", "avar_median", "cost_median"):
            assert np.isfinite(rep[key]), (a, key)
        assert len(rep["avar"]) == R


def test_rejections_before_device_work(monkeypatch):
    from riskaversetrajopt_amd import scp
    from riskaversetrajopt_amd import driving
    ok = [_model(50, 20, 0.1, 61), _model(50, 20, 0.2, 62)]
    with pytest.raises(ValueError, match="saa"):
        scp.run_drone_reduced_batch(ok + [_model(50, 20, 0.1, 63, method='baseline')], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="same S and M"):
        scp.run_drone_reduced_batch(ok + [_model(50, 30, 0.1, 64)], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="same S and M"):
        scp.run_drone_reduced_batch(ok + [_model(64, 20, 0.1, 65)], num_scp_iters_max=3)
    car = driving.Model(32, 'saa', 0.1, S=20)
    with pytest.raises(ValueError, match="drone"):
        scp.run_drone_reduced_batch(ok + [car], num_scp_iters_max=3)
    with pytest.raises(ValueError):
        scp.run_drone_reduced_batch([ok[0], ok[0]], num_scp_iters_max=3)
    monkeypatch.setenv("RATO_PY_CUT_LOOP", "1")
    with pytest.raises(ValueError, match="native"):
        scp.run_drone_reduced_batch(ok, num_scp_iters_max=3)
    for m in ok:    # nothing ran: no cut solver was even built
        assert getattr(m, "_cut_solver", None) is None
