"""GPU: the reduced SCP of many driving problems in ONE lockstep batch (scp.run_driving_reduced_batch ->
rato_scp_batch_run_car) against each problem solved alone by the native loop (scp.run_driving_reduced(native_loop=True) ->
rato_scp_run_car) on a separate, identically built Model: the same iterates, cut counts, t_risk and kept cuts, bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _model(M, S, alpha, seed, method='saa'):
    from riskaversetrajopt_amd import driving
    return driving.Model(M, method, alpha, S=S, rng=np.random.RandomState(seed))


def _solo(model, iters):
    from riskaversetrajopt_amd import scp
    return scp.run_driving_reduced(model, num_scp_iters_max=iters, native_loop=True)


def _assert_bitwise(rb, mb, rs, ms, k):
    assert rb["loop"].startswith("native batch (rato_scp_batch_run_car)"), (k, rb["loop"])
    assert rs["loop"].startswith("native (rato_scp_run_car)"), (k, rs["loop"])
    assert rb["us_hist"].shape == rs["us_hist"].shape, k
    for i in range(rs["us_hist"].shape[0]):
        assert np.array_equal(rb["us_hist"][i], rs["us_hist"][i]), (k, i, np.abs(rb["us_hist"][i] - rs["us_hist"][i]).max())
    assert np.array_equal(rb["cuts"], rs["cuts"]), (k, rb["cuts"], rs["cuts"])
    assert rb["t_risk"] == rs["t_risk"], k
    assert np.array_equal(rb["us"], rs["us"]) and np.array_equal(rb["L2_error"], rs["L2_error"]), k
    assert mb._cut_solver.keep == ms._cut_solver.keep and mb._cut_solver.idle == ms._cut_solver.idle, k


def _run_and_compare(M, S, alphas, seeds, iters, follow_up=True, n_threads=None):
    from riskaversetrajopt_amd import scp
    grid = [(a, s) for a in alphas for s in seeds]
    mb = [_model(M, S, a, s) for a, s in grid]
    ms = [_model(M, S, a, s) for a, s in grid]
    rb = scp.run_driving_reduced_batch(mb, num_scp_iters_max=iters, n_threads=n_threads)
    rs = [_solo(m, iters) for m in ms]
    for k in range(len(grid)):
        _assert_bitwise(rb[k], mb[k], rs[k], ms[k], k)
        if follow_up:   # the solvers were left as a solo run leaves them: the next subproblem agrees too
            ub, tb, ib = mb[k].solve_reduced(rb[k]["us"], iters, final_rows='native')
            us_, ts, is_ = ms[k].solve_reduced(rs[k]["us"], iters, final_rows='native')
            assert np.array_equal(ub, us_) and tb == ts and ib["cuts"] == is_["cuts"], k
            assert mb[k]._cut_solver.keep == ms[k]._cut_solver.keep, k
    total_trips = sum(int(np.sum(r["cuts"])) for r in rs)
    assert 0 < rb[0]["rounds"] <= total_trips + len(grid) * iters
    assert len(rb[0]["define_s"]) == iters and (rb[0]["cumulative_s"] > 0).all()
    return rb, rs


def test_batch_equals_solo_runs_at_the_reference_size():
    """K = 8 (the reference's alphas 0.01 / 0.02 / 0.05 / 0.1 x 2 sample batches), M = 50, S = 20, 15 iterations: bitwise
    against solo runs, and the problems leave their subproblems at different rounds (lockstep with early finishers).
    alpha = 0.01 and 0.02 have alpha M <= 1: the VaR is the maximum of the m values."""
    rb, rs = _run_and_compare(50, 20, (0.01, 0.02, 0.05, 0.1), (11, 12), 15, n_threads=4)
    cuts = np.stack([r["cuts"] for r in rb])
    assert (cuts.max(axis=0) != cuts.min(axis=0)).any()
    # fewer batched round trips than the problems' round trips together
    trips = sum(int(np.sum(r["cuts"])) for r in rs)
    assert rb[0]["rounds"] < trips


def test_batch_multi_block_samples():
    """M = 1000 (four sample blocks, the last one partial), K = 3, 8 iterations"""
    _run_and_compare(1000, 20, (0.02, 0.05, 0.1), (21,), 8)


def test_batch_long_horizon_x_beyond_the_argument_limit():
    """S = 100: 2 S > XARG_MAX, the solo oracle takes x and the staged inputs through device memory as the batch always does"""
    _run_and_compare(100, 100, (0.05, 0.1), (31,), 3)


def test_single_threaded_batch_is_the_same():
    _run_and_compare(50, 20, (0.05, 0.1), (41,), 8, follow_up=False, n_threads=1)


def _bad_samples(M, S, seed):
    from riskaversetrajopt_amd import driving
    st, ws, wr, DWs = driving.sample_uncertain_parameters(M, 'saa', S, np.random.RandomState(seed))
    DWs = DWs.copy()
    DWs[3, 5, 6] = np.nan      # (a pedestrian-velocity noise column: rows 6..7 of DWs are what the dynamics read)
    return st, ws, wr, DWs


def test_failure_is_isolated():
    """a NaN in one problem's noise: that problem fails with the exception class (and status) the solo path gives for the
    same Model, the others are bitwise their solo runs"""
    from riskaversetrajopt_amd import _lib, driving, scp
    M, S, iters = 50, 20, 8
    bad = lambda: driving.Model(M, 'saa', 0.1, S=S, samples=_bad_samples(M, S, 51))
    # what the solo path does with that Model (the ego's rows carry no noise: the NaN shows in the oracle's m values, at the
    # first iteration with the CVaR rows)
    with pytest.raises(_lib.RatoError) as solo:
        _solo(bad(), iters)
    solo_type = type(solo.value)
    assert issubclass(solo_type, _lib.RatoNonFiniteError)
    grid = [(0.05, 52), (0.1, 53)]
    for on_error in ("return", "raise"):
        mb = [_model(M, S, *grid[0]), bad(), _model(M, S, *grid[1])]
        if on_error == "raise":
            with pytest.raises(solo_type, match="problem 1"):
                scp.run_driving_reduced_batch(mb, num_scp_iters_max=iters, on_error="raise")
            continue
        rb = scp.run_driving_reduced_batch(mb, num_scp_iters_max=iters, on_error="return")
        assert type(rb[1]["error"]) is solo_type and rb[1]["status"] == solo_type.status == _lib.RATO_ENONFINITE
        assert 0 <= rb[1]["done"] < iters
        for k, (a, s) in zip((0, 2), grid):
            ms = _model(M, S, a, s)
            _assert_bitwise(rb[k], mb[k], _solo(ms, iters), ms, k)


def test_reference_experiment_grid():
    """the reference's whole driving experiment: 4 alphas x 30 repeats = 120 problems at M = 50, S = 20, 15 iterations in ONE
    batch, every cell on samples of its own, then the Monte-Carlo report per alpha at M = 10000; six cells spread over the
    grid are bitwise their solo runs"""
    from riskaversetrajopt_amd import driving, scp
    S = 20
    mc = driving.Model(10000, 'saa', 0.1, S=S, rng=np.random.RandomState(99))
    alphas, R = (0.01, 0.02, 0.05, 0.1), 30
    out = scp.driving_saa_experiment(alphas=alphas, num_repeats=R, M=50, S=S, iters=15, seed=0, mc_model=mc)
    assert out["us"].shape == (4, R, S, 2) and np.isfinite(out["us"]).all()
    draws = scp.draw_driving_saa_batches(alphas, R, 50, S, 0)
    for i, r in ((0, 0), (0, 29), (1, 7), (2, 13), (3, 21), (3, 29)):
        ms = driving.Model(50, 'saa', alphas[i], S=S, samples=draws[i][r])
        _assert_bitwise(out["results"][i][r], out["models"][i * R + r], _solo(ms, 15), ms, (i, r))
    trips = sum(int(np.sum(out["results"][i][r]["cuts"])) for i in range(4) for r in range(R))
    assert out["rounds"] < trips
    for a in alphas:
        rep = out["reports"][a]
        for key in ("frac_satisfied_mean", "avar_mean", "cost_mean", "frac_satisfied_median", "avar_median", "cost_median"):
            assert np.isfinite(rep[key]), (a, key)
        assert len(rep["avar"]) == R


def test_result_files(tmp_path):
    from riskaversetrajopt_amd import scp
    out = scp.driving_saa_experiment(alphas=(0.05, 0.1), num_repeats=2, M=50, S=20, iters=3, seed=1, results_dir=str(tmp_path))
    for i, a in enumerate(out["alphas"]):
        for r in range(2):
            us, xs = scp.load_results(str(tmp_path / f"driving_alpha={a}_repeat={r}.npy"), 2)
            assert np.array_equal(us, out["us"][i, r]) and xs.shape == (50, 21, 8)


def test_rejections_before_device_work(monkeypatch):
    from riskaversetrajopt_amd import drone_risk, scp
    from riskaversetrajopt_amd import drone_params as DP
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    ok = [_model(50, 20, 0.05, 61), _model(50, 20, 0.1, 62)]
    drone = drone_risk.Model(20, *sample_uncertain_parameters('saa', M=50, S=20, dt=DP.T / 20, rng=np.random.RandomState(66)),
                             'saa', 0.1)
    with pytest.raises(ValueError, match="driving"):
        scp.run_driving_reduced_batch(ok + [drone], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="saa"):
        scp.run_driving_reduced_batch(ok + [_model(50, 20, 0.1, 63, method='baseline')], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="same S and M"):
        scp.run_driving_reduced_batch(ok + [_model(50, 30, 0.1, 64)], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="same S and M"):
        scp.run_driving_reduced_batch(ok + [_model(64, 20, 0.1, 65)], num_scp_iters_max=3)
    with pytest.raises(ValueError, match="twice"):
        scp.run_driving_reduced_batch([ok[0], ok[0]], num_scp_iters_max=3)
    with pytest.raises(ValueError):
        scp.run_driving_reduced_batch([], num_scp_iters_max=3)
    monkeypatch.setenv("RATO_PY_CUT_LOOP", "1")
    with pytest.raises(ValueError, match="native"):
        scp.run_driving_reduced_batch(ok, num_scp_iters_max=3)
    for m in ok:    # nothing ran: no cut solver was even built
        assert getattr(m, "_cut_solver", None) is None


def test_a_batch_runs_only_with_its_own_system():
    """C level: rato_scp_batch_run_drone answers RATO_EINVAL for a driving batch and rato_scp_batch_run_car for a drone batch
    (before reading any other argument), and solvers of both systems do not make a batch"""
    import torch
    from riskaversetrajopt_amd import _lib, drone_risk
    from riskaversetrajopt_amd import drone_params as DP
    from riskaversetrajopt_amd.drone_utils import sample_uncertain_parameters
    lib = _lib.load()
    cars = [_model(50, 20, 0.05, 71), _model(50, 20, 0.1, 72)]
    drones = [drone_risk.Model(20, *sample_uncertain_parameters('saa', M=50, S=20, dt=DP.T / 20, rng=np.random.RandomState(s)),
                               'saa', 0.1) for s in (73, 74)]
    handles = {}
    for name, models in (("car", cars), ("drone", drones)):
        solvers = [m._native_loop_solver() for m in models]
        assert all(cs is not None and cs.native_loop_applies() for cs in solvers)
        handles[name] = [cs._native_solver() for cs in solvers]
    keep = []                                                   # (buffers that outlive the batches)

    def create(hs):
        arr = (C.c_void_p * len(hs))(*hs)
        d, h = C.c_size_t(0), C.c_size_t(0)
        rc = lib.rato_scp_batch_bytes(arr, len(hs), C.byref(d), C.byref(h))
        if rc != 0:
            return rc, None
        dev = torch.empty(d.value + 256, dtype=torch.uint8, device=cars[0].device)
        host = torch.zeros(h.value + 16, dtype=torch.uint8).pin_memory()
        keep.extend((dev, host, arr))
        b = C.c_void_p()
        rc = lib.rato_scp_batch_create(C.byref(b), arr, len(hs), 2, (dev.data_ptr() + 255) // 256 * 256, d.value,
                                       (host.data_ptr() + 15) // 16 * 16, h.value)
        return rc, b

    assert create([handles["car"][0], handles["drone"][0]])[0] == -1
    rc, b_car = create(handles["car"])
    assert rc == 0
    rc, b_drone = create(handles["drone"])
    assert rc == 0
    try:
        nine = [None] * 9
        assert lib.rato_scp_batch_run_drone(b_car, None, 1, 2, 1e-9, 400, 1e-11, 1, *nine, None) == -1
        assert lib.rato_scp_batch_run_car(b_drone, None, None, 1, 1, 1e-9, 400, 1e-11, 1, *nine, None) == -1
    finally:
        lib.rato_scp_batch_destroy(b_car)
        lib.rato_scp_batch_destroy(b_drone)
