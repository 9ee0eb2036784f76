"""GPU: the reduced SCP of the driving problem as ONE native call (scp.run_driving_reduced(native_loop=True) ->
rato_scp_run_car) against its per-iteration checker (native_loop=False, final_rows='native': one rato_cut_begin + one
rato_cut_solve call per iteration from Python, the same native final rows) on a separate, identically built Model: the same
iterates, cut counts, t_risk, L2 errors and kept cuts, bit for bit, and the same next subproblem."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _model(M, S, alpha, seed, method='saa'):
    from riskaversetrajopt_amd import driving
    return driving.Model(M, method, alpha, S=S, rng=np.random.RandomState(seed))


@pytest.mark.parametrize("M,S,iters,alpha", [
    (50, 20, 15, 0.05),     # the reference's size
    (300, 12, 6, 0.05),     # two sample blocks, the last one partial
    (100, 100, 3, 0.05),    # 2 S > 192: x and the staged inputs go through device memory
])
def test_native_loop_equals_the_per_iteration_loop(M, S, iters, alpha):
    from riskaversetrajopt_amd import scp
    mn, mp = _model(M, S, alpha, 7), _model(M, S, alpha, 7)
    rn = scp.run_driving_reduced(mn, num_scp_iters_max=iters, native_loop=True)
    rp = scp.run_driving_reduced(mp, num_scp_iters_max=iters, native_loop=False, final_rows='native')
    assert rn["loop"].startswith("native (rato_scp_run_car)"), rn["loop"]
    assert rp["loop"].startswith("python"), rp["loop"]
    assert rn["us_hist"].shape == rp["us_hist"].shape == (iters, S, 2)
    for i in range(iters):
        assert np.array_equal(rn["us_hist"][i], rp["us_hist"][i]), (i, np.abs(rn["us_hist"][i] - rp["us_hist"][i]).max())
    assert np.array_equal(rn["cuts"], rp["cuts"]), (rn["cuts"], rp["cuts"])
    assert rn["cuts"][0] == 0 and rn["cuts"][1:].max() >= 1          # (iteration 0 has no CVaR rows: driving.py:411-415)
    assert rn["t_risk"] == rp["t_risk"]
    assert np.array_equal(rn["L2_error"], rp["L2_error"])
    assert np.array_equal(rn["us"], rp["us"]) and np.isfinite(rn["us"]).all()
    assert mn._cut_solver.keep == mp._cut_solver.keep and mn._cut_solver.idle == mp._cut_solver.idle
    assert len(rn["define_s"]) == iters and (rn["cumulative_s"] > 0).all()
    # the solver was left as the per-iteration loop leaves it: one further subproblem agrees too
    un, tn, i_n = mn.solve_reduced(rn["us"], iters, final_rows='native')
    up, tp, i_p = mp.solve_reduced(rp["us"], iters, final_rows='native')
    assert np.array_equal(un, up) and tn == tp and i_n["cuts"] == i_p["cuts"]
    assert mn._cut_solver.keep == mp._cut_solver.keep and mn._cut_solver.idle == mp._cut_solver.idle


def test_native_loop_stays_within_the_reduced_vs_full_tolerance_of_the_default_path():
    """the native final rows differ from NumPy's in the last bits only: the native loop's solution is the default path's
    to the tolerance the reduced SCP is held to against the full one (test_driving_reduced_scp_matches_full_scp)"""
    from riskaversetrajopt_amd import scp
    M, S, iters = 16, 20, 10
    nat = scp.run_driving_reduced(_model(M, S, 0.1, 3), num_scp_iters_max=iters, native_loop=True)
    ref = scp.run_driving_reduced(_model(M, S, 0.1, 3), num_scp_iters_max=iters)
    np.testing.assert_allclose(nat["us"], ref["us"], rtol=0, atol=1e-5)
    assert abs(nat["t_risk"] - ref["t_risk"]) < 1e-5


def test_defaults_keep_the_python_loop_and_the_numpy_rows():
    from riskaversetrajopt_amd import scp
    M, S, iters = 50, 20, 4
    a, b = _model(M, S, 0.1, 5), _model(M, S, 0.1, 5)
    ra = scp.run_driving_reduced(a, num_scp_iters_max=iters)
    assert ra["loop"].startswith("python"), ra["loop"]
    rb = scp.run_drone_reduced(b, num_scp_iters_max=iters)            # (the shared driver does not pick the native loop either)
    assert rb["loop"].startswith("python"), rb["loop"]
    assert np.array_equal(ra["us_hist"], rb["us_hist"])
    # ... and its rows are ego_final_rows', to the bit
    _, _, info = a.solve_reduced(ra["us"], iters)
    du, rhs = a.ego_final_rows(ra["us"])
    assert np.array_equal(info["final_du"], du) and np.array_equal(info["final_rhs"], rhs)


def test_native_rows_need_the_rollout_form_and_a_known_name():
    from riskaversetrajopt_amd import scp
    m = _model(32, 20, 0.1, 9)
    us = m.initial_guess_us_mat()
    with pytest.raises(ValueError, match="rollout"):
        m.solve_reduced(us, 1, rollout=False, final_rows='native')
    with pytest.raises(ValueError, match="final_rows"):
        m.solve_reduced(us, 1, final_rows='fast')
    with pytest.raises(ValueError, match="final_rows"):
        scp.run_driving_reduced(m, num_scp_iters_max=1, final_rows='fast')


def test_native_loop_does_not_apply_without_the_native_cut_loop(monkeypatch):
    """RATO_PY_CUT_LOOP=1 switches the native cut loop off: scp_run_native says so (None) and native_loop=True is an error,
    not a quiet Python run"""
    from riskaversetrajopt_amd import scp
    m = _model(32, 20, 0.1, 9)
    monkeypatch.setenv("RATO_PY_CUT_LOOP", "1")
    assert m.scp_run_native(m.initial_guess_us_mat(), 2) is None
    with pytest.raises(RuntimeError, match="native"):
        scp.run_driving_reduced(m, num_scp_iters_max=2, native_loop=True)
