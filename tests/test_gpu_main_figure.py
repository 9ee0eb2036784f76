"""GPU: scp.drone_main_figure_experiment -- the Monte-Carlo block behind the paper's main figure
(drone_main_plot.py:603-710) end to end at a small size: solve, one Euclidean evaluation with trajectories / maxima /
arg-max, statistics, histogram, the reference's nine-array result file."""
import os

import numpy as np
import pytest

from oracle import drone as od
from tests import _euclid as E
from tests import _tol as tol

pytestmark = pytest.mark.gpu
M, S, ITERS, M_MC, BINS = 8, 20, 3, 300, 100


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from riskaversetrajopt_amd import scp
    d = str(tmp_path_factory.mktemp("main_figure"))
    return scp.drone_main_figure_experiment(alpha=0.1, M=M, S=S, iters=ITERS, M_mc=M_MC, seed=0, bins=BINS,
                                            results_dir=d), d


def test_result_file_round_trips_with_the_reference_shapes(run):
    from riskaversetrajopt_amd import scp
    r, d = run
    arrays = scp.load_results(os.path.join(d, "drone_main_monte_carlo.npy"), 9)
    names = ("us", "xs", "xs_MC", "obs_Qs", "B_satisfied_vec", "constraints_vec", "percentage_safe", "var_val", "avar_val")
    shapes = ((S, 3), (M, S + 1, 6), (M_MC, S + 1, 6), (M_MC, 3, 3, 3), (M_MC,), (M_MC,), (), (), ())
    for a, name, shape in zip(arrays, names, shapes):
        assert a.shape == shape, name
        assert np.array_equal(a, np.asarray(r[name])), name
    assert arrays[4].dtype == bool
    with open(os.path.join(d, "drone_main_monte_carlo.npy"), "rb") as f:       # nine arrays, no more
        for _ in range(9):
            np.load(f)
        assert f.read() == b""


def test_samples_are_the_script_s_continuing_stream(run):
    from riskaversetrajopt_amd import scp
    r, _ = run
    _, mc = scp.draw_main_figure_batches(M, M_MC, S, 0)
    assert np.array_equal(r["obs_Qs"], mc[2])
    rng = np.random.RandomState(0)
    od.sample_uncertain_parameters(rng, 'saa', M=M, S=S, dt=od.T / S)
    DWs, masses, obs_Qs = od.sample_uncertain_parameters(rng, 'saa', M=M_MC, S=S, dt=od.T / S)     # no reseed in between
    assert np.array_equal(mc[0], DWs) and np.array_equal(mc[1], masses) and np.array_equal(mc[2], obs_Qs)


def test_report_values(run):
    from riskaversetrajopt_amd import stats
    r, _ = run
    Z, B = r["constraints_vec"], r["B_satisfied_vec"]
    assert np.array_equal(B, Z <= E.THR)
    assert r["percentage_safe"] == 1.0 - B.mean()                              # the reference's name: the UNSAFE share (:697)
    assert abs(r["var_val"] - stats.monte_carlo_var(Z, 0.1)) <= tol.RISK_ATOL
    assert abs(r["avar_val"] - stats.monte_carlo_avar(Z, 0.1)) <= tol.RISK_ATOL
    assert abs(r["mean"] - Z.mean()) <= tol.RISK_ATOL
    assert r["var_val"] == np.sort(Z)[M_MC - int(np.floor(0.1 * M_MC)) - 1]    # drone_main_plot.py:649-651, exactly
    assert np.array_equal(r["hist_counts"], E.histogram(Z, -0.6, 0.4, BINS)) and r["hist_counts"].sum() == M_MC
    assert np.array_equal(r["hist_edges"], -0.6 + np.arange(BINS + 1) * (1.0 / BINS))
    assert r["us"].shape == (S, 3) and np.abs(r["us"][:, 2]).max() > 0         # (the all-axes guess moves the third control)


def test_maxima_against_fp64_at_the_returned_controls(run):
    r, _ = run
    rng = np.random.RandomState(0)
    od.sample_uncertain_parameters(rng, 'saa', M=M, S=S, dt=od.T / S)
    model = od.Model(S, *od.sample_uncertain_parameters(rng, 'saa', M=M_MC, S=S, dt=od.T / S))
    xs, a, g = E.model_rows(model, r["us"])
    assert a.min() >= E.A_MIN                                                  # (the solved trajectory avoids the obstacles)
    arg_ref = E.first_argmax(g)
    zlim = E.z_bound(a, arg_ref)
    Z_ref = g.reshape(M_MC, -1).max(axis=1)
    assert not (~(np.abs(r["constraints_vec"] - Z_ref) <= zlim)).any()
    tol.assert_satisfied_close(r["B_satisfied_vec"], Z_ref, thr=E.THR)
    decided = E.top_two_gap(g) > zlim
    assert (~decided).mean() <= 0.05 and np.array_equal(r["arg"][decided], arg_ref[decided])
    assert r["arg"].dtype == np.int32 and r["arg"].min() >= 0 and r["arg"].max() < 3 * S
    np.testing.assert_allclose(r["xs_MC"], xs, rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)
