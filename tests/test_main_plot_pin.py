"""CPU pin of the main-figure path (drone_main_plot.py): the fp64 restatement of its Euclidean rows and closures
(tests/_euclid.py) against the fixture recorded from the reference's own text
(tests/golden/make_reference_golden_main_plot.py), the experiment's sampler against the fixture's draws, the new entry
points in the header and the binding, and the conditions the GPU tests put on their inputs."""
import hashlib
import os
import re

import numpy as np
import pytest

from oracle import drone as od
from tests import _euclid as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = 1e-11                              # the oracle's own pin standard
NEW_ENTRY_POINTS = ("rato_drone_eval_metric", "rato_drone_eval_batch_metric", "rato_drone_obstacle_constraints_metric",
                    "rato_histogram")


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_drone_main_plot_S20_M16.npz"))


def test_fixture_matches_the_reference_where_it_exists(ref):
    path = os.path.join(os.environ.get("RATO_REFERENCE", "/root/reference"), "drone", "drone_main_plot.py")
    if os.path.exists(path):
        digest = hashlib.sha256(open(path, "rb").read()).digest()
        assert bytes(ref["ref_sha256__drone__drone_main_plot_py"]) == digest


def test_restatement_equals_the_reference(ref):
    S, M = int(ref["S"]), int(ref["M"])
    model = od.Model(S, ref["DWs"], ref["masses"], ref["obs_Qs"])
    xs, a, g = E.model_rows(model, ref["us"])
    assert xs.shape == ref["xs"].shape == (M, S + 1, 6) and g.shape == ref["g"].shape == (M, 3, S)
    assert np.abs(xs - ref["xs"]).max() <= PIN
    assert np.abs(xs - ref["xs_mc"]).max() <= PIN          # the closure's trajectories are the batched rollout's
    assert np.abs(g - ref["g"]).max() <= PIN
    Z = g.reshape(M, -1).max(axis=1)                       # the RAW maximum: nothing subtracted (drone_main_plot.py:637)
    assert np.abs(Z - ref["Z"]).max() <= PIN
    assert float(ref["osqp_tol"]) == od.OSQP_TOL
    assert np.array_equal(Z <= E.THR, ref["satisfied"])
    assert np.abs(E.rows(ref["xs"], ref["obs_Qs"]) - ref["g"]).max() <= PIN        # the rows alone, on the reference's xs
    arg = E.first_argmax(g)
    assert np.array_equal(g.reshape(M, -1)[np.arange(M), arg], Z)
    from oracle import stats as ostats
    assert abs(ostats.monte_carlo_var(ref["Z"], float(ref["alpha"])) - float(ref["var"])) <= PIN
    assert abs(ostats.monte_carlo_var(ref["Z"], 0.3) - float(ref["var_03"])) <= PIN


def test_sampler_reproduces_the_reference_draws(ref):
    from riskaversetrajopt_amd import scp
    saa, mc = scp.draw_main_figure_batches(M=int(ref["M_saa"]), M_mc=int(ref["M"]), S=int(ref["S"]), seed=0)
    for got, want in zip(saa, (ref["saa_DWs"], ref["saa_masses"], ref["saa_obs_Qs"])):
        assert np.array_equal(got, want)
    for got, want in zip(mc, (ref["DWs"], ref["masses"], ref["obs_Qs"])):        # the SAME stream, continued
        assert np.array_equal(got, want)


def test_all_axes_initial_guess_is_the_main_plot_one(ref):
    us = np.zeros((int(ref["S"]), 3))
    us[:, :] = (od.u_max - od.u_max) / 2.0 + 1e-2
    assert np.array_equal(us, ref["init_us"])                                   # drone_main_plot.py:137-148
    src = open(os.path.join(ROOT, "riskaversetrajopt_amd", "drone_risk.py")).read()
    assert "def initial_guess_us_mat(self, all_axes=False)" in src


def test_header_and_binding_declare_the_new_entry_points():
    from tests.test_abi import header_functions
    from riskaversetrajopt_amd import _lib
    fns = header_functions()
    for name in NEW_ENTRY_POINTS:
        assert name in fns, f"{name} missing from include/rato_saa.h"
        assert name in _lib.SIGNATURES, f"{name} missing from _lib.SIGNATURES"
    hdr = open(os.path.join(ROOT, "include", "rato_saa.h")).read()
    assert re.search(r"#define\s+RATO_DRONE_METRIC_QUADRATIC\s+0\b", hdr)
    assert re.search(r"#define\s+RATO_DRONE_METRIC_EUCLIDEAN\s+1\b", hdr)
    assert re.search(r"#define\s+RATO_ABI_VERSION\s+12\b", hdr)
    assert _lib.DRONE_METRICS == {"quadratic": 0, "euclidean": 1}


def test_histogram_rule_restatement():
    lo, hi, bins = -0.6, 0.4, 7
    lo32, hi32 = np.float32(lo), np.float32(hi)
    z = np.array([lo32, hi32, np.nextafter(hi32, np.float32(-np.inf)), np.nextafter(lo32, np.float32(-np.inf)), np.nan,
                  np.inf, -np.inf, 0.0], dtype=np.float32)
    c = E.histogram(z, lo, hi, bins)
    assert c.sum() == z.size
    assert c[0] == 2 and c[bins + 1] == 2 and c[bins + 2] == 1                 # below: nextafter(lo), -inf; above: hi, +inf
    assert c[1] == 1 and c[bins] == 1                                          # lo opens bin 0; nextafter(hi) closes the last
    assert c[1 + int((np.float32(0.0) - lo32) * (np.float32(bins) / (hi32 - lo32)))] == 1


@pytest.mark.parametrize("S", E.S_CASES)
def test_gpu_test_inputs_meet_their_conditions(S):
    """What the fp64 bound of the GPU tests asks of the inputs, on the oracle alone: no row with a < 1e-2 (the bound
    degenerates at an obstacle's centre; nothing is masked), and the fp64 arg-max decided by more than the Z bound for at
    least 95 % of every batch of more than one wave's edge (M = 1: that one sample must be decided)."""
    b = E.batch(S)
    for name, c in b["cases"].items():
        assert c["a"].min() >= E.A_MIN, (S, name, c["a"].min())
        undecided = c["gap"] <= E.z_bound(c["a"], c["arg"])
        for M in E.M_CASES:
            assert undecided[:M].mean() <= 0.05, (S, name, M, undecided[:M].mean())
    if S > 1:
        safe = b["cases"]["skirt"]["Z"] <= E.THR
        assert 0.2 < safe.mean() < 0.8                                         # both values of the satisfied flag occur
        assert len(set(b["cases"]["through"]["arg"])) > 1
