"""CPU: the ``driver`` argument of the drone Gaussian interior-point solve, and the designed states of test_gpu_ipm_driver.py
checked on the host alone: every branch they exercise keeps its comparison at least 1e-6 (relative) away from its threshold,
so that no decision of the device driver can flip on rounding."""
import numpy as np
import pytest

import _drone_gaussian_ipm as T
import _ipm_driver as D
from riskaversetrajopt_amd import drone_gaussian_ipm as ipm

S, ALPHAS = 3, (0.05, 0.3)


def solve(**kw):
    return ipm.solve_batch(T.models(S, ALPHAS), T.starts(S, ALPHAS), tol=T.TOL, max_iter=300, backend='numpy',
                           callbacks=T.host_callbacks(S, ALPHAS), **kw)


def test_unknown_driver_is_refused():
    with pytest.raises(ValueError, match="driver"):
        solve(driver='bogus')


def test_device_driver_needs_the_device_backend():
    with pytest.raises(ValueError, match="driver"):
        solve(driver='device')


def test_host_driver_is_what_omitting_the_argument_gives():
    for (Z0, i0), (Z1, i1) in zip(solve(), solve(driver='host')):
        assert Z0.tobytes() == Z1.tobytes()
        assert set(i0) == set(i1) and "driver" not in i1
        for key, val in i0.items():
            if isinstance(val, np.ndarray):
                assert val.tobytes() == i1[key].tobytes(), key
            else:
                assert val == i1[key], key


def test_entry_points_refuse_an_unknown_driver():
    from riskaversetrajopt_amd import scp
    model = T.models(S, ALPHAS[:1])[0]
    with pytest.raises(ValueError, match="driver"):
        scp.run_drone_gaussian(model, Z0=T.starts(S, ALPHAS[:1])[0], solver='ipm', callbacks=T.host_callbacks(S, ALPHAS[:1])[0],
                               driver='bogus')
    with pytest.raises(ValueError, match="driver"):                  # the device driver is the interior-point method's
        scp.run_drone_gaussian(model, Z0=T.starts(S, ALPHAS[:1])[0], solver='trust-constr',
                               callbacks=T.host_callbacks(S, ALPHAS[:1])[0], driver='device')
    with pytest.raises(ValueError, match="driver"):
        model.solve(T.starts(S, ALPHAS[:1])[0], backend='numpy', driver='device')


@pytest.mark.parametrize("pattern", D.PATTERNS)
@pytest.mark.parametrize("shape", D.SHAPES, ids=lambda s: "n%d_mE%d_mI%d" % s)
def test_designed_states_keep_every_branch_away_from_its_threshold(shape, pattern):
    des = D.designed(*shape, pattern)
    ps, passes, accepted, log = D.host_chain(des)
    assert [p.status for p in ps] == [None, None, "line_search", "converged"]
    assert passes == [2, 0, 0, 0], passes                            # the mu loop fires twice, and not at the floor
    assert ps[1].mu == D.TOL / 10.0 and not np.isfinite(ps[2].E0)
    assert sorted(accepted[0] + accepted[1]) == [0, 1], accepted     # both running problems end their search in two rounds
    kinds = {w for w, _, _, _ in log}
    assert {"E0 <= tol", "E_mu <= 10 mu", "nu < nu_trial", "Armijo"} <= kinds
    for what, margin in log.margins():
        assert margin >= D.MARGIN, (what, margin)


def test_designed_cases_take_both_sides_of_every_branch():
    seen = {}
    for shape in D.SHAPES:
        for pattern in D.PATTERNS:
            for what, _, _, result in D.host_chain(D.designed(*shape, pattern))[3]:
                seen.setdefault(what, set()).add(result)
    assert all(seen[w] == {True, False} for w in ("E0 <= tol", "E_mu <= 10 mu", "nu < nu_trial", "Armijo")), seen
