"""CPU: what the hopper solve under ``driver='device'`` rests on and a host can check -- the objective as (curv, lin), the
inverse fold map, the argument checks -- and the designed batches with a linear objective term the GPU tests run
(tests/_hopper_ipm_driver.py)."""
import numpy as np
import pytest

import _hopper_ipm as H
import _hopper_ipm_driver as HD
import _ipm_driver as D

LD = np.longdouble


def model_of(S, M, method, phases, alpha=0.2):
    from riskaversetrajopt_amd import hopper
    return hopper.Model.host_only(M, method=method, alpha=alpha, S=S, phases=phases)


def points(model, count=3):
    rng = np.random.RandomState(31 * model.S + model.M)
    return [rng.uniform(-2, 2, model.num_vars) * 10.0 ** rng.randint(-3, 4, model.num_vars) for _ in range(count)]


@pytest.mark.parametrize("S,M,method,phases", H.map_cases())
def test_objective_as_curvature_and_linear_term(S, M, method, phases):
    from riskaversetrajopt_amd import hopper
    m = model_of(S, M, method, phases)
    curv, lin = m.curv, m.lin
    n = m.num_vars
    assert curv.shape == lin.shape == (n,) and curv.dtype == lin.dtype == np.float64
    nX = hopper.n_x * (S + 1)
    ui = nX + hopper.n_u * np.arange(S)
    want_c, want_l = np.zeros(n), np.zeros(n)
    want_c[ui] = want_c[ui + 1] = 2.0
    want_l[8 * S], want_l[-2] = -10000.0, 1e7
    assert np.array_equal(curv, want_c) and np.array_equal(lin, want_l)
    assert not np.any((curv != 0) & (lin != 0))                      # disjoint supports
    with pytest.raises(ValueError):
        curv[0] = 1.0                                                # read-only
    with pytest.raises(ValueError):
        lin[0] = 1.0
    for Z in points(m):
        assert m.grad_f(Z).tobytes() == (curv * Z + lin).tobytes()
        c, l, z = curv.astype(LD), lin.astype(LD), Z.astype(LD)
        ref, mag = 0.5 * np.sum(c * z * z) + np.sum(l * z), 0.5 * np.sum(c * z * z) + np.sum(np.abs(l * z))
        assert abs(LD(m.f(Z)) - ref) <= H.gamma(n + 3) * mag, (float(abs(LD(m.f(Z)) - ref)), float(mag))


@pytest.mark.parametrize("S,M,method,phases", H.map_cases())
def test_inverse_fold_map_reproduces_fold_multipliers(S, M, method, phases):
    m = model_of(S, M, method, phases)
    lay = m.nlp_layout()
    index, scale = m.fold_map()
    assert index.shape == scale.shape == (lay["ncon"],) and index.dtype == np.int64
    used = index >= 0
    assert np.unique(index[used]).size == np.count_nonzero(used) == np.count_nonzero(lay["lam_rows_index"] >= 0)
    assert np.all(np.abs(scale[used]) == 1.0) and not np.any(scale[~used])
    rng = np.random.RandomState(S + 10 * M)
    lams = rng.uniform(-2, 2, (3, lay["ncon"])) * 10.0 ** rng.randint(-3, 4, (3, lay["ncon"]))
    lams[:, rng.rand(lay["ncon"]) < 0.2] = 0.0
    lam_dyn, lam_rows = m.fold_multipliers(lams)
    got = np.zeros((3, 2 * (S + 1)))                                 # what rato_scatter_f64 does on a zeroed destination
    got[:, index[used]] = scale[used] * lams[:, used]
    assert got.tobytes() == lam_rows.tobytes()
    assert np.ascontiguousarray(lams[:, :8 * S]).tobytes() == lam_dyn.tobytes()


def test_argument_errors():
    from riskaversetrajopt_amd import hopper_ipm, scp
    m = model_of(2, 4, 'saa', None)
    with pytest.raises(ValueError, match="backend='device'"):
        hopper_ipm.solve_batch([m], driver='device', backend='numpy')
    with pytest.raises(ValueError, match="driver must be"):
        hopper_ipm.solve_batch([m], driver='x')
    with pytest.raises(ValueError, match="arrow"):
        hopper_ipm.solve_batch([m], driver='device', newton='arrow')
    with pytest.raises(ValueError, match="driver must be"):
        m.solve(driver='x')
    with pytest.raises(ValueError, match="arrow"):
        scp.run_hopper(m, driver='device', newton='arrow')
    with pytest.raises(ValueError, match="fold"):
        m.nlp_device(np.zeros((1, m.num_vars)), fold='x')


@pytest.mark.parametrize("shape", HD.SHAPES, ids=lambda s: "n%d_mE%d_mI%d" % s)
def test_designed_batches_with_a_linear_term(shape):
    """the rebuilt batch keeps the designed residuals and statuses, its lin is graded, of mixed sign and holds exact zeros, and
    the host driver goes through every phase on it with every comparison at the margin the device needs to decide alike"""
    des, base = HD.designed_lin(*shape), D.designed(*shape, HD.PATTERN)
    assert des is not base and des["JTy"] is not base["JTy"] and all(not hasattr(m, "lin") for m in base["models"])
    n = des["n"]
    for k, m in enumerate(des["models"]):
        s = des["state"][k]
        assert m.lin.shape == (n,) and m.grad_f(s["v"][:n]).tobytes() == (m.curv * s["v"][:n] + m.lin).tobytes()
        if n >= 65:
            assert np.any(m.lin > 0) and np.any(m.lin < 0) and np.any(m.lin == 0)
            assert np.max(np.abs(m.lin)) / np.min(np.abs(m.lin[m.lin != 0])) >= 1e6
        # the designed dual residual is the base design's, up to the rounding of the shift
        r0 = s["sf"] * (base["models"][k].curv * s["v"][:n]) + base["JTy"][k]
        r1 = s["sf"] * m.grad_f(s["v"][:n]) + des["JTy"][k]
        assert np.all(np.abs(r1 - r0) <= 8 * np.finfo(float).eps * (np.abs(r0) + 2 * s["sf"] * np.abs(m.lin) + np.abs(base["JTy"][k])))
    ps, passes, accepted, logs = HD.host_chain(des)
    ps0, passes0, accepted0, _ = D.host_chain(base)
    assert [p.status for p in ps] == [None, None, "line_search", "converged"] == [p.status for p in ps0]
    assert passes == passes0
    assert sorted(accepted[0] + accepted[1]) == [0, 1]               # both running problems end their search in two rounds
    print("decided:", [HD.decided(log) for log in logs], "worst margin:", min(m for log in logs for _, m in log.margins()))
    assert all(HD.decided(log) for log in logs)                      # the GPU test compares every decision of these batches
