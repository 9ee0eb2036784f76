"""GPU: whole solves under ``driver='device_grid'`` (csrc/ipm_driver_grid.hip).  The grid form of the driver's
vector kernels returns the bits of the workgroup form, so a solve under ``driver='device_grid'`` is held BITWISE to the one under
``driver='device'``: Z, every multiplier and every scalar of info but the driver's name."""
import numpy as np
import pytest

import _drone_gaussian as R
import _drone_gaussian_ipm as T
import _hopper_ipm as H
from test_gpu_chol_grid_solvers import hopper_model, hopper_problems

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bitwise(got, ref):
    """(Z, info) under 'device_grid' against 'device': everything but the driver's name"""
    (Z0, i0), (Z1, i1) = got, ref
    same = lambda a, b: a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else (a == b or (a != a and b != b))
    assert i0["driver"] == "device_grid" and i1["driver"] == "device" and set(i0) == set(i1)
    return Z0.tobytes() == Z1.tobytes() and all(same(i0[k], i1[k]) for k in i0 if k != "driver")


@pytest.mark.parametrize("chol", ["workgroup", "grid"])
@pytest.mark.parametrize("newton", ["dense", "arrow"])
def test_hopper_solve_is_bitwise_the_device_driver(newton, chol):
    from riskaversetrajopt_amd import hopper_ipm
    e = hopper_problems()
    kw = dict(newton=newton, chol=chol, max_iter=1000)
    ref = hopper_ipm.solve_batch(e["models"], e["Z0s"], driver='device', **kw)
    got = hopper_ipm.solve_batch(e["models"], e["Z0s"], driver='device_grid', **kw)
    for k in range(len(ref)):
        assert got[k][1]["status"] == "converged"
        assert (got[k][1]["status"], got[k][1]["iterations"], got[k][1]["factorizations"]) == \
            (ref[k][1]["status"], ref[k][1]["iterations"], ref[k][1]["factorizations"])
        assert bitwise(got[k], ref[k]), k
        H.check_solution(e["models"][k], e["fields"], *got[k])


def test_hopper_solve_with_rows_beyond_one_workgroup():
    """M = 300 samples put n, nv and m of the S = 6 problem beyond the rows of one workgroup.  The solve is cut at 12 iterations:
    whatever the status, the two drivers stop in the same state"""
    from riskaversetrajopt_amd import _lib, hopper_ipm
    S, M = H.S_SMALL, 300
    flds = H.fields(M)
    models = [hopper_model(S, M, 'saa', a, flds) for a in (0.1, 0.5)]
    st = hopper_ipm.structure(models[0])
    assert min(st["n"], st["ncon"]) > _lib.load().rato_ipm_grid_rows()
    base = hopper_model(S, M, 'baseline', 0.1, flds)
    Z0s = [H.warm_start(mm, base.initial_guess()) for mm in models]
    kw = dict(newton='arrow', max_iter=12)
    ref = hopper_ipm.solve_batch(models, Z0s, driver='device', **kw)
    got = hopper_ipm.solve_batch(models, Z0s, driver='device_grid', **kw)
    print([(i["status"], i["iterations"], i["factorizations"]) for _, i in ref])
    for k in range(2):
        assert ref[k][1]["iterations"] >= 1
        assert bitwise(got[k], ref[k]), k
    solo, = hopper_ipm.solve_batch(models[1:], Z0s[1:], driver='device_grid', **kw)
    assert bitwise(solo, ref[1])


@pytest.mark.parametrize("S", sorted(T.CASES))
def test_drone_gaussian_solve_is_bitwise_the_device_driver(S):
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm as m
    alphas = T.CASES[S]
    models = [dg.Model(S, alpha=a, device=DEV) for a in alphas]
    kw = dict(tol=T.TOL, max_iter=300, backend='device')
    ref = m.solve_batch(models, T.starts(S, alphas), driver='device', **kw)
    got = m.solve_batch(models, T.starts(S, alphas), driver='device_grid', **kw)
    for k, a in enumerate(alphas):
        assert got[k][1]["status"] == "converged"
        assert bitwise(got[k], ref[k]), a
        T.check_solution(S, a, *got[k])


def test_entry_points_take_the_driver():
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm as m, hopper_ipm, scp
    S, a = 5, T.CASES[5][0]
    Z0 = R.start_point(S, a)
    (Zb, ib), = m.solve_batch([dg.Model(S, alpha=a, device=DEV)], [Z0], tol=T.TOL, max_iter=300, backend='device', driver='device')
    Z, info = dg.Model(S, alpha=a, device=DEV).solve(Z0, max_iter=300, driver='device_grid')
    assert bitwise((Z, info), (Zb, ib))
    r = scp.run_drone_gaussian(dg.Model(S, alpha=a, device=DEV), Z0=Z0, maxiter=300, solver='ipm', driver='device_grid')
    assert bitwise((r["Z"], r["info"]), (Zb, ib)) and r["status"] == "converged" and r["nit"] == ib["iterations"]
    e = hopper_problems()
    (Zh, ih), = hopper_ipm.solve_batch(e["models"][:1], e["Z0s"][:1], driver='device', max_iter=1000)
    r = scp.run_hopper(e["models"][0], Z0=e["Z0s"][0], max_iter=1000, driver='device_grid')
    assert r["Z"].tobytes() == Zh.tobytes() and r["status"] == ih["status"] == "converged"
    assert r["info"]["driver"] == "device_grid" and r["info"]["iterations"] == ih["iterations"]
    Zm, im = e["models"][0].solve(e["Z0s"][0], max_iter=1000, driver='device_grid')
    assert bitwise((Zm, im), (Zh, ih))


def test_the_driver_needs_the_device_backend():
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm as m, hopper, hopper_ipm, scp
    e = hopper_problems()
    with pytest.raises(ValueError, match="backend='device'"):
        hopper_ipm.solve_batch(e["models"], e["Z0s"], backend='numpy', driver='device_grid')
    with pytest.raises(ValueError, match="backend='device'"):
        m.solve_batch([dg.Model(3, alpha=0.1, device=DEV)], backend='numpy', driver='device_grid')
    with pytest.raises(ValueError, match="solver='ipm'"):
        scp.run_drone_gaussian(dg.Model(3, alpha=0.1, device=DEV), solver='trust-constr', driver='device_grid')
    errors = []
    for driver in ("device", "device_grid"):                         # the same refusal as for 'device': a CPU model, fp32
        with pytest.raises(ValueError, match="newton='arrow'") as err:
            hopper_ipm.solve_batch([hopper.Model.host_only(H.M_SMALL, method='saa', alpha=0.1, S=H.S_SMALL)], newton='arrow',
                                   driver=driver)
        errors.append(str(err.value))
    assert errors[0] == errors[1]
