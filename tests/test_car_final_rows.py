"""CPU: rato_car_ego_final_rows (the final-state rows of the ego on the host, fp64 -- what the native driving SCP loops
compute per iteration) against the NumPy formulas of driving.Model.ego_final_rows (driving.py:283-288), restated here
because a Model cannot be built without a device.

The two differ only by the <= 1-ulp cos / sin of the two libraries and by the summation order over <= S terms (NumPy:
pairwise sums, reversed cumulative sums, a BLAS dot; the library: sequential sums in ascending k), so
  rows 2, 3 of final_du (they are dt)                          bit-equal,
  rows 0, 1 of final_du                                        within 64 S eps max|final_du|,
  final_rhs                                                    within 64 S eps (max|x_S - goal| + sum |final_du . u|).

Measured maxima over all cases below (x86-64, glibc libm): final_du 2.1e-14 absolute (S = 20, |u| <= 100; 1.3e-3 of the
bound at most, at the initial guess), final_rhs 2.0e-12 absolute (S = 100, |u| <= 100; 5.4e-3 of the bound at most, S = 20
at the initial guess); S = 1 and 2 agree to the bit (one term per sum at most)."""
import ctypes as C

import numpy as np
import pytest

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def _params(S):
    from riskaversetrajopt_amd import _lib
    from riskaversetrajopt_amd import driving_params as P
    p = _lib.CarParams()
    p.M, p.S, p.dt = 50, S, P.T / S
    p.dt64 = float(P.T / S)
    for i in range(4):
        p.ego_init[i] = float(P.state_init[i])
        p.ego_init64[i] = float(P.state_init[i])
    return p


def _goal():
    from riskaversetrajopt_amd import driving_params as P
    return np.concatenate((P.position_ego_goal, P.velocity_ego_goal)).astype(np.float64)


def _numpy_rows(S, us):
    """driving.Model.ego_final_rows, statement for statement -> (final_du, final_rhs, x_S)"""
    from riskaversetrajopt_amd import driving_params as P
    n_u, dt = 2, float(P.T / S)
    us = np.asarray(us, dtype=np.float64).reshape(S, n_u)
    x0, y0, v0, ph0 = (float(a) for a in P.state_init[:4])
    v = v0 + dt * np.concatenate(([0.0], np.cumsum(us[:, 0])))
    ph = ph0 + dt * np.concatenate(([0.0], np.cumsum(us[:, 1])))
    cs, sn = np.cos(ph[:S]), np.sin(ph[:S])
    xS = np.array([x0 + dt * np.sum(v[:S] * cs), y0 + dt * np.sum(v[:S] * sn), v[S], ph[S]])
    after = lambda a: np.concatenate((np.cumsum(a[::-1])[::-1][1:], [0.0]))
    E = np.zeros((4, S, n_u))
    E[0, :, 0], E[0, :, 1] = dt * dt * after(cs), -dt * dt * after(v[:S] * sn)
    E[1, :, 0], E[1, :, 1] = dt * dt * after(sn), dt * dt * after(v[:S] * cs)
    E[2, :, 0] = dt
    E[3, :, 1] = dt
    E = E.reshape(4, S * n_u)
    return E, -(xS - _goal()) + E @ us.reshape(-1), xS


def _native_rows(lib, S, us):
    us = np.ascontiguousarray(us, dtype=np.float64).reshape(S, 2)
    goal = _goal()
    du, rhs = np.full((4, 2 * S), np.nan), np.full(4, np.nan)
    p = _params(S)
    assert lib.rato_car_ego_final_rows(C.byref(p), us.ctypes.data, goal.ctypes.data, du.ctypes.data, rhs.ctypes.data) == 0
    return du, rhs


def _controls(S):
    from riskaversetrajopt_amd import driving_params as P
    rng = np.random.RandomState(1000 + S)
    yield "initial guess", np.zeros((S, 2)) + 1e-2                 # Model.initial_guess_us_mat: (u_max + u_min) / 2 + 1e-2
    yield "random, the whole box", rng.uniform(-P.u_max, P.u_max, (S, 2))
    yield "random, |u| <= 1", rng.uniform(-1.0, 1.0, (S, 2))
    yield "random, |u| <= 0.05", rng.uniform(-0.05, 0.05, (S, 2))


@pytest.mark.parametrize("S", [1, 2, 20, 100])
def test_native_final_rows_match_the_numpy_formulas(lib, S):
    for name, us in _controls(S):
        E, rhs, xS = _numpy_rows(S, us)
        du, rhs_n = _native_rows(lib, S, us)
        assert np.isfinite(du).all() and np.isfinite(rhs_n).all(), name
        assert np.array_equal(du[2:], E[2:]), name                      # dt, and zeros
        bound_du = 64 * S * EPS * np.abs(E).max()
        err_du = np.abs(du[:2] - E[:2]).max()
        bound_rhs = 64 * S * EPS * (np.abs(xS - _goal()).max() + np.abs(E * us.reshape(-1)[None, :]).sum())
        err_rhs = np.abs(rhs_n - rhs).max()
        print(f"S={S} {name}: final_du {err_du:.3e} (bound {bound_du:.3e})  final_rhs {err_rhs:.3e} (bound {bound_rhs:.3e})")
        assert err_du <= bound_du, (name, err_du, bound_du)
        assert err_rhs <= bound_rhs, (name, err_rhs, bound_rhs)


def test_structure_of_the_rows(lib):
    """rows 2 and 3 select the accelerations / the turn rates with weight dt; the last control moves neither position"""
    S = 20
    du, _ = _native_rows(lib, S, np.zeros((S, 2)) + 1e-2)
    dt = _params(S).dt64
    want = np.zeros((2, 2 * S))
    want[0, 0::2] = dt
    want[1, 1::2] = dt
    assert np.array_equal(du[2:], want)
    assert np.array_equal(du[:2, -2:], np.zeros((2, 2)))


def test_invalid_arguments_are_refused(lib):
    S = 4
    p = _params(S)
    us, goal, du, rhs = np.zeros((S, 2)), _goal(), np.zeros((4, 2 * S)), np.zeros(4)
    assert lib.rato_car_ego_final_rows(None, us.ctypes.data, goal.ctypes.data, du.ctypes.data, rhs.ctypes.data) == -1
    assert lib.rato_car_ego_final_rows(C.byref(p), None, goal.ctypes.data, du.ctypes.data, rhs.ctypes.data) == -1
    assert lib.rato_car_ego_final_rows(C.byref(p), us.ctypes.data, None, du.ctypes.data, rhs.ctypes.data) == -1
    p.dt64 = 0.0
    assert lib.rato_car_ego_final_rows(C.byref(p), us.ctypes.data, goal.ctypes.data, du.ctypes.data, rhs.ctypes.data) == -1
