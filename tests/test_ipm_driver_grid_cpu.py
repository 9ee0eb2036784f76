"""CPU: what ``driver='device_grid'`` rests on and a host can check -- the driver's name at the entry points, and the
identity by which the grid form's residual phase runs the mu loop without walking the rows again.

The identity.  comp(mu) = max_i |fl(x_i - mu)| with x_i = z_i d_i EXACT and one rounding (the kernels' comp_term is a fused
multiply-add).  Rounding to nearest is monotone, so the maximum is reached at the largest or at the smallest exact product:
comp(mu) = max(|fl(x_max - mu)|, |fl(x_min - mu)|).  The device orders exact products as pairs (p, e), p = fl(z d), e = z d - p.
Both are restated here in exact rational arithmetic (``fractions.Fraction``; float(Fraction) rounds to nearest even), on
random and graded factors over 12 orders of magnitude with +-inf, +-0.0, equal extremes and products that differ only below
the rounding of p, for the values of mu the loop can hold.  The issue's unfused form of the identity (products rounded first)
is checked in NumPy as well: it is what holds at mu = 0, where comp is max |fl(x_i)|."""
from fractions import Fraction

import numpy as np
import pytest


def test_the_drivers_names():
    from riskaversetrajopt_amd import ipm
    assert ipm.DRIVERS == ("host", "device", "device_grid")
    assert ipm.on_device("device") and ipm.on_device("device_grid") and not ipm.on_device("host")
    ipm.check_driver("device_grid", "device")
    ipm.check_driver("device", "device")
    ipm.check_driver("host", "numpy")
    with pytest.raises(ValueError, match="backend='device'"):
        ipm.check_driver("device_grid", "numpy")
    for bad in ("grid", "device-grid", "DEVICE_GRID", None):
        with pytest.raises(ValueError, match="driver must be"):
            ipm.check_driver(bad, "device")


def test_entry_points_refuse_what_the_driver_cannot_serve():
    """as for 'device': the numpy backend, a solver that is not the interior-point method, and newton='arrow' on a host-only
    fp32 model"""
    from riskaversetrajopt_amd import hopper, hopper_ipm, scp
    m = hopper.Model.host_only(4, method='saa', alpha=0.2, S=2)
    errors = {}
    for driver in ("device", "device_grid"):
        for name, call in (("solve_batch", lambda: hopper_ipm.solve_batch([m], driver=driver, newton='arrow')),
                           ("solve", lambda: m.solve(driver=driver, newton='arrow')),
                           ("run_hopper", lambda: scp.run_hopper(m, driver=driver, newton='arrow'))):
            with pytest.raises(ValueError, match="newton='arrow'") as err:
                call()
            errors.setdefault(name, []).append(str(err.value))
        with pytest.raises(ValueError, match="backend='device'"):
            hopper_ipm.solve_batch([m], driver=driver, backend='numpy')
    assert all(a == b for a, b in errors.values())
    with pytest.raises(ValueError, match="solver='ipm'"):
        scp.run_drone_gaussian(None, solver='trust-constr', driver='device_grid')
    with pytest.raises(ValueError, match="driver must be"):
        scp.run_drone_gaussian(None, solver='ipm', driver='grid')


# ---- the extremes identity -----------------------------------------------------------------------------------------------------
def mus(tol=1e-8, start=(0.1, 7.0, 1e3)):
    """what the loop can hold: mu <- max(tol / 10, min(0.2 mu, mu sqrt(mu))) from a few starts down to the floor, and 0 (E0)"""
    out = [0.0]
    for mu in start:
        while True:
            out.append(mu)
            if mu <= tol / 10.0:
                break
            mu = max(tol / 10.0, min(0.2 * mu, mu * np.sqrt(mu)))
    return out


def fused(z, d, mu):
    """|fl(z d - mu)|, one rounding"""
    if not (np.isfinite(z) and np.isfinite(d)):
        with np.errstate(invalid='ignore'):
            return abs(np.float64(z) * np.float64(d) - mu)           # an infinite product: nothing to round
    x = Fraction(float(z)) * Fraction(float(d)) - Fraction(float(mu))
    try:
        return abs(float(x))
    except OverflowError:
        return np.inf


def pick(zs, ds):
    """the device's order: by p = fl(z d), then by e = z d - p (exact here) -> (index of the largest, of the smallest)"""
    key = []
    for z, d in zip(zs, ds):
        with np.errstate(over='ignore'):
            p = float(np.float64(z) * np.float64(d))
        e = Fraction(float(z)) * Fraction(float(d)) - Fraction(p) if np.isfinite(p) and np.isfinite(z) and np.isfinite(d) else Fraction(0)
        key.append((p, e))
    order = sorted(range(len(key)), key=key.__getitem__)
    return order[-1], order[0]


def factor_sets():
    rng = np.random.RandomState(11)
    sets = []
    for size in (1, 2, 7, 300):
        z = 10.0 ** rng.uniform(-6, 6, size)
        d = 10.0 ** rng.uniform(-6, 6, size) * rng.choice([-1.0, 1.0], size, p=[0.1, 0.9])
        sets.append((z, d))
    z = 10.0 ** rng.uniform(-2, -1, 50)                              # the mu_loop problem's: products within [0.01, 0.1] of mu
    sets.append((z, 10.0 ** rng.uniform(-2, -1, 50) / z))
    sets.append((np.array([3.0, 3.0, 3.0]), np.array([0.1, 0.1, 0.1])))                        # equal extremes
    sets.append((np.array([0.0, -0.0, 1e-3, 0.0]), np.array([1.0, 5.0, 0.0, -2.0])))           # +-0.0
    sets.append((np.array([1.0, np.inf, 2.0]), np.array([0.5, 1.0, 3.0])))                     # +inf
    sets.append((np.array([1.0, 2.0, 1e200]), np.array([0.5, -np.inf, 1e200])))                # -inf, and an overflowing product
    one = 1.0 + 2.0 ** -30                                                                      # products that agree in p and differ in e
    sets.append((np.array([one, 1.0, one - 2.0 ** -52]), np.array([one, one * one, one + 2.0 ** -52])))
    return sets


def test_the_maximum_is_reached_at_an_extreme_exact_product():
    for zs, ds in factor_sets():
        hi, lo = pick(zs, ds)
        for mu in mus():
            terms = [fused(z, d, mu) for z, d in zip(zs, ds)]
            want = max(terms)
            got = max(fused(zs[hi], ds[hi], mu), fused(zs[lo], ds[lo], mu))
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (zs, ds, mu)


def test_the_unfused_identity_of_rounded_products():
    rng = np.random.RandomState(12)
    cases = [10.0 ** rng.uniform(-6, 6, size) * rng.choice([-1.0, 1.0], size) for size in (1, 3, 64, 1000)]
    cases += [np.array([0.3, 0.3]), np.array([0.0, -0.0, 1e-300]), np.array([1.0, np.inf]), np.array([-np.inf, 2.0, 5.0])]
    for p in cases:
        pmax, pmin = np.max(p), np.min(p)
        for mu in mus():
            want = np.max(np.abs(p - mu))
            got = max(abs(pmax - mu), abs(pmin - mu))
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (p, mu)


def test_nan_and_empty_sides():
    """a NaN product is kept out of the picks and flagged: the side's maximum is NaN, as np.max's; a side without a bound
    yields the -inf the maximum starts from, which Python's max(0, .) turns into 0"""
    p = np.array([0.3, np.nan, 0.1])
    with np.errstate(invalid='ignore'):
        assert np.isnan(np.max(np.abs(p - 0.02)))
    flagged = bool(np.any(np.isnan(p)))
    side = np.nan if flagged else max(abs(np.nanmax(p) - 0.02), abs(np.nanmin(p) - 0.02))
    assert np.isnan(side)
    pymax = lambda a, b: b if b > a else a                           # Python's max(a, b): a unless b compares greater
    assert pymax(0.0, side) == 0.0                                   # ... which drops a NaN on the right, as the host driver does
    empty = -np.inf
    assert pymax(pymax(0.0, empty), empty) == 0.0
