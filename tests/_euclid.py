"""fp64 restatement of the main-figure script's Euclidean obstacle rows (drone_main_plot.py:198-208, :254-269), of the
arg-max rule of ``rato_drone_eval_metric`` and of the float32 bin rule of ``rato_histogram`` -- NumPy only, shared by the
CPU pin (tests/test_main_plot_pin.py) and the GPU tests.

The rows are computed on ``oracle.drone.Model``'s trajectories: the main-plot ``Model`` rolls out exactly like
drone_risk.py's (the fixture's ``xs`` pins that), only the constraint differs.
"""
import numpy as np

from oracle import drone as od

from tests import _tol

EPS32 = float(np.finfo(np.float32).eps)
THR = od.OSQP_TOL + 1e-6          # B_satisfied = max_constraint <= OSQP_TOL + 1e-6 (drone_main_plot.py:638)
A_MIN = 1e-2                      # the g bound below degenerates at an obstacle's centre: test inputs keep a above this


def controls(S, scale=1.0, phase=0.0):
    """the 'graze' family of the goldens: a sweep through the obstacle field"""
    t = np.arange(S)[:, None]
    return scale * np.hstack([0.6 * np.cos(0.3 * t + phase) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)])


def quad_rows(xs, obs_Qs):
    """a[m, j, t] = (p - o_j)' Q_j[:2,:2] (p - o_j) at p = xs[m, t+1, :2] -> (M, n_obs, S)"""
    xs, Q = np.asarray(xs, dtype=np.float64), np.asarray(obs_Qs, dtype=np.float64)
    d = xs[:, None, 1:, :2] - od.obs_positions[None, :, None, :2]               # (M, n_obs, S, 2)
    return np.einsum('mjta,mjab,mjtb->mjt', d, Q[:, :, :2, :2], d)


def rows(xs, obs_Qs):
    """g = 1 - sqrt(a) -> (M, n_obs, S)"""
    return 1.0 - np.sqrt(quad_rows(xs, obs_Qs))


def model_rows(model, us):
    """-> (xs (M,S+1,6), a (M,n_obs,S), g (M,n_obs,S)) of an ``oracle.drone.Model`` at controls ``us``"""
    xs = model.us_to_state_trajectories(np.asarray(us, dtype=np.float64))
    a = quad_rows(xs, model.obs_Qs)
    return xs, a, 1.0 - np.sqrt(a)


def g_bound(a):
    """|g_dev - g_ref| allowed per entry: the project's tolerance of the quadratic row 1 - a (tests/_tol.py: G_ATOL +
    G_RTOL |1 - a|) carried through the square root (d sqrt(a) = da / (2 sqrt(a))), plus the root's and the subtraction's
    own fp32 roundings (each at most eps32 / 2 of max(1, sqrt(a)); 4 eps32 covers them with the input's rounding)."""
    a = np.asarray(a, dtype=np.float64)
    r = np.sqrt(a)
    return (_tol.G_ATOL + _tol.G_RTOL * np.abs(1.0 - a)) / (2.0 * r) + 4.0 * EPS32 * np.maximum(1.0, r)


def first_argmax(g):
    """g (M, n_obs, S) -> (M,) the flat row j*S + t of the FIRST maximum in the kernels' loop order (t ascending, then j
    ascending, strict >), -1 where no row compares greater than -inf (all NaN)."""
    g = np.asarray(g)
    M, J, S = g.shape
    arg = np.full(M, -1, dtype=np.int64)
    best = np.full(M, -np.inf, dtype=g.dtype)
    for t in range(S):
        for j in range(J):
            gt = g[:, j, t] > best                   # (NaN compares false)
            arg[gt] = j * S + t
            best[gt] = g[gt, j, t]
    return arg


def top_two_gap(g):
    """g (M, n_obs, S) -> (M,) difference between the largest and the second largest row of each sample"""
    s = np.sort(np.asarray(g).reshape(g.shape[0], -1), axis=1)
    return s[:, -1] - s[:, -2] if s.shape[1] > 1 else np.full(g.shape[0], np.inf)


def z_bound(a, arg):
    """the g bound at each sample's arg-max row -> (M,)"""
    a = np.asarray(a)
    return g_bound(a.reshape(a.shape[0], -1)[np.arange(a.shape[0]), arg])


def histogram(z, lo, hi, bins):
    """rato_histogram's rule restated in float32 NumPy -> int64 [bins + 3]: below | bins | at-or-above | NaN"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    lo, hi = np.float32(lo), np.float32(hi)
    inv_w = np.float32(bins) / (hi - lo)
    assert inv_w.dtype == np.float32
    counts = np.zeros(bins + 3, dtype=np.int64)
    nan = np.isnan(z)
    below, above = z < lo, z >= hi                    # (both false for NaN)
    inside = ~(nan | below | above)
    with np.errstate(over='ignore', invalid='ignore'):
        x = (z[inside] - lo) * inv_w
    assert x.dtype == np.float32
    b = np.minimum(x.astype(np.int64), bins - 1)
    counts[0], counts[bins + 1], counts[bins + 2] = below.sum(), above.sum(), nan.sum()
    counts[1:bins + 1] = np.bincount(b, minlength=bins)
    return counts


# ---- the inputs of the GPU tests: chosen on the CPU so that the ORACLE ALONE keeps every row's a above A_MIN and the
# arg-max unambiguous for at least 95 % of a batch (tests/test_main_plot_pin.py re-checks both for every shape used)
M_MAX = 257
M_CASES = (1, 63, 64, 65, 257)
S_CASES = (1, 16, 17, 33, 65)
_THROUGH = {16: 0.6, 33: 0.6}              # (scale 1: one arg-max row for all at S = 16; 4e-4 from a centre at S = 33)
_SKIRT = {1: (1.0, 1.0), 16: (0.7, 5.0), 17: (0.8, 3.5), 20: (1.1, 6.0), 33: (0.9, 5.0), 65: (1.2, 5.5)}


def test_controls(S):
    """-> {'through': a sweep through the obstacle field (every sample unsafe, the maximum at varying rows),
           'skirt': a pass beside it (about half of the samples safe)}"""
    t = np.arange(S)[:, None]
    sx, sy = _SKIRT[S]
    skirt = (20.0 / S) * np.hstack([sx * (0.6 * np.cos(0.3 * t * 20 / S) + 0.3), sy * (0.15 * np.sin(0.5 * t * 20 / S) + 0.02),
                                    0.05 * np.cos(t)])
    return {"through": controls(S, _THROUGH.get(S, 1.0) * 20.0 / S), "skirt": skirt}


test_controls.__test__ = False          # (not a test: pytest collects test_* names of imported helpers too)

_cache = {}


def batch(S):
    """the M_MAX-sample batch of horizon S (smaller M: its first M samples) and, per control family, the fp64 reference
    -> dict(DWs, masses, obs_Qs, cases={name: dict(us, xs, a, g, Z, arg, gap)})"""
    if S not in _cache:
        rng = np.random.RandomState(S)
        DWs, masses, obs_Qs = od.sample_uncertain_parameters(rng, 'saa', M=M_MAX, S=S, dt=od.T / S)
        model = od.Model(S, DWs, masses, obs_Qs)
        cases = {}
        for name, us in test_controls(S).items():
            xs, a, g = model_rows(model, us)
            arg = first_argmax(g)
            cases[name] = dict(us=us, xs=xs, a=a, g=g, Z=g.reshape(M_MAX, -1).max(axis=1), arg=arg, gap=top_two_gap(g))
            for v in cases[name].values():
                v.setflags(write=False)
        _cache[S] = dict(DWs=DWs, masses=masses, obs_Qs=obs_Qs, cases=cases)
    return _cache[S]
