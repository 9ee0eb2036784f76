"""Test helper (host only, NumPy): designed inputs with closed-form answers, fp64 references and the derived bounds for the
PRODUCERS of the cut oracle -- rato_drone_rowmax_rollout / rato_car_rowmax_rollout, rato_drone_rowmax_implicit,
rato_drone_linearize_generators and the by-value | device-memory switch of rato_cut_oracle_rollout (csrc/cvar.hip,
csrc/drone.hip).  tests/test_cut_designs.py checks the designs on the CPU; tests/test_gpu_cut_producers.py runs them.

Three kinds of things live here.
  * References.  ``drone_dense`` / ``car_dense`` are the fp64 oracle (oracle.drone.Model / oracle.driving.Model) evaluated in
    chunks of samples (its dense rows g + G x grow with S^2); ``drone_direct`` / ``car_direct`` restate the same rows as a
    tangent recursion beside the rollout, in any dtype (np.longdouble: a second, independent evaluation of the same numbers).
    The spread between the two is the conditioning term of every bound (``once_rounded_bound``).
  * Designs.  ``drone_still`` / ``car_still`` (nothing moves: every step of a row group has the same value, so the answer is
    the smallest row of the best group, in closed form), ``implicit_design`` (tables in exact arithmetic: ties placed at
    will).  Each records what it expects; nothing here is fitted to a kernel's output.
  * Mistakes.  ``rowmax_model`` restates the kernels' selection rule and the ways to get it wrong; ``pad_last`` and the
    ``semi_implicit`` switch of the direct forms model a consumed clamped load and a control of step S - 1 entering a row.
Checker only: nothing in the package imports this."""
import contextlib
from dataclasses import dataclass, field

import numpy as np

EPS32 = 2.0 ** -24        # one rounding fp64 -> fp32, relative
MARGIN = 8.0              # on the measured spread: the kernel's fma order is a third evaluation order
ROLLOUT_BATCH = 16        # drone / driving rowmax rollout: double batches of 8 steps
IMPLICIT_BATCH = 8        # drone_rowmax_implicit_kernel: batches of 8 steps


def r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@contextlib.contextmanager
def patched(module, **values):
    """module constants replaced for the duration (the oracle reads its constants from module globals)"""
    old = {k: getattr(module, k) for k in values}
    try:
        for k, v in values.items():
            setattr(module, k, v)
        yield module
    finally:
        for k, v in old.items():
            setattr(module, k, v)


def chunks(M, n):
    return [slice(i, min(i + n, M)) for i in range(0, M, n)]


def once_rounded_bound(ref, spread, extra=0.0):
    """|device - ref| for an output that is fp64 arithmetic rounded once to fp32: the rounding, MARGIN x the spread between
    two fp64 evaluations of ref, and whatever systematic term the caller measured on the reference side"""
    return EPS32 * np.abs(ref) + MARGIN * spread + extra


def m_limit(m_ref, scale, spread):
    """the bound on m: derived, and never looser than what tests/test_gpu_scp.py holds m to (6e-8 |m| + 2e-9 scale)"""
    return np.minimum(once_rounded_bound(m_ref, spread), 6.0e-8 * np.abs(m_ref) + 2e-9 * scale)


def clear_rows(rows2d, scale):
    """samples whose top two reference rows are distinguishable (the rule of tests/test_gpu_scp.py)"""
    if rows2d.shape[1] < 2:
        return np.ones(rows2d.shape[0], bool)
    srt = np.sort(rows2d, axis=1)
    return (srt[:, -1] - srt[:, -2]) > 1e-8 * scale


# ---- drone: constants, the oracle in chunks, the direct restatement ------------------------------------------------
@dataclass
class DroneConst:
    dt: float
    beta: float
    kp: float
    kd: float
    drag: float
    tol: float
    x_init: np.ndarray
    x_final: np.ndarray
    obs_xy: np.ndarray
    patch: dict = field(default_factory=dict)     # what to replace in oracle.drone for the same constants


def drone_const(S, dt=None, beta=None, x_init=None, obs_xy=None):
    from oracle import drone as od
    patch = {}
    if dt is not None:
        patch["T"] = dt * S
    if beta is not None:
        patch["beta"] = beta
    if x_init is not None:
        patch["x_init"] = np.asarray(x_init, dtype=np.float64)
    if obs_xy is not None:
        patch["obs_positions"] = np.hstack([np.asarray(obs_xy, dtype=np.float64), np.zeros((3, 1))])
    return DroneConst(dt=od.T / S if dt is None else dt, beta=od.beta if beta is None else beta,
                      kp=-float(od.FEEDBACK_GAIN[0, 0]), kd=-float(od.FEEDBACK_GAIN[0, 3]), drag=od.drag_coefficient,
                      tol=od.OSQP_TOL, x_init=np.asarray(od.x_init if x_init is None else x_init, dtype=np.float64),
                      x_final=np.asarray(od.x_final, dtype=np.float64),
                      obs_xy=np.asarray(od.obs_positions[:, :2] if obs_xy is None else obs_xy, dtype=np.float64), patch=patch)


def apply_drone_const(p, c):
    """overwrite the fields of a rato_drone_params (ctypes) with the constants of a design"""
    p.dt, p.dt64, p.beta, p.beta64 = c.dt, c.dt, c.beta, c.beta
    for i in range(6):
        p.x_init[i], p.x_init64[i] = float(c.x_init[i]), float(c.x_init[i])
    for j in range(3):
        for a in range(2):
            p.obs_xy[j][a], p.obs_xy64[j][a] = float(c.obs_xy[j, a]), float(c.obs_xy[j, a])
    return p


def drone_dense(c, samples, uk, x=None, arg=None, chunk=64):
    """The fp64 oracle on (DWs (M,S,6), masses (M,), Q (M,3,3,3)) at u_k, chunk by chunk.  -> dict: g (M,3,S), g_up (M,3,S),
    W (M,3,S,2), e22 (M,S,3), Z (M,), fdu (M,S,6) = d(p_a, v_a)_S / d u_{s,a}, rhs (M,6); with x: rows (M,3,S) = g + G x;
    with arg (M,) as well: G_arg (M,3S) and g_arg (M,), the rows a cut is summed from."""
    from oracle import drone as od
    DWs, masses, Q = samples
    M, S = DWs.shape[0], uk.shape[0]
    out = {"g": np.empty((M, 3, S)), "g_up": np.empty((M, 3, S)), "W": np.empty((M, 3, S, 2)), "e22": np.empty((M, S, 3)),
           "Z": np.empty(M), "fdu": np.empty((M, S, 6)), "rhs": np.empty((M, 6))}
    if x is not None:
        out["rows"] = np.empty((M, 3, S))
    if arg is not None:
        out["G_arg"], out["g_arg"] = np.empty((M, 3 * S)), np.empty(M)
    with patched(od, **c.patch):
        for sl in chunks(M, chunk):
            o = od.Model(S, DWs[sl], masses[sl], Q[sl], 'saa', 0.2)
            assert o.dt == c.dt and o.beta == c.beta
            fdu, flo, _, gdu, gup = o.get_all_constraints_coeffs(uk)
            n = gdu.shape[0]
            G = gdu.reshape(n, 3 * S, 3 * S)
            g = -(gup.reshape(n, 3 * S) - G @ uk.reshape(-1))
            xs = o.us_to_state_trajectories(uk)
            out["g"][sl] = o.obstacle_avoidance_constraints(xs, o.obs_Qs)
            out["g_up"][sl] = gup
            d = xs[:, 1:, None, :2] - od.obs_positions[None, None, :, :2]                   # (n,S,3,2)
            Q2 = o.obs_Qs[:, :, :2, :2]
            out["W"][sl] = -np.einsum('mjab,mtjb->mjta', Q2 + np.swapaxes(Q2, -1, -2), d)
            out["e22"][sl] = o.dt * (c.kd + 2.0 * c.drag * np.abs(xs[:, :S, 3:6])) / o.masses[:, None, None]
            out["Z"][sl] = out["g"][sl].reshape(n, -1).max(axis=1) - c.tol
            for a in range(3):
                out["fdu"][sl, :, a] = fdu[:, a, a::3]
                out["fdu"][sl, :, 3 + a] = fdu[:, 3 + a, a::3]
            out["rhs"][sl] = flo
            if x is not None:
                out["rows"][sl] = (g + G @ x.reshape(-1)).reshape(n, 3, S)
            if arg is not None:
                i = np.arange(n)
                out["G_arg"][sl], out["g_arg"][sl] = G[i, arg[sl]], g[i, arg[sl]]
    return out


def drone_direct(c, samples, uk, x=None, dtype=np.float64, round_e22=False, semi_implicit=False):
    """The same quantities as ``drone_dense`` by the recursions themselves, in ``dtype``: the rollout in the reference's form,
    the response d x to x (rows) and to u_k (g_up) as the tangent of the step, the final-state Jacobian as the adjoint from
    S down.  round_e22: the tangent to u_k and the adjoint use a22 = 1 - float(e22), what rato_drone_linearize_generators
    documents (its table holds e22 as a float and its consumers must see the same numbers).  semi_implicit (a MISTAKE):
    d p advances with the new d v, so the control of step t enters row t."""
    DWs, masses, Q = samples
    f = lambda a: np.asarray(a, dtype=dtype)
    M, S = DWs.shape[0], uk.shape[0]
    dt, kp, kd, drag, beta = (dtype(v) for v in (c.dt, c.kp, c.kd, c.drag, c.beta))
    m = f(masses)[:, None]
    xi = f(DWs)[:, :, 3:6]
    Q2 = f(Q)[:, :, :2, :2]
    Qs = Q2 + np.swapaxes(Q2, -1, -2)
    obs = f(c.obs_xy)
    uk = f(uk)
    xx = f(np.zeros((S, 3)) if x is None else x)
    p, v = np.tile(f(c.x_init[:3]), (M, 1)), np.tile(f(c.x_init[3:]), (M, 1))
    z = np.zeros((M, 3), dtype=dtype)
    dpx, dvx, dpu, dvu = z, z, z, z
    out = {k: np.empty(s, dtype=dtype) for k, s in (("g", (M, 3, S)), ("g_up", (M, 3, S)), ("W", (M, 3, S, 2)), ("e22", (M, S, 3)),
                                                   ("rows", (M, 3, S)), ("fdu", (M, S, 6)), ("rhs", (M, 6)))}
    a22_u = np.empty((M, S, 3), dtype=dtype)
    a21, dtm, sq = -kp * dt / m, dt / m, np.sqrt(dt)
    for t in range(S):
        e = dt * (kd + 2 * drag * np.abs(v)) / m
        out["e22"][:, t] = e
        a22 = 1 - e
        a22_u[:, t] = 1 - (e.astype(np.float32).astype(dtype) if round_e22 else e)
        ndv = a21 * dpx + a22 * dvx + dtm * xx[t]
        dpx, dvx = dpx + dt * (ndv if semi_implicit else dvx), ndv
        dpu, dvu = dpu + dt * dvu, a21 * dpu + a22_u[:, t] * dvu + dtm * uk[t]
        acc = (uk[t] - (kp * p + kd * v)) / m - drag * np.abs(v) * v / m
        p, v = p + dt * v, v + dt * acc + sq * (beta / m) * xi[:, t]
        d = p[:, None, :2] - obs[None]
        g = 1 - (d * np.einsum('mjab,mjb->mja', Q2, d)).sum(-1)
        w = -np.einsum('mjab,mjb->mja', Qs, d)
        out["g"][:, :, t], out["W"][:, :, t] = g, w
        out["rows"][:, :, t] = g + (w * dpx[:, None, :2]).sum(-1)
        out["g_up"][:, :, t] = -g + (w * dpu[:, None, :2]).sum(-1)
    out["Z"] = out["g"].reshape(M, -1).max(axis=1) - dtype(c.tol)
    one, zero = np.ones((M, 3), dtype=dtype), np.zeros((M, 3), dtype=dtype)
    mP0, mP1, mV0, mV1 = one, zero, zero, one
    for s in range(S - 1, -1, -1):
        out["fdu"][:, s, :3], out["fdu"][:, s, 3:] = mP1 * dtm, mV1 * dtm
        if s > 0:
            a22 = a22_u[:, s]
            mP0, mP1 = mP0 + mP1 * a21, mP0 * dt + mP1 * a22
            mV0, mV1 = mV0 + mV1 * a21, mV0 * dt + mV1 * a22
    xf = f(c.x_final)
    out["rhs"][:, :3] = -(p - xf[:3]) + (out["fdu"][:, :, :3] * uk[None]).sum(axis=1)
    out["rhs"][:, 3:] = -(v - xf[3:]) + (out["fdu"][:, :, 3:] * uk[None]).sum(axis=1)
    if x is None:
        del out["rows"]
    return out


def block_sums(per_sample, M, block=256):
    """(M, ...) -> (ceil(M / block), ...): the sums a workgroup of 256 samples leaves in its row of ``part``"""
    return np.stack([per_sample[b:b + block].sum(axis=0) for b in range(0, M, block)])


# ---- driving -------------------------------------------------------------------------------------------------------
@dataclass
class CarConst:
    dt: float
    beta: float
    v_des: float
    d_min: float
    patch: dict = field(default_factory=dict)


def car_const(S, dt=None, beta=None):
    from oracle import driving as ocar
    patch = {}
    if dt is not None:
        patch["T"] = dt * S
    if beta is not None:
        patch["BETA"] = beta
    return CarConst(dt=ocar.T / S if dt is None else dt, beta=ocar.BETA if beta is None else beta, v_des=ocar.speed_ped_des,
                    d_min=float(ocar.min_separation_distance), patch=patch)


def apply_car_const(p, c):
    p.dt, p.dt64, p.beta, p.beta64 = c.dt, c.dt, c.beta, c.beta
    return p


def car_dense(c, samples, uk, x, arg=None, chunk=32):
    """The fp64 oracle on (states_init (M,8), omegas_speed, omegas_repulsive, DWs (M,S,8)), chunk by chunk -> dict: rows (M,S)
    = g + G x, g (M,S); with arg: G_arg (M,2S), g_arg (M,)"""
    from oracle import driving as ocar
    x0, ws, wr, DWs = samples
    M, S = DWs.shape[0], uk.shape[0]
    out = {"rows": np.empty((M, S)), "g": np.empty((M, S))}
    if arg is not None:
        out["G_arg"], out["g_arg"] = np.empty((M, 2 * S)), np.empty(M)
    with patched(ocar, **c.patch), np.errstate(invalid="ignore", divide="ignore"):
        for sl in chunks(M, chunk):
            o = ocar.Model(x0[sl], ws[sl], wr[sl], DWs[sl], method='saa', alpha=0.2)
            assert o.dt == c.dt and o.beta == c.beta
            _, _, _, gdu, gup = o.get_all_constraints_coeffs(uk)
            g = -(gup - gdu @ uk.reshape(-1))
            out["g"][sl], out["rows"][sl] = g, g + gdu @ x.reshape(-1)
            if arg is not None:
                i = np.arange(gdu.shape[0])
                out["G_arg"][sl], out["g_arg"][sl] = gdu[i, arg[sl]], g[i, arg[sl]]
    return out


def car_direct(c, samples, uk, x, dtype=np.float64, semi_implicit=False):
    """rows (M,S) = g + G x of the driving problem as the tangent of the step beside the rollout, in ``dtype``"""
    x0, ws, wr, DWs = samples
    f = lambda a: np.asarray(a, dtype=dtype)
    M, S = DWs.shape[0], uk.shape[0]
    dt, beta, v_des, d_min = (dtype(v) for v in (c.dt, c.beta, c.v_des, c.d_min))
    ws, wr, xi, uk, x = f(ws), f(wr)[:, None], f(DWs)[:, :, 6:8], f(uk), f(x)
    e, ev, eph = f(x0[0, 0:2]).copy(), dtype(x0[0, 2]), dtype(x0[0, 3])
    de, dev, deph = np.zeros(2, dtype=dtype), dtype(0), dtype(0)
    q, qv = f(x0[:, 4:6]).copy(), f(x0[:, 6:8]).copy()
    dq, dqv = np.zeros((M, 2), dtype=dtype), np.zeros((M, 2), dtype=dtype)
    rows = np.empty((M, S), dtype=dtype)
    sq = np.sqrt(dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(S):
            d = e[None] - q
            r = np.sqrt((d * d).sum(-1))[:, None]
            n = d / r
            F = -wr * n + (ws * (v_des - qv[:, 1]))[:, None]
            dd = de[None] - dq
            dF = -wr * (dd - n * (n * dd).sum(-1)[:, None]) / r - (ws * dqv[:, 1])[:, None]
            cs, sn = np.cos(eph), np.sin(eph)
            ndev, ndeph = dev + dt * x[t, 0], deph + dt * x[t, 1]
            tv = ndev if semi_implicit else dev
            de = de + dt * np.array([tv * cs - ev * sn * deph, tv * sn + ev * cs * deph], dtype=dtype)
            e = e + dt * ev * np.array([cs, sn], dtype=dtype)
            ev, eph, dev, deph = ev + dt * uk[t, 0], eph + dt * uk[t, 1], ndev, ndeph
            q, qv = q + dt * qv, qv + dt * F + sq * beta * xi[:, t]
            dq, dqv = dq + dt * dqv, dqv + dt * dF
            d1 = e[None] - q
            r1 = np.sqrt((d1 * d1).sum(-1))
            rows[:, t] = -(r1 - d_min) - ((d1 / r1[:, None]) * (de[None] - dq)).sum(-1)
    return rows


# ---- the selection rule and the ways to get it wrong ---------------------------------------------------------------
def _first_max(v):
    return int(np.argmax(v))


def _last_max(v):
    return int(len(v) - 1 - np.argmax(v[::-1]))


def rowmax_model(rows, rule="ok", batch=ROLLOUT_BATCH):
    """rows (M, R, S) -> (m (M,), arg (M,)): the largest row and, among equal ones, the SMALLEST row index j S + t -- per
    group a strict > over ascending t, then a strict > over ascending groups -- or one of the mistakes:
      '>= over t'           the largest t among equal values of a group
      '>= over groups'      the largest group among equal group maxima
      'largest row'         both
      'last step dropped'   steps 0 .. S - 2 only
      'remainder skipped'   only whole batches: steps 0 .. S - (S mod batch) - 1
      'second half skipped' the remainder's second half batch (steps >= floor(S / batch) batch + batch / 2) never runs
    An empty selection gives (-inf, 0), as the kernels' initial values do."""
    M, R, S = rows.shape
    keep = {"last step dropped": S - 1, "remainder skipped": S - S % batch,
            "second half skipped": min(S, S - S % batch + batch // 2)}.get(rule, S)
    t_pick = _last_max if rule in (">= over t", "largest row") else _first_max
    j_pick = _last_max if rule in (">= over groups", "largest row") else _first_max
    m, arg = np.full(M, -np.inf), np.zeros(M, dtype=np.int64)
    if keep == 0:
        return m, arg
    for i in range(M):
        ts = [t_pick(rows[i, j, :keep]) for j in range(R)]
        best = np.array([rows[i, j, ts[j]] for j in range(R)])
        j = j_pick(best)
        m[i], arg[i] = best[j], j * S + ts[j]
    return m, arg


SELECTION_MISTAKES = (">= over t", ">= over groups", "largest row", "last step dropped", "remainder skipped",
                      "second half skipped")


def pad_last(S, batch=ROLLOUT_BATCH):
    """the horizon a kernel would run if the steps behind the guards of its last batch were executed"""
    return (S + batch - 1) // batch * batch


def repeat_last(a, S_ext, axis):
    """``a`` with its last entry along ``axis`` repeated up to length S_ext: what loads clamped to row S - 1 deliver"""
    a = np.asarray(a)
    n = S_ext - a.shape[axis]
    if n <= 0:
        return a
    last = np.take(a, [a.shape[axis] - 1], axis=axis)
    return np.concatenate([a, np.repeat(last, n, axis=axis)], axis=axis)


# ---- standing still: drone ------------------------------------------------------------------------------------------
STILL_DT, STILL_BETA, STILL_MASS = 0.25, 2.0 ** -5, 32.0      # sqrt(dt) beta / m = 2^-11: every product below is exact
STILL_OBS = np.array([[-1.5, 0.25], [-1.5, -0.25], [1.0, 0.5]])    # obstacles 0 and 1 mirror each other about the x axis
# kind -> (q00, qs, q11) of the three obstacles.  At p = 0 obstacle j is worth 1 - q00 ox^2 - qs ox oy - q11 oy^2:
#   (2,0,4) at 0 and 1: -3.75;  (1,1,4) at 0 and (1,-1,4) at 1: -1.125;  (4,1,4) at 2: -4.5;  (1,0,15) at 2: -3.75;  (1,1,2) at 2: -1
STILL_Q = {
    "best0": ((1, 1, 4), (2, 0, 4), (4, 1, 4)),
    "best1": ((2, 0, 4), (1, -1, 4), (4, 1, 4)),
    "best2": ((2, 0, 4), (2, 0, 8), (1, 1, 2)),
    "tie01": ((2, 0, 4), (2, 0, 4), (4, 1, 4)),          # the mirrored pair, equal Q with qs = 0: exactly equal values
    "tie12": ((4, 0, 4), (2, 0, 4), (1, 0, 15)),
    "tie_all": ((2, 0, 4), (2, 0, 4), (1, 0, 15)),
}
STILL_KINDS = ("best0", "best1", "best2", "tie01", "tie12", "tie_all", "last_row", "last_noise")


def _still_value(q, o):
    return 1.0 - q[0] * o[0] * o[0] - q[1] * o[0] * o[1] - q[2] * o[1] * o[1]


def designed_slots(M, n):
    """where the n designed samples sit: the first n, the n in front of the first block edge, the last n of 513"""
    idx = [i for base in (0, 256 - n, 513 - n) for i in range(base, base + n) if 0 <= i < M]
    return np.array(sorted(set(idx)))


@dataclass
class Still:
    S: int
    M: int
    const: object
    samples: tuple
    idx: np.ndarray            # designed samples
    kind: list                 # their kinds
    still: np.ndarray          # (M,) bool: designed samples in which nothing ever moves (every row of a group equal)
    m: np.ndarray              # expected m (fp64: exact numbers, exactly representable in fp32) of the designed samples
    arg: np.ndarray            # expected arg-max rows of the designed samples
    s: int                     # the step of ``x_step``
    uk0: np.ndarray
    uk_last: np.ndarray        # u_k non-zero only at step S - 1: enters no row
    x0: np.ndarray
    x_last: np.ndarray         # x non-zero only at step S - 1: enters no row
    x_step: np.ndarray         # x non-zero only at step s: rows t <= s unchanged, later rows of the best groups lower


def drone_still(S, M=513, seed=0):
    """x_init = 0, u_k = 0, zero noise for the designed samples: p = v = 0 for ever, so every step of obstacle j is worth
    1 - q00 ox^2 - qs ox oy - q11 oy^2 (dyadic numbers: exact in any order of evaluation) and
        m = float(max_j value_j),   arg = j* S + 0   with j* the SMALLEST j among equal values.
    'last_row' (S >= 2): noise 2^10 (-1, 1/2) at step S - 2 alone -- it reaches v at S - 1 and p at S, i.e. row S - 1 only --
    moves the drone to (-1/8, 1/16), towards obstacle 0: row S - 1 of obstacle 0 is the strict maximum, arg = S - 1.  Only
    the last step of the last (guarded) batch sees it.  'last_noise': noise 2^12 at step S - 1 alone reaches v_S and no row:
    the answer of 'best1'.  The other samples are random ones of the sampler."""
    from oracle import drone as od
    c = drone_const(S, dt=STILL_DT, beta=STILL_BETA, x_init=np.zeros(6), obs_xy=STILL_OBS)
    DWs, masses, Q = [r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(seed + S), 'saa', M=M, S=S)]
    idx = designed_slots(M, len(STILL_KINDS))
    kind, m_exp, a_exp = [], [], []
    still = np.zeros(M, bool)
    for n, i in enumerate(idx):
        k = STILL_KINDS[n % len(STILL_KINDS)]
        if k == "last_row" and S < 2:
            k = "best0"
        kind.append(k)
        DWs[i], masses[i] = 0.0, STILL_MASS
        qs = STILL_Q[{"last_row": "best0", "last_noise": "best1"}.get(k, k)]
        Q[i] = 0.0
        for j, (q00, q01, q11) in enumerate(qs):
            Q[i, j, 0, 0], Q[i, j, 0, 1], Q[i, j, 1, 0], Q[i, j, 1, 1] = q00, q01 / 2.0, q01 / 2.0, q11
        vals = [_still_value(q, STILL_OBS[j]) for j, q in enumerate(qs)]
        if k == "last_row":
            DWs[i, S - 2, 3:5] = (-2.0 ** 10, 2.0 ** 9)
            p = STILL_DT * (np.sqrt(STILL_DT) * STILL_BETA / STILL_MASS) * DWs[i, S - 2, 3:5]
            assert tuple(p) == (-0.125, 0.0625)
            d = p - STILL_OBS[0]
            v = 1.0 - qs[0][0] * d[0] * d[0] - qs[0][1] * d[0] * d[1] - qs[0][2] * d[1] * d[1]
            assert v == -0.7734375 and v > max(vals)
            m_exp.append(v), a_exp.append(S - 1)
        else:
            if k == "last_noise":
                DWs[i, S - 1, 3:6] = (-2.0 ** 12, -2.0 ** 10, 2.0 ** 12)     # (towards obstacle 1, were it ever consumed)
            still[i] = True
            m_exp.append(max(vals)), a_exp.append(int(np.argmax(vals)) * S)
    m_exp = np.array(m_exp)
    assert np.array_equal(m_exp, r32(m_exp))
    z = np.zeros((S, 3))
    uk_last, x_last, x_step = z.copy(), z.copy(), z.copy()
    uk_last[S - 1] = (3.0, -2.0, 1.0)
    x_last[S - 1] = (5.0, -3.0, 2.0)
    s = S // 2 - 1 if S >= 4 else 0
    x_step[s] = (1.0, -1.0, 0.5)      # d p along (1, -1): away from every obstacle that is a maximum of some design
    return Still(S, M, c, (DWs, masses, Q), idx, kind, still, m_exp, np.array(a_exp), s, z, uk_last, z, x_last, x_step)


# ---- standing still: driving ---------------------------------------------------------------------------------------
CAR_STILL_D = ((4.0, 0.0), (0.0, -8.0), (8.0, 0.0), (0.0, 2.0), (16.0, 0.0))     # ego - pedestrian: |d| a power of two
CAR_STILL_KINDS = ("d0", "d1", "d2", "d3", "d4", "last_row", "last_noise", "d0")


def car_still(S, M=513, seed=0):
    """w_speed = w_rep = 0, pedestrian at rest, no noise, ego at rest (ego_init[2] = 0, u_k = 0): every row is d_min - |d| and
    the arg is 0.  |d| is a power of two along an axis, so |d|^2, 1 / |d| and |d|^2 / |d| are exact.  'last_row' (S >= 2): noise
    2^10 along x at step S - 2 alone gives the pedestrian the velocity sqrt(dt) beta 2^10 = 16 at S - 1 and moves it by 4, from
    |d| = 8 to 4, at S: row S - 1 is the strict maximum.  'last_noise': noise at step S - 1 alone, no row."""
    from oracle import driving as ocar
    c = car_const(S, dt=STILL_DT, beta=STILL_BETA)
    x0, ws, wr, DWs = [r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(seed + S), M, 'saa', S)]
    x0[:, 2] = 0.0                                             # the ego at rest (sample independent)
    ego = x0[0, 0:2].copy()
    idx = designed_slots(M, len(CAR_STILL_KINDS))
    kind, m_exp, a_exp = [], [], []
    still = np.zeros(M, bool)
    for n, i in enumerate(idx):
        k = CAR_STILL_KINDS[n % len(CAR_STILL_KINDS)]
        if k == "last_row" and S < 2:
            k = "d2"
        kind.append(k)
        d = np.array(CAR_STILL_D[{"last_row": 2, "last_noise": 1}.get(k, int(k[1]) if k[0] == "d" else 0)])
        DWs[i], ws[i], wr[i] = 0.0, 0.0, 0.0
        x0[i, 4:6], x0[i, 6:8] = ego - d, 0.0
        dist = float(np.hypot(*d))
        if k == "last_row":
            DWs[i, S - 2, 6] = 2.0 ** 10
            assert STILL_DT * (np.sqrt(STILL_DT) * STILL_BETA * 2.0 ** 10) == 4.0
            m_exp.append(c.d_min - 4.0), a_exp.append(S - 1)
        else:
            if k == "last_noise":
                DWs[i, S - 1, 6:8] = (0.0, -2.0 ** 10)                        # (towards the ego, were it ever consumed)
            still[i] = True
            m_exp.append(c.d_min - dist), a_exp.append(0)
    z = np.zeros((S, 2))
    uk_last, x_last, x_step = z.copy(), z.copy(), z.copy()
    uk_last[S - 1] = (3.0, -0.5)
    x_last[S - 1] = (-5.0, -0.25)
    s = S // 2 - 1 if S >= 4 else 0
    x_step[s] = (1.0, 0.5)            # the ego's response is along +x (heading 0): away from every pedestrian with d_x > 0
    return Still(S, M, c, (x0, ws, wr, DWs), idx, kind, still, np.array(m_exp), np.array(a_exp), s, z, uk_last, z, x_last, x_step)


# ---- rato_drone_rowmax_implicit: tables in exact arithmetic ----------------------------------------------------------
IMPLICIT_KINDS = ("edge_tie", "all_equal", "last_batch", "order_tie", "plain")
IMPLICIT_DT = 0.5


@dataclass
class ImplicitDesign:
    S: int
    M: int
    ld: int
    axes: int
    sign: float
    A22: np.ndarray            # (S, axes, ld) fp32
    W: np.ndarray              # (3, S, 2, ld) fp32
    base: np.ndarray           # (3, S, ld) fp32
    mass: np.ndarray           # (ld,) fp32
    xs: np.ndarray             # (S, 3) fp64
    kind: list
    values: np.ndarray         # (M, 3, S): the exact value of every row
    m: np.ndarray
    arg: np.ndarray


def implicit_targets(kind, S):
    """(3, S) integers: what the rows of one sample are worth.  Background -11 .. -1, the maxima (5) placed per kind."""
    j, t = np.meshgrid(np.arange(3), np.arange(S), indexing="ij")
    T = -((7 * j + 3 * t) % 11) - 1.0
    if kind == "edge_tie":            # the last row of group 0 and the first of group 1
        T[0, S - 1] = T[1, 0] = 5.0
        arg = S - 1
    elif kind == "all_equal":
        T[:] = 3.0
        arg = 0
    elif kind == "last_batch":        # a step only the final, partial batch of 8 reaches
        T[2, S - 1] = 5.0
        arg = 3 * S - 1
    elif kind == "order_tie":         # met first at (2, 0), then at the SMALLER row (0, S - 1): the order of the loop is not the rule
        T[2, 0] = T[0, S - 1] = 5.0
        arg = S - 1
    else:
        T[1, S // 2] = 5.0
        arg = S + S // 2
    return T, arg


def implicit_design(S, axes, sign, seed=0):
    """kp64 = 0 (a21 = 0), dt = 1/2, masses 1, 2, 4, a22 = 1 (the table holds 1 with a22_axes = 2 and 1 - a22 = 0 with 3), small
    integers for W and x: p_{t+1} is a multiple of 1/16 below 2^10 and every partial result exact in fp64.  base is chosen so
    that row (j, t) = W . p_{t+1} + sign base is exactly the integer ``implicit_targets`` wants; base is exact in fp32."""
    rng = np.random.RandomState(seed + 31 * S + axes)
    M = 2 * len(IMPLICIT_KINDS) + 1
    ld = M + 3
    mass = np.full(ld, np.nan, dtype=np.float32)
    mass[:M] = 2.0 ** (np.arange(M) % 3)
    xs = rng.randint(-2, 3, size=(S, 3)).astype(np.float64)
    A22 = np.full((S, axes, ld), np.nan, dtype=np.float32)
    A22[:, :, :M] = 1.0 if axes == 2 else 0.0
    Wt = np.full((3, S, 2, ld), np.nan, dtype=np.float32)
    Wt[..., :M] = rng.randint(-3, 4, size=(3, S, 2, M))
    base = np.full((3, S, ld), np.nan, dtype=np.float32)
    kind, values, args = [], np.empty((M, 3, S)), []
    for i in range(M):
        k = IMPLICIT_KINDS[i % len(IMPLICIT_KINDS)]
        T, arg = implicit_targets(k, S)
        p, v = np.zeros(2), np.zeros(2)
        for t in range(S):
            p, v = p + IMPLICIT_DT * v, v + (IMPLICIT_DT / float(mass[i])) * xs[t, :2]
            b = sign * (T[:, t] - (Wt[:, t, 0, i].astype(np.float64) * p[0] + Wt[:, t, 1, i].astype(np.float64) * p[1]))
            assert np.all(b == r32(b)) and np.all(p * 16 == np.round(p * 16))
            base[:, t, i] = b
        kind.append(k), args.append(arg)
        values[i] = T
    m, arg = rowmax_model(values, "ok")
    assert np.array_equal(arg, np.array(args))
    return ImplicitDesign(S, M, ld, axes, sign, A22, Wt, base, mass, xs, kind, values, m, arg)


def implicit_rows(A22, axes, W, base, mass, xs, sign, dt, kp, M, dtype=np.float64, a22_as_stored=False):
    """rows (M, 3, S) of rato_drone_rowmax_implicit from its tables, in ``dtype``.  a22_as_stored (a MISTAKE): the number in
    the table is taken for a22 whatever the layout says."""
    f = lambda a: np.asarray(a, dtype=dtype)
    S = xs.shape[0]
    inv_m = 1 / f(mass[:M])
    a21, dtm = -dtype(kp) * dtype(dt) * inv_m, dtype(dt) * inv_m
    p, v = np.zeros((M, 2), dtype=dtype), np.zeros((M, 2), dtype=dtype)
    rows = np.empty((M, 3, S), dtype=dtype)
    for t in range(S):
        a = f(A22[t, :2, :M]).T
        a22 = a if (axes == 2 or a22_as_stored) else 1 - a
        p, v = p + dtype(dt) * v, a21[:, None] * p + a22 * v + dtm[:, None] * f(xs[t, :2])[None]
        rows[:, :, t] = (f(W[:, t, 0, :M]) * p[:, 0] + f(W[:, t, 1, :M]) * p[:, 1] + dtype(sign) * f(base[:, t, :M])).T
    return rows
