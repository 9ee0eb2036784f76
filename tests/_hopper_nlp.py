"""fp64 NumPy restatement of the hopper's NLP callbacks (hopper/hopper.py): every row of g, its Jacobian and the Hessian of
lam . g, what the HIP kernels (csrc/hopper_nlp.hip) and ``hopper.Model``'s NLP members are compared with.  It lives here
because oracle/ is frozen; the slip rows (the sample axis) are taken from oracle/hopper.py, which restates them already.

z = (x_0 .. x_S (8 each), u_0 .. u_{S-1} (4 each), ys (M), slack, t_risk) (:105-132).

Restated lines of hopper/hopper.py:
  :166-171  end_effector_position
  :218-231  b(x, u) = (q_dot, M^-1 (-C + B u_robot + J^T f)) with the diagonal M^-1 of :192-199, C of :202-207, B of :210-215
            and J of :174-179, written out per component
  :239-254  dynamics_constraints: the RK4 defect of every step
  :256-298  initial, final, contact, leg-over-ground and no-slip rows
  :369-438  length / speed, control and slack rows with their bounds
  :441-453  f
  :491-562  g and gL_gU: the ten groups in the script's order
  :599-620  the variable bounds

Derivatives.  Every non-linear quantity is carried as a second-order Taylor jet (value, gradient, Hessian) over the 12 local
variables (x_t, u_t) of a step, for all steps at once, with the product, sin and cos rules written out in ``Jet``: no
closed-form derivative of the dynamics appears here.  The Hessian of lam . g is assembled block by block; that nothing lies
outside the blocks is checked against the reference's numbers (tests/test_hopper_nlp_pin.py), not assumed.
"""
import numpy as np

N_X, N_U, N_L = 8, 4, 12
N_PAIRS = N_L * (N_L + 1) // 2
T_HORIZON = 2.0                                                  # :46
MASS_BODY, MASS_LEG = 3.0, 0.3                                   # :61-62
INERTIA_BODY, INERTIA_LEG = 0.75, 0.075                          # :63-64
GRAVITY = 9.81                                                   # :65
U_MAX, MAX_CONTACT_FORCE = 1000.0, 1000.0                        # :60, :66
STATE_INITIAL = np.array([1e-6, 1.0, -1e-6, 1.0, 0., 0., 0., 0.]) + 2e-7      # :83-85
STATE_FINAL = np.array([0.15, 1., -1e-6, 1., 0., 0., 0., 0.]) + 2e-7          # :87-89
TRIL_R, TRIL_C = np.tril_indices(N_L)


def constants(S, dt=None):
    return dict(S=S, dt=T_HORIZON / S if dt is None else dt, mt=MASS_BODY + MASS_LEG, it=INERTIA_BODY + INERTIA_LEG,
                ml=MASS_LEG, g=GRAVITY)


def nvar_of(S, M):
    return N_X * (S + 1) + N_U * S + M + 2


# ---- second-order jets ----------------------------------------------------------------------------------------------------
class Jet:
    """value v (...), gradient g (..., n), Hessian h (..., n, n)"""
    __array_ufunc__ = None                                       # ndarray (op) Jet defers to the reflected operator

    def __init__(self, v, g, h):
        self.v, self.g, self.h = v, g, h

    @staticmethod
    def variable(v, i, n):
        g = np.zeros(v.shape + (n,))
        g[..., i] = 1.0
        return Jet(v, g, np.zeros(v.shape + (n, n)))

    @staticmethod
    def lift(x, like):
        return x if isinstance(x, Jet) else Jet(np.broadcast_to(np.asarray(x, dtype=np.float64), like.v.shape),
                                                np.zeros_like(like.g), np.zeros_like(like.h))

    def __add__(self, o):
        o = Jet.lift(o, self)
        return Jet(self.v + o.v, self.g + o.g, self.h + o.h)
    __radd__ = __add__

    def __neg__(self):
        return Jet(-self.v, -self.g, -self.h)

    def __sub__(self, o):
        return self + (-Jet.lift(o, self))

    def __rsub__(self, o):
        return Jet.lift(o, self) + (-self)

    def __mul__(self, o):
        if not isinstance(o, Jet):
            return Jet(self.v * o, self.g * o, self.h * o)
        outer = self.g[..., :, None] * o.g[..., None, :]
        return Jet(self.v * o.v, self.v[..., None] * o.g + o.v[..., None] * self.g,
                   self.v[..., None, None] * o.h + o.v[..., None, None] * self.h + outer + np.swapaxes(outer, -1, -2))
    __rmul__ = __mul__

    def _compose(self, f, df, d2f):
        return Jet(f, df[..., None] * self.g,
                   df[..., None, None] * self.h + d2f[..., None, None] * (self.g[..., :, None] * self.g[..., None, :]))

    def sin(self):
        s, c = np.sin(self.v), np.cos(self.v)
        return self._compose(s, c, -s)

    def cos(self):
        s, c = np.sin(self.v), np.cos(self.v)
        return self._compose(c, -s, -c)


def _b(c, x, u):
    """:218-231 on a list of 8 + 4 jets (or floats)"""
    s, cs = x[2].sin(), x[2].cos()
    return [x[4], x[5], x[6], x[7],
            (u[2] - s * u[1]) * (1.0 / c["mt"]),
            (cs * u[1] + u[3] - c["mt"] * c["g"]) * (1.0 / c["mt"]),
            (u[0] + x[3] * (cs * u[2] + s * u[3])) * (1.0 / c["it"]),
            (u[1] + s * u[2] - cs * u[3]) * (1.0 / c["ml"])]


def split(Z, S):
    Z = np.asarray(Z, dtype=np.float64)
    return Z[:N_X * (S + 1)].reshape(S + 1, N_X), Z[N_X * (S + 1):N_X * (S + 1) + N_U * S].reshape(S, N_U)


def local(Z, S, dt=None):
    """the per-step quantities the kernels write, with the second derivatives:
    defect (S, 8), d_defect (S, 8, 12), d2_defect (S, 8, 12, 12) over (x_t, u_t);
    rows (S+1, 2), d_rows (S+1, 2, 4) over (x2, x3, x6, x7), d2_rows (S+1, 2, 8, 8) over x_t."""
    c = constants(S, dt)
    xs, us = split(Z, S)
    x = [Jet.variable(xs[:-1, i], i, N_L) for i in range(N_X)]
    u = [Jet.variable(us[:, i], N_X + i, N_L) for i in range(N_U)]
    h = c["dt"]
    k1 = _b(c, x, u)
    k2 = _b(c, [x[i] + k1[i] * (0.5 * h) for i in range(N_X)], u)
    k3 = _b(c, [x[i] + k2[i] * (0.5 * h) for i in range(N_X)], u)
    k4 = _b(c, [x[i] + k3[i] * h for i in range(N_X)], u)
    eq = [xs[1:, i] - (x[i] + (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) * (h / 6.0)) for i in range(N_X)]
    y = [Jet.variable(xs[:, i], i, N_X) for i in range(N_X)]
    s, cs = y[2].sin(), y[2].cos()
    slip = y[4] + y[3] * cs * y[6] + s * y[7]                   # J_T @ q_dot, J_T = (1, 0, x3 cos x2, sin x2) (:288-293)
    height = y[1] - y[3] * cs                                   # :166-171
    sel = [2, 3, 6, 7]
    return dict(defect=np.stack([e.v for e in eq], -1), d_defect=np.stack([e.g for e in eq], -2),
                d2_defect=np.stack([e.h for e in eq], -3),
                rows=np.stack([slip.v, height.v], -1), d_rows=np.stack([slip.g[:, sel], height.g[:, sel]], -2),
                d_rows_full=np.stack([slip.g, height.g], -2), d2_rows=np.stack([slip.h, height.h], -3))


def blocks_of(loc, lam_dyn, lam_rows, add=None):
    """Hessian blocks (S+1, 12, 12) of sum lam_dyn . defect + sum lam_rows . rows (+ add, given as (S+1, 78))"""
    S = loc["defect"].shape[0]
    H = np.zeros((S + 1, N_L, N_L))
    H[:S] = np.einsum("ti,tiab->tab", lam_dyn, loc["d2_defect"])
    H[:, :N_X, :N_X] += np.einsum("ti,tiab->tab", lam_rows, loc["d2_rows"])
    if add is not None:
        H += untril78(add)
    return H


def tril78(B):
    return np.asarray(B)[..., TRIL_R, TRIL_C]


def untril78(v):
    v = np.asarray(v)
    B = np.zeros(v.shape[:-1] + (N_L, N_L))
    B[..., TRIL_R, TRIL_C] = v
    B[..., TRIL_C, TRIL_R] = v
    return B


# ---- the script's row order (:491-514) --------------------------------------------------------------------------------------
def layout(S, M, tj, tl, method):
    """offsets of the ten groups of g and ncon"""
    n_state = tj + (S + 1 - tl)                                  # states of [:tj] and [tl:] (:270-272, :295-297)
    C = tj + (S - tl)                                            # contact steps (:306-311)
    n_risk = (1 + M + M * C + 1) if method == 'saa' else M * C
    names = ("dyn", "x0", "xf", "slip", "contact", "over", "risk", "control", "slack", "len")
    counts = (N_X * S, N_X, 2, n_state, n_state, tl - tj, n_risk, N_U * S, 1, 3 * S)
    off, o = {}, 0
    for n, k in zip(names, counts):
        off[n] = o
        o += k
    off["ncon"], off["C"], off["n_state"], off["n_risk"] = o, C, n_state, n_risk
    return off


def contact_states(S, tj, tl):
    return np.concatenate([np.arange(0, tj), np.arange(tl, S + 1)]).astype(np.int64)


def fold_lam(lam, S, M, tj, tl, method):
    """the multipliers of g -> lam_dyn (S, 8), lam_rows (S+1, 2): no-slip and contact weights on the contact states, minus the
    leg-over-ground multiplier on the flight states"""
    L = layout(S, M, tj, tl, method)
    lam = np.asarray(lam, dtype=np.float64)
    lam_rows = np.zeros((S + 1, 2))
    st = contact_states(S, tj, tl)
    lam_rows[st, 0] = lam[L["slip"]:L["slip"] + L["n_state"]]
    lam_rows[st, 1] = lam[L["contact"]:L["contact"] + L["n_state"]]
    lam_rows[tj:tl, 1] = -lam[L["over"]:L["over"] + (tl - tj)]
    return lam[:N_X * S].reshape(S, N_X).copy(), lam_rows


def _oracle(fields, method, alpha, S):
    from oracle import hopper as oh
    o = oh.Model(*fields, method=method, alpha=alpha, S=S)
    return o


def g_full(Z, S, M, method, alpha, fields, loc=None):
    """:491-514 with the phases of oracle/hopper.py (S // 3, 2 S // 3)"""
    o = _oracle(fields, method, alpha, S)
    tj, tl = o.time_jump, o.time_land
    loc = loc or local(Z, S)
    xs, us = split(Z, S)
    st = contact_states(S, tj, tl)
    return np.concatenate([loc["defect"].reshape(-1), xs[0] - STATE_INITIAL, (xs[-1] - STATE_FINAL)[4:6],
                           loc["rows"][st, 0], loc["rows"][st, 1], -loc["rows"][tj:tl, 1], o.slip_risk_constraints(np.asarray(Z)),
                           us.reshape(-1), [Z[-2]], xs[1:, 3], xs[1:, 7], xs[1:, 6]])


def jac_dense(Z, S, M, method, alpha, fields, loc=None):
    """jacrev(g) (:569), dense (ncon, nvar)"""
    o = _oracle(fields, method, alpha, S)
    tj, tl = o.time_jump, o.time_land
    L = layout(S, M, tj, tl, method)
    loc = loc or local(Z, S)
    nvar = nvar_of(S, M)
    J = np.zeros((L["ncon"], nvar))
    nX = N_X * (S + 1)
    for t in range(S):
        r = slice(N_X * t, N_X * t + N_X)
        J[r, N_X * t:N_X * t + N_X] = loc["d_defect"][t][:, :N_X]
        J[r, nX + N_U * t:nX + N_U * t + N_U] = loc["d_defect"][t][:, N_X:]
        J[r, N_X * (t + 1):N_X * (t + 2)] += np.eye(N_X)
    J[L["x0"] + np.arange(N_X), np.arange(N_X)] = 1.0
    J[L["xf"] + np.arange(2), N_X * S + 4 + np.arange(2)] = 1.0
    for i, t in enumerate(contact_states(S, tj, tl)):
        J[L["slip"] + i, N_X * t:N_X * t + N_X] = loc["d_rows_full"][t, 0]
        J[L["contact"] + i, N_X * t:N_X * t + N_X] = loc["d_rows_full"][t, 1]
    for i, t in enumerate(range(tj, tl)):
        J[L["over"] + i, N_X * t:N_X * t + N_X] = -loc["d_rows_full"][t, 1]
    J[L["risk"]:L["risk"] + L["n_risk"]] = o.slip_jacobian(np.asarray(Z)).toarray()
    J[L["control"] + np.arange(N_U * S), nX + np.arange(N_U * S)] = 1.0
    J[L["slack"], nvar - 2] = 1.0
    for j, comp in enumerate((3, 7, 6)):
        J[L["len"] + j * S + np.arange(S), N_X * (1 + np.arange(S)) + comp] = 1.0
    return J


def block_vars(S, t):
    """global indices of the local variables (x_t, u_t) of block t (the u part of block S does not exist: -1)"""
    u = N_X * (S + 1) + N_U * t + np.arange(N_U) if t < S else -np.ones(N_U, dtype=np.int64)
    return np.concatenate([N_X * t + np.arange(N_X), u]).astype(np.int64)


def blocks_from_dense(H, S):
    """(S+1, 12, 12) step blocks of a dense (nvar, nvar) Hessian, and the dense matrix with the blocks removed"""
    out = np.zeros((S + 1, N_L, N_L))
    rest = np.array(H, dtype=np.float64)
    for t in range(S + 1):
        v = block_vars(S, t)
        ok = v >= 0
        out[t][np.ix_(ok, ok)] = H[np.ix_(v[ok], v[ok])]
        rest[np.ix_(v[ok], v[ok])] = 0.0
    return out, rest


def slip_blocks(Z, lam, S, M, method, alpha, fields):
    """the slip rows' share of the Hessian (oracle/hopper.py: slip_hessian) as step blocks (S+1, 12, 12), and what is left
    outside them (must be nothing)"""
    o = _oracle(fields, method, alpha, S)
    L = layout(S, M, o.time_jump, o.time_land, method)
    r0 = L["risk"] + (1 + M if method == 'saa' else 0)
    lam_s = np.asarray(lam)[r0:r0 + M * L["C"]].reshape(M, L["C"])
    Hs = o.slip_hessian(np.asarray(Z), lam_s).toarray()
    return blocks_from_dense(Hs, S)


def hess_blocks_full(Z, lam, S, M, method, alpha, fields, obj_factor=0.0, loc=None):
    """blocks (S+1, 12, 12) of obj_factor hess_f + hess(lam . g) (:622-628)"""
    o = _oracle(fields, method, alpha, S)
    loc = loc or local(Z, S)
    lam_dyn, lam_rows = fold_lam(lam, S, M, o.time_jump, o.time_land, method)
    H = blocks_of(loc, lam_dyn, lam_rows)
    Hs, rest = slip_blocks(Z, lam, S, M, method, alpha, fields)
    assert not np.any(rest)
    H += Hs
    H[:S, 8, 8] += 2.0 * obj_factor                               # f = sum R (u0^2 + u1^2) + linear terms, R = 1 (:441-453)
    H[:S, 9, 9] += 2.0 * obj_factor
    return H


def dense_from_blocks(B, S, nvar):
    H = np.zeros((nvar, nvar))
    for t in range(S + 1):
        v = block_vars(S, t)
        ok = v >= 0
        H[np.ix_(v[ok], v[ok])] += B[t][np.ix_(ok, ok)]
    return H


def objective(Z, S):
    xs, us = split(Z, S)
    return float(np.sum(us[:, 0] ** 2 + us[:, 1] ** 2) - 10000 * xs[-1, 0] + 10000000 * Z[-2])


def grad_objective(Z, S):
    g = np.zeros(len(Z))
    nX = N_X * (S + 1)
    xs, us = split(Z, S)
    g[nX + N_U * np.arange(S)] = 2 * us[:, 0]
    g[nX + N_U * np.arange(S) + 1] = 2 * us[:, 1]
    g[N_X * S] = -10000.0
    g[-2] = 10000000.0
    return g


def bounds_g(S, M, tj, tl, method):
    """gL_gU (:515-562)"""
    L = layout(S, M, tj, tl, method)
    g_L, g_U = np.zeros(L["ncon"]), np.zeros(L["ncon"])
    g_L[L["over"]:] = -1e15
    cl, cu = np.zeros((S, N_U)), np.zeros((S, N_U))
    cl[:, :2], cu[:, :2] = -U_MAX, U_MAX
    cu[:tj, 2:] = MAX_CONTACT_FORCE
    cu[tl:, 2:] = MAX_CONTACT_FORCE
    g_L[L["control"]:L["slack"]], g_U[L["control"]:L["slack"]] = cl.reshape(-1), cu.reshape(-1)
    g_L[L["slack"]], g_U[L["slack"]] = 0.0, 1e6
    g_L[L["len"]:] = np.concatenate([0.25 * np.ones(S), -4.0 * np.ones(S), -2.5 * np.ones(S)])
    g_U[L["len"]:] = np.concatenate([1.0 * np.ones(S), 4.0 * np.ones(S), 2.5 * np.ones(S)])
    return g_L, g_U


def bounds_x(S, M):
    """:599-620"""
    nvar = nvar_of(S, M)
    x_L, x_U = -np.ones(nvar) * 1000.0, np.ones(nvar) * 1000.0
    lo = np.array([-3, 0.5, -np.pi / 2, 0.1, -500, -500, -500, -500])
    hi = np.array([3, 10, np.pi / 2, 3, 500, 500, 500, 500])
    x_L[:N_X * (S + 1)] = np.tile(lo, S + 1)
    x_U[:N_X * (S + 1)] = np.tile(hi, S + 1)
    return x_L, x_U


# ---- documented input builders ----------------------------------------------------------------------------------------------
def problem(S, M, seed):
    """a perturbed iterate with every state and control component alive (velocities included), and ys, slack, t_risk"""
    rng = np.random.RandomState(1000 + 17 * S + seed)
    xs = np.zeros((S + 1, N_X))
    xs[:, 0] = np.linspace(0, 0.15, S + 1)
    xs[:, 1] = 1.0
    xs[:, 2] = 0.2 * np.sin(np.linspace(0, 3, S + 1))
    xs[:, 3] = 0.9 + 0.1 * np.cos(np.linspace(0, 2, S + 1))
    xs += 0.1 * rng.uniform(-1, 1, xs.shape)
    xs[:, 4:] += 0.5 * rng.uniform(-1, 1, (S + 1, 4))
    us = np.zeros((S, N_U))
    us[:, 0] = 2.0 * rng.uniform(-1, 1, S)
    us[:, 1] = 20.0 + 10.0 * rng.uniform(-1, 1, S)
    us[:, 3] = 32.0 + rng.randn(S)
    us[:, 2] = 0.08 * us[:, 3] + 0.3 * rng.randn(S)
    return np.concatenate([xs.reshape(-1), us.reshape(-1), 0.1 * rng.rand(M), [0.03, -0.4]])


def lam_pair(S, seed):
    """mixed-sign lam_dyn (S, 8), lam_rows (S+1, 2)"""
    rng = np.random.RandomState(2000 + 17 * S + seed)
    return rng.uniform(-1, 1, (S, N_X)), rng.uniform(-1, 1, (S + 1, 2))


def directions(n, count=3, seed=3):
    """seeded directions normalised to max |v| = 1"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        v = rng.uniform(-1, 1, n)
        out.append(v / np.max(np.abs(v)))
    return out


def rel_err(a, b):
    """max |a - b| relative to max |b|"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), np.finfo(float).tiny)) if a.size else 0.0


def rel_err_blocks(a, b, block_ndim=2):
    """the same per Hessian block (the last ``block_ndim`` axes), the worst block; a block that is all zero in the reference
    must be all zero"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    width = int(np.prod(a.shape[a.ndim - block_ndim:]))
    a2, b2 = a.reshape(-1, width), b.reshape(-1, width)
    worst = 0.0
    for x, y in zip(a2, b2):
        m = np.max(np.abs(y))
        if m == 0.0:
            assert not np.any(x), "a block that is exactly 0 in the reference"
            continue
        worst = max(worst, float(np.max(np.abs(x - y)) / m))
    return worst
