"""Driving Gaussian baseline -- the reference's ``class Model`` of ``car/driving_gaussian.py:66-456`` with its define step
(jacfwd of the S-step mean / covariance recursion, :303-354) as one HIP launch (rato_car_gaussian_linearize).

The SCP is a sequence of small QPs in z = (u (2S), alphas_risk (S), slack (1)) solved on the host by ``qp.OSQP`` with the
reference's arguments.  The define step has no sample axis but a tangent axis: one lane per control direction, one workgroup
per problem, so ``linearize_device`` takes K problems (the reference's four alphas) in one launch.  The reference fixes S as
a module constant; here it is a keyword (default 20) and dt = T / S.

The row assembly (``all_constraints_coeffs`` ... ``constraints_coeffs``) is a pure host function of the kernel's arrays.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _lib, qp, qp_ipm
from . import driving_params as P

n_x, n_u = P.n_x, P.n_u
OSQP_TOL = 1e-8                                                  # driving_gaussian.py:27 (not driving_params.OSQP_TOL)
BETA = 3e-2                                                      # :77
MAX_S = 64                                                       # rato_car_gaussian_linearize: 2S lanes in one workgroup
SOLVERS = ('osqp', 'ipm')


def gauss_params(S, outer_product=False):
    """rato_car_gauss_params from driving_params (:72-91); ``outer_product``: the rank-one omega terms instead of the
    reference's scalar (rato_saa.h)."""
    p = _lib.CarGaussParams()
    p.S, p.outer_product, p.dt = int(S), int(bool(outer_product)), float(P.T / S)
    p.omega_speed_nom, p.omega_repulsive_nom = float(P.omega_speed_nom), float(P.omega_repulsive_nom)
    p.omega_speed_var = float((2 * P.omega_speed_del) ** 2 / 12.0)
    p.omega_repulsive_var = float((2 * P.omega_repulsive_del) ** 2 / 12.0)
    p.beta, p.speed_ped_des = BETA, float(P.speed_ped_des)
    p.min_separation_distance = float(P.min_separation_distance)
    goal = np.concatenate((P.position_ego_goal, P.velocity_ego_goal))
    var = np.diag(P.variance_ped_initial_state)
    for i in range(8):
        p.mean_init[i] = float(P.state_init[i])
    for i in range(4):
        p.ped_var_init[i], p.ego_goal[i] = float(var[i]), float(goal[i])
    return p


# ---- row assembly: host functions of the kernel's arrays of ONE problem (:303-426) ------------------------------------
def all_constraints_coeffs(lin, us_mat, alphas_risk):
    """get_all_constraints_coeffs (:303-354) from ``lin`` = dict(g_obs (S,), g_obs_du (S, 2S), g_obs_dalpha (S,) [the diagonal],
    v_final (4,), v_final_du (4, 2S)) -> the reference's five arrays."""
    us_vec = np.reshape(np.asarray(us_mat, dtype=np.float64), -1, 'C')
    alphas_risk = np.asarray(alphas_risk, dtype=np.float64)
    S = alphas_risk.shape[0]
    v_final_du, g_obs_du = np.asarray(lin["v_final_du"]), np.asarray(lin["g_obs_du"])
    g_obs_dalphas = np.diag(np.asarray(lin["g_obs_dalpha"]))
    v_final_du_dalphas = np.concatenate((v_final_du, np.zeros((4, S))), axis=-1)   # the ego does not see alphas_risk
    g_obs_du_dalphas = np.concatenate((g_obs_du, g_obs_dalphas), axis=-1)
    val_final = -np.asarray(lin["v_final"]) + v_final_du @ us_vec
    g_up = -np.asarray(lin["g_obs"]) + (g_obs_du @ us_vec + g_obs_dalphas @ alphas_risk)          # :349-351
    return v_final_du_dalphas, val_final, val_final.copy(), g_obs_du_dalphas, g_up


def all_constraints_coeffs_all(coeffs):
    """get_all_constraints_coeffs_all (:357-381): + the zero slack column, the obstacle rows one-sided."""
    final_du_dalphas, final_low, final_up, gs_obs_du_dalphas, gs_obs_up = coeffs
    S = gs_obs_up.shape[0]
    final_dparams = np.concatenate((final_du_dalphas, np.zeros((final_du_dalphas.shape[0], 1))), axis=-1)
    obs_dparams = np.zeros((S, n_u * S + S + 1))
    obs_dparams[:, :(n_u * S + S)] = gs_obs_du_dalphas
    return (np.vstack([final_dparams, obs_dparams]), np.hstack([final_low, -np.inf * np.ones(S)]),
            np.hstack([final_up, gs_obs_up.flatten()]))


def control_risk_constraints_coeffs_all(S, alpha, u_min, u_max):
    """get_control_risk_constraints_coeffs_all (:271-301): u_min <= u <= u_max, 100 OSQP_TOL <= alpha_t <= alpha and the
    same bounds on sum_t alpha_t."""
    n = n_u * S + S + 1
    A = np.zeros((n, n))
    l, u = np.zeros(n), np.zeros(n)
    k = n_u * S
    A[np.arange(k), np.arange(k)] = 1.0
    l[:k], u[:k] = u_min, u_max
    A[np.arange(k, k + S), np.arange(k, k + S)] = 1.0
    l[k:k + S], u[k:k + S] = 100 * OSQP_TOL, alpha
    A[-1, k:k + S] = 1.0
    l[-1], u[-1] = 100 * OSQP_TOL, alpha
    return A, l, u


def _pattern(S, relaxed):
    """The structural non-zeros of the stacked constraint matrix: the 4 final rows against the controls, obstacle row r
    against u[t'] for t' <= r and against its own alpha_r, then the bound rows.  With ``relaxed`` (scp_iter < 1) the rows
    from n_x = 8 on are zero.  Structural rather than value driven, so that ``update(Ax=...)`` always fits the set-up."""
    n = n_u * S + S + 1
    top = np.zeros((4 + S, n), dtype=bool)
    top[:4, :n_u * S] = True
    r = np.arange(S)
    top[4:, :n_u * S] = np.repeat(r[None, :] <= r[:, None], n_u, axis=1)
    top[4 + r, n_u * S + r] = True
    if relaxed:
        top[n_x:] = False
    return np.vstack([top, control_risk_constraints_coeffs_all(S, 1.0, -1.0, 1.0)[0] != 0.0])


def constraints_coeffs(lin, us_mat, alphas_risk, scp_iter, alpha, u_min=-P.u_max, u_max=P.u_max):
    """get_constraints_coeffs (:403-426) -> (A csc, l, u).  ``scp_iter < 1`` as written there: ``As[n_x:] *= 0`` with
    n_x = 8 although there are 4 final rows, so the first 4 separation rows stay, and ``ls[n_x:] *= 0`` turns the -inf of
    the one-sided rows into nan (``qp.OSQP`` reads a nan bound as no bound, like osqp)."""
    S = np.asarray(alphas_risk).shape[0]
    A_con, l_con, u_con = control_risk_constraints_coeffs_all(S, alpha, u_min, u_max)
    As, ls, us = all_constraints_coeffs_all(all_constraints_coeffs(lin, us_mat, alphas_risk))
    if scp_iter < 1:                                             # remove separation distance avoidance
        with np.errstate(invalid="ignore"):
            As[n_x:] *= 0
            ls[n_x:] *= 0
            us[n_x:] *= 0
    dense = np.vstack([As, A_con])
    mask = _pattern(S, scp_iter < 1)
    if np.any(dense[~mask] != 0.0):
        raise _lib.RatoError("the linearization has entries outside the structural pattern of the QP")
    cols, rows = np.nonzero(mask.T)
    indptr = np.concatenate(([0], np.cumsum(mask.sum(axis=0))))
    A = sp.csc_matrix((dense[rows, cols], rows, indptr), shape=dense.shape)
    return A, np.hstack([ls, l_con]), np.hstack([us, u_con])


def objective_coeffs(S, dt):
    """get_objective_coeffs (:383-401): dt u^T R u on the controls, nothing on alphas_risk and the slack."""
    n = n_u * S + S + 1
    Pm = sp.lil_matrix((n, n))
    for t in range(S):
        Pm[t * n_u:(t + 1) * n_u, t * n_u:(t + 1) * n_u] = 2 * dt * P.R
    return sp.csc_matrix(Pm), np.zeros(n)


class Model:
    def __init__(self, method='gaussian', alpha=0.1, S=P.S, device='cuda:0', outer_product=False, verbose=False,
                 solver='osqp'):
        """``solver``: 'osqp' (``qp.OSQP`` with the reference's arguments) or 'ipm' (``qp_ipm.IPM``: the batched interior-point
        solver on the device, tol = OSQP_TOL, every solve a cold start)"""
        import torch
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        self.solver = solver
        if not 1 <= S <= MAX_S:
            raise ValueError(f"S must be in 1..{MAX_S} (one lane per control direction), got {S}")
        if verbose:
            print("Initializing Model with")
            print("> method     =", method)
            print("> alpha      =", alpha)
        self.method = method
        self.u_max = P.u_max
        self.u_min = -self.u_max
        self.alpha = alpha
        self.beta = BETA
        self.S, self.dt = int(S), P.T / S
        self.outer_product = bool(outer_product)
        self.omega_speed_nominal, self.omega_repulsive_nominal = P.omega_speed_nom, P.omega_repulsive_nom
        self.omegas_speed_variance = (2 * P.omega_speed_del) ** 2 / 12.0
        self.omegas_repulsive_variance = (2 * P.omega_repulsive_del) ** 2 / 12.0
        self.state_mean_init = P.state_init
        self.state_covariance_init = np.zeros((n_x, n_x))
        self.state_covariance_init[4:, 4:] = P.variance_ped_initial_state
        self.device = torch.device(device)
        self._lib = _lib.load()
        self._params = gauss_params(self.S, self.outer_product)

    # ---- layout helpers (:93-113) --------------------------------------------------------------------------------------
    def convert_us_vec_to_us_mat(self, us_vec):
        return np.reshape(np.asarray(us_vec), (n_u, self.S), 'F').T.copy()

    def convert_us_mat_to_us_jaxvec(self, us_mat):
        return np.reshape(np.asarray(us_mat), (self.S * n_u), 'C')

    def initial_guess_us_mat(self):
        return np.zeros((self.S, n_u)) + (self.u_max + self.u_min) / 2.0 + 1e-2

    def initial_guess_alphas_risk(self):
        return (self.alpha / self.S) * np.ones(self.S)

    # ---- the kernel -----------------------------------------------------------------------------------------------------
    def linearize_device(self, us_batch, alphas_batch, want_trajectory=False):
        """K problems in ONE launch (rato_car_gaussian_linearize).  us_batch (K, S, 2), alphas_batch (K, S), host arrays or
        device tensors -> dict of fp64 DEVICE tensors: g_obs (K, S), g_obs_du (K, S, 2S), g_obs_dalpha (K, S) [the diagonal],
        v_final (K, 4), v_final_du (K, 4, 2S), and with ``want_trajectory`` mus (K, S+1, 8), Sigmas (K, S+1, 8, 8)."""
        import torch
        S = self.S

        def dev(a, shape, name):
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
            t = t.to(device=self.device, dtype=torch.float64).contiguous()
            if t.dim() != len(shape) + 1 or tuple(t.shape[1:]) != shape:
                raise ValueError(f"{name} must be (K,{','.join(str(s) for s in shape)}), got {tuple(t.shape)}")
            return t
        us, al = dev(us_batch, (S, n_u), "us_batch"), dev(alphas_batch, (S,), "alphas_batch")
        K = us.shape[0]
        if K < 1 or al.shape[0] != K:
            raise ValueError(f"us_batch and alphas_batch must hold the same K >= 1 problems, got {K} and {al.shape[0]}")
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
        out = {"g_obs": new(K, S), "g_obs_du": new(K, S, n_u * S), "g_obs_dalpha": new(K, S), "v_final": new(K, 4),
               "v_final_du": new(K, 4, n_u * S)}
        mus = new(K, S + 1, n_x) if want_trajectory else None
        Sigmas = new(K, S + 1, n_x, n_x) if want_trajectory else None
        _lib.check(self._lib.rato_car_gaussian_linearize(
            C.byref(self._params), K, _lib.ptr(us), _lib.ptr(al), _lib.ptr(mus), _lib.ptr(Sigmas), _lib.ptr(out["g_obs"]),
            _lib.ptr(out["g_obs_du"]), _lib.ptr(out["g_obs_dalpha"]), _lib.ptr(out["v_final"]), _lib.ptr(out["v_final_du"]),
            _lib.current_stream()), "rato_car_gaussian_linearize")
        if want_trajectory:
            out["mus"], out["Sigmas"] = mus, Sigmas
        return out

    def _linearize_host(self, us_mat, alphas_risk, want_trajectory=False):
        r = self.linearize_device(np.asarray(us_mat)[None], np.asarray(alphas_risk)[None], want_trajectory)
        return {k: v[0].cpu().numpy() for k, v in r.items()}

    # ---- mean, covariance, constraints (:171-264) --------------------------------------------------------------------------
    def us_to_state_trajectory(self, us_mat):
        return self._linearize_host(us_mat, self.initial_guess_alphas_risk(), True)["mus"]

    def us_to_covariance_trajectory(self, us_mat):
        return self._linearize_host(us_mat, self.initial_guess_alphas_risk(), True)["Sigmas"]

    def final_constraints(self, xs):
        return np.asarray(xs)[-1, :4] - np.concatenate((P.position_ego_goal, P.velocity_ego_goal))

    def separation_distances_at_all_times(self, mus, Sigmas, alphas_risk):
        """:237-264, on the host from a trajectory (scipy's ppf as in the reference; the kernel's own -g_obs is the device
        form of the same rows)."""
        from scipy.stats import norm
        mus, Sigmas = np.asarray(mus)[1:], np.asarray(Sigmas)[1:]
        d = mus[:, 0:2] - mus[:, 4:6]
        dist = np.linalg.norm(d, axis=-1)
        n = d / dist[:, None]
        pad = norm.ppf(1 - np.asarray(alphas_risk)) * np.sqrt(np.einsum("ti,tij,tj->t", n, Sigmas[:, 4:6, 4:6], n))
        return dist - pad - P.min_separation_distance

    # ---- QP rows (:271-426) ---------------------------------------------------------------------------------------------
    def get_control_risk_constraints_coeffs_all(self):
        return control_risk_constraints_coeffs_all(self.S, self.alpha, self.u_min, self.u_max)

    def get_all_constraints_coeffs(self, us_mat, alphas_risk, lin=None):
        lin = self._linearize_host(us_mat, alphas_risk) if lin is None else lin
        return all_constraints_coeffs(lin, us_mat, alphas_risk)

    def get_all_constraints_coeffs_all(self, us_mat, alphas_risk, lin=None):
        return all_constraints_coeffs_all(self.get_all_constraints_coeffs(us_mat, alphas_risk, lin))

    def get_objective_coeffs(self):
        return objective_coeffs(self.S, self.dt)

    def get_constraints_coeffs(self, us_mat, alphas_risk, scp_iter, lin=None):
        lin = self._linearize_host(us_mat, alphas_risk) if lin is None else lin
        return constraints_coeffs(lin, us_mat, alphas_risk, scp_iter, self.alpha, self.u_min, self.u_max)

    # ---- host QP (:428-456) ---------------------------------------------------------------------------------------------
    def define_problem(self, us_mat_p, alphas_risk_p, scp_iter=0, verbose=False, lin=None):
        """``lin``: this problem's slice of a K-problem ``linearize_device`` call (host arrays), else one launch here."""
        self.P, self.q = self.get_objective_coeffs()
        self.A, self.l, self.u = self.get_constraints_coeffs(us_mat_p, alphas_risk_p, scp_iter, lin)
        if self.solver == 'ipm':
            if scp_iter == 0 or scp_iter == 1:
                self.osqp_prob = qp_ipm.IPM(device=str(self.device))
                self.osqp_prob.setup(self.P, self.q, self.A, self.l, self.u, tol=OSQP_TOL)
            else:
                self.osqp_prob.update(l=self.l, u=self.u)
                self.osqp_prob.update(Ax=self.A.data)
        elif scp_iter == 0 or scp_iter == 1:
            self.osqp_prob = qp.OSQP()
            self.osqp_prob.setup(self.P, self.q, self.A, self.l, self.u, eps_abs=OSQP_TOL, eps_rel=OSQP_TOL,
                                 linsys_solver="qdldl", warm_start=True, verbose=verbose, polish=P.OSQP_POLISH)
        else:
            self.osqp_prob.update(l=self.l, u=self.u)
            self.osqp_prob.update(Ax=self.A.data)
        return True

    def solve(self, verbose=False):
        self.res = self.osqp_prob.solve()
        return self.solution(verbose)

    def solution(self, verbose=False):
        """(us, alphas_risk) of ``self.res`` (left by ``solve``, or by a batched solve of several models' problems)"""
        S = self.S
        if self.res.info.status != 'solved' and verbose:
            print("[solve]: Problem infeasible.")
        us_sol = self.convert_us_vec_to_us_mat(self.res.x[:(n_u * S)])
        alphas_sol = self.res.x[(n_u * S):-1]
        return us_sol, alphas_sol
