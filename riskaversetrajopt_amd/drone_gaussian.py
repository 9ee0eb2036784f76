"""Drone Gaussian baseline -- the reference's ``class Model`` of ``drone/drone_gaussian.py:64-396`` and the callbacks its
solve block hands to IPOPT (:409-498), with g, jacfwd(g) and jacfwd(jacfwd(lam . g)) as HIP launches
(rato_drone_gaussian_linearize / rato_drone_gaussian_hessian, csrc/drone_gaussian.hip) for K problems per call.

z = (u (3S), state allocations (S n_obs), obstacle allocations (n_obs)) in the reference's layout (include/rato_saa.h).  The
device evaluates the n_nl = 6 + n_obs S + 4 (S+1) non-linear rows; the nvar + 1 linear rows (z itself and the sum of the
allocations, :323-349) and the objective's constant Hessian are filled once on the host (``ipopt_callbacks``).  The
reference fixes S as a module constant; here it is the constructor's argument and dt = T / S (as its Model does).
``scp.run_drone_gaussian`` solves the NLP with scipy's trust-constr on these callbacks, one alpha after the other through the
host (``solver='trust-constr'``, the default), or with the batched interior-point method of ``drone_gaussian_ipm``
(``solver='ipm'``; ``Model.solve``): K problems in lockstep, the Newton step on the device on jac_nl and the packed Hessian where
these kernels leave them.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import drone_params as P

n_x, n_u, n_obs = P.n_x, P.n_u, P.n_obs
MAX_S = 64                                                       # 3S lanes in one workgroup
BOUND_HIGH = (0.5, 0.5)                                          # :368
BOUND_LOW = (-2.0, -0.5)                                         # :369
ALPHA_MIN = 1e-6                                                 # :343


def gauss_params(S):
    """rato_drone_gauss_params from drone_params (:27-48, :72-84)"""
    p = _lib.DroneGaussParams()
    p.S, p.reserved, p.dt = int(S), 0, float(P.T / S)
    p.mass_nom, p.mass_var = float(P.mass_nom), float((2 * P.mass_delta) ** 2 / 12.0)
    p.beta, p.drag = float(P.beta), float(P.drag_coefficient)
    p.feedback_kp, p.feedback_kd = float(P.feedback_gain[0, 0]), float(P.feedback_gain[0, 3])
    for i in range(6):
        p.x_init[i], p.x_final[i] = float(P.x_init[i]), float(P.x_final[i])
    for i in range(n_obs):
        p.obs_positions[i][0], p.obs_positions[i][1] = float(P.obs_positions[i, 0]), float(P.obs_positions[i, 1])
        p.obs_radii[i] = float(P.obs_radii[i])
    p.obs_radii_delta = float(P.obs_radii_deltas)
    for i in range(2):
        p.bound_high[i], p.bound_low[i] = BOUND_HIGH[i], BOUND_LOW[i]
    return p


def sizes(S):
    """-> nvar, n_nl, ncon (the script's g has the n_nl non-linear rows, then z, then the allocation sum)"""
    nvar = n_u * S + S * n_obs + n_obs
    n_nl = 6 + n_obs * S + 4 * (S + 1)
    return nvar, n_nl, n_nl + nvar + 1


class Model:
    def __init__(self, S, method='gaussian', alpha=0.1, device='cuda:0', verbose=False):
        if not 1 <= S <= MAX_S:
            raise ValueError(f"S must be in 1..{MAX_S} (one lane per control direction), got {S}")
        if verbose:
            print("Initializing Model with")
            print("> method =", method)
            print("> alpha  =", alpha)
            print("> S      =", S)
        self.method = method
        self.S = int(S)
        self.dt = P.T / S
        self.u_max = P.u_max
        self.u_min = -self.u_max
        self.alpha = alpha
        self.beta = P.beta
        self.drag_coefficient = P.drag_coefficient
        self.mass_nominal = P.mass_nom
        self.mass_variance = (2 * P.mass_delta) ** 2 / 12.0
        self.obs_positions = P.obs_positions
        self.obs_radii = P.obs_radii
        self.nvar, self.n_nl, self.ncon = sizes(self.S)
        self.device = device
        self._lib_handle = None
        self._params = None

    # ---- layout helpers (:86-133) ----------------------------------------------------------------------------------------
    def convert_z_to_variables(self, z):
        z = np.asarray(z)
        return z[:(self.S * n_u)], z[(self.S * n_u):]

    def convert_us_vec_to_us_mat(self, us_vec):
        return np.reshape(np.asarray(us_vec), (n_u, self.S), 'F').T.copy()

    def convert_us_mat_to_us_jaxvec(self, us_mat):
        return np.reshape(np.asarray(us_mat), (self.S * n_u), 'C')

    def initial_guess_us_mat(self, results_dir='results'):
        my_file = os.path.join(results_dir, 'drone' + '_alpha=' + str(self.alpha) + '_repeat=0.npy')
        if not os.path.isfile(my_file):
            raise FileNotFoundError(my_file + " does not exist.\n" + "run drone_risk.py first.")
        with open(my_file, 'rb') as f:
            us = np.load(f)
        return us

    def initial_guess_alphas_risk(self):
        return (self.alpha / (self.S * n_obs + n_obs)) * np.ones(self.S * n_obs + n_obs)

    def initial_guess(self, results_dir='results'):
        Zp = np.zeros(self.nvar)
        Zp[:(n_u * self.S)] = self.convert_us_mat_to_us_jaxvec(self.initial_guess_us_mat(results_dir).flatten())
        Zp[(n_u * self.S):] = self.initial_guess_alphas_risk()
        return Zp

    # ---- the kernels -----------------------------------------------------------------------------------------------------
    def _handle(self):
        if self._lib_handle is None:
            import torch
            self._lib_handle = _lib.load()
            self._params = gauss_params(self.S)
            self.device = torch.device(self.device)
        return self._lib_handle

    def _dev(self, a, width, name):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))
        t = t.to(device=self.device, dtype=torch.float64).contiguous()
        if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
            raise ValueError(f"{name} must be (K >= 1, {width}), got {tuple(t.shape)}")
        return t

    def linearize_device(self, Z_batch, want_trajectory=False):
        """K problems in ONE call (rato_drone_gaussian_linearize).  Z_batch (K, nvar), host array or device tensor -> dict of
        fp64 DEVICE tensors: g_nl (K, n_nl), jac_nl (K, n_nl, nvar), and with ``want_trajectory`` mus (K, S+1, 6),
        Sigmas (K, S+1, 6, 6)."""
        import torch
        lib = self._handle()
        Z = self._dev(Z_batch, self.nvar, "Z_batch")
        K, S = Z.shape[0], self.S
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
        out = {"g_nl": new(K, self.n_nl), "jac_nl": new(K, self.n_nl, self.nvar)}
        mus = new(K, S + 1, n_x) if want_trajectory else None
        Sigmas = new(K, S + 1, n_x, n_x) if want_trajectory else None
        _lib.check(lib.rato_drone_gaussian_linearize(C.byref(self._params), K, _lib.ptr(Z), _lib.ptr(mus), _lib.ptr(Sigmas),
                                                     _lib.ptr(out["g_nl"]), _lib.ptr(out["jac_nl"]), _lib.current_stream()),
                   "rato_drone_gaussian_linearize")
        if want_trajectory:
            out["mus"], out["Sigmas"] = mus, Sigmas
        return out

    def hessian_device(self, Z_batch, lam_batch):
        """K Hessians of lam . g in ONE call (rato_drone_gaussian_hessian): Z_batch (K, nvar), lam_batch (K, n_nl) -> fp64
        DEVICE tensor (K, nvar (nvar + 1) / 2) in np.tril_indices(nvar) order."""
        import torch
        lib = self._handle()
        Z, lam = self._dev(Z_batch, self.nvar, "Z_batch"), self._dev(lam_batch, self.n_nl, "lam_batch")
        K = Z.shape[0]
        if lam.shape[0] != K:
            raise ValueError(f"Z_batch and lam_batch must hold the same K problems, got {K} and {lam.shape[0]}")
        hess = torch.empty((K, self.nvar * (self.nvar + 1) // 2), dtype=torch.float64, device=self.device)
        nbytes = int(lib.rato_drone_gaussian_hessian_workspace_bytes(self.S, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device) if nbytes else None
        _lib.check(lib.rato_drone_gaussian_hessian(C.byref(self._params), K, _lib.ptr(Z), _lib.ptr(lam), _lib.ptr(hess),
                                                   _lib.ptr(ws), nbytes, _lib.current_stream()),
                   "rato_drone_gaussian_hessian")
        return hess

    def device_callbacks(self):
        """the model callbacks ``ipopt_callbacks`` / ``scp.run_drone_gaussian`` run on: linearize(Z) -> (g_nl, jac_nl),
        hessian(Z, lam) -> tril, trajectory(Z) -> (xs, Sigmas), each one launch and one copy back"""
        def linearize(Z):
            r = self.linearize_device(np.asarray(Z)[None])
            return r["g_nl"][0].cpu().numpy(), r["jac_nl"][0].cpu().numpy()

        def hessian(Z, lam):
            return self.hessian_device(np.asarray(Z)[None], np.asarray(lam)[None])[0].cpu().numpy()

        def trajectory(Z):
            r = self.linearize_device(np.asarray(Z)[None], want_trajectory=True)
            return r["mus"][0].cpu().numpy(), r["Sigmas"][0].cpu().numpy()
        return dict(linearize=linearize, hessian=hessian, trajectory=trajectory)

    # ---- mean, covariance, constraints (:161-382) ----------------------------------------------------------------------------
    def _z_of(self, us_mat):
        return np.concatenate([self.convert_us_mat_to_us_jaxvec(us_mat), self.initial_guess_alphas_risk()])

    def us_to_state_trajectory(self, us_mat):
        return self.device_callbacks()["trajectory"](self._z_of(us_mat))[0]

    def us_to_covariance_trajectory(self, us_mat):
        return self.device_callbacks()["trajectory"](self._z_of(us_mat))[1]

    def get_control_and_risk_constraints(self, Z):
        """(:323-349) -> gs, gs_l, gs_u: the controls, the allocations and their sum (host: linear in Z)"""
        S = self.S
        us_vec, alphas_risk = self.convert_z_to_variables(Z)
        n = n_u * S + S * n_obs + n_obs + 1
        gs, gs_l, gs_u = np.zeros(n), np.zeros(n), np.zeros(n)
        gs[:(S * n_u)], gs_l[:(S * n_u)], gs_u[:(S * n_u)] = us_vec, self.u_min, self.u_max
        gs[(S * n_u):-1], gs_l[(S * n_u):-1], gs_u[(S * n_u):-1] = alphas_risk, ALPHA_MIN, self.alpha
        gs[-1], gs_l[-1], gs_u[-1] = np.sum(alphas_risk), 0.0, self.alpha
        return gs, gs_l, gs_u

    def get_all_state_constraints(self, Z, linearize=None):
        """(:351-382) -> g_final (6,), g_obs (n_obs S + 4 (S+1),): the non-linear rows, one launch"""
        g_nl = (linearize or self.device_callbacks()["linearize"])(Z)[0]
        return g_nl[:6], g_nl[6:]

    def f(self, Z):
        us = self.convert_us_vec_to_us_mat(self.convert_z_to_variables(Z)[0])
        return float(np.sum(2 * self.dt * np.diag(P.R)[None, :] * us ** 2))

    def g_bounds(self):
        """gL_gU (:423-444): equalities on the 6 final rows, one-sided (-1e15) obstacle and bound rows, two-sided linear rows"""
        _, gs_l, gs_u = self.get_control_and_risk_constraints(np.zeros(self.nvar))
        g_L, g_U = np.zeros(self.ncon), np.zeros(self.ncon)
        g_L[6:] = -1e15
        g_L[self.n_nl:], g_U[self.n_nl:] = gs_l, gs_u
        return g_L, g_U

    def solve(self, Z0=None, tol=1e-8, max_iter=3000, backend='device', results_dir='results', driver='host',
              chol='workgroup'):
        """the NLP by ``drone_gaussian_ipm.solve_batch`` (a batch of one) from ``Z0`` (default: the script's start,
        ``initial_guess(results_dir)``) -> (Z, info).  ``driver``: 'host', 'device' or 'device_grid', ``chol``: 'workgroup' or 'grid' (``solve_batch``'s)"""
        from . import drone_gaussian_ipm
        (Z, info), = drone_gaussian_ipm.solve_batch([self], None if Z0 is None else [Z0], tol=tol, max_iter=max_iter,
                                                    backend=backend, results_dir=results_dir, driver=driver, chol=chol)
        return Z, info

    # ---- the script's IPOPT callbacks (:409-498) -----------------------------------------------------------------------------
    def ipopt_callbacks(self, host=None):
        """-> dict(eval_f, eval_grad_f, eval_g, eval_jac_g, eval_h, g_L, g_U, x_L, x_U, eval_jac_g_sparsity_indices,
        eval_h_sparsity_indices, nvar, ncon): the arguments of the script's ``ipyopt.Problem(...)`` call (:503-518), same
        signatures (the callbacks write into ``out``), dense row-major Jacobian, tril Hessian obj_factor hess_f + hess(lam . g).
        ``host``: a dict(linearize, hessian) to run on instead of the device (tests).  The constant rows of the Jacobian and
        the objective's Hessian are filled once; eval_g and eval_jac_g at the same x share one launch (cached on x's bytes)."""
        impl = host if host is not None else self.device_callbacks()
        S, nvar, n_nl, ncon = self.S, self.nvar, self.n_nl, self.ncon
        D = n_u * S
        jac = np.zeros((ncon, nvar))
        jac[n_nl + np.arange(nvar), np.arange(nvar)] = 1.0       # gs = Z
        jac[-1, D:] = 1.0                                        # the allocation sum
        curv = np.zeros(nvar)
        curv[:D] = np.tile(4 * self.dt * np.diag(P.R), S)        # f = sum 2 dt R_ii u^2
        rows, cols = np.tril_indices(nvar)
        hess_f = np.where(rows == cols, curv[rows], 0.0)
        cache = {}

        def lin(x):
            key = np.asarray(x, dtype=np.float64).tobytes()
            if cache.get("key") != key:
                cache["key"], cache["val"] = key, impl["linearize"](np.asarray(x, dtype=np.float64))
            return cache["val"]

        def eval_f(x):
            return self.f(x)

        def eval_grad_f(x, out):
            out[:] = curv * np.asarray(x)
            return out

        def eval_g(x, out):
            x = np.asarray(x)
            out[:n_nl] = lin(x)[0]
            out[n_nl:-1] = x
            out[-1] = np.sum(x[D:])
            return out

        def eval_jac_g(x, out):
            jac[:n_nl] = lin(x)[1]
            out[:] = jac.reshape(-1)
            return out

        def eval_h(x, lagrange, obj_factor, out):
            out[:] = obj_factor * hess_f + impl["hessian"](np.asarray(x, dtype=np.float64),
                                                           np.asarray(lagrange, dtype=np.float64)[:n_nl])
            return out

        g_L, g_U = self.g_bounds()
        i1, i2 = np.indices((ncon, nvar))
        return dict(eval_f=eval_f, eval_grad_f=eval_grad_f, eval_g=eval_g, eval_jac_g=eval_jac_g, eval_h=eval_h, g_L=g_L,
                    g_U=g_U, x_L=-np.ones(nvar) * 1000.0, x_U=np.ones(nvar) * 1000.0,
                    eval_jac_g_sparsity_indices=(i1.flatten(), i2.flatten()),
                    eval_h_sparsity_indices=(rows.flatten(), cols.flatten()), nvar=nvar, ncon=ncon)
