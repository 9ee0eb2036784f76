"""Hopper uncertain-friction NLP -- the reference's ``class Model`` (hopper/hopper.py:90-453) and the callbacks its solve block
hands to IPOPT (:486-640) on the MI355X.

  * The sample-dependent part (:68-81, :300-367, :901-958): the slip rows, their Jacobian and Hessian slices and the Monte-Carlo
    check, fp32 over the sample axis (csrc/hopper.hip).
  * The rest of the NLP (:239-298, :369-453): the RK4 defect of the 8-state leg, the no-slip and end-effector rows, their
    derivatives and the Hessian of lam . g as one 12 x 12 block per step, fp64, for K problems per call
    (rato_hopper_nlp_linearize / rato_hopper_nlp_hessian, csrc/hopper_nlp.hip); rato_scatter_f64 places the local blocks
    into the CSC values of the Jacobian and into the tril-packed Hessian.  The kernels are phase-agnostic: the contact /
    flight masks, the constant unit coefficients and the script's row order live here.
  * ``Model(..., precision='f64')``: the sample-dependent part at the precision of the rest, from Z on the device for K problems
    per call (rato_hopper_slip_f64 / rato_hopper_slip_hess_blocks_f64, csrc/hopper_slip64.hip); 'f32' stays the default and
    the Monte-Carlo / large-M path.  ``fields=`` of ``slip_device_f64`` / ``nlp_device`` gives every problem of a call friction
    fields of its own (rato_hopper_slip_f64_fields; ``stack_fields_f64``): a grid of alphas x resampled terrains is one batch.
  * ``Model.eval_batch_device``: the script's Monte-Carlo block (:960-1007) for K solutions on the model's fields in one call
    (rato_hopper_eval_batch, csrc/hopper.hip): Z, the contact that slips and the risk record of every solution.
  * The evaluation of the NLP at Z on the device is a sequence of stages, each written once here and read by everyone -- the
    callbacks below, ``nlp_device`` and the two device backends of ``hopper_ipm`` / ``hopper_arrow``: the one params struct
    (``_slip_params``), ``_device_rows`` (host array or device tensor in), ``nlp_linearize_device``, ``det_jacobian_values``,
    ``slip_device_f64`` / ``_slip_f64``, ``hess_blocks_device`` (fold, slip share, Hessian), ``hess_tril_device`` (the only owner
    of the O(nvar^2) tril template), ``g_values_device`` and on the host ``assemble_g`` / ``_risk_rows`` / ``objective_blocks``.
  * ``Model.ipopt_callbacks()``: eval_f, eval_grad_f, eval_g, eval_jac_g, eval_h with the script's signatures, and its bounds.
  * ``Model.initial_guess()`` and ``Model.solve()``: the script's start and its solve (:136-164, :642-669) with the batched
    interior-point method of ``ipm`` on the backends of ``hopper_ipm`` (Newton step: csrc/hopper_ipm.hip, csrc/chol.hip) in
    IPOPT's place.  ``solve(driver='device')`` keeps the iterate on the device: the objective as ``curv`` / ``lin``,
    g assembled by rato_hopper_g_f64 and W x by rato_hopper_block_symv_f64 (csrc/hopper_g.hip), the multipliers folded where
    they lie (``fold_multipliers_device``)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, stats

# hopper.py:44-69
MAX_HOST_CONTACTS = 128   # RATO_HOPPER_MAX_HOST_CONTACTS (include/rato_saa.h)
S = 30
M = 30
T = 2.0
n_x = 8
n_u = 4
mu_nom = 0.10
num_mu_features = 30
# hopper.py:60-66, :83-89
u_max = 1000.0
mass_body, mass_leg = 3.0, 0.3
inertia_body, inertia_leg = 0.75, 0.075
gravity = 9.81
max_contact_force = 1000.0
state_initial = np.array([1e-6, 1.0, -1e-6, 1.0, 0., 0., 0., 0.]) + 2e-7
state_final = np.array([0.15, 1., -1e-6, 1., 0., 0., 0., 0.]) + 2e-7
n_l = n_x + n_u                      # local variables (x_t, u_t) of a step block
n_pairs = n_l * (n_l + 1) // 2       # 78: the lower triangle of a block in np.tril_indices(12) order


def phase_times(S):
    """time_jump, time_land (hopper.py:48-49: 10, 20 at S=30)."""
    return S // 3, (2 * S) // 3


def sample_friction_fields(M, rng=None):
    """hopper.py:70-74 / :975-979, same draw order on the global stream."""
    rng = np.random if rng is None else rng
    intensities = rng.uniform(0, 1, (M, num_mu_features))
    intensities = np.sqrt(2 / num_mu_features) * intensities
    intensities = 0.025 * intensities
    thetas = rng.uniform(0, np.pi, (M, num_mu_features))
    taus = rng.uniform(0, 2 * np.pi, (M, num_mu_features))
    return intensities, thetas, taus


def sample_friction_fields_device(M, seed=1, device='cuda:0'):
    """Synthetic fields (hopper.py:70-74 distributions) drawn in HBM by the library's Philox sampler
    (rato_hopper_sample), kernel layout [30][M] (fp32)."""
    lib = _lib.load()
    dev = torch.device(device)
    a, th, tau = (torch.empty((num_mu_features, M), dtype=torch.float32, device=dev) for _ in range(3))
    with torch.cuda.device(dev):
        _lib.check(lib.rato_hopper_sample(M, int(seed), _lib.ptr(a), _lib.ptr(th), _lib.ptr(tau),
                                          _lib.current_stream()), "rato_hopper_sample")
    return a, th, tau


# ---- the deterministic NLP rows: device-level calls (include/rato_saa.h, csrc/hopper_nlp.hip) ---------------------------------
def nlp_params(S, time_jump=None, time_land=None, dt=None):
    """rato_hopper_nlp_params from the script's constants (:44-89)"""
    tj, tl = phase_times(S)
    p = _lib.HopperNlpParams()
    p.S, p.reserved = int(S), 0
    p.time_jump, p.time_land = int(tj if time_jump is None else time_jump), int(tl if time_land is None else time_land)
    p.dt = float(T / S if dt is None else dt)
    p.mass_body, p.mass_leg, p.inertia_body, p.inertia_leg = mass_body, mass_leg, inertia_body, inertia_leg
    p.gravity = gravity
    for i in range(n_x):
        p.state_initial[i], p.state_final[i] = float(state_initial[i]), float(state_final[i])
    return p


def _rows_of(Z, nmin):
    """(K, ldz) of a device fp64 tensor [K][ldz] whose rows are contiguous"""
    if Z.dim() != 2 or Z.dtype != torch.float64 or not Z.is_cuda or Z.stride(1) != 1 or Z.shape[1] < nmin or Z.shape[0] < 1:
        raise ValueError(f"Z must be a device float64 tensor (K >= 1, >= {nmin}) with contiguous rows, got {tuple(Z.shape)}")
    return Z.shape[0], (Z.stride(0) if Z.shape[0] > 1 else max(Z.stride(0), Z.shape[1]))


def nlp_linearize_device(params, Z, want=("defect", "d_defect", "rows", "d_rows")):
    """rato_hopper_nlp_linearize on a device tensor Z [K][ldz] (a row-strided view is fine) -> dict of the fp64 device tensors
    named in ``want``: defect (K, S, 8), d_defect (K, S, 8, 12), rows (K, S+1, 2), d_rows (K, S+1, 2, 4)"""
    S = params.S
    K, ldz = _rows_of(Z, n_x * (S + 1) + n_u * S)
    shapes = {"defect": (K, S, n_x), "d_defect": (K, S, n_x, n_l), "rows": (K, S + 1, 2), "d_rows": (K, S + 1, 2, 4)}
    out = {k: torch.empty(shapes[k], dtype=torch.float64, device=Z.device) for k in want}
    with torch.cuda.device(Z.device):
        _lib.check(_lib.load().rato_hopper_nlp_linearize(
            C.byref(params), K, _lib.ptr(Z), ldz, *(_lib.ptr(out.get(k)) for k in ("defect", "d_defect", "rows", "d_rows")),
            _lib.current_stream()), "rato_hopper_nlp_linearize")
    return out


def nlp_hessian_device(params, Z, lam_dyn, lam_rows, add=None):
    """rato_hopper_nlp_hessian: Z [K][ldz], lam_dyn (K, S, 8), lam_rows (K, S+1, 2), add (K, S+1, 78) or None, all device fp64
    -> hess_blocks (K, S+1, 78)"""
    S = params.S
    K, ldz = _rows_of(Z, n_x * (S + 1) + n_u * S)
    for t, shape, name in ((lam_dyn, (K, S, n_x), "lam_dyn"), (lam_rows, (K, S + 1, 2), "lam_rows"), (add, (K, S + 1, n_pairs), "add")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != Z.device):
            raise ValueError(f"{name} must be a contiguous device float64 tensor of shape {shape}")
    out = torch.empty((K, S + 1, n_pairs), dtype=torch.float64, device=Z.device)
    with torch.cuda.device(Z.device):
        _lib.check(_lib.load().rato_hopper_nlp_hessian(
            C.byref(params), K, _lib.ptr(Z), ldz, _lib.ptr(lam_dyn), _lib.ptr(lam_rows), _lib.ptr(add), _lib.ptr(out),
            _lib.current_stream()), "rato_hopper_nlp_hessian")
    return out


def scatter_f64(src, index_map, dst, scale=None):
    """rato_scatter_f64: dst[k][map[i]] = scale[i] src[k][i]; src (K, n), dst (K, n_dst) device fp64, map (n,) device int64
    (entries outside [0, n_dst) are not emitted), scale (n,) device fp64 or None"""
    K, n = src.shape
    if dst.shape[0] != K or index_map.shape != (n,) or index_map.dtype != torch.int64 or src.dtype != torch.float64 or \
            dst.dtype != torch.float64 or not (src.is_contiguous() and dst.is_contiguous() and index_map.is_contiguous()):
        raise ValueError("scatter_f64: src (K, n) and dst (K, n_dst) float64, map (n,) int64, all contiguous")
    if scale is not None and (scale.shape != (n,) or scale.dtype != torch.float64 or not scale.is_contiguous()):
        raise ValueError("scatter_f64: scale must be (n,) float64")
    with torch.cuda.device(src.device):
        _lib.check(_lib.load().rato_scatter_f64(K, n, _lib.ptr(src), n, _lib.ptr(index_map), _lib.ptr(scale), _lib.ptr(dst),
                                                dst.shape[1], dst.shape[1], _lib.current_stream()), "rato_scatter_f64")
    return dst


def g_device(params, M, saa, Z, defect, rows, h, h_strides, malpha, out=None):
    """rato_hopper_g_f64 (csrc/hopper_g.hip): g (K, ncon) in the script's row order from device fp64 tensors -- Z (K, ldz >= nvar),
    defect (K, S, 8) and rows (K, S+1, 2) of ``nlp_linearize_device``, the slip values ``h`` of K x M x C entries (None when no
    step is in contact) read with ``h_strides`` = (sample, contact): (C, 1) for slip_rows, (1, M) for slip_h -- and malpha (K,)
    = M alpha per problem (saa only).  ``out``: a (K, ldg >= ncon) tensor to write into; its padding is left as it is."""
    S = params.S
    Cn = params.time_jump + (S - params.time_land)
    n_state = params.time_jump + (S + 1 - params.time_land)
    ncon = n_x * S + n_x + 2 + 2 * n_state + (params.time_land - params.time_jump) + \
        ((1 + M + M * Cn + 1) if saa else M * Cn) + n_u * S + 1 + 3 * S
    K, ldz = _rows_of(Z, n_x * (S + 1) + n_u * S + M + 2)
    for t, shape, name in ((defect, (K, S, n_x), "defect"), (rows, (K, S + 1, 2), "rows")):
        if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != Z.device:
            raise ValueError(f"{name} must be a contiguous device float64 tensor of shape {shape}")
    if Cn > 0 and (h is None or h.numel() != K * M * Cn or h.dtype != torch.float64 or not h.is_contiguous() or h.device != Z.device):
        raise ValueError(f"h must be a contiguous device float64 tensor of K M C = {K * M * Cn} entries")
    if saa and (malpha is None or tuple(malpha.shape) != (K,) or malpha.dtype != torch.float64 or malpha.device != Z.device):
        raise ValueError(f"malpha must be a device float64 tensor ({K},)")
    g = torch.empty((K, ncon), dtype=torch.float64, device=Z.device) if out is None else out
    if g.dim() != 2 or g.shape[0] != K or g.shape[1] < ncon or g.dtype != torch.float64 or not g.is_contiguous() or g.device != Z.device:
        raise ValueError(f"out must be a contiguous device float64 tensor ({K}, >= {ncon})")
    with torch.cuda.device(Z.device):
        _lib.check(_lib.load().rato_hopper_g_f64(
            C.byref(params), K, M, int(bool(saa)), _lib.ptr(Z), ldz, _lib.ptr(defect), _lib.ptr(rows), _lib.ptr(h if Cn > 0 else None),
            int(h_strides[0]), int(h_strides[1]), _lib.ptr(malpha if saa else None), _lib.ptr(g), g.shape[1],
            _lib.current_stream()), "rato_hopper_g_f64")
    return g


def block_symv(S, blocks, x, n=None, out=None):
    """rato_hopper_block_symv_f64 (csrc/hopper_g.hip): W x for W given as its step blocks (K, S+1, 78); x (K, ldx >= n) device
    fp64 -> (K, n) (``out``: a (K, ldo >= n) tensor to write into); the entries behind the blocks' variables are +0"""
    K = blocks.shape[0]
    n = x.shape[1] if n is None else int(n)
    if tuple(blocks.shape) != (K, S + 1, n_pairs) or blocks.dtype != torch.float64 or not blocks.is_contiguous() or \
            x.dim() != 2 or x.shape[0] != K or x.shape[1] < n or x.dtype != torch.float64 or not x.is_contiguous() or x.device != blocks.device:
        raise ValueError(f"blocks must be a contiguous device float64 tensor (K, {S + 1}, {n_pairs}) and x (K, >= {n})")
    o = torch.empty((K, n), dtype=torch.float64, device=x.device) if out is None else out
    if o.dim() != 2 or o.shape[0] != K or o.shape[1] < n or o.dtype != torch.float64 or not o.is_contiguous() or o.device != x.device:
        raise ValueError(f"out must be a contiguous device float64 tensor ({K}, >= {n})")
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().rato_hopper_block_symv_f64(K, S, n, _lib.ptr(blocks), _lib.ptr(x), x.shape[1], _lib.ptr(o), o.shape[1],
                                                          _lib.current_stream()), "rato_hopper_block_symv_f64")
    return o


def stack_fields_f64(models):
    """The friction fields of K models of one M on one device as what ``fields=`` of ``Model.slip_device_f64`` / ``nlp_device``
    takes: (a, theta, tau), each a contiguous fp64 device tensor (K, 30, M) whose row k is ``models[k].fields_f64()`` (so models
    built with fields='device' / ``from_device`` take part, upcast once).  K x 3 x 30 x M x 8 bytes of device memory."""
    models = list(models)
    if not models:
        raise ValueError("stack_fields_f64 needs at least one model")
    triples = [m.fields_f64() for m in models]
    shape, dev = (num_mu_features, models[0].M), triples[0][0].device
    if any(tuple(t.shape) != shape or t.device != dev for f in triples for t in f):
        raise ValueError(f"the models' fields must all be {shape} on one device")
    return tuple(torch.stack([f[j] for f in triples]).contiguous() for j in range(3))


def _check_fields(fields, K, M, device):
    """``fields`` = (a, theta, tau) per problem -> ldf = 30 M, or a ValueError before anything is launched"""
    shape = (K, num_mu_features, M)
    if not isinstance(fields, (tuple, list)) or len(fields) != 3:
        raise ValueError("fields must be (a, theta, tau)")
    for t, name in zip(fields, ("a", "theta", "tau")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous() or \
                t.device.type != device.type or (device.index is not None and t.device.index != device.index):
            raise ValueError(f"fields: {name} must be a contiguous float64 tensor {shape} on {device}, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    return num_mu_features * M


def block_variables(S, t):
    """indices in z of the local variables (x_t (8), u_t (4)) of step block t; the u part of block S does not exist (-1)"""
    u = n_x * (S + 1) + n_u * t + np.arange(n_u) if t < S else -np.ones(n_u, dtype=np.int64)
    return np.concatenate([n_x * t + np.arange(n_x), u]).astype(np.int64)


def objective_blocks(S, factor, out=None):
    """factor hess_f as step blocks (S+1, 78): 2 R on u0 and u1 of every step, R = 1 (:443-448); added into ``out`` when given"""
    add = np.zeros((S + 1, n_pairs)) if out is None else out
    tr, tc = np.tril_indices(n_l)
    add[:S, np.flatnonzero((tr == tc) & ((tr == n_x) | (tr == n_x + 1)))] += 2.0 * float(factor)
    return add


class Model:
    def __init__(self, M, method='baseline', alpha=0.1, S=S, fields=None, device='cuda:0', rng=None,
                 verbose=False, phases=None, precision='f32'):
        """precision: 'f32' -- the risk group (the slip rows, their Jacobian and Hessian share) from the fp32 throughput kernel
        (csrc/hopper.hip), gathered on the host one problem per call; 'f64' -- from the fp64 kernels of csrc/hopper_slip64.hip,
        computed from Z on the device for K problems per call, like every other row of the NLP."""
        # hopper.py:91-104
        if precision not in ('f32', 'f64'):
            raise ValueError(f"precision must be 'f32' or 'f64', got {precision!r}")
        self.precision = precision
        if verbose:
            print("Initializing Model with")
            print("> method =", method)
            print("> alpha  =", alpha)
        self.method, self.alpha, self.S, self.M = method, alpha, S, M
        self.time_jump, self.time_land = phase_times(S) if phases is None else (int(phases[0]), int(phases[1]))
        self.dt = T / S
        self.device = torch.device(device)
        self._lib = _lib.load()
        self.num_vars = (S + 1) * n_x + S * n_u + M + 2
        if fields is None:
            fields = sample_friction_fields(M, rng)
        if fields != 'device':
            z = 0.0 if method == 'baseline' else 1.0
            self.intensities, self.thetas, self.taus = (z * np.asarray(f, dtype=np.float64) for f in fields)
            self._a, self._th, self._tau = (
                torch.as_tensor(f, device=self.device).t().contiguous().float()
                for f in (self.intensities, self.thetas, self.taus))
            if precision == 'f64':
                self._fields64 = tuple(torch.as_tensor(np.ascontiguousarray(f.T), device=self.device)
                                       for f in (self.intensities, self.thetas, self.taus))

    @classmethod
    def from_device(cls, a, theta, tau, method='saa', alpha=0.1, S=S, precision='f32'):
        self = cls(a.shape[1], method, alpha, S=S, fields='device', device=a.device, precision=precision)
        self._a, self._th, self._tau = (_lib.require_f32_device(t, n) for t, n in
                                        ((a, "a"), (theta, "theta"), (tau, "tau")))
        return self

    def fields_f64(self):
        """the friction fields [30][M] as fp64 device tensors: from the host fp64 arrays, or upcast once from the fp32 device
        arrays (from_device / fields='device')"""
        f = getattr(self, "_fields64", None)
        if f is None:
            f = self._fields64 = tuple(_lib.require_f32_device(t, n).double() for t, n in
                                       ((self._a, "a"), (self._th, "theta"), (self._tau, "tau")))
        return f

    # ---- variable layout (hopper.py:105-132) -------------------------------
    def convert_z_to_variables(self, z):
        nx, nu = (self.S + 1) * n_x, self.S * n_u
        return z[:nx], z[nx:nx + nu], z[nx + nu:-2], z[-2], z[-1]

    def convert_z_to_xs_us_mats(self, z):
        xs_vec, us_vec, _, _, _ = self.convert_z_to_variables(np.asarray(z))
        return (np.reshape(xs_vec, (n_x, self.S + 1), 'F').T.copy(),
                np.reshape(us_vec, (n_u, self.S), 'F').T.copy())

    def end_effector_position(self, x):
        x = np.asarray(x)
        return np.stack([x[..., 0] + x[..., 3] * np.sin(x[..., 2]),
                         x[..., 1] - x[..., 3] * np.cos(x[..., 2])], axis=-1)

    def end_effector_x_derivatives(self, x):
        """Chain-rule factors of the (sample-independent) map state -> end-effector x position p = x0 + x3 sin x2
        (hopper.py:166-171) that carry dh/dpx and d2h/dpx2 to the NLP variables (x0, x2, x3) in jac_g / the
        Hessian (hopper.py:569,577-580):  -> (J (...,3) = dp/d(x0,x2,x3),  H (...,3,3) = d2p/d(x0,x2,x3)^2)."""
        x = np.asarray(x, dtype=np.float64)
        s, c = np.sin(x[..., 2]), np.cos(x[..., 2])
        J = np.stack([np.ones_like(s), x[..., 3] * c, s], axis=-1)
        H = np.zeros(x.shape[:-1] + (3, 3))
        H[..., 1, 1] = -x[..., 3] * s
        H[..., 1, 2] = H[..., 2, 1] = c
        return J, H

    def contact_chain(self, Z):
        """The factors above at the contact steps of ``contact_inputs(Z)``: J (C,3), H (C,3,3).  With the device
        outputs:  dh_ic/d(x0,x2,x3)_c = dh_dpx[i,c] J[c];  sum_i lam_ic d2h_ic/d(.)2 = D2[c] J[c] J[c]' + (sum_i lam_ic
        dh_dpx[i,c]) H[c];  mixed with fz: D1[c] J[c]."""
        xs_mat, _ = self.convert_z_to_xs_us_mats(Z)
        xc = np.concatenate([xs_mat[:self.time_jump], xs_mat[self.time_land:-1]])
        return self.end_effector_x_derivatives(xc)

    def contact_inputs(self, Z):
        """Contact-phase mask of hopper.py:305-311 -> (px (C,), forces (C,2))."""
        xs_mat, us_mat = self.convert_z_to_xs_us_mats(Z)
        ee_x = self.end_effector_position(xs_mat)[:, 0]
        px = np.concatenate([ee_x[:self.time_jump], ee_x[self.time_land:-1]])
        forces = np.concatenate([us_mat[:self.time_jump, 2:], us_mat[self.time_land:, 2:]])
        return px, forces

    # ---- device path (K5) --------------------------------------------------
    def slip_device(self, px, forces, lam=None, want_Z=True, want_h=True, want_deriv=False, reduce=True, staged=None):
        """lam: [C][M] multipliers or None.
        -> dict of device tensors: Z [M], h/dh_dfz/dh_dpx [C][M], hess [C][2] (float64).
        reduce=False: the per-workgroup partial sums of the lambda-weighted second derivatives come back as "part"
        (hess=None) for a caller that folds their second stage into the statistics launch
        (stats.sums_and_risk_stats_device).
        px / forces change with every NLP iterate and come from the host.  staged=False: they travel in the kernel's
        argument block (rato_hopper_slip_host_inputs: no staging buffer, no upload in front of the kernel);
        staged=True: one pinned staging buffer + one asynchronous upload into a device buffer the kernel reads
        (rato_hopper_slip).  Default: by value, except inside a hipGraph capture (where by-value inputs would be frozen
        into the graph) and for more than 128 contacts."""
        px = np.ascontiguousarray(px, dtype=np.float32)
        forces = np.asarray(forces, dtype=np.float32)
        Cn, M = px.shape[0], self._a.shape[1]
        dev = self.device
        capturing = torch.cuda.is_current_stream_capturing()
        if staged is None:
            staged = capturing
        if Cn > MAX_HOST_CONTACTS:
            staged = True
        if not staged:
            fx = np.ascontiguousarray(forces[:, 0])
            fz = np.ascontiguousarray(forces[:, 1])
            hp = lambda x: C.c_void_p(x.ctypes.data)
            entry, pxd, fxd, fzd = self._lib.rato_hopper_slip_host_inputs, hp(px), hp(fx), hp(fz)
        else:
            # ONE pinned staging buffer and one asynchronous upload (three pageable copies cost ~40 us, more than the
            # kernel at M = 5e4)
            st = getattr(self, "_stage", None)
            if st is None or st[0].shape[1] != Cn:
                if capturing:
                    raise RuntimeError("hopper.slip_device: the pinned staging buffer cannot be allocated inside a "
                                       "hipGraph capture; call slip_device(..., staged=True) once before capturing")
                st = (torch.empty((3, Cn), dtype=torch.float32).pin_memory(),
                      torch.empty((3, Cn), dtype=torch.float32, device=dev))
                self._stage = st
            host, devbuf = st
            self._stage_event = getattr(self, "_stage_event", None)
            if self._stage_event is not None and not capturing:   # inside a capture: no host-side waits
                self._stage_event.synchronize()      # the previous upload has left the pinned buffer
            host[0].copy_(torch.from_numpy(px))
            host[1].copy_(torch.from_numpy(np.ascontiguousarray(forces[:, 0])))
            host[2].copy_(torch.from_numpy(np.ascontiguousarray(forces[:, 1])))
            devbuf.copy_(host, non_blocking=True)
            if not capturing:
                if self._stage_event is None:
                    self._stage_event = torch.cuda.Event()
                self._stage_event.record()
            entry, pxd, fxd, fzd = self._lib.rato_hopper_slip, _lib.ptr(devbuf[0]), _lib.ptr(devbuf[1]), _lib.ptr(devbuf[2])
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        Z = e(M) if want_Z else None
        h = e(Cn, M) if want_h else None
        dfz = e(Cn, M) if want_deriv else None
        dpx = e(Cn, M) if want_deriv else None
        lamd = part = None
        if lam is not None:
            lamd = (lam if isinstance(lam, torch.Tensor) else torch.as_tensor(np.asarray(lam), device=dev))
            lamd = lamd.float().contiguous()
            if tuple(lamd.shape) != (Cn, M):
                raise ValueError(f"lam must be [C][M] = ({Cn},{M}), got {tuple(lamd.shape)}")
            part = e(self._lib.rato_hopper_nblocks(M), Cn, 2)
        _lib.check(entry(
            M, Cn, pxd, fxd, fzd, _lib.ptr(self._a), _lib.ptr(self._th),
            _lib.ptr(self._tau), _lib.ptr(lamd), _lib.ptr(Z), _lib.ptr(h), _lib.ptr(dfz), _lib.ptr(dpx),
            _lib.ptr(part), _lib.current_stream()), "rato_hopper_slip")
        hess = stats.sum_partials(part) if (part is not None and reduce) else None
        return {"Z": Z, "h": h, "dh_dfz": dfz, "dh_dpx": dpx, "hess": hess, "part": part}

    def slip_risk_constraints(self, Z):
        """hopper.py:300-367 -> gs (1 + M + M*C + 1,) ['saa'] or (M*C,) ['baseline']."""
        Z = np.asarray(Z, dtype=np.float64)
        return self._risk_rows(Z, self._slip_rows_host(Z))

    def _slip_rows_host(self, Z):
        """the slip values of one problem from a launch of their own, on the host in the risk rows' order i C + c"""
        if self.precision == 'f64':
            h = self.slip_device_f64(Z[None], want=("h",))["h"][0]                         # (C,M)
        else:
            h = self.slip_device(*self.contact_inputs(Z), want_Z=False)["h"].double()
        return np.ascontiguousarray(h.cpu().numpy().T).reshape(-1)

    def slip_partials(self, px, forces):
        """(h, dh/dfz, dh/dpx), each (M,C) — the sample-dependent slices of jac_g."""
        r = self.slip_device(px, forces, want_Z=False, want_deriv=True)
        return tuple(r[k].t().double().cpu().numpy() for k in ("h", "dh_dfz", "dh_dpx"))

    def slip_hessian_sums(self, px, forces, lam):
        """(D1 (C,), D2 (C,)): lambda-weighted d2h/(dpx dfz), d2h/dpx^2 summed over samples."""
        hess = self.slip_device(px, forces, lam=np.asarray(lam).T, want_Z=False, want_h=False,
                                want_deriv=True)["hess"].cpu().numpy()
        return hess[:, 0], hess[:, 1]

    # ---- the reference's own matrices (hopper.py:569, :575-580) ---------------
    def contact_steps(self):
        return np.concatenate([np.arange(0, self.time_jump), np.arange(self.time_land, self.S)])

    def _jacobian_pattern(self, Cn):
        """(indices, indptr) of ``jacrev(slip_risk_constraints)`` with EVERY structural entry present, in the value order
        of rato_hopper_emit_jacobian_values (include/rato_saa.h); built once per (M, C, method)."""
        key = (self._a.shape[1], Cn, self.method)
        pat = getattr(self, "_jac_pattern", None)
        if pat is not None and pat[0] == key:
            return pat[1], pat[2]
        M, S = key[0], self.S
        saa = self.method != 'baseline'
        nX, nU = (S + 1) * n_x, S * n_u
        steps = self.contact_steps()
        r0 = 1 + M if saa else 0
        rows_c = r0 + np.arange(M, dtype=np.int64)[None, :] * Cn + np.arange(Cn, dtype=np.int64)[:, None]     # (C, M)
        counts = np.zeros(self.num_vars, dtype=np.int64)
        for k in (0, 2, 3):
            counts[steps * n_x + k] = M
        counts[nX + steps * n_u + 2] = M
        counts[nX + steps * n_u + 3] = M
        parts = [np.repeat(rows_c[:, None, :], 3, axis=1).reshape(-1), np.repeat(rows_c[:, None, :], 2, axis=1).reshape(-1)]
        rows_i = r0 + np.arange(M, dtype=np.int64)[:, None] * Cn + np.arange(Cn, dtype=np.int64)[None, :]     # (M, C)
        if saa:
            ycols = np.concatenate([np.zeros((M, 1), dtype=np.int64), 1 + np.arange(M, dtype=np.int64)[:, None], rows_i], axis=1)
            parts.append(ycols.reshape(-1))
            counts[nX + nU:nX + nU + M] = 2 + Cn
        parts.append(rows_i.reshape(-1))
        counts[self.num_vars - 2] = M * Cn
        if saa:
            parts.append(np.concatenate([[0], rows_i.reshape(-1)]))
            counts[self.num_vars - 1] = 1 + M * Cn
        indices = np.concatenate(parts).astype(np.int32)
        indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert indices.size == int(self._lib.rato_hopper_jacobian_nnz(M, Cn, int(saa))) == indptr[-1]
        self._jac_pattern = (key, indices, indptr)
        return indices, indptr

    def slip_jacobian_device(self, Z, out=None):
        """-> (values [nnz] fp32 device tensor, indices, indptr, shape): ``jacrev(slip_risk_constraints)(Z)`` of the
        reference (hopper.py:569 on the rows of :300-367), rows and columns in its order, as CSC with every structural entry
        present; the values are written on the device (rato_hopper_emit_jacobian_values) from the slip kernel's partials and
        the end-effector chain factors.  ``out``: the value tensor of an earlier call (its constant part is kept).
        precision='f64': the values are fp64, computed from Z on the device (rato_hopper_slip_f64) and placed by
        rato_scatter_f64; ``out`` is not used."""
        Z = np.asarray(Z, dtype=np.float64)
        if self.precision == 'f64':
            lay = self.nlp_layout()
            saa = self.method != 'baseline'
            indices, indptr = self._jacobian_pattern(lay["C"])
            n_rows = (1 + self.M + self.M * lay["C"] + 1) if saa else self.M * lay["C"]
            return self._slip_f64(Z[None])["slip_jac_values"][0], indices, indptr, (n_rows, self.num_vars)
        px, forces = self.contact_inputs(Z)
        Cn, M = px.shape[0], self._a.shape[1]
        r = self.slip_device(px, forces, want_Z=False, want_h=False, want_deriv=True)
        Jee, _ = self.contact_chain(Z)
        chain = np.ascontiguousarray(Jee, dtype=np.float32)
        saa = self.method != 'baseline'
        nnz = int(self._lib.rato_hopper_jacobian_nnz(M, Cn, int(saa)))
        fresh = out is None or out.numel() != nnz
        vals = torch.empty(nnz, dtype=torch.float32, device=self.device) if fresh else out
        chain_dev = None
        if Cn > MAX_HOST_CONTACTS:
            chain_dev = torch.as_tensor(chain, device=self.device)
        _lib.check(self._lib.rato_hopper_emit_jacobian_values(
            M, Cn, int(saa), float(self.alpha), _lib.ptr(r["dh_dfz"]), _lib.ptr(r["dh_dpx"]),
            C.c_void_p(chain.ctypes.data), _lib.ptr(chain_dev), int(fresh), _lib.ptr(vals), _lib.current_stream()),
            "rato_hopper_emit_jacobian_values")
        indices, indptr = self._jacobian_pattern(Cn)
        n_rows = (1 + M + M * Cn + 1) if saa else M * Cn
        return vals, indices, indptr, (n_rows, self.num_vars)

    def slip_jacobian(self, Z):
        """The same matrix as a scipy CSC (fp64 values, exact zeros dropped as the reference's ``csc_matrix(dense)`` drops
        them: the sparsity pattern is the reference's)."""
        import scipy.sparse as sp
        vals, indices, indptr, shape = self.slip_jacobian_device(Z)
        data = vals.double().cpu().numpy()
        if self.method != 'baseline':
            data[indptr[-2]] = self._a.shape[1] * self.alpha       # row 0 of the t_risk column: M alpha in fp64 (a constant)
        A = sp.csc_matrix((data, indices, indptr), shape=shape)
        A.eliminate_zeros()
        A.sort_indices()
        return A

    slip_jacobian_rows = slip_jacobian

    def slip_hessian(self, Z, lam):
        """``hessian(lambda . slip_risk_constraints)(Z)`` (hopper.py:575-580; ``lam`` (M, C): the multipliers of the
        per-sample rows -- every other row is linear) as a scipy CSC (num_vars x num_vars).  The three sample sums per contact
        come from ONE launch (rato_hopper_slip_hessian); the 15 entries per contact are placed on the host."""
        import scipy.sparse as sp
        Z = np.asarray(Z, dtype=np.float64)
        if self.precision == 'f64':
            ncon, r0 = self.risk_rows_offset()
            full = np.zeros(ncon)
            full[r0:r0 + np.size(lam)] = np.asarray(lam, dtype=np.float64).reshape(-1)
            return self._blocks_to_csc(self.slip_hessian_blocks(Z, full))
        px, forces = self.contact_inputs(Z)
        D = self.slip_hessian_sums3(px, forces, lam)
        Jee, Hee = self.contact_chain(Z)
        steps = self.contact_steps()
        nX = (self.S + 1) * n_x
        xi = steps[:, None] * n_x + np.array([0, 2, 3])[None, :]                                   # (C, 3)
        blk = D[:, 1, None, None] * Jee[:, :, None] * Jee[:, None, :] + D[:, 2, None, None] * Hee    # (C, 3, 3)
        mixed = D[:, 0, None] * Jee                                                                  # (C, 3)
        fz = (nX + steps * n_u + 3)[:, None]
        I = np.concatenate([np.repeat(xi, 3, axis=1).reshape(-1), xi.reshape(-1), np.repeat(fz, 3, axis=1).reshape(-1)])
        J = np.concatenate([np.tile(xi, (1, 3)).reshape(-1), np.repeat(fz, 3, axis=1).reshape(-1), xi.reshape(-1)])
        V = np.concatenate([blk.reshape(-1), mixed.reshape(-1), mixed.reshape(-1)])
        H = sp.coo_matrix((V, (I, J)), shape=(self.num_vars, self.num_vars)).tocsc()
        H.eliminate_zeros()
        H.sort_indices()
        return H

    def slip_hessian_sums3(self, px, forces, lam):
        """(C, 3): per contact the lambda-weighted sums over the samples of d2h/(dpx dfz), d2h/dpx^2 and dh/dpx."""
        px = np.ascontiguousarray(px, dtype=np.float32)
        forces = np.asarray(forces, dtype=np.float32)
        Cn, M = px.shape[0], self._a.shape[1]
        lamd = torch.as_tensor(np.ascontiguousarray(np.asarray(lam, dtype=np.float64).T), device=self.device).float().contiguous()
        if tuple(lamd.shape) != (Cn, M):
            raise ValueError(f"lam must be (M, C) = ({M},{Cn})")
        part = torch.empty((self._lib.rato_hopper_nblocks(M), Cn, 3), dtype=torch.float32, device=self.device)
        fx, fz = np.ascontiguousarray(forces[:, 0]), np.ascontiguousarray(forces[:, 1])
        if Cn <= MAX_HOST_CONTACTS:
            args, host = (C.c_void_p(px.ctypes.data), C.c_void_p(fx.ctypes.data), C.c_void_p(fz.ctypes.data)), 1
        else:
            dev = [torch.as_tensor(v, device=self.device) for v in (px, fx, fz)]
            args, host = tuple(_lib.ptr(v) for v in dev), 0
        _lib.check(self._lib.rato_hopper_slip_hessian(
            M, Cn, *args, host, _lib.ptr(self._a), _lib.ptr(self._th), _lib.ptr(self._tau), _lib.ptr(lamd), None, None,
            None, None, _lib.ptr(part), _lib.current_stream()), "rato_hopper_slip_hessian")
        return stats.sum_partials(part).cpu().numpy().reshape(Cn, 3)

    # ---- the fp64 path (precision='f64'): from Z on the device, K problems per call (csrc/hopper_slip64.hip) -----------------
    def risk_rows_offset(self):
        """(ncon, r0): the length of g and the index in g of the slip row of sample 0, contact 0 (row r0 + i C + c), by
        arithmetic alone (no layout is built: M may be large)"""
        S, M, tj, tl = self.S, self.M, self.time_jump, self.time_land
        saa = self.method != 'baseline'
        Cn, n_state = tj + (S - tl), tj + (S + 1 - tl)
        risk = n_x * S + n_x + 2 + 2 * n_state + (tl - tj)
        n_risk = (1 + M + M * Cn + 1) if saa else M * Cn
        return risk + n_risk + n_u * S + 1 + 3 * S, risk + (1 + M if saa else 0)

    def _slip_params(self):
        """the model's one rato_hopper_nlp_params struct: every device call of the model and of its backends reads this one"""
        p = getattr(self, "_slip_p", None)
        if p is None:
            p = self._slip_p = nlp_params(self.S, self.time_jump, self.time_land, self.dt)
        return p

    def _device_rows(self, a):
        """Z or the multipliers, a host array (one row or K) or a device tensor -> a device fp64 tensor (K, ld); a tensor is
        taken as it is"""
        if not isinstance(a, torch.Tensor):
            a = torch.as_tensor(np.ascontiguousarray(np.atleast_2d(np.asarray(a, dtype=np.float64))), device=self.device)
        return a

    def slip_device_f64(self, Zs, lams=None, want=("h", "dh_dfz", "dh_dx", "Zmax"), fields=None):
        """rato_hopper_slip_f64 for K problems.  Zs (K, >= 8(S+1) + 4S) host array or device fp64 tensor (rows may be strided);
        lams (K, ncon) multipliers of g (host array or device fp64 tensor, read in place at the risk rows) or None.
        -> dict of fp64 device tensors, those named in ``want``: h (K, C, M), dh_dfz (K, C, M), dh_dx (K, C, 3, M) = dh/d(x0, x2,
        x3) with the end-effector chain applied, Zmax (K, M); and D (K, C, 3) = (D1, D2, D0), the lambda-weighted sample sums of
        d2h/(dp dfz), d2h/dp2 and dh/dp (None without lams).  One launch, two with lams.
        ``fields`` = (a, theta, tau), each a contiguous fp64 device tensor (K, 30, M) on the model's device (``stack_fields_f64``):
        problem k reads its own friction fields (rato_hopper_slip_f64_fields) and the model's are not read; row k is bitwise the
        K = 1 call on a model that holds fields k.  None: the model's fields for all K problems.  Anything else is a ValueError
        before a launch."""
        S, M, dev = self.S, self.M, self.device
        if not 0 <= self.time_jump <= self.time_land <= S:
            raise ValueError(f"phase times must satisfy 0 <= time_jump <= time_land <= S, got {self.time_jump}, {self.time_land}")
        Zs = self._device_rows(Zs)
        if fields is not None:
            ldf = _check_fields(fields, Zs.shape[0], M, dev)
        K, ldz = _rows_of(Zs, n_x * (S + 1) + n_u * S)
        Cn = self.time_jump + (S - self.time_land)
        params = self._slip_params()
        shapes = {"h": (K, Cn, M), "dh_dfz": (K, Cn, M), "dh_dx": (K, Cn, 3, M), "Zmax": (K, M)}
        e = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        out = {k: e(*shapes[k]) for k in want}
        if Cn == 0 and "Zmax" in out:
            out["Zmax"].fill_(-np.inf)                            # the maximum over no contact; nothing is launched
        lamd = part = D = None
        ldlam = r0 = 0
        if lams is not None:
            ncon, r0 = self.risk_rows_offset()
            lamd = self._device_rows(lams)
            if tuple(lamd.shape) != (K, ncon) or lamd.dtype != torch.float64 or lamd.device != Zs.device or lamd.stride(1) != 1:
                raise ValueError(f"lams must be (K, ncon) = ({K}, {ncon}) float64 with contiguous rows, got {tuple(lamd.shape)}")
            ldlam = lamd.stride(0) if K > 1 else max(lamd.stride(0), ncon)
            part = e(self._lib.rato_hopper_slip_f64_nblocks(M), K, Cn, 3)
            D = e(K, Cn, 3)
        outs = [_lib.ptr(out.get(k)) for k in ("h", "dh_dfz", "dh_dx", "Zmax")] + [_lib.ptr(part), _lib.ptr(D)]
        with torch.cuda.device(dev):
            if fields is not None:                                # C = 0: the library launches nothing, as without fields
                a, th, tau = fields
                _lib.check(self._lib.rato_hopper_slip_f64_fields(
                    C.byref(params), mu_nom, K, M, _lib.ptr(Zs), ldz, _lib.ptr(a), _lib.ptr(th), _lib.ptr(tau), ldf,
                    _lib.ptr(lamd), ldlam, r0, *outs, _lib.current_stream()), "rato_hopper_slip_f64_fields")
            else:
                a, th, tau = self.fields_f64()
                _lib.check(self._lib.rato_hopper_slip_f64(
                    C.byref(params), mu_nom, K, M, _lib.ptr(Zs), ldz, _lib.ptr(a), _lib.ptr(th), _lib.ptr(tau), _lib.ptr(lamd),
                    ldlam, r0, *outs, _lib.current_stream()), "rato_hopper_slip_f64")
        out["D"] = D
        return out

    def slip_hess_blocks_device_f64(self, Zs, D, add):
        """rato_hopper_slip_hess_blocks_f64: adds the slip rows' share of hess(lam . g) into add (K, S+1, 78), in place"""
        Zs = self._device_rows(Zs)
        K, ldz = _rows_of(Zs, n_x * (self.S + 1) + n_u * self.S)
        if tuple(add.shape) != (K, self.S + 1, n_pairs) or add.dtype != torch.float64 or not add.is_contiguous() or \
                tuple(D.shape[:1] + D.shape[2:]) != (K, 3) or not D.is_contiguous():
            raise ValueError(f"add must be a contiguous device float64 tensor ({K}, {self.S + 1}, {n_pairs}) and D (K, C, 3)")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.rato_hopper_slip_hess_blocks_f64(
                C.byref(self._slip_params()), K, _lib.ptr(Zs), ldz, _lib.ptr(D), _lib.ptr(add), _lib.current_stream()),
                "rato_hopper_slip_hess_blocks_f64")
        return add

    def _slip_f64(self, Zs, lams=None, fields=None):
        """one evaluation of the slip kernel and its emission: slip_h (K, C, M), slip_rows (K, M C): h in the risk rows' order
        i C + c, slip_jac_values (K, nnz_slip): the CSC values of ``_jacobian_pattern`` with the constant part in place, D.
        ``fields``: friction fields per problem, as ``slip_device_f64`` takes them"""
        lay = self.nlp_layout()
        Cn, M = lay["C"], self.M
        r = self.slip_device_f64(Zs, lams, want=("h", "dh_dfz", "dh_dx"), fields=fields)
        K = r["h"].shape[0]
        st = getattr(self, "_slip_dev", None)
        if st is None:
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=self.device)
            st = self._slip_dev = dict(const=up(lay["slip_const"]), map_dx=up(lay["map_slip_dx"]), map_dfz=up(lay["map_slip_dfz"]),
                                       map_h=up(lay["map_slip_h"]))
        vals = st["const"][None].repeat(K, 1)
        rows = torch.empty((K, M * Cn), dtype=torch.float64, device=self.device)
        if Cn > 0:
            scatter_f64(r["dh_dx"].view(K, -1), st["map_dx"], vals)
            scatter_f64(r["dh_dfz"].view(K, -1), st["map_dfz"], vals)
            scatter_f64(r["h"].view(K, -1), st["map_h"], rows)
        return dict(slip_h=r["h"], slip_rows=rows, slip_jac_values=vals, D=r["D"])

    def _risk_rows(self, Z, h_rows):
        """the risk group from the slip values in row order i C + c (:339-367)"""
        _, _, ys, slack_var, t_risk = self.convert_z_to_variables(Z)
        M = self.M
        Cn = h_rows.size // M
        h = h_rows.reshape(M, Cn)
        if self.method == 'baseline':
            return (h - slack_var).reshape(M * Cn)
        gs = np.zeros(1 + M + M * Cn + 1)
        gs[0] = (M * self.alpha) * t_risk + np.sum(ys)
        gs[1:1 + M] = -ys
        gs[1 + M:1 + M + M * Cn] = (h - t_risk - ys[:, None] - slack_var).reshape(M * Cn)
        return gs

    def _blocks_to_csc(self, blocks):
        """step blocks (S+1, 78) -> the symmetric scipy CSC (num_vars x num_vars), exact zeros dropped"""
        import scipy.sparse as sp
        tr, tc = np.tril_indices(n_l)
        I, J, V = [], [], []
        for t in np.flatnonzero(np.any(blocks != 0.0, axis=1)):
            v = block_variables(self.S, t)
            gr, gc, val = v[tr], v[tc], blocks[t]
            ok = (gr >= 0) & (gc >= 0)
            off = ok & (gr != gc)
            I += [gr[ok], gc[off]]
            J += [gc[ok], gr[off]]
            V += [val[ok], val[off]]
        cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
        H = sp.coo_matrix((cat(V, np.float64), (cat(I, np.int64), cat(J, np.int64))), shape=(self.num_vars, self.num_vars)).tocsc()
        H.eliminate_zeros()
        H.sort_indices()
        return H

    # ---- Monte-Carlo validation (hopper.py:901-958) ------------------------
    def no_slip_constraints_verification(self, px, forces):
        Zh = self.slip_device(px, forces, want_h=False)["Z"].double().cpu().numpy()
        return Zh <= 1e-6, Zh

    def monte_carlo_statistics(self, px, forces, alpha=None):
        Z = self.slip_device(px, forces, want_h=False)["Z"]
        return stats.risk_stats(Z, self.alpha if alpha is None else alpha)

    avar = staticmethod(stats.monte_carlo_avar)

    # ---- K solutions on the model's fields in one call (the script's report, hopper.py:960-1007) ---------------------------
    def contact_inputs_batch(self, Zs):
        """``contact_inputs`` of K solutions -> (px (K, C), forces (K, C, 2)); row k is bitwise ``contact_inputs(Zs[k])`` (the
        rows may have different lengths: only the states and controls of a solution are read)."""
        rows = [self.contact_inputs(Z) for Z in Zs]
        if not rows:
            raise ValueError("contact_inputs_batch needs at least one solution")
        return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])

    def eval_batch_plan(self, Cn, K):
        """(nw_log2, k_chunk, grid_x, grid_y): the launch rato_hopper_eval_batch picks for K solutions of ``Cn`` contacts on this
        model's fields (rato_hopper_eval_batch_plan; host only)"""
        v = [C.c_int32(0) for _ in range(4)]
        _lib.check(self._lib.rato_hopper_eval_batch_plan(self._a.shape[1], int(Cn), int(K), *(C.byref(x) for x in v)),
                   "rato_hopper_eval_batch_plan")
        return tuple(x.value for x in v)

    def eval_batch_inputs_device(self, inputs, Cn, alphas=None, want_stats=True, want_arg=False, out=None, workspace=None,
                                 shape=None, selection='entry'):
        """``eval_batch_device`` on inputs that already lie on the device: ``inputs`` a float32 tensor (3, K, ldc >= Cn) holding
        px, fx, fz of solution k in row k (read in place at run time: a captured call sees what they hold at replay).
        ``selection``: 'entry' -- the entry point selects (one launch per run of equal alphas); 'rows' -- it runs without
        statistics and ONE ``stats.risk_stats_rows_device`` call follows (``workspace``: a ``stats.new_rows_workspace``)."""
        if selection not in ('entry', 'rows'):
            raise ValueError(f"selection must be 'entry' or 'rows', got {selection!r}")
        dev = self.device
        if not isinstance(inputs, torch.Tensor) or inputs.dtype != torch.float32 or inputs.dim() != 3 or inputs.shape[0] != 3 or \
                not inputs.is_contiguous() or inputs.device.type != 'cuda' or inputs.shape[2] < Cn or inputs.shape[1] < 1:
            raise ValueError("inputs must be a contiguous float32 device tensor (3, K, ldc >= C)")
        K, ldc, M = inputs.shape[1], inputs.shape[2], self._a.shape[1]
        if alphas is None:
            alphas = self.alpha
        al = np.full(K, float(alphas)) if np.ndim(alphas) == 0 else \
            np.array([1.0 if x is None else float(x) for x in alphas], dtype=np.float64)   # None: the baseline's row, at alpha = 1
        if al.shape != (K,):
            raise ValueError(f"alphas must be a scalar or a sequence of K = {K} entries")
        o = out if out is not None else {}
        if want_stats and selection == 'rows':
            r = self.eval_batch_inputs_device(inputs, Cn, want_stats=False, want_arg=want_arg, out=o, shape=shape)
            rec = o.get("_recrows")
            if rec is None or tuple(rec.shape) != (K, stats.N_STATS):
                rec = torch.empty((K, stats.N_STATS), dtype=torch.float64, device=dev)
            ws = workspace if workspace is not None else (o.get("_wsrows") if o.get("_wsrows_shape") == (M, K) else None)
            if ws is None:
                ws = stats.new_rows_workspace(M, K, dev)
            o["_recrows"], o["_wsrows"], o["_wsrows_shape"] = rec, ws, (M, K)
            with torch.cuda.device(dev):
                stats.risk_stats_rows_device(r[0], al, workspace=ws, out=rec)
            return (r[0], rec) + tuple(r[2:])
        Z = o.get("_Zb")
        if Z is None or tuple(Z.shape) != (K, M):
            Z = torch.empty((K, M), dtype=torch.float32, device=dev)
        rec = ws = arg = None
        if want_stats:
            rec = o.get("_recb")
            if rec is None or tuple(rec.shape) != (K, stats.N_STATS):
                rec = torch.empty((K, stats.N_STATS), dtype=torch.float64, device=dev)
            ws = workspace if workspace is not None else o.get("_wsb")
            if ws is None:
                ws = stats.new_workspace(M, dev)
        if want_arg:
            arg = o.get("_argb")
            if arg is None or tuple(arg.shape) != (K, M):
                arg = torch.empty((K, M), dtype=torch.int32, device=dev)
        o["_Zb"], o["_recb"], o["_wsb"], o["_argb"] = Z, rec, ws, arg
        args = (M, int(Cn), K, _lib.ptr(inputs[0]), _lib.ptr(inputs[1]), _lib.ptr(inputs[2]), ldc, _lib.ptr(self._a),
                _lib.ptr(self._th), _lib.ptr(self._tau), _lib.ptr(Z), M, _lib.ptr(arg),
                al.ctypes.data_as(C.POINTER(C.c_double)) if want_stats else None, float(stats.SATISFIED_THRESHOLD), _lib.ptr(ws),
                ws.numel() if ws is not None else 0, _lib.ptr(rec))
        with torch.cuda.device(dev):
            if shape is None:
                _lib.check(self._lib.rato_hopper_eval_batch(*args, _lib.current_stream()), "rato_hopper_eval_batch")
            else:
                _lib.check(self._lib.rato_hopper_eval_batch_shaped(*args, _lib.current_stream(), int(shape[0]), int(shape[1])),
                           "rato_hopper_eval_batch_shaped")
        return (Z, rec, arg) if want_arg else (Z, rec)

    def eval_batch_device(self, px, forces, alphas=None, want_stats=True, want_arg=False, out=None, workspace=None, shape=None,
                          selection='entry'):
        """K solutions on the model's fields in ONE call (rato_hopper_eval_batch): what the script's report does one solution at
        a time (hopper.py:983-1007).  px (K, C), forces (K, C, 2) (``contact_inputs_batch``), converted to fp32 as ``slip_device``
        converts them; one upload of the (3, K, C) inputs, no read-back.
        -> (Z [K][M] device fp32, records [K][N_STATS] device fp64 or None[, arg [K][M] int32 with want_arg]).  Row k of Z and of
        the records is, to the bit, what ``slip_device`` / ``stats.risk_stats_device`` give for solution k; arg[k][m] is the first
        contact (position in the gathered list) whose value is Z[k][m], -1 when that is -inf.
        ``alphas``: a scalar or K entries (default: the model's alpha); an entry of None is meant for the baseline: that row is
        selected at alpha = 1 and the caller drops its VaR and AVaR.  ``shape`` = (nw_log2, k_chunk) forces the launch shape
        (rato_hopper_eval_batch_shaped; -1: the rule's value); ``out``: a dict that keeps the buffers between calls;
        ``selection``: as in ``eval_batch_inputs_device``."""
        px = np.ascontiguousarray(px, dtype=np.float32)
        forces = np.asarray(forces, dtype=np.float32)
        if px.ndim != 2 or forces.shape != px.shape + (2,) or px.shape[0] < 1 or px.shape[1] < 1:
            raise ValueError(f"px must be (K, C) and forces (K, C, 2), got {px.shape} and {forces.shape}")
        host = np.stack([px, forces[..., 0], forces[..., 1]])
        inputs = torch.from_numpy(host).to(self.device)
        return self.eval_batch_inputs_device(inputs, px.shape[1], alphas=alphas, want_stats=want_stats, want_arg=want_arg,
                                             out=out, workspace=workspace, shape=shape, selection=selection)

    # ---- the whole NLP (hopper.py:441-453, :491-562, :569-640) -------------------------------------------------------------
    @classmethod
    def host_only(cls, M, method='saa', alpha=0.1, S=S, phases=None):
        """a Model without friction fields or a device: for the members that compute on the host alone (nlp_layout, gL_gU,
        x_bounds, f, grad_f, fold_multipliers); every device call on it fails"""
        self = cls(M, method, alpha, S=S, fields='device', device='cpu', phases=phases)
        self._a = self._th = self._tau = torch.empty((num_mu_features, M), dtype=torch.float32)
        return self

    def nlp_layout(self):
        """Host-only description of g in the script's order (:503-513), built once: the offsets of the ten groups, the fixed
        structural pattern of jac_g in CSC order and the index maps the device emission uses.
          off        offsets of dyn, x0, xf, slip, contact, over, risk, control, slack, len; ncon; C (contact steps)
          det_*      the deterministic rows' CSC (every row but the risk group's): indices, indptr, constant values
          map_defect [S][8][12] / map_rows [S+1][2][4] -> position in the deterministic CSC values (-1: not emitted),
          scale_rows -1 on the leg-over-ground rows
          map_hess   [S+1][78] -> position in np.tril_indices(nvar) order (-1: the u part of the last block)
          lam_rows_index / lam_rows_sign  [S+1][2]: which multiplier of g weighs the state row (-1: none), and its sign
          jac_indices / jac_indptr / pos_det / pos_slip   the full pattern and where the two value arrays go in it
          nnz_slip, slip_const, map_slip_dx / map_slip_dfz / map_slip_h   the fp64 slip path's emission (precision='f64')"""
        lay = getattr(self, "_nlp_layout", None)
        if lay is not None:
            return lay
        S, M, tj, tl, nvar = self.S, self.M, self.time_jump, self.time_land, self.num_vars
        if not 0 <= tj <= tl <= S:
            raise ValueError(f"phase times must satisfy 0 <= time_jump <= time_land <= S, got {tj}, {tl}, {S}")
        saa = self.method != 'baseline'
        Cn = tj + (S - tl)
        n_state = tj + (S + 1 - tl)
        n_risk = (1 + M + M * Cn + 1) if saa else M * Cn
        names = ("dyn", "x0", "xf", "slip", "contact", "over", "risk", "control", "slack", "len")
        counts = (n_x * S, n_x, 2, n_state, n_state, tl - tj, n_risk, n_u * S, 1, 3 * S)
        off, o = {}, 0
        for name, k in zip(names, counts):
            off[name] = o
            o += k
        ncon = o
        nX = n_x * (S + 1)
        states = np.concatenate([np.arange(0, tj), np.arange(tl, S + 1)]).astype(np.int64)
        rows, cols, consts, src = [], [], [], []        # src: ('d', flat index) / ('r', flat index) / None for a constant

        def put(r, c, v=0.0, s=None):
            rows.append(int(r)), cols.append(int(c)), consts.append(float(v)), src.append(s)
        for t in range(S):
            v = block_variables(S, t)
            for i in range(n_x):
                for j in range(n_l):
                    put(n_x * t + i, v[j], s=('d', (t * n_x + i) * n_l + j))
                put(n_x * t + i, n_x * (t + 1) + i, 1.0)                         # the x_{t+1} coefficient
        for i in range(n_x):
            put(off["x0"] + i, i, 1.0)
        for j in range(2):
            put(off["xf"] + j, n_x * S + 4 + j, 1.0)
        xsel = (2, 3, 6, 7)
        lam_index = -np.ones((S + 1, 2), dtype=np.int64)
        lam_sign = np.zeros((S + 1, 2))
        for i, t in enumerate(states):
            for j in range(4):
                put(off["slip"] + i, n_x * t + xsel[j], s=('r', (t * 2 + 0) * 4 + j))
            put(off["slip"] + i, n_x * t + 4, 1.0)
            for j in range(2):
                put(off["contact"] + i, n_x * t + xsel[j], s=('r', (t * 2 + 1) * 4 + j))
            put(off["contact"] + i, n_x * t + 1, 1.0)
            lam_index[t] = off["slip"] + i, off["contact"] + i
            lam_sign[t] = 1.0, 1.0
        scale_rows = np.ones((S + 1) * 8)
        for i, t in enumerate(range(tj, tl)):
            for j in range(2):
                put(off["over"] + i, n_x * t + xsel[j], s=('r', (t * 2 + 1) * 4 + j))
                scale_rows[(t * 2 + 1) * 4 + j] = -1.0
            put(off["over"] + i, n_x * t + 1, -1.0)
            lam_index[t, 1], lam_sign[t, 1] = off["over"] + i, -1.0
        for k in range(n_u * S):
            put(off["control"] + k, nX + k, 1.0)
        put(off["slack"], nvar - 2, 1.0)
        for j, comp in enumerate((3, 7, 6)):
            for t in range(S):
                put(off["len"] + j * S + t, n_x * (t + 1) + comp, 1.0)
        rows, cols, consts = np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(consts)
        order = np.lexsort((rows, cols))
        where = np.empty_like(order)
        where[order] = np.arange(order.size)
        map_defect = -np.ones(S * n_x * n_l, dtype=np.int64)
        map_rows = -np.ones((S + 1) * 8, dtype=np.int64)
        for e, s in enumerate(src):
            if s is not None:
                (map_defect if s[0] == 'd' else map_rows)[s[1]] = where[e]
        det_indices = rows[order]
        det_indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=nvar))]).astype(np.int64)
        # the tril-packed Hessian: entry e of block t is (v[r], v[c]) of np.tril_indices(nvar); x indices lie below u indices
        tr, tc = np.tril_indices(n_l)
        map_hess = -np.ones((S + 1, n_pairs), dtype=np.int64)
        for t in range(S + 1):
            v = block_variables(S, t)
            gr, gc = v[tr], v[tc]
            ok = (gr >= 0) & (gc >= 0)
            map_hess[t, ok] = gr[ok] * (gr[ok] + 1) // 2 + gc[ok]
        lay = dict(off=off, ncon=ncon, nvar=nvar, C=Cn, n_state=n_state, n_risk=n_risk, states=states, det_indices=det_indices,
                   det_indptr=det_indptr, det_const=consts[order], map_defect=map_defect, map_rows=map_rows,
                   scale_rows=scale_rows, map_hess=map_hess, lam_rows_index=lam_index, lam_rows_sign=lam_sign)
        # the full pattern: the deterministic entries and the risk group's (the slip Jacobian's own pattern), column by column
        if Cn > 0:
            s_idx, s_ptr = self._jacobian_pattern(Cn)
        else:
            s_idx, s_ptr = np.zeros(0, dtype=np.int64), np.zeros(nvar + 1, dtype=np.int64)
        s_cols = np.repeat(np.arange(nvar), np.diff(s_ptr))
        d_cols = np.repeat(np.arange(nvar), np.diff(det_indptr))
        all_rows = np.concatenate([det_indices, off["risk"] + np.asarray(s_idx, dtype=np.int64)])
        all_cols = np.concatenate([d_cols, s_cols])
        order = np.lexsort((all_rows, all_cols))
        where = np.empty_like(order)
        where[order] = np.arange(order.size)
        lay.update(jac_indices=all_rows[order].astype(np.int32),
                   jac_indptr=np.concatenate([[0], np.cumsum(np.bincount(all_cols, minlength=nvar))]).astype(np.int64),
                   pos_det=where[:det_indices.size], pos_slip=where[det_indices.size:])
        # the fp64 slip path (csrc/hopper_slip64.hip): where dh_dx [C][3][M], dh_dfz [C][M] and h [C][M] go -- positions in the
        # slip Jacobian's own CSC values (``_jacobian_pattern`` order) and in the risk rows' order i C + c -- and the constant
        # entries of those values (M alpha in fp64)
        CM = Cn * M
        ci, ii = np.divmod(np.arange(CM, dtype=np.int64), M)
        slip_const = np.zeros(len(s_idx))
        if Cn > 0:
            slip_const[3 * CM:5 * CM].reshape(Cn, 2, M)[:, 0, :] = 1.0                   # d/dfx
            o = 5 * CM
            if saa:
                slip_const[o:o + M * (2 + Cn)] = np.tile(np.concatenate([[1.0, -1.0], -np.ones(Cn)]), M)   # the y_i columns
                o += M * (2 + Cn)
            slip_const[o:o + CM] = -1.0                                                  # slack
            o += CM
            if saa:
                slip_const[o], slip_const[o + 1:o + 1 + CM] = M * self.alpha, -1.0       # t_risk
                o += 1 + CM
            assert o == slip_const.size
        lay.update(nnz_slip=slip_const.size, slip_const=slip_const, map_slip_dx=np.arange(3 * CM, dtype=np.int64),
                   map_slip_dfz=3 * CM + ci * (2 * M) + M + ii, map_slip_h=ii * Cn + ci)
        self._nlp_layout = lay
        return lay

    def f(self, Z):
        """:441-453"""
        Z = np.asarray(Z, dtype=np.float64)
        xs, us = self.convert_z_to_xs_us_mats(Z)
        R = 1.0
        return float(np.sum(R * (us[:, 0] * us[:, 0]) + R * (us[:, 1] * us[:, 1])) - 10000 * xs[-1, 0] + 10000000 * Z[-2])

    def _objective_terms(self):
        """(curv, lin) with f = 1/2 sum curv z^2 + lin . z: host-only, read-only, built once"""
        cl = getattr(self, "_curv_lin", None)
        if cl is None:
            curv, lin = np.zeros(self.num_vars), np.zeros(self.num_vars)
            ui = n_x * (self.S + 1) + n_u * np.arange(self.S)
            curv[ui] = curv[ui + 1] = 2.0                            # R (u0^2 + u1^2), R = 1
            lin[n_x * self.S], lin[-2] = -10000.0, 10000000.0        # -10000 x_S[0] + 1e7 slack
            curv.flags.writeable = lin.flags.writeable = False
            cl = self._curv_lin = (curv, lin)
        return cl

    @property
    def curv(self):
        """the objective's diagonal curvature (num_vars,): 2 on u0 and u1 of every step.  grad_f(Z) == curv * Z + lin bitwise
        (the supports are disjoint); what ``ipm.DeviceState`` uploads for the driver on the device"""
        return self._objective_terms()[0]

    @property
    def lin(self):
        """the objective's linear term (num_vars,): -10000 at x_S[0], 1e7 at the slack"""
        return self._objective_terms()[1]

    def grad_f(self, Z):
        Z = np.asarray(Z, dtype=np.float64)
        g = np.zeros(self.num_vars)
        nX = n_x * (self.S + 1)
        ui = nX + n_u * np.arange(self.S)
        g[ui], g[ui + 1] = 2.0 * Z[ui], 2.0 * Z[ui + 1]
        g[n_x * self.S] = -10000.0
        g[-2] = 10000000.0
        return g

    def gL_gU(self):
        """:515-562"""
        lay = self.nlp_layout()
        off, S, tj, tl = lay["off"], self.S, self.time_jump, self.time_land
        g_L, g_U = np.zeros(lay["ncon"]), np.zeros(lay["ncon"])
        g_L[off["over"]:] = -1e15
        cl, cu = np.zeros((S, n_u)), np.zeros((S, n_u))
        cl[:, :2], cu[:, :2] = -u_max, u_max                     # :401-406
        cu[:tj, 2:] = max_contact_force                          # :409-427: zero in flight
        cu[tl:, 2:] = max_contact_force
        g_L[off["control"]:off["slack"]], g_U[off["control"]:off["slack"]] = cl.reshape(-1), cu.reshape(-1)
        g_L[off["slack"]], g_U[off["slack"]] = 0.0, 1e6          # :430-438
        g_L[off["len"]:] = np.concatenate([0.25 * np.ones(S), -4.0 * np.ones(S), -2.5 * np.ones(S)])   # :369-390
        g_U[off["len"]:] = np.concatenate([1.0 * np.ones(S), 4.0 * np.ones(S), 2.5 * np.ones(S)])
        return g_L, g_U

    def x_bounds(self):
        """:599-620"""
        x_L, x_U = -np.ones(self.num_vars) * 1000.0, np.ones(self.num_vars) * 1000.0
        lo = np.array([-3, 0.5, -np.pi / 2, 0.1, -500, -500, -500, -500])
        hi = np.array([3, 10, np.pi / 2, 3, 500, 500, 500, 500])
        x_L[:n_x * (self.S + 1)] = np.tile(lo, self.S + 1)
        x_U[:n_x * (self.S + 1)] = np.tile(hi, self.S + 1)
        return x_L, x_U

    def initial_guess(self):
        """:136-164: the initial state until landing and the final state after it, the weight carried by u1 and fz in contact"""
        S, tj, tl = self.S, self.time_jump, self.time_land
        Zp = np.zeros(self.num_vars)
        xs = Zp[:n_x * (S + 1)].reshape(S + 1, n_x)
        us = Zp[n_x * (S + 1):n_x * (S + 1) + n_u * S].reshape(S, n_u)
        xs[:tl], xs[tl:] = state_initial, state_final
        nominal_force = (mass_body + mass_leg) * gravity
        for sl in (slice(0, tj), slice(tl, S)):
            us[sl, 1] = us[sl, 3] = nominal_force
        return Zp

    def solve(self, Z0=None, tol=1e-3, max_iter=3000, backend='device', callbacks=None, verbose=False, newton='dense',
              driver='host', chol='workgroup'):
        """The script's solve (:642-669, its options tol = 1e-3, max_iter = 3000) with the batched interior-point method of
        ``hopper_ipm`` in place of IPOPT -> (Z, info); info["status"] is 'converged' only if the final error shows it.
        newton='arrow' eliminates the M sample variables from the Newton step (the path that scales with M).
        driver='device' (backend='device', either newton; 'arrow' needs precision='f64'): the iterate stays on the device
        (``ipm.solve_group_device``, csrc/ipm_driver.hip); info["driver"] = 'device'.  driver='device_grid': the same with the
        driver's vector kernels spread over the rows (csrc/ipm_driver_grid.hip), bitwise the same result.
        chol: 'workgroup' or 'grid', the device Cholesky (``hopper_ipm.solve_batch``); the result does not depend on it."""
        from . import hopper_ipm
        return hopper_ipm.solve_batch([self], None if Z0 is None else [Z0], tol=tol, max_iter=max_iter, backend=backend,
                                      callbacks=None if callbacks is None else [callbacks], verbose=verbose, newton=newton,
                                      driver=driver, chol=chol)[0]

    def _nlp_state(self):
        """device-side constants of the emission, uploaded once and here alone: the maps, and per K the destinations pre-filled
        (jac_templates) or zeroed (tril_templates) by the two functions below, each when it is first asked for"""
        st = getattr(self, "_nlp_dev", None)
        if st is None:
            lay = self.nlp_layout()
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=self.device)
            st = self._nlp_dev = dict(map_defect=up(lay["map_defect"]), map_rows=up(lay["map_rows"]), scale_rows=up(lay["scale_rows"]),
                                      map_hess=up(lay["map_hess"].reshape(-1)), det_const=up(lay["det_const"]),
                                      jac_templates={}, tril_templates={})
        return st

    def det_jacobian_values(self, lin, K):
        """the deterministic rows' Jacobian values (K, n_det) in ``nlp_layout()``'s det_indices / det_indptr order: a copy of the
        constant entries with the partials d_defect and d_rows of ``nlp_linearize_device`` scattered over it (three launches)"""
        st = self._nlp_state()
        if K not in st["jac_templates"]:
            st["jac_templates"][K] = st["det_const"][None].repeat(K, 1).contiguous()
        jac = st["jac_templates"][K].clone()
        scatter_f64(lin["d_defect"].view(K, -1), st["map_defect"], jac)
        scatter_f64(lin["d_rows"].view(K, -1), st["map_rows"], jac, st["scale_rows"])
        return jac

    def hess_tril_device(self, blocks):
        """step blocks (K, S+1, 78) -> the tril-packed Hessian (K, nvar (nvar+1)/2) in np.tril_indices(nvar) order.  Its zeroed
        template is O(M^2) per problem and is made here, for the callers that read hess_tril, and nowhere else"""
        st, K = self._nlp_state(), blocks.shape[0]
        if K not in st["tril_templates"]:
            st["tril_templates"][K] = torch.zeros((K, self.num_vars * (self.num_vars + 1) // 2), dtype=torch.float64, device=self.device)
        return scatter_f64(blocks.view(K, -1), st["map_hess"], st["tril_templates"][K].clone())

    def fold_multipliers(self, lams):
        """(K, ncon) multipliers of g -> lam_dyn (K, S, 8), lam_rows (K, S+1, 2): the no-slip and contact multipliers on the
        contact states and minus the leg-over-ground multiplier on the flight states (host arrays)"""
        lay = self.nlp_layout()
        lams = np.atleast_2d(np.asarray(lams, dtype=np.float64))
        if lams.shape[1] != lay["ncon"]:
            raise ValueError(f"lams must be (K, {lay['ncon']}), got {lams.shape}")
        idx, sign = lay["lam_rows_index"], lay["lam_rows_sign"]
        lam_rows = np.where(idx >= 0, lams[:, np.maximum(idx, 0)], 0.0) * sign
        return np.ascontiguousarray(lams[:, :n_x * self.S]).reshape(-1, self.S, n_x), np.ascontiguousarray(lam_rows)

    def fold_map(self):
        """the inverse of ``nlp_layout()``'s lam_rows_index, host-only, built once: (index (ncon,) int64, scale (ncon,)) with
        lam_rows.reshape(-1)[index[r]] = scale[r] lams[r] for the rows r with index[r] >= 0 (the no-slip, contact and
        leg-over-ground rows; scale is lam_rows_sign) and index[r] = -1 for every other row: what rato_scatter_f64 takes to
        fold the multipliers where they lie"""
        fm = getattr(self, "_fold_map", None)
        if fm is None:
            lay = self.nlp_layout()
            idx, sign = lay["lam_rows_index"].reshape(-1), lay["lam_rows_sign"].reshape(-1)
            used = np.flatnonzero(idx >= 0)
            assert np.unique(idx[used]).size == used.size, "lam_rows_index must be one-to-one on its non-negative entries"
            index, scale = -np.ones(lay["ncon"], dtype=np.int64), np.zeros(lay["ncon"])
            index[idx[used]], scale[idx[used]] = used, sign[used]
            fm = self._fold_map = (index, scale)
        return fm

    def fold_multipliers_device(self, lams):
        """``fold_multipliers`` on a device fp64 tensor lams (K, ld >= ncon) with contiguous rows, without a read-back:
        lam_rows by rato_scatter_f64 through ``fold_map()`` into a zeroed (K, S+1, 2), lam_dyn the contiguous copy of
        lams[:, :8 S] -> (lam_dyn (K, S, 8), lam_rows (K, S+1, 2)) device tensors, bitwise the host's"""
        ncon, S = self.nlp_layout()["ncon"], self.S
        if not isinstance(lams, torch.Tensor) or lams.dim() != 2 or lams.shape[1] < ncon or lams.dtype != torch.float64 or \
                not lams.is_cuda or lams.stride(1) != 1:
            raise ValueError(f"lams must be a device float64 tensor (K, >= {ncon}) with contiguous rows")
        K = lams.shape[0]
        fd = getattr(self, "_fold_dev", None)
        if fd is None:
            index, scale = self.fold_map()
            fd = self._fold_dev = (torch.as_tensor(index, device=self.device), torch.as_tensor(scale, device=self.device))
        lam_rows = torch.zeros((K, S + 1, 2), dtype=torch.float64, device=lams.device)
        ld = lams.stride(0) if K > 1 else max(lams.stride(0), ncon)
        with torch.cuda.device(lams.device):
            _lib.check(self._lib.rato_scatter_f64(K, ncon, _lib.ptr(lams), ld, _lib.ptr(fd[0]), _lib.ptr(fd[1]), _lib.ptr(lam_rows),
                                                  2 * (S + 1), 2 * (S + 1), _lib.current_stream()), "rato_scatter_f64")
        return lams[:, :n_x * S].contiguous().view(K, S, n_x), lam_rows

    def nlp_device(self, Zs, lams=None, add=None, fold='host', fields=None):
        """K problems per call.  Zs (K, nvar) host array or device fp64 tensor (rows may be strided: ldz >= nvar); lams
        (K, ncon) multipliers of g or None; add (K, S+1, 78) blocks added to the Hessian or None.  -> dict of fp64 DEVICE tensors:
        defect (K, S, 8), d_defect (K, S, 8, 12), rows (K, S+1, 2), d_rows (K, S+1, 2, 4), jac_values (K, nnz): the CSC values of
        the deterministic rows' Jacobian in ``nlp_layout()``'s det_indices / det_indptr order; and with lams: hess_blocks
        (K, S+1, 78), hess_tril (K, nvar (nvar+1)/2) in np.tril_indices(nvar) order.  Four launches without lams, six with, plus
        one scatter for the fold (under fold='host' too, which folded on the host before and so has gained that launch).
        precision='f64' adds the risk group, from the same Z on the device (no host gather): slip_h (K, C, M), slip_rows
        (K, M C) = h in the risk rows' order i C + c, slip_jac_values (K, nnz_slip) in ``_jacobian_pattern`` order with the
        constant entries in place; with lams the slip rows' share is inside hess_blocks / hess_tril (the multipliers are read
        where they lie).  Four more launches, seven with lams.
        The multipliers, uploaded first when they are a host array (K, ncon), are folded by ``fold_multipliers_device`` (a device
        tensor may be (K, ld >= ncon)) and nothing of them is read back: ``hess_blocks_device`` is the one sequence under both
        folds.  fold='device': hess_tril is not built (the solver reads the blocks), so its O(nvar^2) template is never made.
        ``fields`` (precision='f64' only): friction fields per problem, (a, theta, tau) each (K, 30, M), as ``slip_device_f64``
        takes them; every other row of the NLP does not depend on them."""
        if fold not in ('host', 'device'):
            raise ValueError(f"fold must be 'host' or 'device', got {fold!r}")
        if fields is not None and self.precision != 'f64':
            raise ValueError("fields per problem are the fp64 slip path's: the model needs precision='f64'")
        Zs = self._device_rows(Zs)
        if fields is not None:
            _check_fields(fields, Zs.shape[0], self.M, self.device)
        if Zs.dim() != 2 or Zs.shape[1] < self.num_vars:
            raise ValueError(f"Zs must be (K, >= {self.num_vars}), got {tuple(Zs.shape)}")
        K = Zs.shape[0]
        out = nlp_linearize_device(self._slip_params(), Zs)
        out["jac_values"] = self.det_jacobian_values(out, K)
        lams, D = None if lams is None else self._device_rows(lams), None
        if self.precision == 'f64':                               # the risk group from the same Z, on the device
            slip = self._slip_f64(Zs, None if lams is None else lams[:, :self.nlp_layout()["ncon"]], fields)
            out.update(slip_h=slip["slip_h"], slip_rows=slip["slip_rows"], slip_jac_values=slip["slip_jac_values"])
            D = slip["D"]
        if lams is not None:
            if add is not None and not isinstance(add, torch.Tensor):
                add = torch.as_tensor(np.ascontiguousarray(add, dtype=np.float64), device=self.device)
            out["hess_blocks"] = self.hess_blocks_device(Zs, lams, add, D)
            if fold == 'host':
                out["hess_tril"] = self.hess_tril_device(out["hess_blocks"])
        return out

    def hess_blocks_device(self, Zs, lams, add=None, D=None, in_place=False):
        """The step blocks of hess(lams . g) + add, (K, S+1, 78), by the one sequence every consumer runs: the multipliers lams
        (device, (K, ld >= ncon)) folded where they lie, the slip rows' share (D (K, C, 3) of ``slip_device_f64`` on the same Zs
        and lams; None: the fp32 path, whose share the caller has put into ``add``) added into a copy of ``add`` (K, S+1, 78)
        -- the caller's tensor is left as it is, unless it is a scratch buffer of the caller's and ``in_place`` says so --
        then rato_hopper_nlp_hessian.  Nothing moves to the host."""
        K = Zs.shape[0]
        lam_dyn, lam_rows = self.fold_multipliers_device(lams)
        if lam_dyn.shape[0] != K:
            raise ValueError(f"Zs and lams must hold the same K problems, got {K} and {lam_dyn.shape[0]}")
        if D is not None and self.nlp_layout()["C"] > 0:
            if not in_place:
                add = torch.zeros((K, self.S + 1, n_pairs), dtype=torch.float64, device=self.device) if add is None else add.clone()
            self.slip_hess_blocks_device_f64(Zs, D, add)
        return nlp_hessian_device(self._slip_params(), Zs, lam_dyn, lam_rows, add)

    def g_values_device(self, Zs, fields=None):
        """what g is assembled from and nothing else, precision='f64': defect (K, S, 8) and rows (K, S+1, 2) (the linearize call
        without its derivatives) and slip_h (K, C, M) (the slip call without its partials), device tensors; two launches"""
        Zs = self._device_rows(Zs)
        out = nlp_linearize_device(self._slip_params(), Zs, want=("defect", "rows"))
        out["slip_h"] = self.slip_device_f64(Zs, want=("h",), fields=fields)["h"]
        return out

    def assemble_g(self, Z, defect, rows, slip_rows):
        """g in the script's order (:491-514), all ten groups (float64), from what the device leaves for one problem (host
        arrays): defect (S, 8), rows (S+1, 2) and the slip values in the risk rows' order i C + c (not read without contacts)"""
        lay = self.nlp_layout()
        xs, us = self.convert_z_to_xs_us_mats(Z)
        st, tj, tl = lay["states"], self.time_jump, self.time_land
        risk = self._risk_rows(Z, slip_rows if lay["C"] > 0 else np.zeros(0))       # no contact: :339-367 with num_contacts = 0
        return np.concatenate([defect.reshape(-1), xs[0] - state_initial, (xs[-1] - state_final)[4:6], rows[st, 0], rows[st, 1],
                               -rows[tj:tl, 1], risk, us.reshape(-1), [Z[-2]], xs[1:, 3], xs[1:, 7], xs[1:, 6]])

    def g(self, Z, _lin=None):
        """``assemble_g`` on one ``nlp_device`` call; the slip values are the fp32 kernel's (``slip_device``), or with
        precision='f64' the fp64 slip rows of the same call"""
        Z = np.asarray(Z, dtype=np.float64)
        r = _lin if _lin is not None else self.nlp_device(Z[None])
        if self.precision == 'f64':
            slip_rows = r["slip_rows"][0].cpu().numpy()
        else:
            slip_rows = self._slip_rows_host(Z) if self.nlp_layout()["C"] > 0 else None
        return self.assemble_g(Z, r["defect"][0].cpu().numpy(), r["rows"][0].cpu().numpy(), slip_rows)

    def jac_g(self, Z, _lin=None):
        """jacrev(g)(Z) (:569) as a scipy CSC (ncon, nvar) in the script's row and column order, with a FIXED structural
        pattern (``nlp_layout()``: jac_indices / jac_indptr), exact zeros stored: the device-written deterministic values
        stacked with the ``slip_jacobian_device`` values.  ``.toarray()`` is what grad_g_jax returns."""
        import scipy.sparse as sp
        Z = np.asarray(Z, dtype=np.float64)
        lay = self.nlp_layout()
        r = _lin if _lin is not None else self.nlp_device(Z[None])
        data = np.zeros(lay["jac_indices"].size)
        data[lay["pos_det"]] = r["jac_values"][0].cpu().numpy()
        if lay["C"] > 0 and self.precision == 'f64':
            data[lay["pos_slip"]] = r["slip_jac_values"][0].cpu().numpy()
        elif lay["C"] > 0:
            vals, _, indptr, _ = self.slip_jacobian_device(Z)
            slip = vals.double().cpu().numpy()
            if self.method != 'baseline':
                slip[indptr[-2]] = self._a.shape[1] * self.alpha   # row 0 of the t_risk column: M alpha in fp64, as slip_jacobian
            data[lay["pos_slip"]] = slip
        return sp.csc_matrix((data, lay["jac_indices"], lay["jac_indptr"]), shape=(lay["ncon"], lay["nvar"]))

    def slip_hessian_blocks(self, Z, lam):
        """the risk group's share of hess(lam . g) as step blocks (S+1, 78), computed as ``slip_hessian`` computes it: per
        contact the 3 x 3 block on (x0, x2, x3) of its step and the mixed entries with fz (local 0, 2, 3 and 11)"""
        lay = self.nlp_layout()
        if self.precision == 'f64':
            Zd = self._device_rows(np.asarray(Z, dtype=np.float64)[None])
            add = torch.zeros((1, self.S + 1, n_pairs), dtype=torch.float64, device=self.device)
            if lay["C"] > 0:
                D = self.slip_device_f64(Zd, np.asarray(lam, dtype=np.float64)[None], want=())["D"]
                self.slip_hess_blocks_device_f64(Zd, D, add)
            return add[0].cpu().numpy()
        blocks = np.zeros((self.S + 1, n_l, n_l))
        Cn, M = lay["C"], self._a.shape[1]
        if Cn > 0:
            r0 = lay["off"]["risk"] + (1 + M if self.method != 'baseline' else 0)
            lam_s = np.asarray(lam, dtype=np.float64)[r0:r0 + M * Cn].reshape(M, Cn)
            px, forces = self.contact_inputs(Z)
            D = self.slip_hessian_sums3(px, forces, lam_s)
            Jee, Hee = self.contact_chain(Z)
            blk = D[:, 1, None, None] * Jee[:, :, None] * Jee[:, None, :] + D[:, 2, None, None] * Hee
            mixed = D[:, 0, None] * Jee
            steps, loc = self.contact_steps(), np.array([0, 2, 3])
            blocks[steps[:, None, None], loc[None, :, None], loc[None, None, :]] = blk
            blocks[steps[:, None], 11, loc[None, :]] = mixed
            blocks[steps[:, None], loc[None, :], 11] = mixed
        tr, tc = np.tril_indices(n_l)
        return blocks[:, tr, tc]

    def _hess_add(self, Z, lam, obj_factor):
        """the fp32 slip share (precision='f64': nlp_device adds it on the device) plus the objective's blocks"""
        return objective_blocks(self.S, obj_factor, out=self.slip_hessian_blocks(Z, lam) if self.precision != 'f64' else None)

    def _hess_device(self, Z, lam, obj_factor):
        Z = np.asarray(Z, dtype=np.float64)
        lam = np.asarray(lam, dtype=np.float64)
        return self.nlp_device(Z[None], lam[None], add=self._hess_add(Z, lam, obj_factor)[None])

    def hess_lagrangian(self, Z, lam, obj_factor=1.0):
        """obj_factor hess_f + hess(lam . g) as the tril-packed vector eval_h writes (:622-628)"""
        return self._hess_device(Z, lam, obj_factor)["hess_tril"][0].cpu().numpy()

    def hess_lagrangian_blocks(self, Z, lam, obj_factor=1.0):
        """the same Hessian as its S + 1 step blocks (S+1, 12, 12) on (x_t, u_t); nothing lies outside them"""
        v = self._hess_device(Z, lam, obj_factor)["hess_blocks"][0].cpu().numpy()
        tr, tc = np.tril_indices(n_l)
        B = np.zeros((self.S + 1, n_l, n_l))
        B[:, tr, tc] = v
        B[:, tc, tr] = v
        return B

    def ipopt_callbacks(self, sparse=False):
        """-> dict(eval_f, eval_grad_f, eval_g, eval_jac_g, eval_h, g_L, g_U, x_L, x_U, eval_jac_g_sparsity_indices,
        eval_h_sparsity_indices, nvar, ncon): the arguments of the script's ``ipyopt.Problem(...)`` call (:646-661), same
        signatures (the callbacks write into ``out``).  sparse=False: the script's dense row-major Jacobian and tril Hessian
        (:633-640).  sparse=True: the index pairs are the structural patterns (CSC order of ``jac_g``; the step blocks of the
        Hessian) and ``out`` holds only those entries.  eval_g and eval_jac_g at the same x share one evaluation; with
        precision='f64' that one evaluation holds the slip kernel's too (one rato_hopper_slip_f64 call for both)."""
        lay = self.nlp_layout()
        nvar, ncon, S = lay["nvar"], lay["ncon"], self.S
        cache = {}

        def lin(x):
            x = np.asarray(x, dtype=np.float64)
            key = x.tobytes()
            if cache.get("key") != key:
                cache["key"], cache["val"] = key, self.nlp_device(x[None])
            return cache["val"]

        def eval_f(x):
            return self.f(x)

        def eval_grad_f(x, out):
            out[:] = self.grad_f(x)
            return out

        def eval_g(x, out):
            out[:] = self.g(x, _lin=lin(x))
            return out
        g_L, g_U = self.gL_gU()
        x_L, x_U = self.x_bounds()
        if not sparse:
            def eval_jac_g(x, out):
                out[:] = self.jac_g(x, _lin=lin(x)).toarray().reshape(-1)
                return out

            def eval_h(x, lagrange, obj_factor, out):
                out[:] = self.hess_lagrangian(x, lagrange, obj_factor)
                return out
            i1, i2 = np.indices((ncon, nvar))
            jac_idx = (i1.flatten(), i2.flatten())
            r, c = np.tril_indices(nvar)
            h_idx = (r.flatten(), c.flatten())
        else:
            keep = np.flatnonzero(lay["map_hess"].reshape(-1) >= 0)
            tr, tc = np.tril_indices(n_l)
            hr = np.concatenate([block_variables(S, t)[tr] for t in range(S + 1)])[keep]
            hc = np.concatenate([block_variables(S, t)[tc] for t in range(S + 1)])[keep]

            def eval_jac_g(x, out):
                out[:] = self.jac_g(x, _lin=lin(x)).data
                return out

            def eval_h(x, lagrange, obj_factor, out):
                out[:] = self._hess_device(x, lagrange, obj_factor)["hess_blocks"][0].cpu().numpy().reshape(-1)[keep]
                return out
            jac_idx = (lay["jac_indices"].astype(np.int64), np.repeat(np.arange(nvar), np.diff(lay["jac_indptr"])))
            h_idx = (hr, hc)
        return dict(eval_f=eval_f, eval_grad_f=eval_grad_f, eval_g=eval_g, eval_jac_g=eval_jac_g, eval_h=eval_h, g_L=g_L, g_U=g_U,
                    x_L=x_L, x_U=x_U, eval_jac_g_sparsity_indices=jac_idx, eval_h_sparsity_indices=h_idx, nvar=nvar, ncon=ncon)
