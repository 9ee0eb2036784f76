"""Launch shapes of the drone row kernel (drone_linearize_rows_kernel) and a dense checker of its outputs against the
fp64 oracle: plain Python / NumPy, no GPU (the digest runs on whatever device its tensor is on).

``drone_rows_shape`` restates the launcher's rule (csrc/rato_rows_plan.h as csrc/drone.hip, drone_linearize_impl, calls it
through prepare_rows_launch of csrc/rato_sample_launch.h, which holds the queue fallback: LDS per workgroup, workgroups
per CU, small-batch split, the tile queue, its grid and its tail parts), so that a GPU test can name the form it means
to run and ``rato_drone_stats_in_launch`` on the device can tell when the table has moved.  ``units`` restates the
kernel's unit -> (tile, part) mapping and which part writes Z and each axis' rows of ``part``.

``check`` compares what the device wrote for a set of samples (the untiled packed Jacobian, or its factors W / Phi /
A22, with g_up and Z) with the fp64 oracle on the same fp32 inputs, using the limits of tests/_tol.py as they are;
``check_part`` holds one tile's row of sample sums to the sum of its samples' limits.  Every comparison is NaN-safe
(``~(err <= limit)``): an unwritten word in a NaN-filled buffer fails.
"""
import hashlib
import os

import numpy as np

from oracle import drone as od
from tests import _tol as tol
from tests._car_shapes import (PLAN_FIELDS, TILE, _check_abs, _check_rowmax, _env_int, _first_bad, plan_fields,  # noqa: F401
                               sample_set, stats_tail_workgroups, switch_array)

NW = 8                       # ROWS_NW: waves per workgroup
LDS_MAX = 160 * 1024         # ROWS_LDS_MAX
CUS = 256                    # compute units of an MI355X
N_OBS = od.n_obs
RHS_RTOL, RHS_ATOL = 1e-5, 2e-5      # one sample's final_low, as test_gpu_drone.test_single_sample_api_... compares it
RHS_MEAN_ATOL = 2e-5                 # rhs_sum / M (with MEAN_RTOL), as tests/test_gpu_drone.py compares it


def rows_lds_bytes(S):
    """rows_lds_floats(S) * 4 (drone.hip)"""
    return 4 * (S * TILE * 5 + S * 3 + 4)


def _per_cu(S):
    """rato_plan::per_cu (rato_rows_plan.h) for the drone kernel's geometry"""
    return max(1, min(LDS_MAX // rows_lds_bytes(S), 32 // NW))


SWITCHES = (("RATO_ROWS_SLOTS_PER_CU", 0), ("RATO_SMALL_SPLIT", 0), ("RATO_ROWS_DYNAMIC", 1), ("RATO_ROWS_QSLOTS", 0),
            ("RATO_DYN_TAIL_SPLIT", 0), ("RATO_DYN_TAIL_TILES", 0))   # rato_drone_rows_plan's `switches`, in its order, with
                                                                      # the unset values


def library_plan(lib, M, S, factored, cus=CUS, env=None, have_queue=True):
    """rato_drone_rows_plan: the rule the launcher itself runs (csrc/rato_rows_plan.h), the switches passed explicitly;
    cus <= 0 asks the device; env = "process": the switches this process' library read from its environment"""
    import ctypes as C
    from riskaversetrajopt_amd import _lib
    out = _lib.RowsPlan()
    sw = None if env == "process" else switch_array(env, SWITCHES)
    assert lib.rato_drone_rows_plan(M, S, int(factored), cus, int(have_queue), sw, C.byref(out)) == 0, (M, S)
    return plan_fields(out)


def drone_rows_shape(M, S, factored, cus=CUS, env=None, have_queue=True):
    """The launch drone_linearize_impl makes for the row kernel: an independent restatement of rato_plan::drone_rows
    (csrc/rato_rows_plan.h), which tests/test_drone_shapes.py compares with the library's rato_drone_rows_plan field by
    field, under the switches in ``env`` (RATO_ROWS_SLOTS_PER_CU, RATO_SMALL_SPLIT, RATO_ROWS_DYNAMIC, RATO_ROWS_QSLOTS,
    RATO_DYN_TAIL_SPLIT, RATO_DYN_TAIL_TILES; read as the library reads them: atoi, unset = the default).  form: 'split'
    (every tile dealt to `split` workgroups), 'static' (one tile per workgroup) or 'queue' (`workgroups` of them take
    units from a global counter: n_whole whole tiles, then the last n_tiles - n_whole tiles as `split` row-interleaved
    parts each).  have_queue=False: the work-queue pool handed out none, the shape keeps the static form.
    stats_in_launch: rato_drone_stats_in_launch, which ignores the switches."""
    env = {} if env is None else env
    lds = rows_lds_bytes(S)
    if S < 2 or lds > LDS_MAX:
        raise ValueError(f"S = {S}: not the row kernel ({lds} B of LDS)")
    n_tiles = (M + TILE - 1) // TILE
    per_cu = _per_cu(S)
    slots_env = _env_int(env, "RATO_ROWS_SLOTS_PER_CU", 0)
    if 1 <= slots_env < per_cu:
        per_cu = slots_env
    slots = cus * per_cu
    max_split = max(1, (S + 3) // 4)                                           # rato_plan::max_split
    split, n_whole, form, qslots = 1, n_tiles, "static", 0
    if n_tiles < slots:                                                        # small batch
        small = _env_int(env, "RATO_SMALL_SPLIT", 0)
        split = small if small > 0 else (2 if 2 * n_tiles <= cus else 1)
        split = max(1, min(split, max_split))
        n_whole = 0 if split > 1 else n_tiles
        form = "split" if split > 1 else "static"
    workgroups = n_whole + (n_tiles - n_whole) * split
    wants_queue = split == 1 and n_tiles > slots and _env_int(env, "RATO_ROWS_DYNAMIC", 1) >= 1
    if wants_queue and have_queue:
        form = "queue"
        qslots_env = _env_int(env, "RATO_ROWS_QSLOTS", 0)
        qslots = qslots_env if qslots_env > 0 else (cus if (not factored and slots_env < 1 and n_tiles >= 1024) else slots)
        workgroups = qslots
        dts, dtt = _env_int(env, "RATO_DYN_TAIL_SPLIT", 0), _env_int(env, "RATO_DYN_TAIL_TILES", 0)
        want_split = min(dts if dts > 0 else (1 if factored else 2), max_split)
        want_tiles = dtt if dtt > 0 else qslots
        if want_split > 1 and want_tiles > 0:
            split = want_split
            n_whole = n_tiles - min(want_tiles, max(n_tiles - qslots, 0))       # (more workgroups than tiles: no tail)
    n_units = n_whole + (n_tiles - n_whole) * split                            # the kernel's unit count
    in_launch = n_tiles <= cus * _per_cu(S) and stats_tail_workgroups(M, NW * 64) > 0
    return dict(M=M, S=S, factored=bool(factored), cus=cus, lds_bytes=lds, n_tiles=n_tiles, per_cu=per_cu, slots=slots,
                qslots=qslots, wants_queue=wants_queue, form=form, split=split, n_whole=n_whole, workgroups=workgroups, n_units=n_units,
                stats_in_launch=in_launch)


def unit_table(shape):
    """the kernel's unit -> (tile, part_id, row_split) mapping (drone_linearize_rows_kernel) as three arrays over the units"""
    u = np.arange(max(shape["n_units"], 0))
    n_whole, s = shape["n_whole"], shape["split"]
    whole = u < n_whole
    return (np.where(whole, u, n_whole + (u - n_whole) // s), np.where(whole, 0, (u - n_whole) % s),
            np.where(whole, 1, s))


def units(shape):
    """[(tile, part_id, row_split, writes_Z, axes)] for every unit of a launch.  Part p of row_split takes the row tasks
    t = p (mod row_split); it writes Z iff S % row_split == p and the rows of ``part`` of the axes a with
    a % row_split == p (drone_linearize_rows_kernel's final-state task)."""
    S = shape["S"]
    return [(int(t), int(p), int(rs), S % rs == p, tuple(a for a in range(3) if a % rs == p))
            for t, p, rs in zip(*unit_table(shape))]


# ---- the fp64 oracle on the device's own fp32 inputs ------------------------------------------------------------------
def oracle_model(dW, mass, Qsym):
    """od.Model on a batch in kernel layout (host arrays: dW [S][3][n], mass [n], Qsym [n_obs][3][n] = (Q00, Q01 + Q10,
    Q11)): the noise in rows 3..5 of DWs, the obstacle matrices upper triangular"""
    dW = np.asarray(dW, dtype=np.float64)
    S, _, n = dW.shape
    DWs = np.zeros((n, S, 6))
    DWs[:, :, 3:6] = dW.transpose(2, 0, 1)
    Qs = np.asarray(Qsym, dtype=np.float64)
    Q = np.zeros((n, N_OBS, 3, 3))
    Q[:, :, 0, 0], Q[:, :, 0, 1], Q[:, :, 1, 1] = Qs[:, 0].T, Qs[:, 1].T, Qs[:, 2].T
    return od.Model(S, DWs, np.asarray(mass, dtype=np.float64), Q, 'saa', 0.1)


def compact_final(fdu, rhs):
    """(n, 6, 3S), (n, 6) -> (n, 6S + 6): a sample's row in the layout of ``part`` (drone_linearize_rows_kernel): [s][0..2] =
    d p_a(S) / d u_{s,a}, [s][3..5] = d v_a(S) / d u_{s,a}, then the six rhs entries"""
    n, S = fdu.shape[0], fdu.shape[2] // 3
    rows = np.empty((n, 6 * S + 6))
    body = rows[:, :6 * S].reshape(n, S, 6)
    for a in range(3):
        body[:, :, a] = fdu[:, a, a::3]
        body[:, :, 3 + a] = fdu[:, 3 + a, a::3]
    rows[:, 6 * S:] = rhs
    return rows


def final_limits(rows, S):
    """per-entry limits of the samples' compact rows: JAC_REL_ROWMAX x the row max of the final-state Jacobian (row k =
    state component k of one sample, over its S columns), RHS_ATOL + RHS_RTOL |rhs| for the rhs"""
    n = rows.shape[0]
    lim = np.empty_like(rows)
    body = np.abs(rows[:, :6 * S].reshape(n, S, 6))
    lim[:, :6 * S] = np.broadcast_to(tol.JAC_REL_ROWMAX * body.max(axis=1, keepdims=True) + 1e-12, body.shape).reshape(n, 6 * S)
    lim[:, 6 * S:] = RHS_ATOL + RHS_RTOL * np.abs(rows[:, 6 * S:])
    return lim


def reference(dW, mass, Qsym, us, want_A22=False, chunk=256):
    """fp64 outputs for the samples of a (small) batch: G dense (n, n_obs, S, 3S), g_up (n, n_obs, S), Z (n,), the
    factors W (n, n_obs, S, 2) = dg/dp and Phi (n, S, 2S) (row t, column 2 s + a: d p_a(t+1) / d u_{s,a}), A22 (n, S, 2)
    (the step Jacobian's d v_a(t+1) / d v_a(t)) when asked, and final (n, 6S + 6): the per-sample final-state rows.
    The oracle's sensitivities are (n, S+1, 3, S, 2): evaluated in chunks."""
    n = np.asarray(mass).shape[0]
    us = np.asarray(us, dtype=np.float64)
    S = us.shape[0]
    acc = {k: [] for k in ("G", "g_up", "Z", "W", "Phi", "A22", "final")}
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        m = oracle_model(dW[:, :, s:e], mass[s:e], Qsym[:, :, s:e])
        fdu, rhs, _, gdu, gup = m.get_all_constraints_coeffs(us)
        xs = m.us_to_state_trajectories(us)
        sens = m.sensitivities(us, xs)
        d = xs[:, None, 1:, :2] - od.obs_positions[None, :, None, :2]                    # oracle/drone.py:189-193
        Q = m.obs_Qs[:, :, :2, :2]
        W = -np.einsum('mjab,mjtb->mjta', Q + np.swapaxes(Q, -1, -2), d)
        Phi = np.zeros((e - s, S, 2 * S))
        for a in range(2):
            Phi[:, :, a::2] = sens[:, 1:, a, :, 0]
        acc["G"].append(gdu)
        acc["g_up"].append(gup)
        acc["Z"].append(m.monte_carlo_no_collisions_constraint_verification(us)[1])
        acc["W"].append(W)
        acc["Phi"].append(Phi)
        acc["A22"].append(1.0 - m.dt * (0.25 + 2.0 * m.drag_coefficient * np.abs(xs[:, :S, 3:5])) / m.masses[:, None, None])
        acc["final"].append(compact_final(fdu, rhs))
    ref = {k: np.concatenate(v) for k, v in acc.items()}
    if not want_A22:
        del ref["A22"]
    return ref


def full_batch(dW, mass, Qsym, us, chunk=500):
    """the whole batch through the oracle, in chunks: Z (M,) and the per-sample final-state rows (M, 6S + 6) from which
    a tile's ``part`` row and du_sum / rhs_sum follow"""
    n = np.asarray(mass).shape[0]
    us = np.asarray(us, dtype=np.float64)
    S = us.shape[0]
    Z, rows = np.empty(n), np.empty((n, 6 * S + 6))
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        m = oracle_model(dW[:, :, s:e], mass[s:e], Qsym[:, :, s:e])
        xs = m.us_to_state_trajectories(us)
        Z[s:e] = m.obstacle_avoidance_constraints(xs, m.obs_Qs).reshape(e - s, -1).max(axis=1) - od.OSQP_TOL
        sens = m.sensitivities(us, xs)[:, S]                                            # (n, 3, S, 2)
        fdu = np.zeros((e - s, 6, 3 * S))
        for a in range(3):                                                               # oracle/drone.py:183-186, :200
            fdu[:, a, a::3] = sens[:, a, :, 0]
            fdu[:, 3 + a, a::3] = sens[:, a, :, 1]
        rhs = -m.final_constraints(xs) + fdu @ m.convert_us_mat_to_us_vec(us)
        rows[s:e] = compact_final(fdu, rhs)
    return Z, rows


# ---- packed layout <-> dense rows ----------------------------------------------------------------------------------
def expand(Gp, S):
    """untiled packed products [n_pairs][2][n_obs][n] -> dense (n, n_obs, S, 3S) (Model.expand_g_obs_du without a device)"""
    Gp = np.asarray(Gp, dtype=np.float64)
    n = Gp.shape[-1]
    dense = np.zeros((n, N_OBS, S, 3 * S))
    for t in range(1, S):
        off = t * (t - 1) // 2
        for a in range(2):
            dense[:, :, t, a:3 * t:3] = np.transpose(Gp[off:off + t, a], (2, 1, 0))
    return dense


def pack(dense):
    """dense (n, n_obs, S, 3S) -> untiled packed products [n_pairs][2][n_obs][n]"""
    n, _, S, _ = dense.shape
    Gp = np.zeros((max(S * (S - 1) // 2, 1), 2, N_OBS, n), dtype=dense.dtype)
    for t in range(1, S):
        off = t * (t - 1) // 2
        for a in range(2):
            Gp[off:off + t, a] = np.transpose(dense[:, :, t, a:3 * t:3], (2, 1, 0))
    return Gp


def expand_phi(Pp, S):
    """untiled packed factor [n_pairs][2][n] -> dense (n, S, 2S), column 2 s + a"""
    Pp = np.asarray(Pp, dtype=np.float64)
    n = Pp.shape[-1]
    dense = np.zeros((n, S, 2 * S))
    for t in range(1, S):
        off = t * (t - 1) // 2
        dense[:, t, :2 * t] = np.transpose(Pp[off:off + t], (2, 0, 1)).reshape(n, 2 * t)
    return dense


def pack_phi(dense):
    """dense (n, S, 2S) -> untiled packed factor [n_pairs][2][n]"""
    n, S, _ = dense.shape
    Pp = np.zeros((max(S * (S - 1) // 2, 1), 2, n), dtype=dense.dtype)
    for t in range(1, S):
        off = t * (t - 1) // 2
        Pp[off:off + t] = np.transpose(dense[:, t, :2 * t].reshape(n, t, 2), (1, 2, 0))
    return Pp


def products(W, Phi):
    """dense (n, n_obs, S, 3S) Jacobian of the factors W (n, n_obs, S, 2) and Phi (n, S, 2S): oracle/drone.py:194-197"""
    n, _, S, _ = W.shape
    G = np.zeros((n, N_OBS, S, 3 * S))
    for a in range(2):
        G[:, :, :, a::3] = W[:, :, :, a, None] * Phi[:, None, :, a::2]
    return G


# ---- the checker ---------------------------------------------------------------------------------------------------
def _zeros(name, dense, ref, idx, what):
    nz = (ref == 0.0) & (dense != 0.0)
    if nz.any():
        _first_bad(nz, idx, f"{what} {name} exact zeros", lambda p: f"device {dense[p]!r} where the oracle is 0")


def check(out, ref, idx, S, what):
    """out: the device's outputs for the samples ``idx`` -- g_up [n_obs][S][n], Z [n] and either G, the untiled packed
    products [n_pairs][2][n_obs][n], or the factors Phi [n_pairs][2][n] and W [n_obs][S][2][n] (and A22 [S][2][n]);
    ref: ``reference`` on the same samples.  Asserts every entry within the limits of tests/_tol.py and the oracle's
    exact zeros (causal pattern, vertical-axis columns) exactly zero.  The factors are held to the row-max criterion
    each (W: the two components of one (obstacle, step) gradient; Phi: a step's row; A22, an entry of the step
    Jacobian: one axis of a sample over the horizon), then their product like the products output.
    -> {quantity: worst error / limit}"""
    worst = {}
    if "G" in out:
        dense = expand(out["G"], S)
    else:
        W = np.transpose(np.asarray(out["W"], dtype=np.float64), (3, 0, 1, 2))
        Phi = expand_phi(out["Phi"], S)
        _zeros("Phi", Phi, ref["Phi"], idx, what)
        worst["W"] = _check_rowmax("W", W, ref["W"], tol.JAC_REL_ROWMAX, idx, what)
        worst["Phi"] = _check_rowmax("Phi", Phi, ref["Phi"], tol.JAC_REL_ROWMAX, idx, what)
        if "A22" in ref:
            worst["A22"] = _check_rowmax("A22", np.transpose(np.asarray(out["A22"], dtype=np.float64), (2, 1, 0)),
                                         np.transpose(ref["A22"], (0, 2, 1)), tol.JAC_REL_ROWMAX, idx, what)
        dense = products(W, Phi)
    assert dense.shape == ref["G"].shape, (dense.shape, ref["G"].shape)
    _zeros("g_obs_du", dense, ref["G"], idx, what)
    worst["g_obs_du"] = _check_rowmax("g_obs_du", dense, ref["G"], tol.JAC_REL_ROWMAX, idx, what)
    worst["g_up"] = _check_abs("g_up", np.transpose(np.asarray(out["g_up"]), (2, 0, 1)), ref["g_up"], tol.GUP_RTOL,
                               tol.GUP_ATOL, idx, what)
    worst["Z"] = _check_abs("Z", out["Z"], ref["Z"], tol.G_RTOL, tol.G_ATOL, idx, what)
    if os.environ.get("RATO_TOL_REPORT"):
        for k, v in worst.items():
            print(f"[tol] {what} {k}: worst error / limit = {v:.3f}")
    return worst


def part_row(rows, tile):
    """fp64 sums over tile's valid samples of the per-sample final-state rows (M, 6S + 6), their limit and n_valid.
    The limit of a sum of n_valid <= 64 samples is the sum of the samples' own limits (n_valid x the per-entry limit):
    |sum e_i| <= sum |e_i|; the fp32 summation error of 64 terms, 64 x 2^-24 x sum |x_i|, is two orders below it."""
    S = (rows.shape[1] - 6) // 6
    r = rows[tile * TILE:(tile + 1) * TILE]
    return r.sum(axis=0), final_limits(r, S).sum(axis=0), r.shape[0]


def check_part(part, rows, tiles, what):
    """the rows ``tiles`` of ``part`` [n_tiles][6S + 6] against the oracle's sums over each tile's valid samples"""
    part = np.asarray(part, dtype=np.float64)
    S = (rows.shape[1] - 6) // 6
    worst = 0.0
    for t in tiles:
        d, lim, nv = part_row(rows, t)
        err = np.abs(part[t] - d)
        bad = ~(err <= lim)
        if bad.any():
            e = int(np.argwhere(bad)[0][0])
            name = f"rhs[{e - 6 * S}]" if e >= 6 * S else f"step {e // 6}, {'pv'[e % 6 // 3]}_{'xyz'[e % 3]}"
            raise AssertionError(f"{what} part: {int(bad.sum())} of {bad.size} entries of tile {t} ({nv} valid samples) "
                                 f"off; first entry {e} ({name}): device {part[t][e]!r}, oracle {d[e]!r}, limit {lim[e]:.2e}")
        worst = max(worst, float(np.max(err / lim)))
    if os.environ.get("RATO_TOL_REPORT"):
        print(f"[tol] {what} part rows of tiles {list(tiles)}: worst error / (n_valid x limit) = {worst:.3f}")
    return worst


def check_means(sums, rows, what):
    """du_sum / M and rhs_sum / M (sums: [6S + 6]) against the oracle's full-batch means: MEAN_RTOL, MEAN_ATOL, and
    atol = 2e-5 on the rhs"""
    M, S = rows.shape[0], (rows.shape[1] - 6) // 6
    mean, got = rows.mean(axis=0), np.asarray(sums, dtype=np.float64) / M
    w = max(_check_abs("du_sum / M", got[:6 * S], mean[:6 * S], tol.MEAN_RTOL, tol.MEAN_ATOL, None, what),
            _check_abs("rhs_sum / M", got[6 * S:], mean[6 * S:], tol.MEAN_RTOL, RHS_MEAN_ATOL, None, what))
    if os.environ.get("RATO_TOL_REPORT"):
        print(f"[tol] {what} du_sum / M, rhs_sum / M ({M} samples): worst error / limit = {w:.3f}")
    return w


def check_Z(Z, Z_ref, what):
    """full-batch Z against the oracle rollout (G_RTOL, G_ATOL); -> worst error / limit"""
    w = _check_abs("Z (full batch)", Z, Z_ref, tol.G_RTOL, tol.G_ATOL, np.arange(len(Z_ref)), what)
    if os.environ.get("RATO_TOL_REPORT"):
        print(f"[tol] {what} Z (full batch, {len(Z_ref)} samples): worst error / limit = {w:.3f}")
    return w


# ---- digests -------------------------------------------------------------------------------------------------------
_K = 0x2545F4914F6CDD1D          # an odd 64-bit constant (< 2^63)


def digest_G(G, M, tiles_per_pass=128):
    """Positional checksum of a tile-blocked G [n_tiles][...][64] (a torch tensor of any strides: the packed buffer's
    tiles are 2 MiB aligned) over the words the kernel owns -- every lane of the full tiles, lanes < M - 64 (n_tiles - 1)
    of the last one: the sum over words of (bit pattern + 1) x (2 position + 1) K in int64 with wrap-around, position =
    the word's index in the back-to-back layout.  Every owned word takes part, and where it lies matters.  Runs on
    G's device."""
    import torch
    n_tiles = G.shape[0]
    payload = G[0].numel()
    pos = torch.arange(payload, dtype=torch.int64, device=G.device).view(G.shape[1:])
    nv = M - (n_tiles - 1) * TILE
    assert 0 < nv <= TILE == G.shape[-1]
    acc = torch.zeros((), dtype=torch.int64, device=G.device)

    def bits(x):
        return (x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) + 1
    for a in range(0, n_tiles - 1, tiles_per_pass):
        b = min(a + tiles_per_pass, n_tiles - 1)
        base = (torch.arange(a, b, dtype=torch.int64, device=G.device) * payload).view(-1, *([1] * pos.dim()))
        acc += (bits(G[a:b]) * (((base + pos) * 2 + 1) * _K)).sum()
    last = (n_tiles - 1) * payload
    acc += (bits(G[-1][..., :nv]) * (((last + pos[..., :nv]) * 2 + 1) * _K)).sum()
    return int(acc.item()) & ((1 << 64) - 1)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()
