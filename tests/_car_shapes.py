"""Launch shapes of the driving row kernel (car_linearize_rows_kernel) and a dense checker of its outputs against the
fp64 oracle: plain Python / NumPy, no GPU.

``car_rows_shape`` restates the launcher's rule (csrc/rato_rows_plan.h as csrc/driving.hip, car_linearize_impl, calls it
through prepare_rows_launch of csrc/rato_sample_launch.h, which holds the queue fallback: LDS per workgroup, workgroups
per CU, the tile queue, small-batch split, queue tail parts), so that a GPU test can name the form it means to run and
``rato_car_stats_in_launch`` on the device can tell when the table has moved.  ``units`` restates the kernel's
unit -> (tile, part) mapping.

``check`` compares what the device wrote for a set of samples (the untiled Jacobian columns, g_up, Z and the
sample-independent final rows) with the fp64 oracle on the same fp32 inputs, using the limits of tests/_tol.py as they
are.  Every comparison is NaN-safe (``~(err <= limit)``): an unwritten lane under RATO_POISON=1 fails.
"""
import os

import numpy as np

from oracle import driving as ocar
from tests import _tol as tol

TILE = 64                    # CROWS_SAMPLES: samples per tile (one wave)
NW = 8                       # CROWS_NW: waves per workgroup
LDS_MAX = 160 * 1024         # CAR_ROWS_LDS_MAX
CUS = 256                    # compute units of an MI355X
FINAL_RHS_RTOL, FINAL_RHS_ATOL = 1e-5, 5e-5     # final_rhs, as tests/test_gpu_driving.py compares it
RS_SMALL_MAX, RS_COOP_KEYS, RS_COOP_MAX_WG = 12 * 1024, 16, 64   # rato_select.h


def car_rows_lds_bytes(S):
    """car_rows_lds_floats(S) * 4 (driving.hip)"""
    return 4 * (S * TILE * 6 + (S + 1) * 2 + S * 8 + S * 2 + 4 + (S + 1) * 2 + NW * 4 + (S + 1) * 6 + 2)


def _env_int(env, name, default):
    v = env.get(name)
    return default if v is None else int(v)


def _per_cu(S):
    """rato_plan::per_cu (rato_rows_plan.h) for the driving kernel's geometry"""
    return max(1, min(LDS_MAX // car_rows_lds_bytes(S), 32 // NW))


def stats_tail_workgroups(M, NT=NW * 64):
    """rato_sel::stats_tail_workgroups (rato_select.h): the extra workgroups of a launch, -1 beyond the one-launch forms"""
    if M <= RS_SMALL_MAX:
        return 1
    g = min((M + NT * 4 - 1) // (NT * 4), RS_COOP_MAX_WG)
    return -1 if g * NT * RS_COOP_KEYS < M else g


SWITCHES = (("RATO_CAR_SLOTS_PER_CU", 0), ("RATO_CAR_SMALL_SPLIT", -1), ("RATO_ROWS_DYNAMIC", 1), ("RATO_CAR_TAIL_SPLIT", 1),
            ("RATO_CAR_TAIL_TILES", -1))          # rato_car_rows_plan's `switches`, in its order, with the unset values
FORMS = ("split", "static", "queue")             # RATO_ROWS_FORM_*
PLAN_FIELDS = ("n_tiles", "per_cu", "slots", "qslots", "wants_queue", "form", "split", "n_whole", "workgroups", "n_units")


def switch_array(env, switches):
    """the switches of ``env`` as the int32 array the library's plan queries take"""
    import ctypes as C
    return (C.c_int32 * len(switches))(*[_env_int(env or {}, name, unset) for name, unset in switches])


def plan_fields(out):
    """a filled rato_rows_plan as a dict in the restatements' terms (form by name, wants_queue a bool)"""
    d = {k: getattr(out, k) for k in PLAN_FIELDS}
    d["form"], d["wants_queue"] = FORMS[d["form"]], bool(d["wants_queue"])
    return d


def library_plan(lib, M, S, cus=CUS, env=None, have_queue=True):
    """rato_car_rows_plan: the rule the launcher itself runs (csrc/rato_rows_plan.h), the switches passed explicitly;
    cus <= 0 asks the device; env = "process": the switches this process' library read from its environment"""
    import ctypes as C
    from riskaversetrajopt_amd import _lib
    out = _lib.RowsPlan()
    sw = None if env == "process" else switch_array(env, SWITCHES)
    assert lib.rato_car_rows_plan(M, S, cus, int(have_queue), sw, C.byref(out)) == 0, (M, S)
    return plan_fields(out)


def car_rows_shape(M, S, cus=CUS, env=None, have_queue=True):
    """The launch car_linearize_impl makes for the row kernel: an independent restatement of rato_plan::car_rows
    (csrc/rato_rows_plan.h), which tests/test_car_shapes.py compares with the library's rato_car_rows_plan field by
    field, under the switches in ``env`` (RATO_CAR_SLOTS_PER_CU, RATO_ROWS_DYNAMIC, RATO_CAR_SMALL_SPLIT,
    RATO_CAR_TAIL_SPLIT, RATO_CAR_TAIL_TILES; read as the library reads them).  form: 'split' (every tile dealt to
    `split` workgroups), 'static' (one tile per workgroup) or 'queue' (qslots workgroups take tiles from a global
    counter; the last n_tiles - n_whole tiles as `split` parts each).  have_queue=False: the work-queue pool handed out
    none, the shape keeps the static form (``queue``: the form is the queue; ``wants_queue``: it would be with one).
    stats_in_launch: rato_car_stats_in_launch, which ignores the switches."""
    env = {} if env is None else env
    lds = car_rows_lds_bytes(S)
    if S < 2 or lds > LDS_MAX:
        raise ValueError(f"S = {S}: not the row kernel ({lds} B of LDS)")
    n_tiles = (M + TILE - 1) // TILE
    per_cu = _per_cu(S)
    slots_env = _env_int(env, "RATO_CAR_SLOTS_PER_CU", 0)
    if 1 <= slots_env < per_cu:
        per_cu = slots_env
    slots = cus * per_cu
    wants_queue = _env_int(env, "RATO_ROWS_DYNAMIC", 1) != 0 and n_tiles > slots
    queue = wants_queue and have_queue
    qslots = cus * 2 if (slots_env < 1 and per_cu > 2) else slots             # at most two queue workgroups per CU
    max_split = max(1, (S + 3) // 4)                                           # rato_plan::max_split
    if queue:                                                                  # the queue and its tail parts
        split = min(max(1, _env_int(env, "RATO_CAR_TAIL_SPLIT", 1)), max_split)
        tail_env = _env_int(env, "RATO_CAR_TAIL_TILES", -1)
        tail_tiles = min(tail_env if tail_env >= 0 else qslots // 2, n_tiles)
        n_whole = n_tiles - tail_tiles if split > 1 else n_tiles
        workgroups, form = qslots, "queue"
    else:                                                                      # static, or every tile split
        split = 1
        if n_tiles < slots:
            small = _env_int(env, "RATO_CAR_SMALL_SPLIT", -1)
            split = small if small >= 1 else (2 if slots // n_tiles >= 2 else 1)
            split = max(1, min(split, max_split))
        n_whole, workgroups = 0, n_tiles * split
        form = "split" if split > 1 else "static"
    n_units = n_whole + (n_tiles - n_whole) * split                            # the kernel's unit count
    in_launch = n_tiles <= cus * _per_cu(S) and stats_tail_workgroups(M) > 0
    return dict(M=M, S=S, cus=cus, lds_bytes=lds, n_tiles=n_tiles, per_cu=per_cu, slots=slots, qslots=qslots,
                wants_queue=wants_queue, queue=queue, form=form, split=split, n_whole=n_whole, parted_tiles=n_tiles - n_whole if split > 1 else 0,
                workgroups=workgroups, n_units=n_units, stats_in_launch=in_launch)


def units(shape):
    """The kernel's unit -> (tile, part_id, row_split) mapping (car_linearize_rows_kernel) for every unit of a launch"""
    out = []
    loop = shape["queue"]
    for u in range(shape["n_units"]):
        if loop and u < shape["n_whole"]:
            out.append((u, 0, 1))
        else:
            v = u - shape["n_whole"] if loop else u
            s = shape["split"]
            out.append(((shape["n_whole"] if loop else 0) + v // s, v % s, s))
    return out


def sample_set(M, every=61):
    """Every lane of tiles {0, 1, middle, last - 1, last}, every 61st sample (61 and 64 are coprime: every lane position
    and every tile is hit) and the last sample; sorted, < M"""
    n = (M + TILE - 1) // TILE
    tiles = sorted({t for t in (0, 1, n // 2, n - 2, n - 1) if 0 <= t < n})
    idx = np.concatenate([np.arange(t * TILE, (t + 1) * TILE) for t in tiles] + [np.arange(0, M, every), [M - 1]])
    return np.unique(idx[idx < M]).astype(np.int64)


# ---- the fp64 oracle on the device's own fp32 inputs ------------------------------------------------------------------
def oracle_model(dW, x0_ped, w_speed, w_rep):
    """ocar.Model on a batch in kernel layout (host arrays: dW [S][2][n], x0_ped [4][n], w_speed [n], w_rep [n]), the
    construction of test_ragged_last_tile_at_the_C5_shard_size"""
    dW = np.asarray(dW, dtype=np.float64)
    S, _, n = dW.shape
    DWs = np.zeros((n, S, ocar.n_x))
    DWs[:, :, 6:8] = dW.transpose(2, 0, 1)
    ego0 = np.tile(np.asarray(ocar.state_init, dtype=np.float64)[:4], (n, 1))
    x0 = np.asarray(x0_ped, dtype=np.float64).T
    return ocar.Model(np.concatenate([ego0, x0], axis=1), np.asarray(w_speed, dtype=np.float64),
                      np.asarray(w_rep, dtype=np.float64), DWs)


def reference(dW, x0_ped, w_speed, w_rep, us, chunk=256):
    """fp64 outputs for the samples of a (small) batch: G dense (n, S, 2S), g_up (n, S), Z (n,), final_du (4, 2S),
    final_rhs (4,), and amp (n, S) = max(1, 1 / r_{t+1}), r_{t+1} = |p_ego - p_ped| at the time of row t: the
    near-contact factor of that row's limits.  The oracle's sensitivities are (n, S+1, 8, 2S): evaluated in chunks."""
    n = np.asarray(w_speed).shape[0]
    gdu, gup, Z, amp = [], [], [], []
    fdu = frhs = None
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        m = oracle_model(dW[:, :, s:e], x0_ped[:, s:e], w_speed[s:e], w_rep[s:e])
        fd, fl, _, g, gu = m.get_all_constraints_coeffs(us)
        gdu.append(g)
        gup.append(gu)
        xs = m.us_to_state_trajectories(us)
        Z.append((-m.separation_distances_at_all_times(xs)).max(axis=1) - ocar.OSQP_TOL)
        amp.append(np.maximum(1.0, 1.0 / np.linalg.norm(xs[:, 1:, 0:2] - xs[:, 1:, 4:6], axis=-1)))
        if fdu is None:
            fdu, frhs = fd[0], fl[0]
    return dict(G=np.concatenate(gdu), g_up=np.concatenate(gup), Z=np.concatenate(Z), final_du=fdu, final_rhs=frhs,
                amp=np.concatenate(amp))


def oracle_Z(dW, x0_ped, w_speed, w_rep, us, chunk=16384):
    """fp64 Z = max_t g_t - tol of every sample of a batch (the rollout only), in chunks"""
    n = np.asarray(w_speed).shape[0]
    out = np.empty(n)
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        m = oracle_model(dW[:, :, s:e], x0_ped[:, s:e], w_speed[s:e], w_rep[s:e])
        out[s:e] = m.monte_carlo_separation_constraints_verification(us)[1]
    return out


# ---- packed layout <-> dense rows ----------------------------------------------------------------------------------
def expand(Gp, S):
    """untiled packed [n_pairs][2][n] -> dense (n, S, 2S) (Model.expand_g_obs_du without a device)"""
    Gp = np.asarray(Gp, dtype=np.float64)
    n = Gp.shape[-1]
    dense = np.zeros((n, S, 2 * S))
    for t in range(1, S):
        off = t * (t - 1) // 2
        dense[:, t, :2 * t] = np.transpose(Gp[off:off + t], (2, 0, 1)).reshape(n, 2 * t)
    return dense


def pack(dense):
    """dense (n, S, 2S) -> untiled packed [n_pairs][2][n] (the entries below the causal diagonal)"""
    n, S, _ = dense.shape
    Gp = np.zeros((S * (S - 1) // 2, 2, n), dtype=dense.dtype)
    for t in range(1, S):
        off = t * (t - 1) // 2
        Gp[off:off + t] = np.transpose(dense[:, t, :2 * t].reshape(n, t, 2), (1, 2, 0))
    return Gp


# ---- the checker ---------------------------------------------------------------------------------------------------
def _first_bad(bad, idx, what, detail):
    pos = np.argwhere(bad)[0]
    where = ""
    if idx is not None:
        m = int(idx[pos[0]])
        where = f" at sample {m} (tile {m // TILE}, lane {m % TILE})"
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries off; first{where}, index "
                         f"{tuple(int(i) for i in pos)}: {detail(tuple(pos))}")


def _check_abs(name, actual, desired, rtol, atol, idx, what, amp=1.0):
    a, d = np.asarray(actual, dtype=np.float64), np.asarray(desired, dtype=np.float64)
    assert a.shape == d.shape, (name, a.shape, d.shape)
    lim = (atol + rtol * np.abs(d)) * amp
    err = np.abs(a - d)
    bad = ~(err <= lim)
    if bad.any():
        _first_bad(bad, idx, f"{what} {name}", lambda p: f"device {a[p]!r}, oracle {d[p]!r}, limit {lim[p]:.2e}")
    return float(np.max(err / lim)) if err.size else 0.0


def _check_rowmax(name, actual, desired, rel, idx, what, amp=1.0):
    """tol.assert_jac_close's criterion (error relative to the row's max |entry|), NaN-safe; ``amp`` scales the row
    scale (the near-contact factor)"""
    a, d = np.asarray(actual, dtype=np.float64), np.asarray(desired, dtype=np.float64)
    assert a.shape == d.shape, (name, a.shape, d.shape)
    scale = np.max(np.abs(d), axis=-1, keepdims=True) * amp
    err = np.abs(a - d)
    bad = ~(err <= rel * np.maximum(scale, 1e-30) + 1e-12)
    if bad.any():
        _first_bad(bad, idx, f"{what} {name}", lambda p: f"device {a[p]!r}, oracle {d[p]!r}, row max "
                   f"{float(scale[p[:-1]][0]):.3e}, limit {rel:.0e} x row max")
    return float(np.max(err / (np.maximum(scale, 1e-30) + 1e-12 / rel)) / rel) if err.size else 0.0


def check(out, ref, idx, S, what):
    """out: the device's outputs for the samples ``idx`` -- G untiled packed [n_pairs][2][n], g_up [S][n], Z [n],
    final_du [4][2S], final_rhs [4]; ref: ``reference`` on the same samples.  Asserts every entry within the limits of
    tests/_tol.py and the oracle's exact zeros (the causal pattern) exactly zero.  -> {quantity: worst error / limit}

    Row t is built on the unit normal n = (p_ego - p_ped) / r at time t + 1: where r < 1 the fp32 rollout's position
    error reaches the row amplified by 1 / r (dn/dp ~ 1 / r).  That row's Jacobian and g_up limits are scaled by
    ref["amp"] = 1 / r, the rule of test_gpu_driving.test_pedestrian_near_contact applied per row.  Every other row
    (amp = 1) is held to the plain limits."""
    dense = expand(out["G"], S)
    assert dense.shape == ref["G"].shape, (dense.shape, ref["G"].shape)
    zeros = ref["G"] == 0.0
    nz = zeros & (dense != 0.0)
    if nz.any():
        _first_bad(nz, idx, f"{what} g_obs_du causal zeros", lambda p: f"device {dense[p]!r} where the oracle is 0")
    worst = {
        "g_obs_du": _check_rowmax("g_obs_du", dense, ref["G"], tol.JAC_REL_ROWMAX_DRIVING, idx, what,
                                  ref["amp"][:, :, None]),
        "g_up": _check_abs("g_up", np.asarray(out["g_up"]).T, ref["g_up"], tol.GUP_RTOL, tol.GUP_ATOL, idx, what,
                           ref["amp"]),
        "Z": _check_abs("Z", out["Z"], ref["Z"], tol.G_RTOL, tol.G_ATOL, idx, what),
        "final_du": _check_rowmax("final_du", out["final_du"], ref["final_du"], tol.JAC_REL_ROWMAX, None, what),
        "final_rhs": _check_abs("final_rhs", out["final_rhs"], ref["final_rhs"], FINAL_RHS_RTOL, FINAL_RHS_ATOL, None,
                                what),
    }
    if os.environ.get("RATO_TOL_REPORT"):
        near = ref["amp"] > 1.0
        print(f"[tol] {what}: {int(near.sum())} of {near.size} rows within 1 of the pedestrian (their limits x up to "
              f"{ref['amp'].max():.1f})")
        for k, v in worst.items():
            print(f"[tol] {what} {k}: worst error / limit = {v:.3f}")
    return worst


def check_Z(Z, Z_ref, what):
    """full-batch Z against the oracle rollout (G_RTOL, G_ATOL); -> worst error / limit"""
    w = _check_abs("Z (full batch)", Z, Z_ref, tol.G_RTOL, tol.G_ATOL, None, what)
    if os.environ.get("RATO_TOL_REPORT"):
        print(f"[tol] {what} Z (full batch, {len(Z_ref)} samples): worst error / limit = {w:.3f}")
    return w
