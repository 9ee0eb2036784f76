"""GPU: the driving row kernel (car_linearize_rows_kernel) at every launch shape.  The launcher deals a batch out as
split tiles, one static tile per workgroup or a tile queue (tests/_car_shapes.py restates the rule); these tests run
both sides of each edge against the fp64 oracle on the device's own inputs, every launch structure against the
one-tile-per-workgroup launch bit for bit, and the driving eval on both sides of its switch to the plain kernel at
M = 2^20.  The library reads its switches once per process: one child process per variant."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import driving as ocar
from tests import _car_shapes as cs
from tests import _tol as tol
from tests.test_car_shapes import BASE, CASES, VARIANTS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = [0, 2, 4, 5, 7, 8, 9, 10]          # stats record: var, frac_satisfied, max, counts, rank, t_star
SUMS = [1, 3, 6]                           # cvar, mean, tail_sum (fp64 sums)


def swerve(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.4 * np.cos(0.4 * t) - 0.2, 0.05 * np.sin(0.35 * t) + 0.01]) * (20.0 / S)


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch(M, S, seed, regenerate=False):
    """device-drawn inputs (rato_car_sample) and a Model on them: the noise materialised, or regenerated in the kernel"""
    from riskaversetrajopt_amd import driving
    dW, x0, ws, wr = driving.sample_uncertain_parameters_device(M, S, seed=seed, want_dW=not regenerate)
    if regenerate:
        return driving.Model.from_device(S, None, x0, ws, wr, 'saa', 0.05, noise_seed=seed), (dW, x0, ws, wr)
    return driving.Model.from_device(S, dW, x0, ws, wr, 'saa', 0.05), (dW, x0, ws, wr)


def host(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def columns(G, idx):
    """packed tile-blocked G [n_tiles][n_pairs][2][64] -> the untiled columns [n_pairs][2][len(idx)] of samples idx"""
    import torch
    ti = torch.as_tensor(idx, device=G.device)
    return G[ti // cs.TILE, :, :, ti % cs.TILE].permute(1, 2, 0).cpu().numpy()


# ---- 1. the slot count on the device -----------------------------------------------------------------------------
def bisect_slots(lib, S):
    """the largest tile count at which rato_car_stats_in_launch is still 1 (no launch)"""
    lo, hi = 1, 8192                                           # in launch at lo tiles, not at hi tiles
    assert lib.rato_car_stats_in_launch(64 * lo, S) == 1 and lib.rato_car_stats_in_launch(64 * hi, S) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.rato_car_stats_in_launch(64 * mid, S) == 1 else (lo, mid)
    return lo


def test_plan_query_asks_the_device():
    """rato_car_rows_plan with cus <= 0 takes the device's CU count: at the shapes this file runs it is the restatement
    at that count, field by field, and its slots are the ones the bisection finds (no launch)"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    n = cus()
    shapes = sorted(set(CASES) | {(40, 16384), (40, 16385), (40, 32768), (40, 32769), (20, 65536), (20, 65537), (90, 16384),
                                  (90, 16385)})
    for S, M in shapes:
        want = cs.car_rows_shape(M, S, n)
        assert cs.library_plan(lib, M, S, cus=0) == {k: want[k] for k in cs.PLAN_FIELDS}, (S, M, n)
    for S in sorted({S for S, _ in shapes}):
        assert cs.library_plan(lib, 1, S, cus=-1)["slots"] == bisect_slots(lib, S), S


@pytest.mark.parametrize("S", [20, 40, 90])
def test_stats_in_launch_flips_at_the_slot_count(S):
    """rato_car_stats_in_launch(M, S) is 1 while the tiles fit the resident slots (the statistics workgroups fit up to
    M = 524,288): its flip, found by bisection on the device, is 64 x slots"""
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    n = cus()
    sh = cs.car_rows_shape(1, S, n)
    lo = bisect_slots(lib, S)
    assert lo == sh["slots"], (f"S = {S}: the device has {lo} row-kernel slots, tests/_car_shapes.py says "
                               f"{sh['slots']} ({n} CUs x {sh['per_cu']}): the shape table moved, the edge tests below "
                               f"no longer run the shapes they name")
    assert lib.rato_car_stats_in_launch(64 * lo + 1, S) == 0 and lib.rato_car_stats_in_launch(64 * lo, S) == 1
    assert cs.car_rows_shape(64 * lo, S, n)["stats_in_launch"] and not cs.car_rows_shape(64 * lo + 1, S, n)["stats_in_launch"]
    print(f"S = {S}: {lo} slots on {n} CUs ({sh['per_cu']} per CU, {sh['lds_bytes']} B of LDS per workgroup)")


# ---- 2. fp64 parity on both sides of each edge ---------------------------------------------------------------------
@pytest.mark.parametrize("S,M,form", [(40, 16384, "split"), (40, 16385, "static"), (40, 32768, "static"),
                                      (40, 32769, "queue"), (40, 125001, "queue"), (20, 65536, "static"),
                                      (20, 65537, "queue"), (90, 16384, "static"), (90, 16385, "queue")])
def test_fp64_parity_at_the_shape_edges(S, M, form):
    import torch
    from riskaversetrajopt_amd import _lib
    from riskaversetrajopt_amd.driving import untile
    sh = cs.car_rows_shape(M, S, cus())
    assert sh["form"] == form, sh
    d, (dW, x0, ws, wr) = batch(M, S, seed=S + M % 97)
    us = swerve(S)
    r, rec = d.step_device(us)                              # fused: statistics in the launch where it fits
    _, _, g = d.eval_device(us, want_g=True)
    torch.cuda.synchronize()
    assert _lib.load().rato_car_stats_in_launch(M, S) == int(sh["stats_in_launch"])
    what = f"S={S} M={M} ({form})"
    # every lane of the first, middle and last tiles and every 61st sample against the oracle
    idx = cs.sample_set(M)
    ti = torch.as_tensor(idx, device=dW.device)
    out = {"G": columns(r["G"], idx), "g_up": r["g_up"][:, ti].cpu().numpy(), "Z": r["Z"][ti].cpu().numpy(),
           "final_du": r["final_du"].cpu().numpy(), "final_rhs": r["final_rhs"].cpu().numpy()}
    ref = cs.reference(*host(dW[:, :, ti], x0[:, ti], ws[ti], wr[ti]), us)
    cs.check(out, ref, idx, S, what)
    # the whole batch: Z against the oracle rollout, nothing left unwritten, linearity g_up + g = G.u
    Zh = r["Z"].double().cpu().numpy()
    cs.check_Z(Zh, cs.oracle_Z(*host(dW, x0, ws, wr), us), what)
    Gp = untile(r["G"], M)
    assert bool(torch.isfinite(Gp).all()) and bool(torch.isfinite(r["g_up"]).all()), what
    u = torch.as_tensor(us, dtype=torch.float32, device=g.device)
    Gu = torch.zeros_like(g)
    for t in range(1, S):
        off = t * (t - 1) // 2
        Gu[t] = (Gp[off:off + t] * u[:t, :, None]).sum(dim=(0, 1))
    tol.assert_below((r["g_up"] + g - Gu).abs().max().item(), tol.LINEARITY_ABS_DRIVING,
                     f"{what} linearity |g_up + g - G.u|")
    # the statistics of the same fp32 Z (in the launch up to 64 x slots samples, behind it above)
    b = rec.cpu().numpy()
    srt = np.sort(Zh)
    k = M - int(np.floor(0.05 * M)) - 1
    assert b[0] == srt[k] and b[4] == srt[-1], (what, b)
    cvar = srt[k] + np.maximum(Zh - srt[k], 0).sum() / (0.05 * M)
    assert abs(b[1] - cvar) < 1e-9 * max(1.0, abs(cvar)), (what, b[1], cvar)


# ---- 3. every launch structure gives the same bits -------------------------------------------------------------------
def digests(cases):
    """{case: {sha256, samples}} of the row kernel's outputs under this process's switches: the untiled G of samples
    < M (lanes past M are never written), g_up, Z, final_du, final_rhs and the exact fields of the fused statistics
    record; each case with the noise read and regenerated (one digest: test_gpu_philox.py shows the two bitwise equal)"""
    import torch
    res = {}
    for S, M in cases:
        us = np.hstack([0.4 * np.cos(0.3 * np.arange(S))[:, None] + 0.1,
                        0.03 * np.sin(0.5 * np.arange(S))[:, None] + 0.004]) * (20.0 / S)
        for regen in (False, True):
            d, _ = batch(M, S, seed=7 + S, regenerate=regen)
            r, rec = d.step_device(us)
            torch.cuda.synchronize()
            G = r["G"]
            nv = M - (G.shape[0] - 1) * cs.TILE
            h = hashlib.sha256()
            for a in (G[:-1], G[-1, ..., :nv], r["g_up"], r["Z"], r["final_du"], r["final_rhs"], rec[EXACT]):
                h.update(a.contiguous().cpu().numpy().tobytes())
            idx = [0, 63, 64, M // 2, M - 1]
            res[f"S{S}_M{M}_{'regen' if regen else 'read'}"] = {
                "sha256": h.hexdigest(),
                "Z": [float(r["Z"][i]) for i in idx], "g_up": [float(r["g_up"][S - 1, i]) for i in idx],
                "G": [float(G[i // cs.TILE, -1, 1, i % cs.TILE]) for i in idx], "sums": rec[SUMS].tolist()}
            del d, r, rec, G
    return res


CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_gpu_driving_shapes as T
json.dump(T.%(fn)s(%(arg)r), open(%(path)r, "w"))
'''


def run_child(tmp_path, name, env, fn, arg, timeout=300):
    path = str(tmp_path / (name + ".json"))
    e = {k: v for k, v in os.environ.items() if not k.startswith(("RATO_ROWS_DYNAMIC", "RATO_CAR_", "RATO_EVAL_TILES"))}
    e.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT, fn=fn, arg=arg, path=path)], env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (name, p.returncode, p.stderr[-3000:])
    with open(path) as f:
        return json.load(f)


def test_launch_structures_are_bit_identical(tmp_path):
    """base: RATO_ROWS_DYNAMIC=0 RATO_CAR_SMALL_SPLIT=1, one tile per workgroup at any M.  Every other variant
    (tests/test_car_shapes.py pins the forms they make of each case: split 2 / 3 / 4, static, a queue over one
    workgroup per CU, a queue with halves / quarters of every tile / thirds of the last tile at its end) must
    reproduce it bit for bit, with the noise read or regenerated."""
    base = run_child(tmp_path, "base", BASE, "digests", CASES)
    for key, v in base.items():
        assert v["sha256"] == base[key.replace("_regen", "_read")]["sha256"], ("noise read vs regenerated", key, v)
    for name, env in VARIANTS.items():
        got = run_child(tmp_path, name, env, "digests", CASES)
        for key in base:
            assert got[key]["sha256"] == base[key]["sha256"], (name, key, {k: (base[key][k], got[key][k])
                                                                           for k in ("Z", "g_up", "G")})
            np.testing.assert_allclose(got[key]["sums"], base[key]["sums"], rtol=1e-12, atol=1e-300)


# ---- 4. the driving eval at its switch to the plain kernel --------------------------------------------------------
EVAL_MS = (1 << 20, (1 << 20) + 1)
EVAL_S = 40


def eval_outputs(Ms):
    """digests of Z and g of eval_device (sampled entries for the oracle), Z of a second sequence, eval_batch_device
    of both sequences, and the statistics records of mc_step_device / eval_batch_device next to rato_risk_stats on
    the same Z, at each M"""
    import torch
    from riskaversetrajopt_amd import stats
    res = {}
    us = swerve(EVAL_S)
    us2 = us * 0.8 + 0.01
    h = lambda *ts: hashlib.sha256(b"".join(t.contiguous().cpu().numpy().tobytes() for t in ts)).hexdigest()
    for M in Ms:
        d, _ = batch(M, EVAL_S, seed=21)
        Z, _, g = d.eval_device(us, want_g=True)
        Z = Z.clone()
        Z2 = d.eval_device(us2)[0].clone()
        _, rec = d.mc_step_device(us)
        Zb, recb = d.eval_batch_device(np.stack([us, us2]))
        ref, ref2 = stats.risk_stats_device(Z, d.alpha), stats.risk_stats_device(Z2, d.alpha)
        torch.cuda.synchronize()
        idx = cs.sample_set(M, every=523)
        ti = torch.as_tensor(idx, device=g.device)
        res[str(M)] = {"Z1": h(Z), "g": h(g), "Z2": h(Z2), "batch": [h(Zb[0]), h(Zb[1])], "idx": idx.tolist(),
                       "Z_at": Z[ti].tolist(), "g_at": g[:, ti].T.tolist(), "rec": rec.tolist(),
                       "recb": recb.tolist(), "ref": ref.tolist(), "ref2": ref2.tolist()}
    return res


def test_eval_at_the_tiles_switch(tmp_path):
    """M = 2^20 and 2^20 + 1 at S = 40: the tiled eval kernel (forced with RATO_EVAL_TILES_MAX_M above M) and the plain
    one behind the ego prologue (RATO_EVAL_TILES_MAX_M=0; the default above 2^20) give the same Z and g bit for bit,
    both match the fp64 oracle on ~2,000 samples including the last one, eval_batch_device (always tiled) reproduces
    the single calls, and the statistics records are rato_risk_stats' on that Z."""
    import torch
    from riskaversetrajopt_amd import driving
    tiled = run_child(tmp_path, "tiled", {"RATO_EVAL_TILES_MAX_M": str(1 << 22)}, "eval_outputs", EVAL_MS)
    plain = run_child(tmp_path, "plain", {"RATO_EVAL_TILES_MAX_M": "0"}, "eval_outputs", EVAL_MS)
    us = swerve(EVAL_S)
    for M in EVAL_MS:
        a, b = tiled[str(M)], plain[str(M)]
        for k in ("Z1", "g", "Z2"):
            assert a[k] == b[k], ("tiled vs plain eval kernel", M, k)
        for name, v in (("tiled", a), ("plain", b)):
            assert v["batch"] == [v["Z1"], v["Z2"]], ("eval_batch_device row vs the single call", name, M)
            rec, recb, ref, ref2 = (np.asarray(v[k]) for k in ("rec", "recb", "ref", "ref2"))
            for x, y in ((rec, ref), (recb[0], ref), (recb[1], ref2)):
                assert np.array_equal(x[EXACT], y[EXACT]), (name, M, x, y)
                np.testing.assert_allclose(x[SUMS], y[SUMS], rtol=1e-12, atol=1e-300)
        idx = np.asarray(a["idx"])
        assert idx[-1] == M - 1 and len(idx) >= 2000
        dW, x0, ws, wr = driving.sample_uncertain_parameters_device(M, EVAL_S, seed=21)
        ti = torch.as_tensor(idx, device=dW.device)
        m = cs.oracle_model(*host(dW[:, :, ti], x0[:, ti], ws[ti], wr[ti]))
        del dW, x0, ws, wr
        g_o = -m.separation_distances_at_all_times(m.us_to_state_trajectories(us))
        what = f"eval M={M}"
        w = max(cs._check_abs("g", np.asarray(a["g_at"]), g_o, tol.G_RTOL, tol.G_ATOL, idx, what),
                cs._check_abs("Z", np.asarray(a["Z_at"]), g_o.max(axis=1) - ocar.OSQP_TOL, tol.G_RTOL, tol.G_ATOL, idx,
                              what))
        tol.report(f"{what} Z, g vs fp64 ({len(idx)} samples): worst error / limit", w, 1.0)
