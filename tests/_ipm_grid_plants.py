"""Shared by test_ipm_grid_plants_cpu.py and test_gpu_ipm_driver_grid_long.py (host only): planted copies of a designed batch
(``_ipm_driver.designed(n, mE, mI, "both")``: every entry has both bounds) in which ONE row of problem 0 (``mu_loop``) alone
decides a scalar of ``rec``, at a row the caller chooses.  With the designed random data the row that decides E0, prim, dual,
the number of mu passes, a_max or a_dual lies wherever the draw put it; a plant puts it into a chosen (block, wave, lane) of the
grid form (csrc/ipm_driver_grid.hip) and, past ``FINISH_WIDTH`` blocks, into a chosen trip of the finishing fold.

A plant leaves the other residuals at their designed size: a changed zl / zu is compensated in J'y (a variable's row:
rz = gradf + J'y - zl + zu) or in y (a slack's row: rs = -y - zl + zu).  The magnitudes were chosen on the host so that every
comparison of the host driver a plant moves stays ``_ipm_driver.MARGIN`` away from its threshold at every position
(test_ipm_grid_plants_cpu.py):

  plant          change at ``pos``                         what the row decides
  hi_L, hi_U     zl (zu) := HI / d, HI = 0.5               E0 = |fl(z d)| = 0.5 (designed products are <= 0.1, residuals 0.05);
                                                           E_mu(0.02) = 0.48 > 0.2: one mu pass instead of two
  lo_L, lo_U     zl (zu) := -LO / d, LO = 2                E0 = |fl(z d)| = 2 through the side's SMALLEST product;
                                                           E_mu(0.1) = 2.1 > 1: no mu pass.  A negative product is what makes the
                                                           smallest one visible: for a positive one |x_min - mu| <= max(x_max, mu)
  nan_L, nan_U   zl (zu) := NaN                            at a variable's row rz is NaN: E0 NaN, status 'line_search'.  At a
                                                           slack's row the host's max(a, b) rules drop the NaN from dual and drop
                                                           the whole SIDE from the complementarity; the problem keeps running.
                                                           That is visible only where the dropped side held the deciding product,
                                                           so at a slack's row the plant stands on the side's hi plant at row
                                                           ``ANCHOR`` (a variable, another lane of block 0) and is compared with
                                                           that state: E0 0.5 -> at most 0.1, one pass -> two
  prim           g[row] := the row's gL (or v) + PRIM      prim = |fl(g - gL)| (|fl(g - v)|) = 7 = E0, no mu pass
  dual_z         J'y[pos] += DUAL (pos < n)                dual = |designed rz + 9| = E0, no mu pass
  dual_s         y[row] += DUAL (an inequality row)        dual = |designed rs - 9| = E0, no mu pass
  a_max          dv[pos] := -STEP dL, STEP = 100           a_max = fl(fl(-tau dL) / dv) ~ tau / 100; the designed steps give >= 0.99
  a_dual         dv[pos] := +STEP dL                       dzl ~ -101 zl: a_dual = fl(fl(-tau zl) / dzl) ~ tau / 101; designed >= 0.49

Positions are rows of the vector a plant lives on (``length``): nv for the multipliers and dv, m for prim and dual_s, n for
dual_z."""
import numpy as np

import _ipm_driver as D

FINISH_WIDTH = 256           # ID_BLOCK: the lanes of the finishing workgroup that fold the per-block partials
HI, LO, PRIM, DUAL, STEP = 0.5, 2.0, 7.0, 9.0, 100.0
ANCHOR = 0
PLANTS = ("hi_L", "hi_U", "lo_L", "lo_U", "nan_L", "nan_U", "prim", "dual_z", "dual_s", "a_max", "a_dual")
SETUP_PLANTS = ("a_max", "a_dual")
# (shape name, plant) of ``cases``, in its order (dual_z lives on the n variables: 5 of them at 'short' and 'long')
PAIRS = [("short", p) for p in PLANTS] + [("long", p) for p in PLANTS if p != "dual_z"] + [("long_n", "dual_z")]


def positions(length, R):
    """the standard rows of a vector of ``length`` entries, R rows to a workgroup: the ends of the four waves' lanes in block 0,
    the seam to block 1, the end of block 1, and past FINISH_WIDTH blocks the last row of block 255, the first of block 256
    (the first partial of lane 0's second trip) and of block 257; the last row"""
    std = [0, 63, 64, 191, 192, R - 1, R, 2 * R - 1]
    if length > FINISH_WIDTH * R:
        std += [FINISH_WIDTH * R - 1, FINISH_WIDTH * R, (FINISH_WIDTH + 1) * R]
    std.append(length - 1)
    out = []
    for p in std:
        if 0 <= p < length and p not in out:
            out.append(p)
    return out


def shapes(R):
    """name -> (n, mE, mI): three blocks with the last one holding one row; FINISH_WIDTH + 2 blocks of nv and nearly as many
    of m; FINISH_WIDTH + 2 blocks of n = nv with m in block 0 (dual_z's positions run over n)"""
    L = (FINISH_WIDTH + 1) * R + 1
    return dict(short=(5, 5, 2 * R + 1 - 5), long=(5, 2, L - 5), long_n=(L, 3, 0))


def chain_shapes(R):
    """[((n, mE, mI), pattern)] for the driver's whole chain past FINISH_WIDTH blocks: nv and m both long; n = nv long and m in
    block 0 only; m alone long with 2 FINISH_WIDTH + 1 blocks -- the residual finish takes three trips there, the setup
    finish one"""
    L = (FINISH_WIDTH + 1) * R + 1
    return [((5, 2, L - 5), "mixed"), ((L, 3, 0), "both"), ((5, 2 * FINISH_WIDTH * R + 1, 3), "none")]


def length(des, plant):
    return des["m"] if plant in ("prim", "dual_s") else des["n"] if plant == "dual_z" else des["n"] + des["nI"]


def cases(R):
    """[(shape name, plant, [positions])]: every plant at every position of the short shape; at the long shapes the rows from
    the last one of block 255 on.  The GPU tests run exactly this list; test_ipm_grid_plants_cpu.py holds every pair of it"""
    out = []
    for name, shape in shapes(R).items():
        des = D.designed(*shape, "both")
        for plant in PLANTS if name != "long_n" else ("dual_z",):
            if plant == "dual_s" and des["nI"] == 0:
                continue
            pos = positions(length(des, plant), R)
            if name != "short":
                pos = [p for p in pos if p >= FINISH_WIDTH * R - 1]
            if pos:
                out.append((name, plant, pos))
    return out


def _set_multiplier(p, JTy, side, i, value):
    """zl (zu) [i] := value, compensated in J'y (i < n) or in the slack's y so that the dual residual keeps its designed size"""
    z = p.zl if side == "L" else p.zu
    delta = (value - z[i]) * (1.0 if side == "L" else -1.0)          # rz and rs hold -zl + zu
    z[i] = value
    if i < p.n:
        JTy[0, i] += delta
    else:
        p.y[np.flatnonzero(p.I)[i - p.n]] -= delta


def planted(des, plant, pos, anchor=False):
    """-> dict(ps, g, JTy, dv, ...): fresh Problems and copies of the designed g, J'y and dv with ``plant`` at row ``pos`` of
    problem 0; the cached ``des`` is not touched.  ``anchor``: the hi plant of the side at row ANCHOR and nothing else -- the
    state a NaN at a slack's row is compared with.  Besides the arrays the dict names what was planted: ``row`` (the constraint
    row whose y or g changed, or None), ``slack`` (pos is a slack's entry), ``z``, ``d`` (the planted side's factors) and
    ``base`` (what g is measured against in prim; the designed residual in dual_*)."""
    assert plant in PLANTS and 0 <= pos < length(des, plant), (plant, pos)
    ps = D.problems(des)
    g, JTy, dv = des["g"].copy(), des["JTy"].copy(), des["dv"].copy()
    p = ps[0]
    n = p.n
    assert np.all(p.hasL & p.hasU), "the plants need both bounds at every entry: pattern 'both'"
    out = dict(ps=ps, g=g, JTy=JTy, dv=dv, plant=plant, pos=pos, row=None, slack=False)
    side = plant[-1]
    dist = lambda i: p.v[i] - p.vL[i] if side == "L" else p.vU[i] - p.v[i]
    if plant[:2] in ("hi", "lo") or plant[:3] == "nan":
        out["slack"] = pos >= n
        if out["slack"]:
            out["row"] = int(np.flatnonzero(p.I)[pos - n])
        if plant[:3] == "nan":
            if out["slack"]:
                assert pos != ANCHOR
                _set_multiplier(p, JTy, side, ANCHOR, HI / dist(ANCHOR))
                out["z"], out["d"] = (p.zl if side == "L" else p.zu)[ANCHOR], dist(ANCHOR)
            if not anchor:
                (p.zl if side == "L" else p.zu)[pos] = np.nan        # nothing to compensate: the residual is NaN
        else:
            assert not anchor
            value = HI / dist(pos) if plant[:2] == "hi" else -LO / dist(pos)
            _set_multiplier(p, JTy, side, pos, value)
            out["z"], out["d"] = value, dist(pos)
    elif plant == "prim":
        out["row"] = pos
        sl = int(np.sum(p.I[:pos]))
        out["base"] = p.v[n + sl] if p.I[pos] else p.model.gL[pos]
        g[0, pos] = out["base"] + PRIM
    elif plant == "dual_z":
        assert pos < n
        out["base"] = (p.sf * p.model.grad_f(p.z) + JTy[0, :n] - p.zl[:n] + p.zu[:n])[pos]
        JTy[0, pos] += DUAL
    elif plant == "dual_s":
        assert p.I[pos], ("dual_s needs an inequality row", pos)
        out["row"] = pos
        i = n + int(np.sum(p.I[:pos]))
        out["base"] = -p.y[pos] - p.zl[i] + p.zu[i]
        p.y[pos] += DUAL
    else:
        dL = p.v[pos] - p.vL[pos]
        dv[0, pos] = -STEP * dL if plant == "a_max" else STEP * dL
        out["d"], out["z"] = dL, p.zl[pos]
    return out


def product(pl):
    """|fl(z d)| of the planted side's factors: what E0 must be, exactly"""
    return abs(np.float64(pl["z"]) * np.float64(pl["d"]))


def prim_value(pl):
    """|fl(g - base)| of the planted row: what prim must be, exactly"""
    return abs(np.float64(pl["g"][0, pl["row"]]) - np.float64(pl["base"]))


def dual_value(pl):
    """what dual must be within 1e-6 (relative): the designed residual moved by DUAL.  The bound is the rounding of the
    designed compensation (g and J'y are set from residuals of 0.05 next to terms of up to 1e6: about 1e-10 relative to 9)
    with four orders of room"""
    return abs(pl["base"] + DUAL) if pl["plant"] == "dual_z" else abs(pl["base"] - DUAL)


def step_value(pl, mu, dzl=None):
    """a_max (a_dual, from the row's ``dzl`` as the driver computed it) of the planted row for the barrier parameter the
    residual phase left: fl(fl(-tau x) / dx), the order of ``ipm._max_step`` and of setup_row"""
    tau = max(0.99, 1.0 - mu)
    if pl["plant"] == "a_max":
        return float(-tau * np.float64(pl["d"]) / np.float64(pl["dv"][0, pl["pos"]]))
    return float(-tau * np.float64(pl["z"]) / np.float64(dzl))
