"""GPU: the grid form of the interior-point driver's vector kernels (csrc/ipm_driver_grid.hip) where it pays and in
the parts that decide its scalars.

Past 256 row blocks.  The finishing launches fold the per-block partials with a loop of stride 256 (the finishing workgroup's
width, ``_ipm_grid_plants.FINISH_WIDTH``); R = ``rato_ipm_grid_rows()`` rows make a block, so the loop takes a second trip only
beyond 256 R rows.  L = 257 R + 1 rows are 258 blocks, the last one holding one row.  The driver's whole chain runs there
against the workgroup form byte for byte, as test_gpu_ipm_driver_grid.py runs it at up to three blocks, and one hopper solve
has more than 256 R constraint rows.

Planted extremes (tests/_ipm_grid_plants.py).  E0, prim, dual, the number of mu passes, a_max and a_dual are each decided by
one row, whose value travels through the lane's ``offer`` / ``nanmax`` / ``fmin``, six shuffle steps, four LDS slots, the
partial in ``work`` and the finishing fold.  A plant makes a chosen row decide: the ends of the waves of block 0, the seam to
block 1, the first and the last row of the finishing fold's second trip, the last row.  Each run is the workgroup form's byte
for byte, shows the value the planted row must give (exactly: |fl(z d)|, |fl(g - gL)|, fl(fl(-tau x) / dx)) and differs from
the unplanted run, so that a plant the kernels did not see fails.  The smallest products (``lo_*``) are visible only because
the planted product is negative; the order of equal products (p, e) cannot be seen through ``rec`` at all and stays with
tests/test_ipm_driver_grid_cpu.py.  test_ipm_grid_plants_cpu.py holds the same (plant, position) list on the host driver."""
import functools

import numpy as np
import pytest

import _hopper_ipm as H
import _ipm_driver as D
import _ipm_grid_plants as P
from test_gpu_chol_grid_solvers import hopper_model
from test_gpu_ipm_driver_grid import DEV, PAD, VECS, assert_same_trails, chain, differing, method, raw, rows, up
from test_gpu_ipm_driver_grid_solvers import bitwise

pytestmark = pytest.mark.gpu
EVERYONE = list(range(D.K))


def fields():
    from riskaversetrajopt_amd import _lib
    return {f: i for i, f in enumerate(_lib.IPM_FIELDS)}


@pytest.mark.parametrize("case", range(3), ids=["nv_and_m-mixed", "n-both", "m-none"])
def test_every_phase_past_256_blocks_is_bitwise_the_workgroup_form(case):
    (n, mE, mI), pattern = P.chain_shapes(rows())[case]
    assert max(n + mI, mE + mI) > P.FINISH_WIDTH * rows()
    des = D.designed(n, mE, mI, pattern)
    grid = chain(des, EVERYONE, "grid")
    assert len(grid) == 17
    assert_same_trails("batch", grid, chain(des, EVERYONE, "workgroup"))
    F = fields()
    rec = grid[-1][1]["rec"]
    assert rec[:, F["status"]].tolist() == [-1.0, -1.0, 2.0, 0.0]
    assert rec[0, F["dw"]] == 8.0 * 1e-4 and rec[1, F["dw"]] == 0.0 and np.all(rec[:2, F["trials"]] >= 1.0)
    del grid
    if case == 0:
        assert_same_trails(("solo", D.KINDS[0]), chain(des, [0], "grid"), chain(des, [0], "workgroup"))


# ---- planted extremes ---------------------------------------------------------------------------------------------------------
def residual_phase(des, pl, vec):
    """the residual phase on a planted copy -> the raw state"""
    n, m = des["n"], des["m"]
    st = method().DeviceState(pl["ps"], DEV, ldv=n + des["nI"] + PAD, ldm=m + PAD, vec=vec)
    st.residuals(up(pl["g"], m + PAD), up(pl["JTy"], n + PAD))
    return raw(st)


def to_setup(des, pl, vec):
    """the chain up to the step setup on a planted copy -> the raw state after it"""
    (phase, state), = chain(dict(des, g=pl["g"], JTy=pl["JTy"], dv=pl["dv"]), EVERYONE, vec, ps=pl["ps"], keep={"setup"}, upto="setup")
    assert phase == "setup"
    return state


def both_forms(run, des, pl, what):
    got = {vec: run(des, pl, vec) for vec in VECS}
    assert not differing(got["grid"], got["workgroup"]), (what, differing(got["grid"], got["workgroup"]))
    return got["grid"]


@functools.lru_cache(maxsize=None)
def unplanted_rec(name):
    """problem 0's record of the unplanted batch after the step setup (which leaves E0, prim, dual, the passes and the status
    of the residual phase as they are), the same under both forms: computed once per shape; do not modify"""
    des = D.designed(*P.shapes(rows())[name], "both")
    pl = dict(ps=D.problems(des), g=des["g"], JTy=des["JTy"], dv=des["dv"])
    rec = both_forms(to_setup, des, pl, ("unplanted", name))["rec"][0].copy()
    F = fields()
    assert rec[F["status"]] == -1.0 and rec[F["mu_passes"]] == 2.0 and 0.05 <= rec[F["E0"]] <= 0.1
    assert rec[F["a_max"]] >= 0.99 and rec[F["a_dual"]] >= 0.49
    return rec


@pytest.mark.parametrize("name,plant", P.PAIRS, ids=lambda v: v)
def test_a_planted_row_decides_its_scalar(name, plant):
    R = rows()
    F = fields()
    des = D.designed(*P.shapes(R)[name], "both")
    positions, = [pos for s, p, pos in P.cases(R) if (s, p) == (name, plant)]
    base = unplanted_rec(name)
    anchor = None
    for pos in positions:
        at = (name, plant, pos)
        pl = P.planted(des, plant, pos)
        state = both_forms(to_setup if plant in P.SETUP_PLANTS else residual_phase, des, pl, at)
        rec = state["rec"][0]
        E0, prim, dual, passes, status = (rec[F[k]] for k in ("E0", "prim", "dual", "mu_passes", "status"))
        print(at, "E0 %r prim %r dual %r passes %r status %r a_max %r a_dual %r" % (E0, prim, dual, passes, status, rec[F["a_max"]],
                                                                                 rec[F["a_dual"]]))
        assert state["rec"][1:, F["status"]].tolist() == [-1.0, 2.0, 0.0], at
        if plant[:2] in ("hi", "lo"):
            assert E0 == P.product(pl) and passes == (1.0 if plant[:2] == "hi" else 0.0) and status == -1.0, at
            assert E0 != base[F["E0"]] and passes != base[F["mu_passes"]], at
        elif plant[:3] == "nan" and not pl["slack"]:
            assert np.isnan(E0) and status == 2.0, at
            assert status != base[F["status"]], at
        elif plant[:3] == "nan":
            if anchor is None:                                       # the side's hi plant at row ANCHOR alone: once per side
                anchor = both_forms(residual_phase, des, P.planted(des, plant, pos, anchor=True), (at, "anchor"))["rec"][0]
                assert anchor[F["E0"]] == P.product(pl) and anchor[F["mu_passes"]] == 1.0 and anchor[F["status"]] == -1.0, at
            assert status == -1.0 and np.isfinite(E0) and E0 < P.HI and passes == 2.0, at
            assert E0 != anchor[F["E0"]] and passes != anchor[F["mu_passes"]], at
        elif plant == "prim":
            assert prim == P.prim_value(pl) and E0 == prim and passes == 0.0 and status == -1.0, at
            assert prim != base[F["prim"]] and E0 != base[F["E0"]] and passes != base[F["mu_passes"]], at
        elif plant[:4] == "dual":
            want = P.dual_value(pl)
            assert abs(dual - want) <= 1e-6 * want and E0 == dual and passes == 0.0 and status == -1.0, at
            assert dual != base[F["dual"]] and E0 != base[F["E0"]] and passes != base[F["mu_passes"]], at
        elif plant == "a_max":
            assert rec[F["a_max"]] == P.step_value(pl, rec[F["mu"]]) and rec[F["alpha"]] == rec[F["a_max"]], at
            assert 10.0 * rec[F["a_max"]] < base[F["a_max"]] and rec[F["mu"]] == base[F["mu"]], at
        else:
            dzl = state["dzl"][0, pos]
            assert dzl < 0.0 and rec[F["a_dual"]] == P.step_value(pl, rec[F["mu"]], dzl), at
            assert 10.0 * rec[F["a_dual"]] < base[F["a_dual"]] and rec[F["mu"]] == base[F["mu"]], at


# ---- a whole solve ------------------------------------------------------------------------------------------------------------
def test_hopper_solve_with_more_than_256_blocks_of_rows():
    """test_gpu_ipm_driver_grid_solvers.test_hopper_solve_with_rows_beyond_one_workgroup with more constraint rows than 256 R:
    S = 30 (the workload's), where a sample brings 21 rows, and the smallest M that reaches the count (one sample less does
    not).  Cut at 3 iterations: whatever the status, the two drivers stop in the same state.
    Why S = 30 and not the S = 6 of that test.  What this test costs is not the solve (3 iterations take 44 ms under
    'device' and 18 ms under 'device_grid' at S = 6) but the host's index lists of ``hopper_ipm.structure``, which hold an
    n x n table: n = M + 12 S + 10, so the fewer rows a sample brings the larger M and the cost.  Measured on one MI355X host
    for the models and their structure: S = 2 (M = 32 745) 29.7 s, S = 3 13.1 s, S = 4 7.5 s, S = 6 (M = 13 085) 4.8 s; fewer
    iterations or a smaller S make it no quicker, a larger S does."""
    from riskaversetrajopt_amd import hopper, hopper_ipm
    S, M = 30, 3097
    flds = H.fields(M)
    models = [hopper_model(S, M, 'saa', a, flds) for a in (0.1, 0.5)]
    st = hopper_ipm.structure(models[0])
    one_less = hopper.Model.host_only(M - 1, method='saa', alpha=0.1, S=S).nlp_layout()["ncon"]
    assert one_less <= P.FINISH_WIDTH * rows() < st["ncon"], (one_less, st["ncon"])
    base = hopper_model(S, M, 'baseline', 0.1, flds)
    Z0s = [H.warm_start(mm, base.initial_guess()) for mm in models]
    kw = dict(newton='arrow', max_iter=3)
    ref = hopper_ipm.solve_batch(models, Z0s, driver='device', **kw)
    got = hopper_ipm.solve_batch(models, Z0s, driver='device_grid', **kw)
    print([(i["status"], i["iterations"], i["factorizations"]) for _, i in ref])
    for k in range(2):
        assert ref[k][1]["iterations"] >= 1
        assert bitwise(got[k], ref[k]), k
