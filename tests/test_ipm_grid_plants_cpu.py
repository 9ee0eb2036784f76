"""CPU: the planted extremes of tests/_ipm_grid_plants.py on the HOST driver (``_ipm_driver.host_residual_phase`` /
``host_step_setup``).  Every plant at every position must decide what its table says, exactly where the table says so, and
every comparison the host driver makes on the planted problem must stay ``_ipm_driver.MARGIN`` away from its threshold, so
that no decision of the device driver can flip on rounding.  The (plant, position) pairs that pass here are the ones
test_gpu_ipm_driver_grid_long.py runs on the device: both take them from ``_ipm_grid_plants.cases``."""
import numpy as np
import pytest

import _ipm_driver as D
import _ipm_grid_plants as P

PAIRS = P.PAIRS


def rows():
    from riskaversetrajopt_amd import _lib
    return int(_lib.load().rato_ipm_grid_rows())


def host(des, pl, setup=False, without=None):
    """the host driver on problem 0 of a planted copy -> (p, passes, log).  ``without`` = (side, i): entry i is left out of the
    side's complementarity products"""
    log = D.Log()
    p = pl["ps"][0]
    if without is not None:
        side, i = without
        has = (p.hasL if side == "L" else p.hasU).copy()
        has[i] = False
        setattr(p, "has" + side, has)
    passes = D.host_residual_phase(p, pl["g"][0], pl["JTy"][0], False, log)
    if setup:
        assert not p.done
        p.dv = pl["dv"][0].copy()
        D.host_step_setup(p, des["Hdv"][0][:p.n] + p.sf * p.model.curv * p.dv[:p.n], log)
    return p, passes, log


def unplanted(des):
    return dict(ps=D.problems(des), g=des["g"], JTy=des["JTy"], dv=des["dv"])


def test_the_case_list():
    R = rows()
    listed = P.cases(R)
    assert [(s, p) for s, p, _ in listed] == PAIRS
    L = (P.FINISH_WIDTH + 1) * R + 1
    assert P.shapes(R) == dict(short=(5, 5, 2 * R + 1 - 5), long=(5, 2, L - 5), long_n=(L, 3, 0))
    assert P.positions(2 * R + 1, R) == [0, 63, 64, 191, 192, R - 1, R, 2 * R - 1, 2 * R]
    assert P.positions(L, R) == [0, 63, 64, 191, 192, R - 1, R, 2 * R - 1, 256 * R - 1, 256 * R, 257 * R]
    assert P.positions(5, R) == [0, 4] and P.positions(256 * R, R)[-1] == 256 * R - 1 and len(P.positions(256 * R, R)) == 9
    for s, p, pos in listed:
        des = D.designed(*P.shapes(R)[s], "both")
        if s == "short":
            assert pos == P.positions(P.length(des, p), R)
        else:
            assert pos and min(pos) == 256 * R - 1 and pos == [q for q in P.positions(P.length(des, p), R) if q >= 256 * R - 1]
    by = {(s, p): pos for s, p, pos in listed}
    assert by[("long", "hi_L")] == [256 * R - 1, 256 * R, 257 * R] and by[("long", "prim")] == [256 * R - 1, 256 * R, 257 * R - 3]
    assert by[("long_n", "dual_z")] == [256 * R - 1, 256 * R, 257 * R]


@pytest.mark.parametrize("name", ["short", "long", "long_n"])
def test_the_unplanted_batch_shows_the_designed_values(name):
    des = D.designed(*P.shapes(rows())[name], "both")
    ps = D.problems(des)
    log = D.Log()
    passes = [D.host_residual_phase(p, des["g"][k], des["JTy"][k], False, log) for k, p in enumerate(ps)]
    assert passes == [2, 0, 0, 0] and [p.status for p in ps] == [None, None, "line_search", "converged"]
    p, _, log0 = host(des, unplanted(des), setup=True)
    assert 0.05 <= p.E0 <= 0.1 and p.prim <= 0.05 * (1 + 1e-9) and p.dual <= 0.05 * (1 + 1e-9)
    assert p.a_max >= 0.99 and p.a_dual >= 0.49
    for what, margin in list(log.margins()) + list(log0.margins()):
        assert margin >= D.MARGIN, (what, margin)
    before = [a.tobytes() for a in (des["g"], des["JTy"], des["dv"])] + [s[k].tobytes() for s in des["state"] for k in ("v", "zl", "zu", "y")]
    for plant in P.PLANTS:
        if P.length(des, plant) and not (plant == "dual_s" and des["nI"] == 0):
            pos = P.length(des, plant) - 1
            if plant != "dual_s" or ps[0].I[pos]:
                P.planted(des, plant, pos)
    after = [a.tobytes() for a in (des["g"], des["JTy"], des["dv"])] + [s[k].tobytes() for s in des["state"] for k in ("v", "zl", "zu", "y")]
    assert before == after                                           # a plant never writes into the cached batch


@pytest.mark.parametrize("case", range(3))
def test_the_long_chain_shapes_go_where_the_batch_is_designed_to_go(case):
    """the shapes test_gpu_ipm_driver_grid_long.py runs the whole chain at: two problems end in the residual phase, the mu loop
    fires twice, both running problems end their search within the two rounds"""
    (n, mE, mI), pattern = P.chain_shapes(rows())[case]
    assert max(n + mI, mE + mI) > P.FINISH_WIDTH * rows()
    ps, passes, accepted, log = D.host_chain(D.designed(n, mE, mI, pattern))
    assert [p.status for p in ps] == [None, None, "line_search", "converged"] and passes == [2, 0, 0, 0]
    assert ps[0].dw == 8.0 * 1e-4 and ps[1].dw == 0.0 and sorted(accepted[0] + accepted[1]) == [0, 1]
    for what, margin in log.margins():
        assert margin >= D.MARGIN, (what, margin)


@pytest.mark.parametrize("name,plant", PAIRS, ids=lambda v: v)
def test_a_plant_decides_its_scalar_at_every_position(name, plant):
    R = rows()
    des = D.designed(*P.shapes(R)[name], "both")
    positions, = [pos for s, p, pos in P.cases(R) if (s, p) == (name, plant)]
    base, _, _ = host(des, unplanted(des), setup=plant in P.SETUP_PLANTS)
    for pos in positions:
        at = (name, plant, pos)
        pl = P.planted(des, plant, pos)
        p, passes, log = host(des, pl, setup=plant in P.SETUP_PLANTS)
        if plant[:2] == "hi":
            assert p.E0 == P.product(pl) and abs(p.E0 - P.HI) <= 1e-15 and passes == 1 and p.status is None, at
        elif plant[:2] == "lo":
            assert p.E0 == P.product(pl) and abs(p.E0 - P.LO) <= 1e-15 and passes == 0 and p.status is None, at
            q, passes_without, _ = host(des, P.planted(des, plant, pos), without=(plant[-1], pos))
            assert passes_without == 2 and q.E0 <= 0.1, at           # the planted row alone stopped the loop
        elif plant[:3] == "nan" and not pl["slack"]:
            assert np.isnan(p.E0) and p.status == "line_search" and passes == 0, at
        elif plant[:3] == "nan":
            a, a_passes, a_log = host(des, P.planted(des, plant, pos, anchor=True))
            assert a.E0 == P.product(pl) and abs(a.E0 - P.HI) <= 1e-15 and a_passes == 1 and a.status is None, at
            assert p.status is None and np.isfinite(p.E0) and 0.05 <= p.E0 <= 0.1 and passes == 2, at
            log = D.Log(list(log) + list(a_log))
        elif plant == "prim":
            assert p.prim == P.prim_value(pl) and abs(p.prim - P.PRIM) <= 1e-8 and p.E0 == p.prim and passes == 0, at
            assert p.dual == base.dual, at
        elif plant[:4] == "dual":
            assert abs(p.dual - P.dual_value(pl)) <= 1e-6 * P.dual_value(pl) and p.E0 == p.dual and passes == 0, at
            assert abs(pl["base"]) <= 0.05 * (1 + 1e-9) and p.prim == base.prim, at
        else:
            assert passes == 2 and p.mu == base.mu, at
            dzl = p.dzl[pos]
            if plant == "a_max":
                assert p.a_max == P.step_value(pl, p.mu) and 10.0 * p.a_max < base.a_max, at
            else:
                assert dzl < 0.0 and p.a_dual == P.step_value(pl, p.mu, dzl) and 10.0 * p.a_dual < base.a_dual, at
                ratio = lambda z, dz: np.where(dz < 0.0, -z / np.where(dz < 0.0, dz, 1.0), np.inf)
                others = np.concatenate([np.delete(ratio(p.zl, p.dzl), pos), ratio(p.zu, p.dzu)])
                assert np.min(others) > 10.0 * p.a_dual, at          # the unique minimum, by a factor 10
        if plant[:3] != "nan" and plant not in ("prim",) + P.SETUP_PLANTS and plant[:4] != "dual":
            assert p.prim == base.prim and abs(p.dual - base.dual) <= 1e-6 * base.dual, at    # the compensation held
        assert len(log) > 0 or plant[:3] == "nan"
        for what, margin in log.margins():
            assert margin >= D.MARGIN, (at, what, margin)
