"""CPU: the driving row kernel's launch-shape table (tests/_car_shapes.py) and its dense fp64 checker.  The table is
pinned at S = 20, 40 and 90 on 256 CUs on both sides of every edge; the checker accepts outputs built from the fp64
oracle and rounded to fp32 as the device stores them, and rejects each way a launch structure can deal a tile, a part
or a row task to the wrong samples."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from oracle import driving as ocar
from tests import _car_shapes as cs

# (S, M) -> (form, n_tiles, workgroups, split, stats in launch) on 256 CUs, default switches
TABLE = {
    (40, 16384): ("split", 256, 512, 2, True), (40, 16385): ("static", 257, 257, 1, True),
    (40, 32768): ("static", 512, 512, 1, True), (40, 32769): ("queue", 513, 512, 1, False),
    (40, 125001): ("queue", 1954, 512, 1, False), (40, 10000): ("split", 157, 314, 2, True),
    (20, 32768): ("split", 512, 1024, 2, True), (20, 32769): ("static", 513, 513, 1, True),
    (20, 65536): ("static", 1024, 1024, 1, True), (20, 65537): ("queue", 1025, 512, 1, False),
    (90, 8192): ("split", 128, 256, 2, True), (90, 8193): ("static", 129, 129, 1, True),
    (90, 16384): ("static", 256, 256, 1, True), (90, 16385): ("queue", 257, 256, 1, False),
    (4, 300): ("static", 5, 5, 1, True),                      # S <= 4: at most one part per tile
}


@pytest.mark.parametrize("S,lds,per_cu,slots,qslots", [(20, 32512, 4, 1024, 512), (40, 64832, 2, 512, 512),
                                                        (90, 145632, 1, 256, 256)])
def test_slots_per_horizon(S, lds, per_cu, slots, qslots):
    """S = 40: 16,208 floats of LDS, two workgroups per CU, 512 slots (not the 768 / three per CU that older launcher
    comments measured against)"""
    sh = cs.car_rows_shape(1, S)
    assert (sh["lds_bytes"], sh["per_cu"], sh["slots"], sh["qslots"]) == (lds, per_cu, slots, qslots)


@pytest.mark.parametrize("S,M", sorted(TABLE))
def test_shape_table(S, M):
    sh = cs.car_rows_shape(M, S)
    assert (sh["form"], sh["n_tiles"], sh["workgroups"], sh["split"], sh["stats_in_launch"]) == TABLE[(S, M)]
    assert sh["n_units"] == (sh["n_tiles"] if sh["form"] != "split" else sh["n_tiles"] * sh["split"])


def test_static_range_edges():
    """the one-tile-per-workgroup form covers M = 64 (slots / 2) + 1 ... 64 slots, for S <= 20, S = 40 and S >= 51"""
    for S, lo, hi in ((20, 32769, 65536), (40, 16385, 32768), (51, 8193, 16384), (90, 8193, 16384)):
        assert cs.car_rows_shape(lo - 1, S)["form"] == "split" and cs.car_rows_shape(hi + 1, S)["form"] == "queue"
        assert cs.car_rows_shape(lo, S)["form"] == cs.car_rows_shape(hi, S)["form"] == "static", S


def test_row_kernel_lds_limit_matches_the_library():
    """the LDS formula restated here decides the same S range for the row kernel as rato_car_linearize_plan"""
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    for S in range(2, 112):
        c, t = C.c_int32(0), C.c_int32(0)
        assert lib.rato_car_linearize_plan(1000, S, C.byref(c), C.byref(t)) > 0
        assert (c.value == -1) == (cs.car_rows_lds_bytes(S) <= cs.LDS_MAX), S
    assert cs.car_rows_lds_bytes(101) <= cs.LDS_MAX < cs.car_rows_lds_bytes(102)


BASE = {"RATO_ROWS_DYNAMIC": "0", "RATO_CAR_SMALL_SPLIT": "1"}
VARIANTS = {"default": {}, "small3": {"RATO_CAR_SMALL_SPLIT": "3"}, "small4": {"RATO_CAR_SMALL_SPLIT": "4"},
            "slots1": {"RATO_CAR_SLOTS_PER_CU": "1"}, "tail2": {"RATO_CAR_TAIL_SPLIT": "2"},
            "tail4_all": {"RATO_CAR_TAIL_SPLIT": "4", "RATO_CAR_TAIL_TILES": "100000"},
            "tail3_one": {"RATO_CAR_TAIL_SPLIT": "3", "RATO_CAR_TAIL_TILES": "1"}}
CASES = [(40, 10000), (40, 24577), (40, 125001), (20, 70001), (90, 12289)]


def variant_forms(shape):
    """shape(M, S, env=...) -> a plan: the restatement's, or the library's"""
    f = lambda env, S, M: (lambda s: (s["form"], s["workgroups"], s["split"], s["n_whole"]))(shape(M, S, env=env))
    for S, M in CASES:
        n = (M + 63) // 64
        assert f(BASE, S, M) == ("static", n, 1, 0)
    assert f({}, 40, 10000) == ("split", 314, 2, 0) and f(VARIANTS["small3"], 40, 10000) == ("split", 471, 3, 0)
    assert f(VARIANTS["small4"], 40, 10000) == ("split", 628, 4, 0) and f(VARIANTS["slots1"], 40, 10000) == ("static", 157, 1, 0)
    assert f({}, 40, 24577) == ("static", 385, 1, 0) and f(VARIANTS["slots1"], 40, 24577) == ("queue", 256, 1, 385)
    assert f(VARIANTS["small3"], 40, 24577) == ("split", 1155, 3, 0)
    assert f({}, 40, 125001) == ("queue", 512, 1, 1954) and f(VARIANTS["tail2"], 40, 125001) == ("queue", 512, 2, 1698)
    assert f(VARIANTS["tail4_all"], 40, 125001) == ("queue", 512, 4, 0)
    assert f(VARIANTS["tail3_one"], 40, 125001) == ("queue", 512, 3, 1953)
    assert f(VARIANTS["slots1"], 40, 125001) == ("queue", 256, 1, 1954)
    assert f({}, 20, 70001) == ("queue", 512, 1, 1094) and f(VARIANTS["tail2"], 20, 70001) == ("queue", 512, 2, 838)
    assert f({}, 90, 12289) == ("static", 193, 1, 0) and f(VARIANTS["small3"], 90, 12289) == ("split", 579, 3, 0)


def test_variant_forms():
    """what the switches of the GPU bit-identity test make of its cases: every form and every tail shape is run"""
    variant_forms(cs.car_rows_shape)


@pytest.mark.parametrize("name", ["base"] + sorted(VARIANTS))
@pytest.mark.parametrize("S,M", CASES)
def test_units_cover_every_row_task_once(name, S, M):
    """the unit -> (tile, part) mapping of every variant: each (tile, row task) exactly once, Z once per tile"""
    sh = cs.car_rows_shape(M, S, env=BASE if name == "base" else VARIANTS[name])
    rows = np.zeros((sh["n_tiles"], S), dtype=np.int64)
    zw = np.zeros(sh["n_tiles"], dtype=np.int64)
    for tile, part, rs in cs.units(sh):
        rows[tile, part::rs] += 1
        zw[tile] += (S % rs) == part
    assert (rows == 1).all() and (zw == 1).all()


# ---- the library's own plan (rato_car_rows_plan: the function the launcher calls) against the restatement -----------
@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def same_plan(lib, M, S, cus=cs.CUS, env=None, have_queue=True):
    """the library's plan, having matched the restatement on every field"""
    got = cs.library_plan(lib, M, S, cus, env, have_queue)
    want = cs.car_rows_shape(M, S, cus, env, have_queue)
    assert got == {k: want[k] for k in cs.PLAN_FIELDS}, (M, S, cus, env, have_queue)
    return got


def test_table_against_the_library(lib):
    """the pinned tables hold for the C++ that launches, not only for the Python copy: every key of TABLE, the pinned
    variant forms, and every (case, variant) of the bit-identity test field by field (the switches passed explicitly)"""
    for (S, M), want in TABLE.items():
        sh = same_plan(lib, M, S)
        assert (sh["form"], sh["n_tiles"], sh["workgroups"], sh["split"]) == want[:4], (S, M)
        assert lib.rato_car_stats_in_launch(M, S) == int(want[4]), (S, M)
    variant_forms(lambda M, S, env: cs.library_plan(lib, M, S, env=env))
    for (S, M), env in itertools.product(CASES, [BASE] + list(VARIANTS.values())):
        same_plan(lib, M, S, env=env)
    # switches == NULL: what this process read from its environment; outside the row kernel's range there is no plan
    mine = {k: os.environ[k] for k, _ in cs.SWITCHES if k in os.environ}
    assert cs.library_plan(lib, 125001, 40, env="process") == cs.library_plan(lib, 125001, 40, env=mine)
    from riskaversetrajopt_amd._lib import RowsPlan
    for M, S in ((1000, 1), (1000, 102), (0, 40)):
        assert lib.rato_car_rows_plan(M, S, 256, 1, None, C.byref(RowsPlan())) == -1              # RATO_EINVAL


SWEEP_S = (2, 4, 5, 20, 33, 34, 40, 50, 51, 90, 101)
SWEEP_CUS = (256, 64, 304)


@pytest.fixture(scope="module")
def sweep(lib):
    """[(M, S, cus, env, have_queue, the library's plan)] on both sides of every edge of the rule: library ==
    restatement on every field, asserted here; pure calls"""
    out = []
    for S, cus, env in itertools.product(SWEEP_S, SWEEP_CUS, [BASE] + list(VARIANTS.values())):
        sh = cs.car_rows_shape(1, S, cus, env)
        slots, qslots = sh["slots"], sh["qslots"]
        ts = {1, 2, cus // 2 - 1, cus // 2, cus // 2 + 1, slots - 1, slots, slots + 1, 1023, 1024, 1025, qslots + 1,
              2 * slots + 1}
        for t, have_queue in itertools.product(sorted(t for t in ts if t >= 1), (True, False)):
            for M in (64 * t - 63, 64 * t):
                out.append((M, S, cus, env, have_queue, same_plan(lib, M, S, cus, env, have_queue)))
    return out


def test_edge_sweep_library_equals_restatement(sweep):
    forms = {(p["form"], have_queue) for *_, have_queue, p in sweep}
    assert forms == {("split", True), ("static", True), ("queue", True), ("split", False), ("static", False)}
    assert any(p["wants_queue"] and p["form"] == "static" for *_, p in sweep)          # the pool-exhausted fallback
    assert any(p["form"] == "queue" and p["split"] > 1 and 0 < p["n_whole"] < p["n_tiles"] for *_, p in sweep)
    assert len(sweep) > 10000


def test_edge_sweep_units_cover_every_tile(sweep):
    """n_units == n_whole + (n_tiles - n_whole) * split with 0 <= n_whole <= n_tiles, in every form"""
    for *what, p in sweep:
        assert 0 <= p["n_whole"] <= p["n_tiles"] and 1 <= p["split"] <= max(1, (what[1] + 3) // 4), (what, p)
        assert p["n_units"] == p["n_whole"] + (p["n_tiles"] - p["n_whole"]) * p["split"] >= p["n_tiles"], (what, p)
        assert p["workgroups"] == (p["qslots"] if p["form"] == "queue" else p["n_units"]), (what, p)


def test_stats_in_launch_is_the_plans_slot_count(lib, sweep):
    """rato_car_stats_in_launch(M, S) == the tiles fit the slots of the library's plan under default switches and the
    statistics workgroups fit M (without a device the library assumes 256 CUs)"""
    for M, S in sorted({(M, S) for M, S, cus, *_ in sweep if cus == 256}):
        p = cs.library_plan(lib, M, S, 256)
        want = p["n_tiles"] <= p["slots"] and cs.stats_tail_workgroups(M) > 0
        assert lib.rato_car_stats_in_launch(M, S) == int(want), (M, S, p)


# ---- the checker on synthetic outputs -------------------------------------------------------------------------------
S, M = 12, 5 * 64 + 3               # 6 tiles, the last one ragged (3 samples)


@pytest.fixture(scope="module")
def batch():
    """a batch in kernel layout (fp32, as the device holds it), the oracle on it, and outputs an exact kernel would
    store: the oracle rounded to fp32, untiled [..., M]"""
    x0, ws, wr, DWs = ocar.sample_uncertain_parameters(np.random.RandomState(2), M, 'saa', S)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    inp = (f32(DWs[:, :, 6:8].transpose(1, 2, 0)), f32(x0[:, 4:8].T), f32(ws), f32(wr))
    us = np.hstack([0.4 * np.cos(0.4 * np.arange(S))[:, None] - 0.2, 0.05 * np.sin(0.35 * np.arange(S))[:, None] + 0.01])
    us = us * (20.0 / S)
    ref = cs.reference(*inp, us, chunk=100)
    dev = {"G": cs.pack(ref["G"]).astype(np.float32), "g_up": ref["g_up"].T.astype(np.float32),
           "Z": ref["Z"].astype(np.float32), "final_du": ref["final_du"].astype(np.float32),
           "final_rhs": ref["final_rhs"].astype(np.float32)}
    return inp, us, ref, dev


def at(full, idx):
    """the checker's view of full outputs: the sample columns idx"""
    return {"G": full["G"][..., idx], "g_up": full["g_up"][:, idx], "Z": full["Z"][idx], "final_du": full["final_du"],
            "final_rhs": full["final_rhs"]}


def ref_at(ref, idx):
    return {"G": ref["G"][idx], "g_up": ref["g_up"][idx], "Z": ref["Z"][idx], "final_du": ref["final_du"],
            "final_rhs": ref["final_rhs"], "amp": ref["amp"][idx]}


def test_exact_outputs_pass(batch):
    _, _, ref, dev = batch
    idx = cs.sample_set(M)
    assert set(idx // 64) == set(range(6)) and idx[-1] == M - 1 and set(idx % 64) >= {0, 63}
    worst = cs.check(at(dev, idx), ref_at(ref, idx), idx, S, "exact")
    assert max(worst.values()) <= 1.0
    full = np.arange(M)
    cs.check(at(dev, full), ref_at(ref, full), full, S, "exact, every sample")
    cs.check_Z(dev["Z"], ref["Z"], "exact")
    m = cs.oracle_model(*batch[0])
    _, Z = m.monte_carlo_separation_constraints_verification(batch[1])
    assert np.array_equal(Z, ref["Z"]) and (ref["amp"] >= 1.0).all()
    assert np.array_equal(cs.expand(cs.pack(ref["G"]), S), ref["G"])


def tile_cols(t):
    return slice(t * 64, min((t + 1) * 64, M))


def swap_tiles(d):
    a, b = tile_cols(1), tile_cols(3)
    for k in ("G", "g_up", "Z"):
        x = d[k]
        x[..., a], x[..., b] = x[..., b].copy(), x[..., a].copy()


def row_from_neighbour(d):
    t, off = 7, 7 * 6 // 2
    d["G"][off:off + t, :, tile_cols(2)] = d["G"][off:off + t, :, tile_cols(3)]
    d["g_up"][t, tile_cols(2)] = d["g_up"][t, tile_cols(3)]


def ragged_unwritten(d):
    for k in ("G", "g_up", "Z"):
        d[k][..., 320:] = np.nan


def dropped_part(fill):
    def f(d):   # tile 1 dealt as 3 row-interleaved parts; part 1 (rows 1, 4, 7, 10) never written
        for t in range(1, S, 3):
            off = t * (t - 1) // 2
            d["G"][off:off + t, :, tile_cols(1)] = fill
            d["g_up"][t, tile_cols(1)] = fill
    return f


def shifted_Z(d):
    d["Z"][:-1] = d["Z"][1:].copy()


MUTANTS = {"swapped tiles": swap_tiles, "row task from the neighbouring tile": row_from_neighbour,
           "ragged last tile unwritten": ragged_unwritten, "dropped part (NaN)": dropped_part(np.nan),
           "dropped part (stale zeros)": dropped_part(0.0), "shifted Z": shifted_Z}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutants_are_rejected(batch, name):
    _, _, ref, dev = batch
    d = {k: v.copy() for k, v in dev.items()}
    MUTANTS[name](d)
    idx = cs.sample_set(M)
    with pytest.raises(AssertionError, match=r"sample \d+ \(tile \d+, lane \d+\)"):
        cs.check(at(d, idx), ref_at(ref, idx), idx, S, name)


def test_neighbouring_tiles_noise_is_rejected(batch):
    """the static form's first-unit noise prefetch aimed at the wrong tile: tile 2 computed on tile 3's noise"""
    inp, us, ref, dev = batch
    dW = inp[0].copy()
    dW[:, :, tile_cols(2)] = inp[0][:, :, 192:256]
    wrong = cs.reference(dW, *inp[1:], us)
    d = {"G": cs.pack(wrong["G"]).astype(np.float32), "g_up": wrong["g_up"].T.astype(np.float32),
         "Z": wrong["Z"].astype(np.float32), "final_du": dev["final_du"], "final_rhs": dev["final_rhs"]}
    idx = cs.sample_set(M)
    with pytest.raises(AssertionError, match=r"tile 2, lane"):
        cs.check(at(d, idx), ref_at(ref, idx), idx, S, "noise of tile 3")
    with pytest.raises(AssertionError):
        cs.check_Z(d["Z"], ref["Z"], "noise of tile 3")


def test_near_contact_factor(batch):
    """amp = max(1, 1 / r_{t+1}) per row: the ego - pedestrian distance at the row's time, from the oracle's trajectories"""
    inp, us, ref, _ = batch
    xs = cs.oracle_model(*inp).us_to_state_trajectories(us)
    r = np.linalg.norm(xs[:, 1:, 0:2] - xs[:, 1:, 4:6], axis=-1)
    assert np.array_equal(ref["amp"], np.maximum(1.0, 1.0 / r))
    assert (ref["amp"] == 1.0).any()


def test_final_rows_are_checked(batch):
    _, _, ref, dev = batch
    idx = cs.sample_set(M)
    for k in ("final_du", "final_rhs"):
        d = dict(dev)
        d[k] = dev[k].copy()
        d[k].flat[1] = np.nan
        with pytest.raises(AssertionError, match=k):
            cs.check(at(d, idx), ref_at(ref, idx), idx, S, "final rows")
