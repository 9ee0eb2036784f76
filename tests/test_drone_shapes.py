"""CPU: the drone row kernel's launch-shape table (tests/_drone_shapes.py), its dense fp64 checker and its positional
digest.  The table is pinned on 256 CUs on both sides of every edge of the launcher; the checker accepts outputs built
from the fp64 oracle and rounded to fp32 as the device stores them, and rejects each way a launch structure can deal a
tile, a part or a row task to the wrong samples, naming the sample, tile and lane (or the tile of a ``part`` row)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from oracle import drone as od
from tests import _drone_shapes as ds

# (S, M, factored) -> (form, n_tiles, workgroups, split, n_whole) on 256 CUs, default switches
TABLE = {
    (50, 8192, False): ("split", 128, 256, 2, 0), (50, 8192, True): ("split", 128, 256, 2, 0),
    (50, 8193, False): ("static", 129, 129, 1, 129), (50, 8193, True): ("static", 129, 129, 1, 129),
    (50, 32768, False): ("static", 512, 512, 1, 512), (50, 32769, False): ("queue", 513, 512, 2, 512),
    (50, 32769, True): ("queue", 513, 512, 1, 513),
    (50, 65472, False): ("queue", 1023, 512, 2, 512), (50, 65473, False): ("queue", 1024, 256, 2, 768),
    (50, 100000, False): ("queue", 1563, 256, 2, 1307), (50, 100000, True): ("queue", 1563, 512, 1, 1563),
    (50, 100003, False): ("queue", 1563, 256, 2, 1307),      # the bench's form with a ragged last tile (35 samples)
    (20, 65536, False): ("static", 1024, 1024, 1, 1024), (20, 65537, False): ("queue", 1025, 256, 2, 769),
    (36, 49152, False): ("static", 768, 768, 1, 768), (36, 49153, False): ("queue", 769, 768, 2, 768),
    (90, 16384, False): ("static", 256, 256, 1, 256), (90, 16385, False): ("queue", 257, 256, 2, 256),
    (2, 70000, False): ("queue", 1094, 256, 1, 1094),        # S <= 4: at most one part per tile
}


def graze(S):
    t = np.arange(S)[:, None]
    return np.hstack([0.6 * np.cos(0.3 * t) + 0.3, 0.15 * np.sin(0.5 * t) + 0.02, 0.05 * np.cos(t)]) * (20.0 / S)


@pytest.mark.parametrize("S,M,factored", sorted(TABLE))
def test_shape_table(S, M, factored):
    sh = ds.drone_rows_shape(M, S, factored)
    assert (sh["form"], sh["n_tiles"], sh["workgroups"], sh["split"], sh["n_whole"]) == TABLE[(S, M, factored)]
    assert sh["n_units"] == sh["n_whole"] + (sh["n_tiles"] - sh["n_whole"]) * sh["split"]
    assert sh["stats_in_launch"] == (sh["form"] != "queue")          # the statistics ride in a launch without a queue


def test_every_form_on_both_sides_of_every_edge():
    """cus / 2 (split | static), slots (static | queue) in each band of slots, 1024 tiles (slots | one workgroup per CU
    for the products), the W switch, and S <= 4"""
    forms = {k: v[0] for k, v in TABLE.items()}
    assert forms[(50, 8192, False)] == "split" and forms[(50, 8193, False)] == "static"
    for S, M in ((50, 32768), (20, 65536), (36, 49152), (90, 16384)):
        assert forms[(S, M, False)] == "static" and forms[(S, M + 1, False)] == "queue"
    assert TABLE[(50, 65472, False)][2] == 512 and TABLE[(50, 65473, False)][2] == 256
    assert TABLE[(50, 100000, False)][3:] == (2, 1307) and TABLE[(50, 100000, True)][3:] == (1, 1563)
    assert TABLE[(2, 70000, False)][3] == 1


@pytest.mark.parametrize("S,per_cu", [(20, 4), (31, 4), (32, 3), (42, 3), (43, 2), (63, 2), (64, 1), (126, 1)])
def test_slots_per_horizon(S, per_cu):
    sh = ds.drone_rows_shape(1, S, False)
    assert (sh["per_cu"], sh["slots"]) == (per_cu, 256 * per_cu)


def test_row_kernel_lds_limit_matches_the_library():
    """the LDS formula restated here decides the same S range for the row kernel as rato_drone_linearize_plan"""
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    for S in range(2, 140):
        c, l, t = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        assert lib.rato_drone_linearize_plan(1000, S, 1000, C.byref(c), C.byref(l), C.byref(t)) > 0
        assert (c.value == -1) == (ds.rows_lds_bytes(S) <= ds.LDS_MAX) == (S <= 126), S
    assert ds.rows_lds_bytes(127) == 164100
    with pytest.raises(ValueError):
        ds.drone_rows_shape(1000, 127, False)


BASE = {"RATO_ROWS_DYNAMIC": "0", "RATO_SMALL_SPLIT": "1"}
VARIANTS = {"default": {}, "small3": {"RATO_SMALL_SPLIT": "3"}, "small4": {"RATO_SMALL_SPLIT": "4"},
            "slots1": {"RATO_ROWS_SLOTS_PER_CU": "1"}, "qslots300": {"RATO_ROWS_QSLOTS": "300"},
            "tail1": {"RATO_DYN_TAIL_SPLIT": "1"},
            "tail4_all": {"RATO_DYN_TAIL_SPLIT": "4", "RATO_DYN_TAIL_TILES": "100000"},
            "tail3_one": {"RATO_DYN_TAIL_SPLIT": "3", "RATO_DYN_TAIL_TILES": "1"},
            "qslots_over": {"RATO_ROWS_QSLOTS": "512"}}      # above the 313 tiles of (90, 20001)
CASES = [(50, 10000), (50, 40001), (50, 100003), (20, 70001), (36, 50001), (90, 20001)]


def variant_forms(shape):
    """shape(M, S, factored, env=...) -> a plan: the restatement's, or the library's"""
    def f(name, S, M, fact=False):
        s = shape(M, S, fact, env=BASE if name == "base" else VARIANTS[name])
        return s["form"], s["workgroups"], s["split"], s["n_whole"]
    for S, M in CASES:
        n = (M + 63) // 64
        assert f("base", S, M) == f("base", S, M, True) == ("static", n, 1, n)
    assert f("default", 50, 10000) == f("slots1", 50, 10000) == ("static", 157, 1, 157)
    assert f("small3", 50, 10000) == ("split", 471, 3, 0) and f("small4", 50, 10000, True) == ("split", 628, 4, 0)
    assert f("default", 50, 40001) == ("queue", 512, 2, 512) and f("default", 50, 40001, True) == ("queue", 512, 1, 626)
    assert f("default", 50, 100003) == ("queue", 256, 2, 1307) and f("default", 50, 100003, True) == ("queue", 512, 1, 1563)
    assert f("default", 20, 70001) == ("queue", 256, 2, 838) and f("default", 20, 70001, True) == ("queue", 1024, 1, 1094)
    assert f("default", 36, 50001) == ("queue", 768, 2, 768) and f("default", 36, 50001, True) == ("queue", 768, 1, 782)
    assert f("default", 90, 20001) == ("queue", 256, 2, 256)
    assert f("slots1", 50, 40001) == ("queue", 256, 2, 370) and f("slots1", 36, 50001, True) == ("queue", 256, 1, 782)
    assert f("qslots300", 50, 40001) == ("queue", 300, 2, 326) and f("qslots300", 90, 20001) == ("queue", 300, 2, 300)
    assert f("qslots300", 50, 100003, True) == ("queue", 300, 1, 1563)
    assert f("tail1", 50, 40001) == ("queue", 512, 1, 626) and f("tail1", 50, 100003) == ("queue", 256, 1, 1563)
    assert f("tail4_all", 50, 100003) == ("queue", 256, 4, 256) and f("tail4_all", 50, 100003, True) == ("queue", 512, 4, 512)
    assert f("tail4_all", 20, 70001) == ("queue", 256, 4, 256)
    assert f("tail3_one", 50, 100003) == ("queue", 256, 3, 1562) and f("tail3_one", 90, 20001, True) == ("queue", 256, 3, 312)
    # more queue workgroups than tiles: no tail, every tile whole (unclamped, the launcher ran 114 of the 313 tiles)
    assert f("qslots_over", 90, 20001) == ("queue", 512, 2, 313) and f("qslots_over", 50, 40001) == ("queue", 512, 2, 512)
    assert shape(20001, 90, False, env=VARIANTS["qslots_over"])["n_units"] == 313


def test_variant_forms():
    """what the switches of the GPU bit-identity sweep make of its cases: every form, every band of slots, both sides
    of 1024 tiles, whole tiles / halves / thirds of one tile / quarters of every queued tile at the end of the queue"""
    variant_forms(ds.drone_rows_shape)


@pytest.mark.parametrize("name", ["base"] + sorted(VARIANTS))
@pytest.mark.parametrize("factored", [False, True])
@pytest.mark.parametrize("S,M", CASES)
def test_units_cover_every_row_task_once(name, factored, S, M):
    """the unit -> (tile, part) mapping of every variant: each (tile, row task) exactly once, Z once per tile, each
    axis' rows of ``part`` once per tile"""
    sh = ds.drone_rows_shape(M, S, factored, env=BASE if name == "base" else VARIANTS[name])
    rows = np.zeros((sh["n_tiles"], S), dtype=np.int64)
    zw = np.zeros(sh["n_tiles"], dtype=np.int64)
    axes = np.zeros((sh["n_tiles"], 3), dtype=np.int64)
    for tile, part, rs, writes_Z, ax in ds.units(sh):
        rows[tile, part::rs] += 1
        zw[tile] += writes_Z
        axes[tile, list(ax)] += 1
    assert (rows == 1).all() and (zw == 1).all() and (axes == 1).all()


def test_every_switch_setting_covers_every_tile_once():
    """a grid of batch sizes, horizons, outputs and switch values (RATO_ROWS_QSLOTS and RATO_DYN_TAIL_TILES above and
    below the tile count; slots per CU, small split and tail split 1 ... 8): 0 <= n_whole <= n_tiles and the units
    cover every tile's parts once"""
    seen = set()
    settings = [dict(RATO_ROWS_QSLOTS=q, RATO_DYN_TAIL_TILES=t, RATO_DYN_TAIL_SPLIT=s)
                for q, t, s in itertools.product((0, 1, 100, 300, 512, 5000), (0, 1, 100, 100000), range(0, 9))]
    settings += [dict(RATO_ROWS_SLOTS_PER_CU=c, RATO_SMALL_SPLIT=s, RATO_ROWS_QSLOTS=q)
                 for c, s, q in itertools.product(range(0, 9), range(0, 9), (0, 2000))]
    for M, S, fact in itertools.product((1, 64, 8193, 20001, 40001, 70001), (2, 4, 5, 20, 36, 50, 90, 126), (False, True)):
        for env in settings:
            sh = ds.drone_rows_shape(M, S, fact, env={k: str(v) for k, v in env.items()})
            what = (M, S, fact, env, sh)
            assert 0 <= sh["n_whole"] <= sh["n_tiles"] and sh["n_units"] >= sh["n_tiles"], what
            assert sh["form"] == "queue" or sh["workgroups"] == sh["n_units"], what
            tile, part, rs = ds.unit_table(sh)
            hits = np.zeros((sh["n_tiles"], sh["split"]), dtype=np.int64)
            assert tile.min() >= 0 and tile.max() < sh["n_tiles"], what
            np.add.at(hits, (tile[rs == 1],), 1)                    # a whole tile takes every residue of its row tasks
            np.add.at(hits, (tile[rs > 1], part[rs > 1]), 1)
            assert (hits == 1).all(), what
            assert sh["split"] <= max(1, (S + 3) // 4), what
            seen.add((sh["form"], sh["split"] > 1, sh["n_whole"] == sh["n_tiles"]))
    assert {f for f, _, _ in seen} == {"split", "static", "queue"} and ("queue", True, True) in seen


# ---- the library's own plan (rato_drone_rows_plan: the function the launcher calls) against the restatement ---------
@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def same_plan(lib, M, S, factored, cus=ds.CUS, env=None, have_queue=True):
    """the library's plan, having matched the restatement on every field"""
    got = ds.library_plan(lib, M, S, factored, cus, env, have_queue)
    want = ds.drone_rows_shape(M, S, factored, cus, env, have_queue)
    assert got == {k: want[k] for k in ds.PLAN_FIELDS}, (M, S, factored, cus, env, have_queue)
    return got


def test_table_against_the_library(lib):
    """the pinned tables hold for the C++ that launches, not only for the Python copy: every key of TABLE, the pinned
    variant forms, and every (case, variant) of the bit-identity sweep field by field (the switches passed explicitly)"""
    for (S, M, factored), want in TABLE.items():
        sh = same_plan(lib, M, S, factored)
        assert (sh["form"], sh["n_tiles"], sh["workgroups"], sh["split"], sh["n_whole"]) == want, (S, M, factored)
    variant_forms(lambda M, S, fact, env: ds.library_plan(lib, M, S, fact, env=env))
    for (S, M), env, factored in itertools.product(CASES, [BASE] + list(VARIANTS.values()), (False, True)):
        same_plan(lib, M, S, factored, env=env)
    # switches == NULL: what this process read from its environment; outside the row kernel's range there is no plan
    mine = {k: os.environ[k] for k, _ in ds.SWITCHES if k in os.environ}
    assert ds.library_plan(lib, 100003, 50, False, env="process") == ds.library_plan(lib, 100003, 50, False, env=mine)
    from riskaversetrajopt_amd._lib import RowsPlan
    for M, S in ((1000, 1), (1000, 127), (0, 50)):
        assert lib.rato_drone_rows_plan(M, S, 0, 256, 1, None, C.byref(RowsPlan())) == -1       # RATO_EINVAL


SWEEP_S = (2, 4, 5, 20, 31, 32, 42, 43, 50, 63, 64, 90, 126)
SWEEP_CUS = (256, 64, 304)


def sweep_tiles(cus, slots, qslots):
    ts = {1, 2, cus // 2 - 1, cus // 2, cus // 2 + 1, slots - 1, slots, slots + 1, 1023, 1024, 1025, 2 * slots + 1}
    return sorted(t for t in ts | {q + 1 for q in qslots} if t >= 1)


@pytest.fixture(scope="module")
def sweep(lib):
    """[(M, S, factored, cus, env, have_queue, the library's plan)] on both sides of every edge of the rule: library ==
    restatement on every field, asserted here; pure calls"""
    out = []
    for S, cus, env in itertools.product(SWEEP_S, SWEEP_CUS, [BASE] + list(VARIANTS.values())):
        slots = ds.drone_rows_shape(1, S, False, cus, env)["slots"]
        qslots = {slots, cus} | ({int(env["RATO_ROWS_QSLOTS"])} if "RATO_ROWS_QSLOTS" in env else set())
        for t, factored, have_queue in itertools.product(sweep_tiles(cus, slots, qslots), (False, True), (True, False)):
            for M in (64 * t - 63, 64 * t):
                out.append((M, S, factored, cus, env, have_queue, same_plan(lib, M, S, factored, cus, env, have_queue)))
    return out


def test_edge_sweep_library_equals_restatement(sweep):
    forms = {(p["form"], have_queue) for *_, have_queue, p in sweep}
    assert forms == {("split", True), ("static", True), ("queue", True), ("split", False), ("static", False)}
    assert any(p["wants_queue"] and p["form"] == "static" for *_, p in sweep)          # the pool-exhausted fallback
    assert len(sweep) > 30000


def test_edge_sweep_units_cover_every_tile(sweep):
    """n_units == n_whole + (n_tiles - n_whole) * split with 0 <= n_whole <= n_tiles: what the unclamped tail broke
    (S = 90, M = 20,001 with 512 queue workgroups ran 114 of 313 tiles)"""
    for *what, p in sweep:
        assert 0 <= p["n_whole"] <= p["n_tiles"] and 1 <= p["split"] <= max(1, (what[1] + 3) // 4), (what, p)
        assert p["n_units"] == p["n_whole"] + (p["n_tiles"] - p["n_whole"]) * p["split"] >= p["n_tiles"], (what, p)
        assert p["workgroups"] == (p["qslots"] if p["form"] == "queue" else p["n_units"]), (what, p)


def test_stats_in_launch_is_the_plans_slot_count(lib, sweep):
    """rato_drone_stats_in_launch(M, S) == the tiles fit the slots of the library's plan under default switches and the
    statistics workgroups fit M (without a device the library assumes 256 CUs)"""
    for M, S in sorted({(M, S) for M, S, _, cus, *_ in sweep if cus == 256}):
        p = ds.library_plan(lib, M, S, False, 256)
        want = p["n_tiles"] <= p["slots"] and ds.stats_tail_workgroups(M, ds.NW * 64) > 0
        assert lib.rato_drone_stats_in_launch(M, S) == int(want), (M, S, p)


# ---- the checker on synthetic outputs -------------------------------------------------------------------------------
S, M = 12, 5 * 64 + 3               # 6 tiles, the last one ragged (3 samples)
NAMED = r"sample \d+ \(tile \d+, lane \d+\)"


@pytest.fixture(scope="module")
def batch():
    """a batch in kernel layout (fp32, as the device holds it), the oracle on it, and the outputs an exact kernel would
    store in either representation: the oracle rounded to fp32, untiled [..., M]"""
    DWs, masses, Qs = od.sample_uncertain_parameters(np.random.RandomState(2), 'saa', M=M, S=S)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    Qsym = np.stack([Qs[:, :, 0, 0], Qs[:, :, 0, 1] + Qs[:, :, 1, 0], Qs[:, :, 1, 1]], axis=1)      # (M, 3, n_obs)
    inp = (f32(DWs[:, :, 3:6].transpose(1, 2, 0)), f32(masses), f32(Qsym.transpose(2, 1, 0)))
    us = graze(S)
    ref = ds.reference(*inp, us, want_A22=True, chunk=100)
    return inp, us, ref, device_like(ref)


def device_like(ref):
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    common = {"g_up": f32(ref["g_up"].transpose(1, 2, 0)), "Z": f32(ref["Z"])}
    prod = dict(common, G=f32(ds.pack(ref["G"])))
    fact = dict(common, Phi=f32(ds.pack_phi(ref["Phi"])), W=f32(ref["W"].transpose(1, 2, 3, 0)),
                A22=f32(ref["A22"].transpose(1, 2, 0)))
    rows = ref["final"]
    part = np.stack([rows[t * 64:(t + 1) * 64].sum(axis=0) for t in range((M + 63) // 64)]).astype(np.float32)
    return {"products": prod, "factored": fact, "part": part}


def at(full, idx):
    return {k: v[..., idx] for k, v in full.items()}


def ref_at(ref, idx):
    return {k: v[idx] for k, v in ref.items()}


def copy(d):
    return {k: v.copy() for k, v in d.items()}


def test_exact_outputs_pass(batch):
    inp, us, ref, dev = batch
    idx = ds.sample_set(M)
    assert set(idx // 64) == set(range(6)) and idx[-1] == M - 1 and set(idx % 64) >= {0, 63}
    full = np.arange(M)
    for kind in ("products", "factored"):
        worst = ds.check(at(dev[kind], idx), ref_at(ref, idx), idx, S, "exact " + kind)
        assert max(worst.values()) <= 1.0 and ("A22" in worst) == (kind == "factored")
        ds.check(at(dev[kind], full), ref, full, S, "exact, every sample")
    ds.check_Z(dev["products"]["Z"], ref["Z"], "exact")
    ds.check_part(dev["part"], ref["final"], range(6), "exact")
    ds.check_means(dev["part"].astype(np.float64).sum(axis=0), ref["final"], "exact")
    # the reference is the oracle's: its own tuple, its factors multiply to its Jacobian, A22 is the step its
    # sensitivities take, the full-batch pass gives the same rows and Z
    m = ds.oracle_model(*inp)
    fdu, rhs, _, gdu, gup = m.get_all_constraints_coeffs(us)
    assert np.array_equal(gdu, ref["G"]) and np.array_equal(gup, ref["g_up"])
    assert np.array_equal(ds.products(ref["W"], ref["Phi"]), ref["G"])
    assert np.array_equal(ds.expand(ds.pack(ref["G"]), S), ref["G"])
    assert np.array_equal(ds.expand_phi(ds.pack_phi(ref["Phi"]), S), ref["Phi"])
    sens = m.sensitivities(us, m.us_to_state_trajectories(us))
    for t in range(1, S):                       # d v(t+1) / d u(t-1) = a22_t dt / m
        np.testing.assert_allclose(sens[:, t + 1, :2, t - 1, 1], ref["A22"][:, t] * (m.dt / m.masses)[:, None], rtol=1e-13)
    assert np.array_equal(ref["final"][:, 6 * S:], rhs) and np.array_equal(ref["final"][:, 7 * 6 + 4], fdu[:, 4, 7 * 3 + 1])
    Z, rows = ds.full_batch(*inp, us, chunk=97)
    assert np.array_equal(Z, ref["Z"])
    np.testing.assert_allclose(rows, ref["final"], rtol=1e-13, atol=1e-15)


def tile_cols(t):
    return slice(t * 64, min((t + 1) * 64, M))


def swap_tiles(d):
    a, b = tile_cols(1), tile_cols(3)
    for x in d.values():
        x[..., a], x[..., b] = x[..., b].copy(), x[..., a].copy()


def row_from_neighbour(d):
    t, off = 7, 7 * 6 // 2
    d["G"][off:off + t, ..., tile_cols(2)] = d["G"][off:off + t, ..., tile_cols(3)]
    d["g_up"][:, t, tile_cols(2)] = d["g_up"][:, t, tile_cols(3)]


def ragged_unwritten(d):
    for x in d.values():
        x[..., 320:] = np.nan


def dropped_half(fill):
    def f(d):   # tile 1 dealt as two row-interleaved halves; part 1 (rows 1, 3, 5, ...) never written
        for t in range(1, S, 2):
            off = t * (t - 1) // 2
            d["G"][off:off + t, ..., tile_cols(1)] = fill
            d["g_up"][:, t, tile_cols(1)] = fill
    return f


def shifted_Z(d):
    d["Z"][:-1] = d["Z"][1:].copy()


def phi_from_neighbour(d):
    c = tile_cols(2)
    d["Phi"][..., c] = d["Phi"][..., c.start + 1:c.stop + 1].copy()


MUTANTS = {"swapped tiles": ("products", swap_tiles), "swapped tiles (factored)": ("factored", swap_tiles),
           "row task from the neighbouring tile": ("products", row_from_neighbour),
           "ragged last tile unwritten": ("products", ragged_unwritten),
           "ragged last tile unwritten (factored)": ("factored", ragged_unwritten),
           "dropped half (NaN)": ("products", dropped_half(np.nan)),
           "dropped half (stale zeros)": ("products", dropped_half(0.0)),
           "shifted Z": ("products", shifted_Z),
           "W right, Phi from the neighbouring sample": ("factored", phi_from_neighbour)}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutants_are_rejected(batch, name):
    _, _, ref, dev = batch
    kind, mutate = MUTANTS[name]
    d = copy(dev[kind])
    mutate(d)
    idx = ds.sample_set(M)
    with pytest.raises(AssertionError, match=NAMED):
        ds.check(at(d, idx), ref_at(ref, idx), idx, S, name)


def test_neighbouring_tiles_noise_is_rejected(batch):
    """a noise prefetch aimed at the wrong tile: tile 2 computed on tile 3's noise"""
    inp, us, ref, dev = batch
    dW = inp[0].copy()
    dW[:, :, tile_cols(2)] = inp[0][:, :, tile_cols(3)]
    wrong = device_like(ds.reference(dW, *inp[1:], us, want_A22=True))
    idx = ds.sample_set(M)
    for kind in ("products", "factored"):
        with pytest.raises(AssertionError, match=r"tile 2, lane"):
            ds.check(at(wrong[kind], idx), ref_at(ref, idx), idx, S, "noise of tile 3")
    with pytest.raises(AssertionError, match=r"tile 2, lane"):
        ds.check_Z(wrong["products"]["Z"], ref["Z"], "noise of tile 3")
    with pytest.raises(AssertionError, match=r"tile 2 \(64 valid samples\)"):
        ds.check_part(wrong["part"], ref["final"], range(6), "noise of tile 3")


def test_part_rows_are_checked(batch):
    _, _, ref, dev = batch
    rows = ref["final"]
    # the reduction of the ragged tile let its clamped lanes in: lanes >= M loaded sample M - 1
    p = dev["part"].copy()
    p[5] = (rows[320:].sum(axis=0) + 61 * rows[M - 1]).astype(np.float32)
    with pytest.raises(AssertionError, match=r"tile 5 \(3 valid samples\)"):
        ds.check_part(p, rows, range(6), "clamped lanes")
    # an axis' rows of a parted tile not written by any part (stale zeros, NaN)
    for fill in (0.0, np.nan):
        p = dev["part"].copy()
        p[2, 1:6 * S:3] = fill
        p[2, 6 * S + 1::3] = fill
        with pytest.raises(AssertionError, match=r"tile 2 \(64 valid samples\).*entry 1 \(step 0, p_y\)"):
            ds.check_part(p, rows, range(6), "y rows missing")
    # one sample too few; the rhs of another tile
    p = dev["part"].copy()
    p[0] = rows[:63].sum(axis=0).astype(np.float32)
    with pytest.raises(AssertionError, match=r"tile 0 "):
        ds.check_part(p, rows, range(6), "lane 63 dropped")
    p = dev["part"].copy()
    p[3, 6 * S:] = p[4, 6 * S:]
    with pytest.raises(AssertionError, match=r"tile 3 .*rhs\["):
        ds.check_part(p, rows, range(6), "rhs of tile 4")
    with pytest.raises(AssertionError, match="du_sum / M"):
        ds.check_means(p.astype(np.float64).sum(axis=0) + np.where(np.arange(6 * S + 6) == 4, 1e-2, 0.0), rows, "sums")


# ---- the digest ----------------------------------------------------------------------------------------------------
def test_digest_sees_every_word_and_where_it_lies():
    import torch
    g = torch.Generator().manual_seed(3)
    shape = (6, S * (S - 1) // 2, 2, 3, 64)
    G = torch.randn(shape, generator=g)
    base = ds.digest_G(G, M)
    assert base == ds.digest_G(G.clone(), M, tiles_per_pass=2) and 0 <= base < 1 << 64
    # the 2 MiB-aligned layout: the same tiles with padding between them
    flat = torch.full((6 * (G[0].numel() + 1000),), float("nan"))
    padded = torch.as_strided(flat, shape, (G[0].numel() + 1000,) + G[0].stride())
    padded.copy_(G)
    assert ds.digest_G(padded, M) == base
    # lanes past M of the last tile are nobody's
    H = G.clone()
    H[-1, ..., 3:] = float("nan")
    assert ds.digest_G(H, M) == base
    H = G.clone()
    H[[1, 3]] = G[[3, 1]]
    assert ds.digest_G(H, M) != base                                   # two tiles swapped
    H = G.clone()
    H[2, 40, 1, 2, 17] = -H[2, 40, 1, 2, 17]
    assert ds.digest_G(H, M) != base                                   # one bit of one word
    H = G.clone()
    a, b = H[4, 10, 0, 1, 5].item(), H[4, 10, 0, 1, 6].item()
    H[4, 10, 0, 1, 5], H[4, 10, 0, 1, 6] = b, a
    assert ds.digest_G(H, M) != base                                   # neighbouring lanes exchanged
    # one unit left as it was: a second result in which part 1 of 2 of tile 5 (odd rows) still holds the first
    G2 = torch.randn(shape, generator=g)
    stale = G2.clone()
    for t in range(1, S, 2):
        off = t * (t - 1) // 2
        stale[5, off:off + t] = G[5, off:off + t]
    assert ds.digest_G(stale, M) != ds.digest_G(G2, M)
    H = G.clone()
    H[-1, 0, 0, 0, 2] = 0.0                                            # the last owned lane of the ragged tile
    assert ds.digest_G(H, M) != base
    H = G.clone()
    H[0, 0, 0, 0, 0] = float("nan")
    assert ds.digest_G(H, M) != base
