"""CPU: the designed inputs of tests/_cut_designs.py are what they claim to be, before anything is launched.

For every design (a) the expected outputs are right -- the fp64 oracle's dense rows give them exactly, or the closed form
does -- and (b) each mistake the design is aimed at changes an arg-max row (an integer) or moves m by at least 1000
tolerances, the tolerance being the 2^-24 |m| a correct kernel is entitled to.  The mistakes: a dropped last step, the
remainder batch (or its second half) skipped, a clamped load consumed, >= for >, the largest in place of the smallest row,
a control of step S - 1 entering a row, the sign of the base lost, a table read in the other layout."""
import numpy as np
import pytest

from tests import _cut_designs as cd

# every class of S mod 16: S = 1, a short remainder, the second batch empty / with exactly one step, no remainder
S_STILL = [1, 2, 8, 9, 16, 17, 25]


def _tol(m):
    return cd.EPS32 * np.abs(m)


def _noticed(m_ok, a_ok, m_bad, a_bad):
    with np.errstate(invalid="ignore"):
        return bool(np.any(a_ok != a_bad) or np.any(np.abs(m_bad - m_ok) >= 1000.0 * _tol(m_ok)))


def _variants(d):
    return {"zero": (d.uk0, d.x0), "last": (d.uk_last, d.x_last), "step": (d.uk0, d.x_step)}


# ---- the references themselves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 9, 20])
def test_direct_restatements_agree_with_the_oracle(S):
    from oracle import drone as od, driving as ocar
    M = 12
    rng = np.random.RandomState(S)
    smp = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(1), 'saa', M=M, S=S)]
    c = cd.drone_const(S)
    uk, x = cd.r32(0.5 * rng.randn(S, 3)), 0.3 * rng.randn(S, 3)
    a, b = cd.drone_dense(c, smp, uk, x, chunk=5), cd.drone_direct(c, smp, uk, x)
    ld = cd.drone_direct(c, smp, uk, x, dtype=np.longdouble)
    for k in ("rows", "g", "g_up", "W", "e22", "Z", "fdu", "rhs"):
        scale = max(1.0, np.abs(a[k]).max())
        assert np.abs(a[k] - b[k]).max() <= 1e-11 * scale, k
        assert np.abs(a[k] - ld[k].astype(np.float64)).max() <= 1e-11 * scale, k
    # the documented rounding of the e22 table reaches g_up and the final rows, and nothing else
    r = cd.drone_direct(c, smp, uk, x, round_e22=True)
    assert all(np.array_equal(r[k], b[k]) for k in ("rows", "g", "W", "e22", "Z"))
    assert np.abs(r["g_up"] - b["g_up"]).max() <= 1e-6 * max(1.0, np.abs(b["g_up"]).max())
    smp = [cd.r32(v) for v in ocar.sample_uncertain_parameters(np.random.RandomState(2), M, 'saa', S)]
    cc = cd.car_const(S)
    uk, x = 0.2 * rng.randn(S, 2) * np.array([1.0, 0.05]), 0.3 * rng.randn(S, 2) * np.array([1.0, 0.05])
    a = cd.car_dense(cc, smp, uk, x, chunk=5)["rows"]
    for dtype in (np.float64, np.longdouble):
        assert np.abs(a - cd.car_direct(cc, smp, uk, x, dtype=dtype).astype(np.float64)).max() <= 1e-11 * max(1.0, np.abs(a).max())


# ---- standing still ------------------------------------------------------------------------------------------------
def _still_rows(system, d, uk, x, **kw):
    if system == "drone":
        return cd.drone_direct(d.const, d.samples, uk, x, **kw)["rows"]
    return cd.car_direct(d.const, d.samples, uk, x, **kw)[:, None, :]


def _still_dense(system, d, uk, x):
    if system == "drone":
        return cd.drone_dense(d.const, d.samples, uk, x)["rows"]
    return cd.car_dense(d.const, d.samples, uk, x)["rows"][:, None, :]


@pytest.mark.parametrize("S", S_STILL)
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_standing_still_expectations_are_the_oracles(system, S):
    d = (cd.drone_still if system == "drone" else cd.car_still)(S, M=24)
    assert len(d.idx) == 8 and d.still[d.idx].sum() >= 7 - (S >= 2)
    R = 3 if system == "drone" else 1
    rows = {k: _still_dense(system, d, uk, x) for k, (uk, x) in _variants(d).items()}
    for k, r in rows.items():
        flat = r.reshape(d.M, R * S)
        m, arg = flat.max(axis=1), flat.argmax(axis=1)         # (argmax: the first, i.e. the smallest, row among equal ones)
        sel = d.idx if k != "step" else d.idx[d.still[d.idx]]
        exp = np.isin(d.idx, sel)
        assert np.array_equal(m[sel], d.m[exp]) and np.array_equal(arg[sel], d.arg[exp]), (k, m[sel], d.m[exp], arg[sel])
        # the kernels' rule restated, and the direct form, say the same
        mm, am = cd.rowmax_model(_still_rows(system, d, *_variants(d)[k]))
        assert np.array_equal(mm[sel], d.m[exp]) and np.array_equal(am[sel], d.arg[exp]), k
    # nothing of step S - 1 enters a row: not one bit of any sample moves
    assert np.array_equal(rows["last"], rows["zero"])
    # x at step s: rows t <= s untouched, every later row of a standing sample at or below the maximum, the best groups'
    # strictly below where the response is not orthogonal to the row
    st = d.idx[d.still[d.idx]]
    assert np.array_equal(rows["step"][:, :, :d.s + 1], rows["zero"][:, :, :d.s + 1])
    later = rows["step"][st][:, :, d.s + 1:]
    assert np.all(later <= d.m[d.still[d.idx]][:, None, None])
    if S - d.s - 1 > 0:
        assert np.any(later < rows["zero"][st][:, :, d.s + 1:])
    # the ties are exact ties: the best two rows of a standing sample are equal whenever it has more than one row
    if R * S > 1:
        srt = np.sort(rows["zero"][st].reshape(len(st), -1), axis=1)
        tied = [k for k in np.array(d.kind)[d.still[d.idx]] if S > 1 or k.startswith("tie")]
        assert (srt[:, -1] == srt[:, -2]).sum() == len(tied)


@pytest.mark.parametrize("S", S_STILL)
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_standing_still_notices_every_mistake(system, S):
    d = (cd.drone_still if system == "drone" else cd.car_still)(S, M=24)
    B = cd.ROLLOUT_BATCH
    rows = _still_rows(system, d, d.uk0, d.x0)[d.idx]
    ok = cd.rowmax_model(rows)
    applies = {">= over t": S > 1, ">= over groups": system == "drone", "largest row": S > 1 or system == "drone",
               "last step dropped": True, "remainder skipped": S % B != 0, "second half skipped": S % B > B // 2}
    for rule in cd.SELECTION_MISTAKES:
        bad = cd.rowmax_model(rows, rule)
        assert _noticed(*ok, *bad) == applies[rule], (rule, ok, bad)
    # a clamped load consumed: the steps behind the guards run on row S - 1 of the noise again
    if S % B:
        E = cd.pad_last(S)
        if system == "drone":
            smp = (cd.repeat_last(d.samples[0], E, 1),) + d.samples[1:]
        else:
            smp = d.samples[:3] + (cd.repeat_last(d.samples[3], E, 1),)
        ext = (cd.drone_direct(d.const, smp, cd.repeat_last(d.uk0, E, 0), cd.repeat_last(d.x0, E, 0))["rows"] if system == "drone"
               else cd.car_direct(d.const, smp, cd.repeat_last(d.uk0, E, 0), cd.repeat_last(d.x0, E, 0))[:, None, :])[d.idx]
        flat = ext.reshape(len(d.idx), -1)
        assert np.array_equal(ext[:, :, :S], rows)
        assert _noticed(*ok, flat.max(axis=1), ok[1] + (flat.max(axis=1) > ok[0])), "clamped load consumed"
    # a control of step S - 1 entering row S - 1
    bad = cd.rowmax_model(_still_rows(system, d, d.uk_last, d.x_last, semi_implicit=True)[d.idx])
    assert _noticed(*ok, *bad), "control of step S - 1 enters a row"


# ---- implicit tables -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 7, 8, 9, 16, 17])
@pytest.mark.parametrize("axes", [2, 3])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_implicit_design_is_exact_and_notices_every_mistake(S, axes, sign):
    d = cd.implicit_design(S, axes, sign)
    args = (d.A22, axes, d.W, d.base, d.mass, d.xs, sign, cd.IMPLICIT_DT, 0.0, d.M)
    rows = cd.implicit_rows(*args)
    assert np.array_equal(rows, d.values) and np.array_equal(cd.implicit_rows(*args, dtype=np.longdouble).astype(np.float64), d.values)
    assert np.array_equal(d.m, cd.r32(d.m)) and set(d.kind) == set(cd.IMPLICIT_KINDS)
    ok = (d.m, d.arg)
    B = cd.IMPLICIT_BATCH
    applies = {">= over t": S > 1, ">= over groups": True, "largest row": True, "last step dropped": True,
               "remainder skipped": S % B != 0, "second half skipped": False}
    for rule in cd.SELECTION_MISTAKES:
        if rule == "second half skipped":            # (this kernel has single batches)
            continue
        assert _noticed(*ok, *cd.rowmax_model(rows, rule, batch=B)) == applies[rule], rule
    # the loop meets (2, 0) before (0, S - 1): a strict > in loop order without the row-index rule keeps the first one met
    i = d.kind.index("order_tie")
    if S > 1:
        assert rows[i, 2, 0] == rows[i, 0, S - 1] == d.m[i] and d.arg[i] == S - 1
    flipped = cd.implicit_rows(d.A22, axes, d.W, d.base, d.mass, d.xs, -sign, cd.IMPLICIT_DT, 0.0, d.M)
    assert _noticed(*ok, *cd.rowmax_model(flipped)), "sign of the base"
    if axes == 3 and S > 2:
        other = cd.implicit_rows(*args, a22_as_stored=True)
        assert _noticed(*ok, *cd.rowmax_model(other)), "1 - a22 read as a22"


# ---- the NaN contract ------------------------------------------------------------------------------------------------
def test_a_nan_row_makes_the_oracles_m_nan():
    S, M, k = 9, 6, 2
    from oracle import drone as od, driving as ocar
    DWs, masses, Q = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S)]
    c = cd.drone_const(S)
    uk, x = np.full((S, 3), 0.1), np.full((S, 3), 0.05)
    ref = cd.drone_dense(c, (DWs, masses, Q), uk, x)["rows"].reshape(M, -1).max(axis=1)
    DWs[k, 0, 3] = np.nan
    with np.errstate(invalid="ignore"):
        m = cd.drone_dense(c, (DWs, masses, Q), uk, x)["rows"].reshape(M, -1).max(axis=1)
        md = cd.drone_direct(c, (DWs, masses, Q), uk, x)["rows"].reshape(M, -1).max(axis=1)
    others = np.arange(M) != k
    assert np.isnan(m[k]) and np.isnan(md[k]) and np.array_equal(m[others], ref[others])
    x0, ws, wr, DW = [cd.r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(0), M, 'saa', S)]
    cc = cd.car_const(S)
    uk, x = np.full((S, 2), 0.01), np.full((S, 2), 0.005)
    ref = cd.car_dense(cc, (x0, ws, wr, DW), uk, x)["rows"].max(axis=1)
    x0[k, 4:6] = x0[k, 0:2]                                  # the pedestrian starts where the ego is: |d| = 0
    m = cd.car_dense(cc, (x0, ws, wr, DW), uk, x)["rows"].max(axis=1)
    assert np.isnan(m[k]) and np.isnan(cd.car_direct(cc, (x0, ws, wr, DW), uk, x).max(axis=1)[k])
    assert np.array_equal(m[others], ref[others])
