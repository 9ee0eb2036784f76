"""GPU: the obstacle metric and the arg-max of the drone evaluation (rato_drone_eval_metric, rato_drone_eval_batch_metric,
rato_drone_obstacle_constraints_metric; drone_main_plot.py:198-208, :254-269, :633-639, :791-800).

Bit-exact, no tolerance: the quadratic metric through the new entry points against the old ones; the tiled kernel against
the plain one; a batch row against the single call; Z and arg against the device's own g; the rows on the device's own
trajectories against the fused g; the statistics requested in the call against rato_risk_stats on the returned Z.
Against fp64 (tests/_euclid.py, the fixture recorded from the reference's text): g, Z, the satisfied flags and arg within
the bounds written down there.

Shapes (the smallest that reach every branch): M in {1, 63, 64, 65, 257} -- one lane, a wave's edge, a workgroup of four
tiles plus one; S in {1, 16, 17, 33, 65} -- one noise batch, the hand-over of the two buffers at 16 steps, the second pair
of batches, the reload of the control chunk past 64 steps; row stride M rounded up to 4 and M + 8; K in {1, 3}.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _euclid as E
from tests import _tol as tol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD, EUCL = 0, 1
EXACT = [0, 2, 4, 5, 7, 8, 9, 10]          # var, frac_satisfied, max, count_satisfied, rank, count_above, count_at, t_star
SUMS = [1, 3, 6]                           # cvar, mean, tail_sum (fp64 sums: equal to summation order)
SHAPES = [(M, S) for S in E.S_CASES for M in E.M_CASES]


def lds(M):
    return ((M + 3) // 4 * 4, M + 8)


_models = {}


def device_model(S, M, ld):
    """the first M samples of tests/_euclid.py's batch of horizon S in kernel layout with row stride ld; the ld - M padding
    lanes hold NaN (no kernel may read them into a result)"""
    import torch
    from riskaversetrajopt_amd import drone_risk
    key = (S, M, ld)
    if key not in _models:
        b = E.batch(S)
        dW, mass, Qsym, _ = drone_risk.to_soa_inputs(b["DWs"][:M], b["masses"][:M], b["obs_Qs"][:M], 'cuda:0')
        pad = lambda t: torch.cat([t[..., :M], torch.full(t.shape[:-1] + (ld - M,), float("nan"), device=t.device)], dim=-1).contiguous()
        _models.clear()                    # (one resident batch at a time)
        _models[key] = drone_risk.Model.from_device(S, pad(dW), pad(mass), pad(Qsym), 'saa', 0.1, M=M)
    return _models[key]


def us_dev(d, us):
    import torch
    return torch.as_tensor(np.ascontiguousarray(us, dtype=np.float32), device=d.device)


def raw_eval(d, us, metric=None, xs=False, g=False, arg=False, tol_=None, stats=None, in_launch=False):
    """one call of rato_drone_eval (metric None) / rato_drone_eval_metric on fresh NaN / 0x7f filled outputs
    -> dict of [..][:M] views (+ 'rec': the record, with stats = a workspace)"""
    import torch
    from riskaversetrajopt_amd import _lib, stats as rstats
    M, ld, S = d.M, d._mass.numel(), d.S
    f = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=d.device)
    out = {"Z": f(ld), "xs": f(S + 1, 6, ld) if xs else None, "g": f(3, S, ld) if g else None,
           "arg": torch.full((ld,), 0x7f7f7f7f, dtype=torch.int32, device=d.device) if arg else None}
    p = d._params(M, ld)
    if tol_ is not None:
        p.tol = p.tol64 = tol_
    if stats is not None:
        out["rec"] = torch.full((rstats.N_STATS,), float("nan"), dtype=torch.float64, device=d.device)
        rstats.request_in_launch(p, stats, out["rec"], d.alpha, flags=rstats.STATS_IN_LAUNCH if in_launch else 0)
    u = us_dev(d, us)
    head = (_lib.ptr(u), _lib.ptr(d._dW), _lib.ptr(d._mass), _lib.ptr(d._Qsym), _lib.ptr(out["Z"]))
    tail = (_lib.ptr(out["xs"]), _lib.ptr(out["g"]), _lib.current_stream())
    if metric is None:
        assert not arg
        rc = d._lib.rato_drone_eval(C.byref(p), *head, *tail)
    else:
        rc = d._lib.rato_drone_eval_metric(C.byref(p), metric, *head, _lib.ptr(out["arg"]), *tail)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: (v if v is None or k == "rec" else v[..., :M]) for k, v in out.items()}


def raw_batch(d, us_b, metric=None, arg=False, tol_=None):
    import torch
    from riskaversetrajopt_amd import _lib, stats as rstats
    M, ld, K = d.M, d._mass.numel(), len(us_b)
    Z = torch.full((K, ld), float("nan"), dtype=torch.float32, device=d.device)
    a = torch.full((K, ld), 0x7f7f7f7f, dtype=torch.int32, device=d.device) if arg else None
    rec = torch.full((K, rstats.N_STATS), float("nan"), dtype=torch.float64, device=d.device)
    ws = rstats.new_workspace(M, d.device)
    p = d._params(M, ld)
    if tol_ is not None:
        p.tol = p.tol64 = tol_
    u = us_dev(d, np.stack(us_b))
    args = (_lib.ptr(u), _lib.ptr(d._dW), _lib.ptr(d._mass), _lib.ptr(d._Qsym), _lib.ptr(Z), ld, d.alpha,
            float(rstats.SATISFIED_THRESHOLD), _lib.ptr(ws), ws.numel(), _lib.ptr(rec))
    if metric is None:
        rc = d._lib.rato_drone_eval_batch(C.byref(p), K, *args, _lib.current_stream())
    else:
        rc = d._lib.rato_drone_eval_batch_metric(C.byref(p), metric, K, *args, _lib.ptr(a), _lib.current_stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return Z[:, :M], rec, (a[:, :M] if arg else None)


def raw_rows(d, xs_full, metric=None):
    """rato_drone_obstacle_constraints[_metric] on trajectories [S+1][6][ld]"""
    import torch
    from riskaversetrajopt_amd import _lib
    M, ld = d.M, d._mass.numel()
    g = torch.full((3, d.S, ld), float("nan"), dtype=torch.float32, device=d.device)
    p = d._params(M, ld)
    if metric is None:
        rc = d._lib.rato_drone_obstacle_constraints(C.byref(p), _lib.ptr(xs_full), _lib.ptr(d._Qsym), _lib.ptr(g),
                                                    _lib.current_stream())
    else:
        rc = d._lib.rato_drone_obstacle_constraints_metric(C.byref(p), metric, _lib.ptr(xs_full), _lib.ptr(d._Qsym),
                                                           _lib.ptr(g), _lib.current_stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return g[..., :M]


def full_rows(d, xs_view):
    """[S+1][6][:M] view -> a contiguous [S+1][6][ld] buffer (padding NaN)"""
    import torch
    ld = d._mass.numel()
    full = torch.full(tuple(xs_view.shape[:-1]) + (ld,), float("nan"), dtype=torch.float32, device=d.device)
    full[..., :d.M] = xs_view
    return full


def same(a, b):
    import torch
    return torch.equal(a, b)


def dev_first_argmax(g):
    """the arg-max rule on the device's own g [3][S][M] (fp32, exact)"""
    return E.first_argmax(g.permute(2, 0, 1).cpu().numpy())


@pytest.mark.parametrize("M,S", SHAPES)
def test_quadratic_metric_through_the_new_entries_is_the_old_entries(M, S):
    for ld in lds(M):
        d = device_model(S, M, ld)
        for name, us in E.test_controls(S).items():
            for plain in (False, True):                               # the tiled kernel (no xs) / the plain one
                old = raw_eval(d, us, None, xs=plain, g=True)
                for want_arg in (False, True):
                    new = raw_eval(d, us, QUAD, xs=plain, g=True, arg=want_arg)
                    assert same(new["Z"], old["Z"]) and same(new["g"], old["g"]), (ld, name, plain, want_arg)
                    if plain:
                        assert same(new["xs"], old["xs"])
                    if want_arg:
                        assert np.array_equal(new["arg"].cpu().numpy(), dev_first_argmax(old["g"]))
            xs = raw_eval(d, us, None, xs=True)["xs"]
            assert same(raw_rows(d, full_rows(d, xs), QUAD), raw_rows(d, full_rows(d, xs), None))
        for K in (1, 3):
            us_b = [E.controls(S, (20.0 / S) * (0.5 + 0.1 * k), 0.1 * k) for k in range(K)]
            Zo, ro, _ = raw_batch(d, us_b, None)
            Zn, rn, an = raw_batch(d, us_b, QUAD, arg=True)
            assert same(Zn, Zo) and same(rn, ro)
            for k in range(K):
                assert same(Zn[k], raw_eval(d, us_b[k], None)["Z"])
                assert np.array_equal(an[k].cpu().numpy(), raw_eval(d, us_b[k], QUAD, arg=True)["arg"].cpu().numpy())


@pytest.mark.parametrize("M,S", SHAPES)
def test_euclidean_metric_is_consistent_with_itself(M, S):
    from riskaversetrajopt_amd import drone_params as P
    for ld in lds(M):
        d = device_model(S, M, ld)
        for (name, us), tol_ in zip(E.test_controls(S).items(), (None, 0.0)):
            t32 = np.float32(P.OSQP_TOL if tol_ is None else tol_)
            tiled = raw_eval(d, us, EUCL, g=True, arg=True, tol_=tol_)
            plain = raw_eval(d, us, EUCL, xs=True, g=True, arg=True, tol_=tol_)
            for k in ("Z", "g", "arg"):
                assert same(tiled[k], plain[k]), (ld, name, k)
            assert same(raw_eval(d, us, EUCL, tol_=tol_)["Z"], tiled["Z"])          # without g, without arg: the same Z
            g = tiled["g"].permute(2, 0, 1).cpu().numpy()                            # (M, 3, S) float32
            Z, arg = tiled["Z"].cpu().numpy(), tiled["arg"].cpu().numpy()
            assert np.array_equal(Z, g.reshape(M, -1).max(axis=1) - t32)
            assert np.array_equal(arg, E.first_argmax(g))
            assert np.array_equal(g.reshape(M, -1)[np.arange(M), arg] - t32, Z)
            # the rows on the trajectories the call returned are the fused rows
            assert same(raw_rows(d, full_rows(d, plain["xs"]), EUCL), plain["g"])
        for K in (1, 3):
            us_b = [E.controls(S, (20.0 / S) * (0.5 + 0.1 * k), 0.1 * k) for k in range(K)]
            Zb, rec, ab = raw_batch(d, us_b, EUCL, arg=True, tol_=0.0)
            Zb2, _, none = raw_batch(d, us_b, EUCL, tol_=0.0)
            assert none is None and same(Zb, Zb2)
            for k in range(K):
                one = raw_eval(d, us_b[k], EUCL, arg=True, tol_=0.0)
                assert same(Zb[k], one["Z"]) and same(ab[k], one["arg"]), (ld, K, k)
            from riskaversetrajopt_amd import stats
            r0 = stats.risk_stats_device(Zb[0].contiguous(), d.alpha).cpu().numpy()
            assert np.array_equal(rec[0].cpu().numpy()[EXACT], r0[EXACT])


@pytest.mark.parametrize("M,S", SHAPES)
def test_euclidean_metric_against_fp64(M, S):
    d = device_model(S, M, lds(M)[0])
    for name, c in E.batch(S)["cases"].items():
        a, g_ref, arg_ref = c["a"][:M], c["g"][:M], c["arg"][:M]
        assert a.min() >= E.A_MIN                                                    # (the condition on the inputs)
        r = raw_eval(d, c["us"], EUCL, xs=True, g=True, arg=True, tol_=0.0)
        g = r["g"].permute(2, 0, 1).double().cpu().numpy()
        Z, arg = r["Z"].double().cpu().numpy(), r["arg"].cpu().numpy()
        err, lim = np.abs(g - g_ref), E.g_bound(a)
        tol.report(f"euclidean g M={M} S={S} {name}: worst err / bound", float((err / lim).max()), 1.0)
        assert not (~(err <= lim)).any(), (name, float((err / lim).max()))
        zlim = E.z_bound(a, arg_ref)
        assert not (~(np.abs(Z - c["Z"][:M]) <= zlim)).any(), name
        tol.assert_satisfied_close(Z <= E.THR, c["Z"][:M], thr=E.THR)
        decided = c["gap"][:M] > zlim
        assert (~decided).mean() <= 0.05
        assert np.array_equal(arg[decided], arg_ref[decided]), name
        xs = r["xs"].permute(2, 0, 1).double().cpu().numpy()
        np.testing.assert_allclose(xs, c["xs"][:M], rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)


@pytest.mark.parametrize("M,S", SHAPES)
def test_statistics_requested_in_the_call(M, S):
    """p->stats_* are honoured as rato_drone_eval honours them: behind the kernel, and with RATO_STATS_IN_LAUNCH in the
    launch of the tiled kernel; the record is rato_risk_stats of the returned Z."""
    from riskaversetrajopt_amd import stats
    d = device_model(S, M, lds(M)[1])
    ws = stats.new_workspace(M, d.device)
    us = E.test_controls(S)["skirt"]
    for metric in (QUAD, EUCL):
        for plain in (False, True):
            for in_launch in (False, True):
                r = raw_eval(d, us, metric, xs=plain, arg=True, stats=ws, in_launch=in_launch)
                want = stats.risk_stats_device(r["Z"].contiguous(), d.alpha).cpu().numpy()
                got = r["rec"].cpu().numpy()
                assert np.array_equal(got[EXACT], want[EXACT]), (metric, plain, in_launch, got, want)
                np.testing.assert_allclose(got[SUMS], want[SUMS], rtol=1e-12, atol=1e-300)
                assert same(r["Z"], raw_eval(d, us, metric, xs=plain)["Z"])
                assert not ws[-32:].view(__import__("torch").int32).cpu().numpy().any()      # the signal words are lowered


def test_a_sample_without_a_comparable_row_reports_minus_one():
    """arg = -1 when no row compared greater than -inf.  A sample whose inputs are all NaN (mass and obstacle matrices: what
    an unwritten, poisoned sample looks like) has only NaN rows under the quadratic metric.  Its Z is what rato_drone_eval
    has always given such a sample: fmaxf skips the NaN rows, so -inf, not NaN (bit for bit the old entry's).  A NaN mass
    ALONE leaves row t = 0 finite (p_1 = p_0 + dt v_0 does not depend on the mass) and arg points at it.  The Euclidean
    metric maps a NaN quadratic form to g = 1 (fmaxf(a, 0) in its definition), so there the sample reads as a collision."""
    import torch
    from riskaversetrajopt_amd import drone_risk
    S, M, bad = 17, 65, 64
    b = E.batch(S)
    us = E.test_controls(S)["through"]
    dW, mass, Qsym, _ = drone_risk.to_soa_inputs(b["DWs"][:M], b["masses"][:M], b["obs_Qs"][:M], 'cuda:0')
    mass[bad] = float("nan")
    d = drone_risk.Model.from_device(S, dW, mass, Qsym, 'saa', 0.1, M=M)
    old = raw_eval(d, us, None, g=True)
    for plain in (False, True):
        r = raw_eval(d, us, QUAD, xs=plain, g=True, arg=True)
        a = r["arg"].cpu().numpy()
        assert 0 <= a[bad] < 3 * S and a[bad] % S == 0                               # a row of step 0
        assert np.array_equal(a, dev_first_argmax(r["g"])) and same(r["Z"], old["Z"])
    Qsym[:, :, bad] = float("nan")
    d = drone_risk.Model.from_device(S, dW, mass, Qsym, 'saa', 0.1, M=M)
    old = raw_eval(d, us, None, g=True)
    for plain in (False, True):
        r = raw_eval(d, us, QUAD, xs=plain, g=True, arg=True)
        a, Z = r["arg"].cpu().numpy(), r["Z"].cpu().numpy()
        assert bool(torch.isnan(r["g"][:, :, bad]).all())
        assert a[bad] == -1 and Z[bad] == -np.inf and same(r["Z"], old["Z"])
        assert (a[:bad] >= 0).all() and np.isfinite(Z[:bad]).all()
        e = raw_eval(d, us, EUCL, xs=plain, g=True, arg=True, tol_=0.0)
        assert e["arg"].cpu().numpy()[bad] == 0 and e["Z"].cpu().numpy()[bad] == 1.0
    Zb, _, ab = raw_batch(d, [us, us], QUAD, arg=True)
    assert (ab[:, bad].cpu().numpy() == -1).all() and (Zb[:, bad].cpu().numpy() == -np.inf).all()


def test_bad_arguments_are_refused():
    from riskaversetrajopt_amd import _lib, drone_risk, drone_utils
    d = device_model(17, 65, 68)
    us = E.test_controls(17)["skirt"]
    p = d._params(d.M, 68)
    args = [_lib.ptr(t) for t in (us_dev(d, us), d._dW, d._mass, d._Qsym)]
    for metric in (-1, 2):
        assert d._lib.rato_drone_eval_metric(C.byref(p), metric, *args, None, None, None, None, _lib.current_stream()) == -1
        assert d._lib.rato_drone_obstacle_constraints_metric(C.byref(p), metric, args[1], args[3], args[1],
                                                             _lib.current_stream()) == -1
    with pytest.raises(ValueError):
        d.eval_device(us, metric='manhattan')
    dW, mass, Q = drone_utils.sample_uncertain_parameters_device(64, 17, seed=3, want_dW=False)
    philox = drone_risk.Model.from_device(17, None, mass, Q, 'saa', 0.1, M=64, noise_seed=3)
    with pytest.raises(ValueError):                                                  # regenerated noise: out of scope
        philox.eval_device(us, metric='euclidean')
    with pytest.raises(ValueError):
        philox.eval_batch_device(np.stack([us, us]), metric='euclidean')
    philox.eval_device(us)                                                           # (the quadratic form still runs)


def test_the_reference_fixture_through_the_facade():
    """tests/golden/ref_drone_main_plot_S20_M16.npz (the reference's own text, executed): rows, maxima, flags, shapes"""
    from riskaversetrajopt_amd import drone_risk
    ref = np.load(os.path.join(ROOT, "tests", "golden", "ref_drone_main_plot_S20_M16.npz"))
    S, M = int(ref["S"]), int(ref["M"])
    d = drone_risk.Model(S, ref["DWs"], ref["masses"], ref["obs_Qs"], 'saa', float(ref["alpha"]))
    a = E.quad_rows(ref["xs"], ref["obs_Qs"])
    assert a.min() >= E.A_MIN
    xs, ok, Z = d.monte_carlo_no_collisions_constraint_verification_euclidean(ref["us"])
    assert xs.shape == (M, S + 1, 6) and ok.shape == (M,) and ok.dtype == bool and Z.shape == (M,)
    np.testing.assert_allclose(xs, ref["xs_mc"], rtol=tol.STATE_RTOL, atol=tol.STATE_ATOL)
    arg_ref = E.first_argmax(ref["g"])
    assert not (~(np.abs(Z - ref["Z"]) <= E.z_bound(a, arg_ref))).any()
    tol.assert_satisfied_close(ok, ref["Z"], thr=E.THR)
    g = d.obstacle_avoidance_constraints_euclidean(ref["xs"], ref["obs_Qs"])          # the reference's name and shapes
    assert g.shape == ref["g"].shape == (M, 3, S)
    # (given trajectories: only the rows' own rounding and the fp32 rounding of xs and Q enter -- inside the same bound)
    assert not (~(np.abs(g - ref["g"]) <= E.g_bound(a))).any()
    g1 = d.obstacle_avoidance_constraints_euclidean(ref["xs"][0], ref["obs_Qs"][0])
    assert g1.shape == (3, S) and np.array_equal(g1, g[0])
    Zd, _, gd, arg = d.eval_device(ref["us"], want_g=True, metric='euclidean', want_arg=True, tol=0.0)
    assert np.array_equal(Zd.double().cpu().numpy(), Z)
    decided = E.top_two_gap(ref["g"]) > E.z_bound(a, arg_ref)
    assert np.array_equal(arg.cpu().numpy()[decided], arg_ref[decided])
    Zb, rec, ab = d.eval_batch_device(np.stack([ref["us"], ref["init_us"]]), metric='euclidean', want_arg=True, tol=0.0)
    assert np.array_equal(Zb[0].double().cpu().numpy(), Z) and np.array_equal(ab[0].cpu().numpy(), arg.cpu().numpy())
    assert np.array_equal(d.initial_guess_us_mat(all_axes=True), ref["init_us"])
    assert np.array_equal(d.initial_guess_us_mat()[:, :2], ref["init_us"][:, :2]) and not d.initial_guess_us_mat()[:, 2].any()
