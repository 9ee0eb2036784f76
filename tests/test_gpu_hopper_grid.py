"""GPU: problems with their own friction fields in one batch -- rato_hopper_slip_f64_fields (csrc/hopper_slip64.hip), the
``fields=`` argument of the hopper facade, both device backends of ``hopper_ipm`` on a group of K = 3 field sets, and the grid
of alphas x resampled terrains end to end (``hopper_ipm.solve_batch``, ``scp.hopper_saa_experiment``).

The property everywhere is bitwise: row k of a K-problem call on fields per problem is the K = 1 call of the shared-fields
entry on a model that holds fields k, and problem k of a batch ends with the (Z, info) of its own ``solve_batch([model])``.
Accuracy is held against the fp64 restatement (tests/_hopper_slip64.reference) per problem at the DEV_TOL = 1e-12 of
tests/test_gpu_hopper_slip_f64.py (relative to each array's max |entry|; measured there 1.3e-14 at worst, the same arithmetic
runs here).  No status is required of a solve; where a problem converged, its solution is checked on its own fields."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import _hopper_ipm as H
import _hopper_nlp as R
import _hopper_slip64 as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEV_TOL = 1e-12                # tests/test_gpu_hopper_slip_f64.py
K3 = 3
ALPHAS = (0.05, 0.2, 0.6)
EINVAL, OK = -1, 0
OUTS = ("h", "dh_dfz", "dh_dx", "Zmax")


def up(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def dev_model(S, M, fields, phases=None, alpha=T.ALPHA, method="saa"):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=fields, phases=phases, precision="f64")


def field_sets(S, M, phases):
    """three different field sets (M, 30) x 3, and Zs (3, nvar), lams (3, ncon) of mixed sign"""
    sets = [T.inputs(S, M, 1, phases, seed=s)[0] for s in range(K3)]
    _, Zs, lams, _ = T.inputs(S, M, K3, phases)
    assert not np.array_equal(sets[0][0], sets[1][0]) and not np.array_equal(sets[1][0], sets[2][0])
    return sets, Zs, lams


def raw_call(m, Zd, lamd, a, th, tau, ldf, K=None, M=None, outs=OUTS, sums=True):
    """rato_hopper_slip_f64_fields itself -> (status, dict of the outputs, NaN where nothing was written)"""
    import torch
    from riskaversetrajopt_amd import _lib, hopper
    K, M = Zd.shape[0] if K is None else K, m.M if M is None else M
    Cn = m.time_jump + m.S - m.time_land
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    shapes = {"h": (Zd.shape[0], Cn, m.M), "dh_dfz": (Zd.shape[0], Cn, m.M), "dh_dx": (Zd.shape[0], Cn, 3, m.M), "Zmax": (Zd.shape[0], m.M)}
    out = {k: nan(*shapes[k]) for k in outs}
    ncon, r0 = m.risk_rows_offset()
    part = D = None
    if lamd is not None and sums:
        part, D = nan(int(m._lib.rato_hopper_slip_f64_nblocks(m.M)), Zd.shape[0], Cn, 3), nan(Zd.shape[0], Cn, 3)
    p = _lib.ptr
    rc = m._lib.rato_hopper_slip_f64_fields(
        C.byref(m._slip_params()), hopper.mu_nom, K, M, p(Zd), Zd.stride(0), p(a), p(th), p(tau), ldf, p(lamd),
        0 if lamd is None else lamd.stride(0), r0 if lamd is not None else 0, *(p(out.get(k)) for k in OUTS), p(part), p(D),
        _lib.current_stream())
    torch.cuda.synchronize()
    out["D"] = D
    return rc, out


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 33, 257])
@pytest.mark.parametrize("S", [1, 6])
def test_fields_per_problem_are_bitwise_the_single_calls(S, M):
    """M = 1: one lane; 2: TI = 2; 33: a padded tile; 257: two sample tiles.  S = 1: C = 1; S = 6: several contact groups.  Every
    phase case, with and without lam."""
    import torch
    from riskaversetrajopt_amd import hopper
    worst = {}
    for phase, phases in T.phase_cases(S).items():
        sets, Zs, lams = field_sets(S, M, phases)
        models = [dev_model(S, M, f, phases) for f in sets]
        m0 = models[0]
        Cn = m0.nlp_layout()["C"]
        stack = hopper.stack_fields_f64(models)
        assert all(t.shape == (K3, 30, M) and t.dtype == torch.float64 and t.is_contiguous() for t in stack)
        Zd = up(Zs)
        for lam in (lams, None):
            lamd = None if lam is None else up(lam)
            got = m0.slip_device_f64(Zd, lamd, fields=stack)
            again = m0.slip_device_f64(Zd, lamd, fields=stack)
            assert set(got) == set(OUTS) | {"D"} and (got["D"] is None) == (lam is None)
            names = OUTS + (("D",) if lam is not None else ())
            for name in names:
                assert same(got[name], again[name]), (phase, name, "a second call")
            # the K = 1 calls of the shared-fields entry on each problem's own fields
            for k, mk in enumerate(models):
                one = mk.slip_device_f64(Zd[k:k + 1], None if lam is None else lamd[k:k + 1])
                for name in names:
                    assert same(got[name][k], one[name][0]), (phase, name, k)
            if Cn == 0:
                assert got["h"].shape == (K3, 0, M) and bool(torch.all(got["Zmax"] == -np.inf))
                continue
            # ldf = 0 is the shared-fields entry (on fields 1, so that a read of the wrong set shows)
            shared = models[1].slip_device_f64(Zd, lamd)
            rc, raw0 = raw_call(m0, Zd, lamd, *models[1].fields_f64(), 0)
            assert rc == OK
            for name in names:
                assert same(raw0[name], shared[name]), (phase, name, "ldf = 0")
            # ldf > 30 M with NaN in the padding
            pad = 7
            wide = [torch.full((K3, 30 * M + pad), float("nan"), dtype=torch.float64, device=DEV) for _ in range(3)]
            for w, t in zip(wide, stack):
                w[:, :30 * M] = t.view(K3, -1)
            rc, rawp = raw_call(m0, Zd, lamd, *wide, 30 * M + pad)
            assert rc == OK
            for name in names:
                assert same(rawp[name], got[name]), (phase, name, "padded ldf")
            # against the restatement, per problem
            if lam is not None:
                host = {name: got[name].cpu().numpy() for name in names}
                host.update(T.split_D(host["D"]))
                for k in range(K3):
                    ref = T.reference(sets[k], Zs[k:k + 1], lams[k:k + 1], np.zeros((1, S + 1, 78)), S, phases)
                    errs = T.errors({name: v[k:k + 1] for name, v in host.items()}, ref)
                    assert set(errs) == {"h", "dh_dfz", "dh_dx", "Zmax", "D1", "D2", "D0"}
                    for name, e in errs.items():
                        worst[name] = max(worst.get(name, 0.0), e)
    print("S", S, "M", M, {k: float("%.3g" % v) for k, v in worst.items()})
    assert worst, "at least one phase case has contacts"
    for name, err in worst.items():
        assert err <= DEV_TOL, (name, err)


def test_nlp_device_with_fields_is_bitwise_the_single_models():
    """the facade above the kernel: every tensor ``nlp_device`` returns, under both folds"""
    from riskaversetrajopt_amd import hopper
    S, M = 6, 33
    phases = T.phase_cases(S)["default"]
    sets, Zs, lams = field_sets(S, M, phases)
    models = [dev_model(S, M, f, phases) for f in sets]
    stack = hopper.stack_fields_f64(models)
    Zd, lamd = up(Zs), up(lams)
    for fold in ("host", "device"):
        batch = models[0].nlp_device(Zd, lamd, fold=fold, fields=stack)
        assert {"slip_h", "slip_rows", "slip_jac_values", "hess_blocks", "jac_values"} <= set(batch)
        for k, mk in enumerate(models):
            one = mk.nlp_device(Zd[k:k + 1], lamd[k:k + 1], fold=fold)
            assert set(one) == set(batch)
            for name, t in batch.items():
                assert same(t[k], one[name][0]), (fold, name, k)
    shared = models[0].nlp_device(Zd, lamd)
    assert same(shared["slip_h"][0], batch["slip_h"][0]) and not same(shared["slip_h"][1], batch["slip_h"][1])


def test_bad_arguments_are_refused():
    """valid device buffers, the status only: RATO_EINVAL, and nothing is written"""
    import torch
    from riskaversetrajopt_amd import hopper
    S, M = 6, 33
    phases = T.phase_cases(S)["default"]
    sets, Zs, lams = field_sets(S, M, phases)
    models = [dev_model(S, M, f, phases) for f in sets]
    m0 = models[0]
    a, th, tau = hopper.stack_fields_f64(models)
    Zd, lamd = up(Zs), up(lams)
    Cn = m0.nlp_layout()["C"]

    def refused(rc, out):
        return rc == EINVAL and all(bool(torch.all(torch.isnan(t))) for t in out.values() if t is not None)
    for ldf in (-1, 1, 30 * M - 1, -30 * M):
        assert refused(*raw_call(m0, Zd, lamd, a, th, tau, ldf)), ldf
        assert refused(*raw_call(m0, Zd, None, a, th, tau, ldf)), ldf
    assert refused(*raw_call(m0, Zd, lamd, a, th, tau, 30 * M, K=0)) and refused(*raw_call(m0, Zd, lamd, a, th, tau, 30 * M, K=65536))
    assert refused(*raw_call(m0, Zd, lamd, a, th, tau, 30 * M, M=0))
    assert refused(*raw_call(m0, Zd, lamd, None, th, tau, 30 * M)) and refused(*raw_call(m0, Zd, lamd, a, None, tau, 30 * M))
    assert refused(*raw_call(m0, Zd, lamd, a, th, None, 30 * M))
    assert refused(*raw_call(m0, Zd, lamd, a, th, tau, 30 * M, sums=False)), "lam without part and D"
    rc, out = raw_call(m0, Zd, lamd, a, th, tau, 30 * M)
    assert rc == OK and not any(bool(torch.any(torch.isnan(t))) for t in out.values()) and Cn > 0
    # the facade refuses before the library is reached
    for bad in ((a, th), (a[:2], th[:2], tau[:2]), (a, th, tau.float()), (a.cpu(), th.cpu(), tau.cpu()),
                (a, th, tau.transpose(1, 2).contiguous().transpose(1, 2))):
        with pytest.raises(ValueError, match="fields"):
            m0.slip_device_f64(Zd, lamd, fields=bad)
        with pytest.raises(ValueError, match="fields"):
            m0.nlp_device(Zd, lamd, fields=bad)


# ---- 2. the backends ----------------------------------------------------------------------------------------------------------
def backend_of(newton):
    from riskaversetrajopt_amd import hopper_arrow, hopper_ipm
    return hopper_ipm.DeviceBackend if newton == "dense" else hopper_arrow.ArrowDeviceBackend


def lower(L):
    """the lower triangles of (K, n, lda) factors, as bytes"""
    L = L.cpu().numpy()
    n = L.shape[1]
    return np.ascontiguousarray(np.tril(L[:, :, :n])).tobytes()


@pytest.mark.parametrize("newton", ["dense", "arrow"])
@pytest.mark.parametrize("S,M", [(2, 4), (6, 65)])
def test_a_group_with_three_field_sets_is_bitwise_three_single_backends(S, M, newton):
    """on device tensors (the whole group) and on lists with idx = [0, 2] (problem 1 has left), against the same calls of the
    three single-model backends, which take the shared-fields path"""
    import torch
    from riskaversetrajopt_amd import hopper_ipm
    phases = T.phase_cases(S)["default"]
    sets, _, _ = field_sets(S, M, phases)
    models = [dev_model(S, M, f, phases, alpha=a) for f, a in zip(sets, ALPHAS)]
    Backend = backend_of(newton)
    be, singles = Backend(models), [Backend([m]) for m in models]
    assert be.fields.stack is not None and all(b.fields.stack is None and b.fields.of([0]) is None for b in singles)
    assert Backend([models[0], dev_model(S, M, sets[0], phases, alpha=0.3)]).fields.stack is None, "shared fields: the shared path"
    st = hopper_ipm.structure(models[0])
    n, ncon = st["n"], st["ncon"]
    rng = np.random.RandomState(5 + S + M)
    Zs = np.stack([R.problem(S, M, k) for k in range(K3)])
    Y = 0.01 * rng.uniform(-1, 1, (K3, ncon))
    X, W = rng.randn(K3, n), rng.randn(K3, ncon)
    d, diag = 10.0 ** rng.uniform(-2, 2, (K3, ncon)), 1e3 * (1.0 + rng.rand(K3, n))
    # ---- on tensors
    Zt, Yt, Xt, Wt, dt, dgt = (up(a) for a in (Zs, Y, X, W, d, diag))
    one = lambda t, k: t[k:k + 1].contiguous()
    calls = (("eval_full_t", lambda b, k: b.eval_full_t(*((Zt, Yt) if k is None else (one(Zt, k), one(Yt, k))))),
             ("eval_g_t", lambda b, k: b.eval_g_t(Zt if k is None else one(Zt, k))),
             ("matvec_t", lambda b, k: b.matvec_t(Xt if k is None else one(Xt, k))),
             ("tmatvec_t", lambda b, k: b.tmatvec_t(Wt if k is None else one(Wt, k))),
             ("factor_t", lambda b, k: b.factor_t(*((dt, dgt) if k is None else (one(dt, k), one(dgt, k))))))
    for name, call in calls:
        got = call(be, None).cpu().numpy()
        for k, bk in enumerate(singles):
            assert got[k].tobytes() == call(bk, k).cpu().numpy()[0].tobytes(), (name, k)
        if name == "factor_t":
            assert not np.any(got), "the designed matrices are positive definite"
            for k, bk in enumerate(singles):
                assert lower(be.L[k:k + 1]) == lower(bk.L), ("L", k)
    assert not same(be.eval_g_t(Zt)[1], singles[0].eval_g_t(one(Zt, 1))[0]), "the fields of problem 1 are not those of problem 0"
    # ---- on lists, problem 1 has left
    idx = [0, 2]
    pick = lambda a: [a[i].copy() for i in idx]
    sfs = [0.5, 0.25, 0.125]
    G = be.eval_full(idx, pick(Zs), pick(Y), [sfs[i] for i in idx])
    G1 = be.eval_g(idx, pick(Zs))
    Jx, JTw = be.matvec(idx, pick(X)), be.tmatvec(idx, pick(W))
    info = be.factor(idx, pick(d), pick(diag))
    sol = be.solve(idx, pick(X))
    assert list(info) == [0, 0]
    for j, i in enumerate(idx):
        bk = singles[i]
        g, = bk.eval_full([0], [Zs[i].copy()], [Y[i]], [sfs[i]])
        g1, = bk.eval_g([0], [Zs[i].copy()])
        jx, = bk.matvec([0], [X[i]])
        jtw, = bk.tmatvec([0], [W[i]])
        assert list(bk.factor([0], [d[i]], [diag[i]])) == [0]
        x, = bk.solve([0], [X[i]])
        for name, a, b in (("eval_full", G[j], g), ("eval_g", G1[j], g1), ("matvec", Jx[j], jx), ("tmatvec", JTw[j], jtw),
                           ("solve", sol[j], x)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (name, i)
        assert lower(be.L[i:i + 1]) == lower(bk.L[0:1]), ("L", i)
    torch.cuda.synchronize()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
GRID_ALPHAS, REPEATS = (0.1, 0.5), 3
CAP = 1000


@functools.lru_cache(maxsize=None)
def grid():
    """the M = 4 baseline's solution at S = 6 and the 2 alphas x 3 repeats of SAA problems on the experiment's draws (computed
    once; do not modify)"""
    from riskaversetrajopt_amd import hopper, hopper_ipm, scp
    S, M = H.S_SMALL, H.M_SMALL
    draws, _ = scp.draw_hopper_saa_fields(REPEATS, M, 16, seed=1)
    base = hopper.Model(M, 'baseline', S=S, fields=draws[0], precision='f64')
    (Zb, ib), = hopper_ipm.solve_batch([base], max_iter=CAP)
    assert ib["status"] == "converged"
    models = [hopper.Model(M, 'saa', a, S=S, fields=draws[r], precision='f64') for a in GRID_ALPHAS for r in range(REPEATS)]
    return dict(draws=draws, Zb=Zb, models=models, fields=[draws[k % REPEATS] for k in range(len(models))],
                Z0s=[H.warm_start(m, Zb) for m in models])


def bitwise(r0, r1):
    (Z0, i0), (Z1, i1) = r0, r1
    keys = ("y", "zl", "zu", "s")
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(i0[k].tobytes() == i1[k].tobytes() for k in keys) and \
        all(i0[k] == i1[k] for k in i0 if k not in keys)


@pytest.mark.parametrize("newton,driver", [("dense", "host"), ("dense", "device"), ("arrow", "device")])
def test_grid_in_one_batch_is_bitwise_the_solo_solves(newton, driver, monkeypatch):
    from riskaversetrajopt_amd import hopper_ipm, ipm
    e = grid()
    seen = []
    inner = ipm.solve_groups

    def spy(groups, *args, **kw):
        seen.append([list(g) for g in groups])
        return inner(groups, *args, **kw)
    monkeypatch.setattr(ipm, "solve_groups", spy)
    kw = dict(max_iter=CAP, newton=newton, driver=driver)
    batch = hopper_ipm.solve_batch(e["models"], e["Z0s"], **kw)
    assert seen == [[list(range(len(e["models"])))]], "one lockstep group"
    for k, (m, Z0) in enumerate(zip(e["models"], e["Z0s"])):
        solo, = hopper_ipm.solve_batch([m], [Z0], **kw)
        got = batch[k]
        print(newton, driver, k, got[1]["status"], got[1]["iterations"], got[1]["factorizations"])
        assert got[1]["status"] == solo[1]["status"] and got[1]["status"] in ipm.STATUSES
        assert bitwise(got, solo), ("the batch differs from the solo run", k)
        if got[1]["status"] == "converged":
            H.check_solution(m, e["fields"][k], *got)
    for r in range(1, REPEATS):                                      # the draws matter
        assert not np.array_equal(batch[0][0], batch[r][0])


def test_experiment_solves_one_saa_group_and_validates_every_solution(tmp_path, monkeypatch):
    from riskaversetrajopt_amd import hopper, ipm, scp
    alphas, R_, S, M, M_mc = (0.1, 0.5), 2, H.S_SMALL, H.M_SMALL, 256
    seen = []
    inner = ipm.solve_groups

    def spy(groups, *args, **kw):
        seen.append([list(g) for g in groups])
        return inner(groups, *args, **kw)
    monkeypatch.setattr(ipm, "solve_groups", spy)
    out = scp.hopper_saa_experiment(num_repeats=R_, alphas=alphas, M=M, S=S, M_mc=M_mc, results_dir=str(tmp_path), max_iter=CAP)
    assert seen == [[[0]], [[0, 1, 2, 3]]], "the baseline once, then exactly one SAA group"
    A = len(alphas)
    assert out["alphas"] == list(alphas) and out["base"]["status"] == "converged" and out["wall_s"] > 0
    assert len(out["results"]) == A and all(len(row) == R_ for row in out["results"])
    for name in ("status", "jump", "safe_fraction", "var", "avar"):
        assert out[name].shape == (A, R_), name
    draws, mc_fields = scp.draw_hopper_saa_fields(R_, M, M_mc, seed=1)
    mc = hopper.Model(M_mc, 'saa', S=S, fields=mc_fields)
    nvar = 8 * (S + 1) + 4 * S + M + 2
    for i, a in enumerate(alphas):
        for r in range(R_):
            Z, xs, us, status, info = out["results"][i][r]
            assert Z.shape == (nvar,) and xs.shape == (S + 1, 8) and us.shape == (S, 4)
            assert status == info["status"] == out["status"][i, r] and out["jump"][i, r] == xs[-1, 0]
            px, forces = mc.contact_inputs(Z)                        # the states and controls lead Z, whatever M
            st = mc.monte_carlo_statistics(px, forces, alpha=a)
            assert out["safe_fraction"][i, r] == st["frac_satisfied"] and 0.0 <= st["frac_satisfied"] <= 1.0
            assert out["var"][i, r] == st["var"] and out["avar"][i, r] == st["cvar"] and st["cvar"] >= st["var"]
            fx, fu = scp.load_results(scp.hopper_saa_result_path(str(tmp_path), a, r), 2)
            assert np.array_equal(fx, xs) and np.array_equal(fu, us)
    assert sorted(os.listdir(str(tmp_path))) == sorted(
        [f"hopper_saa_alpha={a}_repeat={r}_results.npy" for a in alphas for r in range(R_)] + ["hopper_saa_grid_report.npy"])
    rep = scp.load_results(str(tmp_path / scp.HOPPER_SAA_REPORT), len(scp.HOPPER_SAA_REPORT_ARRAYS))
    for name, arr in zip(scp.HOPPER_SAA_REPORT_ARRAYS, rep):
        assert np.array_equal(arr, np.asarray(out[name])), name
