"""GPU: the hopper solve under the interior-point driver on the device (``hopper_ipm.solve_batch(driver='device')``; DESIGN
§7.ah) -- the linear objective term of csrc/ipm_driver.hip, rato_hopper_g_f64 and rato_hopper_block_symv_f64
(csrc/hopper_g.hip), the multiplier fold by rato_scatter_f64, ``hopper_ipm.DeviceBackend`` on device tensors, one Newton step
and the whole solve.

Bounds are Higham's (Accuracy and Stability of Numerical Algorithms, §3.1) as in tests/_ipm_driver.py and
tests/_hopper_ipm_driver.py: a sum of len terms of k roundings each is within gamma_(len + k) sum |terms| of its exact value in
any order, fused or not; references are np.longdouble and take the device's own inputs.  What is a copy, a negation or a chain
of additions in the host's order is held bitwise.  Every array handed to a kernel is padded by three columns of NaN, which must
come back untouched and reach no result."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import _hopper_ipm as H
import _hopper_ipm_driver as HD
import _hopper_nlp as R
import _ipm_driver as D
from _drone_gaussian_ipm import padded
from _hopper_ipm import dense_reference, designed_values, gamma

pytestmark = pytest.mark.gpu
LD = np.longdouble
DEV = "cuda:0"
PAD = 3
ALPHAS = (0.05, 0.2, 0.6)


def up(a, ld=None, dtype=np.float64):
    import torch
    a = np.asarray(a, dtype=dtype)
    return torch.as_tensor(np.ascontiguousarray(a if ld is None else padded(a, ld)), device=DEV)


def nans(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def within(what, got, ref, bound):
    got = np.asarray(got, dtype=np.float64)
    assert not np.any(np.isnan(got)), what
    err, bound = np.abs(got.astype(LD) - ref), np.asarray(bound, dtype=LD)
    assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, LD(1e-4000)))))


@contextlib.contextmanager
def nothing_moves_to_the_host(monkeypatch):
    """inside the block .cpu(), .numpy(), .item() and .tolist() of a tensor raise"""
    import torch
    with monkeypatch.context() as mp:
        for name in ("cpu", "numpy", "item", "tolist"):
            def refuse(self, *a, _name=name, **kw):
                raise AssertionError(f"Tensor.{_name}() inside a call that must stay on the device")
            mp.setattr(torch.Tensor, name, refuse)
        yield


def device_model(S, M, method, phases, alpha=0.2):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=H.fields(M), phases=phases, precision='f64')


# ---- the driver's kernels with a linear objective term ------------------------------------------------------------------------
def raw(st):
    return {k: getattr(st, k).cpu().numpy().copy() for k in st.NV + st.N + st.M + ("diag", "rec")}


def same(a, b, rows_a=None, rows_b=None):
    return all(np.ascontiguousarray(a[k] if rows_a is None else a[k][rows_a]).tobytes() ==
               np.ascontiguousarray(b[k] if rows_b is None else b[k][rows_b]).tobytes() for k in a)


def device_chain(des, sel):
    """every phase of the driver on the device for the problems ``sel`` of the designed batch, the other kernels' results
    replaced by the designed vectors (the chain of test_gpu_ipm_driver.py) -> {name: (raw state, downloaded Problems)}, and the
    trial g of the two rounds"""
    import torch
    from riskaversetrajopt_amd import ipm
    n, m = des["n"], des["m"]
    st = ipm.DeviceState([D.problems(des)[k] for k in sel], DEV, ldv=n + des["nI"] + PAD, ldm=m + PAD)
    pick = lambda a, length: up(np.asarray(a)[sel], length + PAD)
    snaps, gts = {}, []

    def snap(name):
        got = [D.problems(des)[k] for k in sel]
        st.download(got)
        snaps[name] = (raw(st), got)
        return got

    def put(name, a):
        rows = [i for i, k in enumerate(sel) if k < 2]               # the problems that are still running
        if rows:
            getattr(st, name)[rows, :a.shape[1]] = up(np.asarray(a)[[sel[i] for i in rows]])

    snap("start")
    st.residuals(pick(des["g"], m), pick(des["JTy"], n))
    snap("residuals")
    st.newton("rhs", pick(des["JTw"], n))
    for attempt in (1, 2):                                           # problem 0's factorization fails twice: dw = 1e-4, 8e-4
        st.newton("ladder", info=torch.as_tensor([int(k == 0) for k in sel], dtype=torch.int32, device=DEV), flag=attempt)
    put("dz", des["dz0"])
    for r in range(2):
        st.newton("q", pick(des["Jdz"][r], m), flag=r == 0)
        st.newton("r", pick(des["Wdz"][r], n), pick(des["JTq"][r], n))
        put("ez", des["ez"][r])
        st.newton("update", pick(des["Jez"][r], m))
    st.newton("finish", pick(des["Jdz"][2], m))
    put("dv", des["dv"])
    snap("finish")
    st.step_setup(pick(des["Hdv"], n))
    snap("setup")
    factors = dict(des, ct_factor=[f[sel] for f in des["ct_factor"]])
    for r in range(2):
        st.trial()
        got = snap("trial%d" % r)
        gt = D.trial_g(factors, got, r)
        st.accept(up(gt, m + PAD))
        gts.append(gt)
        snap("accept%d" % r)
    return snaps, gts


@pytest.mark.parametrize("shape", HD.SHAPES, ids=lambda s: "n%d_mE%d_mI%d" % s)
def test_driver_phases_with_a_linear_objective_term(shape):
    des = HD.designed_lin(*shape)
    n, m, nI = des["n"], des["m"], des["nI"]
    host, passes, accepted, logs = HD.host_chain(des)
    decided = [HD.decided(log) for log in logs]
    print("decided", decided)
    everyone = list(range(D.K))
    snaps, gts = device_chain(des, everyone)
    again, _ = device_chain(des, everyone)
    solo = [device_chain(des, [k])[0] for k in everyone]
    from riskaversetrajopt_amd import ipm
    for name, (state, _) in snaps.items():
        assert same(state, again[name][0]), ("two runs differ", name)
        for k in everyone:
            assert same(state, solo[k][name][0], [k], [0]), ("the batch differs from the K = 1 launch", name, k)
        for field, a in state.items():
            length = {"diag": n, "rec": a.shape[1]}.get(field, n + nI if field in ipm.DeviceState.NV else
                                                        n if field in ipm.DeviceState.N else m)
            assert np.all(np.isnan(a[:, length:])), (name, field)
    assert snaps["start"][0]["lin"][:, :n].tobytes() == np.stack([mdl.lin for mdl in des["models"]]).tobytes()
    for name in ("finish", "setup", "trial0", "accept0", "trial1", "accept1"):
        assert same(snaps[name][0], snaps["residuals"][0], [2, 3], [2, 3]), ("an ended problem changed", name)

    # ---- residuals: the statuses, the mu passes, gradf, prim, dual, E0, rz
    got = snaps["residuals"][1]
    after = [None, None, "line_search", "converged"]
    for k in everyone:
        p, s = got[k], des["state"][k]
        if decided[k]:
            assert p.status == after[k] and int(p.mu_passes) == passes[k], (k, p.status, p.mu_passes)
        if k == 2:
            assert not np.isfinite(p.E0)
            continue
        for name, (ref, bound) in HD.ref_residuals(p, s, des["g"][k], des["JTy"][k]).items():
            within(("residuals", k, name), getattr(p, name), ref, bound)
        if p.status is None:
            within(("prepare", k, "rz"), p.rz, *HD.ref_rz(p, s, p.mu, des["JTy"][k]))
            assert abs(p.mu - host[k].mu) <= 2 * np.spacing(host[k].mu) or not decided[k]
    running = [k for k in (0, 1) if got[k].status is None]
    assert running == [0, 1] or not all(decided)

    # ---- the step setup: Dbar through gradf, the objective's record, phi, the nu rule
    pre_all, post_all = snaps["finish"][1], snaps["setup"][1]
    for k in running:
        pre, post = pre_all[k], post_all[k]
        within(("setup", k, "Dbar"), post.Dbar, *D.ref_setup(post, pre, des["dv"][k], des["Hdv"][k])["Dbar"])
        within(("setup", k, "objective"), post.objective, *HD.ref_objective(post, pre.v))
        within(("setup", k, "phi"), post.phi, *HD.ref_phi(post))
        if decided[k]:
            assert (post.nu != pre.nu) == (host[k].nu != 0.0), ("the nu rule", k)

    # ---- trial and accept: phi_t, the Armijo decision, the trials
    trials = {k: 0 for k in running}
    for r in range(2):
        before = snaps["setup"][1] if r == 0 else snaps["accept0"][1]
        mid_all, post_all = snaps["trial%d" % r][1], snaps["accept%d" % r][1]
        for k in running:
            if before[k].searching != 1.0:
                continue
            trials[k] += 1
            mid, post = mid_all[k], post_all[k]
            within(("phi_t", r, k), post.phi_t, *HD.ref_phi_t(mid, mid, mid.vt, gts[r][k]))
            assert post.trials == trials[k]
            if decided[k]:
                assert (post.accepted == 1.0) == (k in accepted[r]), ("accept / reject", r, k)
    for k in running:
        if decided[k]:
            assert trials[k] == host[k].trials, (k, trials[k], host[k].trials)


def test_a_model_without_a_linear_term_uploads_zeros():
    from riskaversetrajopt_amd import ipm
    des = D.designed(5, 2, 3, "mixed")
    assert not any(hasattr(mdl, "lin") for mdl in des["models"])
    st = ipm.DeviceState(D.problems(des), DEV, ldv=des["n"] + des["nI"] + PAD)
    lin = st.lin.cpu().numpy()
    assert lin[:, :des["n"]].tobytes() == np.zeros((D.K, des["n"])).tobytes() and np.all(np.isnan(lin[:, des["n"]:]))
    ps = D.problems(des)
    st.download(ps)
    assert not any(hasattr(p, "lin") for p in ps)                    # a constant, like curv: not downloaded


# ---- rato_hopper_g_f64 -----------------------------------------------------------------------------------------------------------
G_CASES = H.map_cases() + [(2, M, 'saa', None) for M in (255, 256, 257)]


def host_only(S, M, method, phases, alpha=0.2):
    from riskaversetrajopt_amd import hopper
    return hopper.Model.host_only(M, method=method, alpha=alpha, S=S, phases=phases)


def call_g(model, pc, rows_of, layout, ld_pad=PAD):
    """rato_hopper_g_f64 for the problems ``rows_of`` of the designed pieces, h in the named layout -> (K, ncon + pad) array"""
    from riskaversetrajopt_amd import hopper
    lay = model.nlp_layout()
    K, Cn, M = len(rows_of), lay["C"], model.M
    sl = lambda a: np.asarray(a)[rows_of]
    h, strides = None, (max(Cn, 1), 1)
    if Cn > 0 and layout == "rows":
        h = up(sl(pc["slip_rows"]))
    elif Cn > 0:
        h, strides = up(sl(pc["slip_rows"]).reshape(K, M, Cn).transpose(0, 2, 1)), (1, M)
    out = nans(K, lay["ncon"] + ld_pad)
    g = hopper.g_device(model._slip_params(), M, model.method != 'baseline', up(sl(pc["Z"]), lay["nvar"] + ld_pad), up(sl(pc["defect"])),
                        up(sl(pc["rows"])), h, strides, up(sl(pc["malpha"])) if model.method != 'baseline' else None, out=out)
    assert g is out
    return out.cpu().numpy()


@pytest.mark.parametrize("S,M,method,phases", G_CASES)
def test_g_on_the_device(S, M, method, phases):
    from riskaversetrajopt_amd import hopper_ipm
    K = len(ALPHAS)
    models = [host_only(S, M, method, phases, a) for a in ALPHAS]
    lay = models[0].nlp_layout()
    ncon, Cn = lay["ncon"], lay["C"]
    pc = HD.g_pieces(models[0], K, 11 + S + 10 * M + (100 if method == 'saa' else 0), ALPHAS)
    want = np.stack([hopper_ipm.assemble_g(models[k], pc["Z"][k], pc["defect"][k], pc["rows"][k],
                                           pc["slip_rows"][k] if Cn > 0 else None) for k in range(K)])
    assert want.shape == (K, ncon)
    keep = np.ones(ncon, dtype=bool)
    if method == 'saa':
        keep[lay["off"]["risk"]] = False                             # the sum row
    everyone = list(range(K))
    got = {layout: call_g(models[0], pc, everyone, layout) for layout in ("rows", "cm")}
    assert got["rows"].tobytes() == got["cm"].tobytes()              # the two h layouts
    g = got["rows"]
    assert np.all(np.isnan(g[:, ncon:]))                             # the padding
    assert np.ascontiguousarray(g[:, :ncon][:, keep]).tobytes() == np.ascontiguousarray(want[:, keep]).tobytes()
    if method == 'saa':
        for k in range(K):
            ref, mag = HD.g_sum_row(models[0], pc["Z"][k], pc["malpha"][k])
            within(("sum row", k), g[k, lay["off"]["risk"]], ref, gamma(M + 2) * mag)
    for k in range(K):
        for layout in ("rows", "cm"):
            assert call_g(models[0], pc, [k], layout).tobytes() == g[k:k + 1].tobytes(), (k, layout)


def test_g_and_block_symv_argument_errors():
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    model = host_only(6, 4, 'saa', None)
    lay = model.nlp_layout()
    K, M, Cn, nvar, ncon, S = 2, 4, lay["C"], lay["nvar"], lay["ncon"], 6
    pc = HD.g_pieces(model, K, 5, ALPHAS[:K])
    Z, defect, rows, h, malpha = up(pc["Z"]), up(pc["defect"]), up(pc["rows"]), up(pc["slip_rows"]), up(pc["malpha"])
    out = nans(K, ncon)
    P, s = _lib.ptr, _lib.current_stream()
    good = model._slip_params()
    bad_phase = type(good).from_buffer_copy(good)
    bad_phase.time_jump, bad_phase.time_land = 4, 2
    no_S = type(good).from_buffer_copy(good)
    no_S.S = 0

    def g(p=good, K=K, M=M, saa=1, Z=Z, ldz=nvar, defect=defect, rows=rows, h=h, si=Cn, sc=1, malpha=malpha, out=out, ldg=ncon):
        return lib.rato_hopper_g_f64(None if p is None else C.byref(p), K, M, saa, P(Z), ldz, P(defect), P(rows), P(h), si, sc,
                                     P(malpha), P(out), ldg, s)
    assert g() == 0 and g(si=1, sc=M) == 0
    bad = [g(p=None), g(p=bad_phase), g(p=no_S), g(K=0), g(K=65536), g(M=0), g(Z=None), g(ldz=nvar - 1), g(defect=None),
           g(rows=None), g(h=None), g(si=0), g(sc=0), g(si=Cn + 1), g(si=1, sc=M + 1), g(malpha=None), g(out=None), g(ldg=ncon - 1)]
    n = nvar
    blocks, x, o = up(np.zeros((K, S + 1, 78))), up(np.zeros((K, n))), nans(K, n)

    def symv(K=K, S=S, n=n, blocks=blocks, x=x, ldx=n, o=o, ldo=n):
        return lib.rato_hopper_block_symv_f64(K, S, n, P(blocks), P(x), ldx, P(o), ldo, s)
    assert symv() == 0
    bad += [symv(K=0), symv(K=65536), symv(S=0), symv(n=8 * (S + 1) + 4 * S - 1), symv(blocks=None), symv(x=None), symv(ldx=n - 1),
            symv(o=None), symv(ldo=n - 1)]
    assert all(v == -1 for v in bad), bad                            # RATO_EINVAL
    torch.cuda.synchronize()


# ---- rato_hopper_block_symv_f64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 6])
def test_block_symv(S, M=4, K=3):
    from riskaversetrajopt_amd import hopper
    n = 8 * (S + 1) + 4 * S + M + 2
    rng = np.random.RandomState(70 + S)
    blocks = rng.uniform(-2, 2, (K, S + 1, 78)) * 10.0 ** rng.randint(-3, 4, (K, S + 1, 78))
    x = rng.uniform(-2, 2, (K, n)) * 10.0 ** rng.randint(-3, 4, (K, n))
    tr, tc = np.tril_indices(12)
    blocks[:, S, tr >= 8] = np.nan                                   # the u part of block S does not exist: never read
    out = nans(K, n + PAD)
    bd, xd = up(blocks), up(x, n + PAD)
    assert hopper.block_symv(S, bd, xd, n, out=out) is out
    got = out.cpu().numpy()
    assert np.all(np.isnan(got[:, n:]))
    assert got[:, 12 * S + 8:n].tobytes() == np.zeros((K, M + 2)).tobytes()      # exact +0 on ys, slack, t_risk
    for k in range(K):
        ref, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
        for t in range(S + 1):
            v = R.block_vars(S, t)
            live = np.flatnonzero(v >= 0)
            B = np.zeros((12, 12), dtype=LD)
            B[tr, tc] = blocks[k, t]
            B[tc, tr] = blocks[k, t]
            B = B[np.ix_(live, live)]
            ref[v[live]] = B @ x[k, v[live]].astype(LD)
            mag[v[live]] = np.abs(B) @ np.abs(x[k, v[live]]).astype(LD)
        within(("block symv", S, k), got[k, :n], ref, gamma(13) * mag)
        one = nans(1, n + PAD)
        hopper.block_symv(S, bd[k:k + 1].contiguous(), xd[k:k + 1].contiguous(), n, out=one)
        assert one.cpu().numpy().tobytes() == got[k:k + 1].tobytes(), k


# ---- the multiplier fold on the device ---------------------------------------------------------------------------------------------
def fold_cases():
    seen, out = set(), []
    for S, M, method, phases in H.map_cases():
        if (S, method, phases) not in seen:                          # the fold does not know M
            seen.add((S, method, phases))
            out.append((S, M, method, phases))
    return out


@pytest.mark.parametrize("S,M,method,phases", fold_cases())
def test_device_fold_is_bitwise_the_hosts(S, M, method, phases, monkeypatch):
    model = device_model(S, M, method, phases)
    ncon = model.nlp_layout()["ncon"]
    K = 3
    rng = np.random.RandomState(5 + S)
    lams = rng.uniform(-2, 2, (K, ncon)) * 10.0 ** rng.randint(-3, 4, (K, ncon))
    lams[:, rng.rand(ncon) < 0.2] = 0.0
    Z = np.stack([R.problem(S, M, k) for k in range(K)])
    lam_dyn, lam_rows = model.fold_multipliers(lams)
    host_blocks = model.nlp_device(Z, lams)["hess_blocks"].cpu().numpy()
    model.nlp_device(up(Z), up(lams), fold='device')                 # the maps are uploaded once, outside the guard
    for ld in (ncon, ncon + PAD):
        ld_t, Zt = up(lams, ld), up(Z)
        with nothing_moves_to_the_host(monkeypatch):
            d_dyn, d_rows = model.fold_multipliers_device(ld_t)
            blocks = model.nlp_device(Zt, ld_t, fold='device')["hess_blocks"]
        assert d_dyn.cpu().numpy().tobytes() == lam_dyn.tobytes() and d_rows.cpu().numpy().tobytes() == lam_rows.tobytes()
        assert np.all(np.isnan(ld_t.cpu().numpy()[:, ncon:]))
        assert blocks.cpu().numpy().tobytes() == host_blocks.tobytes(), ld


# ---- the backend on device tensors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,M,method,phases", H.map_cases())
def test_backend_on_tensors_against_the_list_methods(S, M, method, phases, monkeypatch):
    import torch
    from riskaversetrajopt_amd import hopper_ipm as m
    K = len(ALPHAS)
    models = [device_model(S, M, method, phases, a) for a in ALPHAS]
    st, lay = m.structure(models[0]), models[0].nlp_layout()
    n, ncon = st["n"], st["ncon"]
    be, bt = m.DeviceBackend(models), m.DeviceBackend(models)
    everyone = list(range(K))
    # ---- designed values: the two matvecs bitwise, the normal matrix within the product map's bound
    designed = [designed_values(st, 7 + S + 10 * M + 100 * k) for k in range(K)]
    vals, d = np.stack([v for v, _ in designed]), np.stack([w for _, w in designed])
    rng = np.random.RandomState(2)
    hess, diag, sf = rng.randn(K, S + 1, 78), rng.rand(K, n), 10.0 ** rng.uniform(-5, 0, K)
    x, w = rng.randn(K, n), rng.randn(K, ncon)
    for b in (be, bt):
        b.set_values(vals, hess)
    Jx, JTw = np.stack(be.matvec(everyone, list(x))), np.stack(be.tmatvec(everyone, list(w)))
    dg = diag + sf[:, None] * models[0].curv                          # the driver's diagonal carries sf curv
    xt, wt, dt, dgt, out = up(x, n + PAD), up(w, ncon + PAD), up(d, ncon + PAD), up(dg), nans(K, n, n + PAD)
    with nothing_moves_to_the_host(monkeypatch):
        Jx_t, JTw_t = bt.matvec_t(xt), bt.tmatvec_t(wt)
        Kc_t = bt.normal_matrix_t(dt, dgt, out=out)
        Wx_t = bt.hess_apply_t(xt)
        info = bt.factor_t(dt, dgt)
    assert Kc_t is out and info.shape == (K,) and info.dtype == torch.int32
    assert Jx_t.cpu().numpy().tobytes() == Jx.tobytes() and JTw_t.cpu().numpy().tobytes() == JTw.tobytes()
    Kc = Kc_t.cpu().numpy()
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.all(np.isnan(Kc[:, :, :n][:, ~low])) and np.all(np.isnan(Kc[:, :, n:]))
    Wx = Wx_t.cpu().numpy()
    listed = be.normal_matrix(everyone, list(d), list(dg)).cpu().numpy()
    assert np.where(low, Kc[:, :, :n], 0.0).tobytes() == np.where(low, listed, 0.0).tobytes()      # the list method's launch
    for k in range(K):
        _, mag, T = dense_reference(st, vals[k], d[k])
        host = m.normal_matrix_host(st, vals[k], d[k], hess[k], dg[k])
        bound = np.array([gamma(int(t) + 2) for t in T.reshape(-1)], dtype=LD).reshape(T.shape) * mag     # the product map's bound
        assert np.all((np.abs(Kc[k, :, :n].astype(LD) - host.astype(LD)) <= bound)[low]), k
        want = m._hess_apply(st, hess[k], x[k])
        Bf = np.abs(R.untril78(hess[k]))
        magw = np.zeros(n + 1)
        magw[st["block_vars"]] = np.einsum("tab,tb->ta", Bf, np.abs(np.append(x[k], 0.0))[st["block_vars"]])
        assert np.all(np.abs(Wx[k] - want) <= 2 * gamma(13) * magw[:-1]), k                    # both within gamma_13 of the exact sum
    # ---- a real evaluation: g of eval_full / eval_g, bitwise but for the sum row; the values and the blocks left behind
    Zs = [R.problem(S, M, k) for k in range(K)]
    lams = list(rng.uniform(-1, 1, (K, ncon)))
    G = np.stack(be.eval_full(everyone, Zs, lams, [0.0] * K))         # obj_factor 0: the blocks of the constraints alone
    G1 = np.stack(be.eval_g(everyone, Zs))
    bt.eval_full_t(up(np.stack(Zs)), up(np.stack(lams)))              # the emission's constants are uploaded once, outside the guard
    Zt, Yt = up(np.stack(Zs)), up(np.stack(lams), ncon + PAD)
    with nothing_moves_to_the_host(monkeypatch):
        g_t = bt.eval_full_t(Zt, Yt)
        g1_t = bt.eval_g_t(Zt)
    keep = np.ones(ncon, dtype=bool)
    if method == 'saa':
        keep[lay["off"]["risk"]] = False
    for name, got, ref in (("eval_full_t", g_t.cpu().numpy(), G), ("eval_g_t", g1_t.cpu().numpy(), G1)):
        assert got.shape == (K, ncon)
        assert np.ascontiguousarray(got[:, keep]).tobytes() == np.ascontiguousarray(ref[:, keep]).tobytes(), name
        if method == 'saa':
            for k in range(K):
                val, mag = HD.g_sum_row(models[0], Zs[k], M * ALPHAS[k])
                within((name, "sum row", k), got[k, lay["off"]["risk"]], val, gamma(M + 2) * mag)
    assert bt.vals0.cpu().numpy().tobytes() == be.vals0.cpu().numpy().tobytes()
    assert bt.vals1.cpu().numpy().tobytes() == be.vals1.cpu().numpy().tobytes()
    assert np.array_equal(bt.hessd.cpu().numpy(), be.hessd.cpu().numpy())    # + 0.0 of the host's add: equal, a zero's sign aside


# ---- one Newton step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 6])
def test_one_newton_step_of_the_device_driver(S, M=4, alpha=0.2):
    """the construction of test_gpu_ipm_driver.test_one_newton_step_of_the_device_driver: the NumPy backend on the restatement's
    callbacks under the host driver, the device backend under the device driver -> relative residuals in the uncondensed KKT
    system on the restatement's J and W; device <= 100 x NumPy (the project's margin for this pairing)"""
    from riskaversetrajopt_amd import hopper_ipm as m, ipm
    flds = H.fields(M)
    host = H.host_model('saa', alpha, S, M)
    model = device_model(S, M, 'saa', None, alpha)
    be_np, be_dev = m.NumpyBackend([host], [H.RestatementCallbacks(host, flds)]), m.DeviceBackend([model])
    Z0 = R.problem(S, M, 0)
    g0 = be_np.eval_g([0], [Z0])[0]

    def state(mdl):
        p = ipm.Problem(mdl, Z0, g0, H.TOL)
        rng = np.random.RandomState(400 + S)
        p.y = rng.uniform(-1, 1, p.m)
        p.zl, p.zu = p.zl * rng.uniform(0.5, 2.0, p.zl.size), p.zu * rng.uniform(0.5, 2.0, p.zu.size)
        return p

    def residual(p):
        J = R.jac_dense(p.z, S, M, 'saa', alpha, flds)
        W = R.dense_from_blocks(R.hess_blocks_full(p.z, p.y, S, M, 'saa', alpha, flds, obj_factor=p.sf), S, p.n)
        return ipm.kkt_residual(p, J, W)
    p = state(host)
    g, = be_np.eval_full([0], [p.z.copy()], [p.y], [p.sf])
    p.residuals(g, be_np.tmatvec([0], [p.y])[0])
    p.prepare_step()
    assert ipm.newton_steps(be_np, [0], [p]) == [True]
    res_np = residual(p)
    q = state(model)
    st = ipm.DeviceState([q], DEV)
    st.residuals(be_dev.eval_full_t(st.z(), st.y), be_dev.tmatvec_t(st.y))
    fact = [0]
    assert ipm.newton_steps_device(be_dev, st, [0], fact) == [0]
    st.download([q])
    assert q.mu == 0.1 and q.status is None and fact[0] == p.factorizations and q.dw == p.dw     # the same state, the same ladder
    res_dev = residual(q)
    print(f"newton step S={S}: numpy backend, host driver {res_np:.3e}; device backend, device driver {res_dev:.3e}")
    assert np.isfinite(res_dev) and res_dev <= 100.0 * res_np, (res_np, res_dev)


# ---- end to end --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problems():
    """the baseline, then saa 0.1 and 0.3 from the baseline's solution (the fixture of test_hopper_ipm_gpu.py), and the host
    driver's solutions (computed once; do not modify)"""
    from riskaversetrajopt_amd import hopper
    flds = H.fields(H.M_SMALL)
    mk = lambda method, a: hopper.Model(H.M_SMALL, method, a, S=H.S_SMALL, fields=flds, precision='f64')
    models = [mk('baseline', 0.1), mk('saa', 0.1), mk('saa', 0.3)]
    Zb, ib = models[0].solve()
    Z0s = [models[0].initial_guess(), H.warm_start(models[1], Zb), H.warm_start(models[2], Zb)]
    host = [(Zb, ib)] + [models[k].solve(Z0s[k]) for k in (1, 2)]
    return dict(fields=flds, models=models, Z0s=Z0s, host=host)


@functools.lru_cache(maxsize=None)
def device_solutions(which, run=0):
    """``which`` of the problems as one batch under the device driver, max_iter = 10 x the host driver's iterations"""
    from riskaversetrajopt_amd import hopper_ipm
    e = problems()
    return hopper_ipm.solve_batch([e["models"][k] for k in which], [e["Z0s"][k] for k in which], driver='device',
                                  max_iter=10 * max(e["host"][k][1]["iterations"] for k in which))


def bitwise(r0, r1):
    (Z0, i0), (Z1, i1) = r0, r1
    keys = ("y", "zl", "zu", "s")
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(i0[k].tobytes() == i1[k].tobytes() for k in keys) and \
        all(i0[k] == i1[k] for k in i0 if k not in keys)


@pytest.mark.parametrize("k", [0, 1, 2], ids=["baseline", "saa0.1", "saa0.3"])
def test_end_to_end_under_the_device_driver(k):
    e = problems()
    Zh, ih = e["host"][k]
    (Z, info), = device_solutions((k,))
    print(f"problem {k}: host {ih['status']} {ih['iterations']} / {ih['factorizations']}, device {info['status']} "
          f"{info['iterations']} / {info['factorizations']}, |df| {abs(ih['f'] - info['f']):.3e} max |dZ| {np.max(np.abs(Zh - Z)):.3e}")
    assert ih["status"] == "converged" and "driver" not in ih
    assert info["status"] == "converged" and info["driver"] == "device" and info["backend"] == "device"
    assert set(info) == set(ih) | {"driver"}
    H.check_solution(e["models"][k], e["fields"], Z, info)


def test_device_driver_batch_is_bitwise_the_solo_runs_and_repeats():
    batch = device_solutions((1, 2))
    for i, k in enumerate((1, 2)):
        solo, = device_solutions((k,))
        assert batch[i][1]["status"] == "converged"
        assert bitwise(batch[i], solo), ("the batch differs from the solo run", k)      # max_iter differs: it must not matter
    for r0, r1 in zip(batch, device_solutions((1, 2), run=1)):
        assert bitwise(r0, r1)


def test_entry_points_agree_with_solve_batch(tmp_path):
    from riskaversetrajopt_amd import scp
    e = problems()
    cap = 10 * max(ih["iterations"] for _, ih in e["host"])
    (Zb, ib), = device_solutions((0,))
    Z, info = e["models"][0].solve(max_iter=cap, driver='device')
    assert bitwise((Z, info), (Zb, ib))
    r = scp.run_hopper(e["models"][1], e["Z0s"][1], max_iter=cap, driver='device')
    assert bitwise((r["Z"], r["info"]), device_solutions((1,))[0]) and r["status"] == "converged"
    # the experiment: its SAA starts are the DEVICE driver's baseline, so its batch is compared with a batch from that start
    out = scp.hopper_experiment(alphas=(0.1, 0.3), M=H.M_SMALL, S=H.S_SMALL, seed=1, results_dir=str(tmp_path), max_iter=cap,
                                driver='device')
    assert bitwise((out["base"]["Z"], out["base"]["info"]), (Zb, ib))
    assert list(out["status"]) == ["converged", "converged"]
    from riskaversetrajopt_amd import hopper_ipm
    starts = [H.warm_start(e["models"][k], Zb) for k in (1, 2)]
    want = hopper_ipm.solve_batch(e["models"][1:], starts, driver='device', max_iter=cap)
    for sol, ref in zip(out["results"], want):
        assert bitwise((sol["Z"], sol["info"]), ref) and sol["info"]["driver"] == "device"
    for name, sol in (("hopper_base_results.npy", out["base"]), ("hopper_saa_alpha=0.1_results.npy", out["results"][0]),
                      ("hopper_saa_alpha=0.3_results.npy", out["results"][1])):
        xs, us = scp.load_results(str(tmp_path / name), 2)
        assert np.array_equal(xs, sol["xs"]) and np.array_equal(us, sol["us"])
