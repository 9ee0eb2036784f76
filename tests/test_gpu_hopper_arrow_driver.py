"""GPU: the arrowhead Newton step under the interior-point driver on the device (``hopper_ipm.solve_batch(newton='arrow',
driver='device')``) -- the fix-up kernels of csrc/hopper_arrow.hip on designed buffers, ``ArrowDeviceBackend`` on
device tensors against its list methods, one Newton step and the whole solve.

What a fix-up kernel computes is the host's NumPy line operation by operation, so it is held bitwise, on the device's own
``red``.  Where a sum's order differs (the sum row of g, W x) the bound is Higham's: a sum of len terms of k roundings each is
within gamma_(len + k) sum |terms| of its exact value in any order.  K = 3 problems with alphas 0.05 / 0.2 / 0.6, and every
array handed to a kernel with a leading dimension is padded by three columns of NaN, which must come back untouched."""
import functools

import numpy as np
import pytest

import _hopper_ipm as H
import _hopper_ipm_driver as HD
import _hopper_nlp as R
from _drone_gaussian_ipm import padded
from _hopper_ipm import gamma
from test_gpu_hopper_arrow import (Designed, baseline_small, device_model, gershgorin,    # noqa: F401  (baseline_small is a fixture)
                                   shapes)
from test_gpu_hopper_ipm_driver import bitwise, nothing_moves_to_the_host, within

pytestmark = pytest.mark.gpu
LD = np.longdouble
DEV = "cuda:0"
PAD = 3
K3 = 3
ALPHAS = (0.05, 0.2, 0.6)
EINVAL = -1


def up(a, ld=None, dtype=np.float64):
    import torch
    a = np.asarray(a, dtype=dtype)
    return torch.as_tensor(np.ascontiguousarray(a if ld is None else padded(a, ld)), device=DEV)


def bind():
    from riskaversetrajopt_amd import hopper_ipm
    return hopper_ipm


# ---- the fix-up kernels on designed buffers -----------------------------------------------------------------------------------
class Fixups:
    """the designed buffers of ``Designed`` with a z numbering around them: n_c = 5C + 9 core columns of which the q touched ones
    are drawn at random (slack and t_risk the last two), the M sample columns between the first n_c - 2 and those two; every
    launch for the problems ``ks`` -> dict of host arrays"""

    def __init__(self, M, Cn, saa):
        D = self.D = Designed(M, Cn, saa, 2000 * Cn + M)
        rng = np.random.RandomState(7 * Cn + M)
        D.malpha = M * np.asarray(ALPHAS)
        self.M, self.Cn, self.saa, self.q, self.nc = M, Cn, saa, D.q, D.nc
        nc = self.nc
        self.n, self.y0 = nc + M, nc - 2
        self.core_z = np.concatenate([np.arange(nc - 2), [self.n - 2, self.n - 1]])
        self.qcol = np.concatenate([rng.permutation(nc - 2)[:5 * Cn], [nc - 2, nc - 1]]).astype(np.int32)
        self.qz = self.core_z[self.qcol].astype(np.int32)
        self.rr = D.r0 - M - 1 if saa else -1
        g12 = lambda *s: rng.randn(*s) * 10.0 ** rng.uniform(-6, 6, s)
        self.x, self.out0, self.rc0, self.xc = g12(K3, self.n), g12(K3, self.n), g12(K3, nc), g12(K3, nc)
        self.beta0 = g12(K3)                                         # the baseline has no beta of its own

    def run(self, ks):
        import torch
        from riskaversetrajopt_amd import _lib
        m, D = bind(), self.D
        M, Cn, saa, n, nc, q, K = self.M, self.Cn, self.saa, self.n, self.nc, self.q, len(ks)
        r = {}
        pick = lambda a, ld=None: up(np.asarray(a)[ks], ld)
        qz, qcol = up(self.qz, dtype=np.int32), up(self.qcol, dtype=np.int32)
        ma = pick(D.malpha)
        # 1. the sum row of J x after rows mode 0 (saa only)
        if saa:
            red = up(D.rows(ks, 0)["red"])
            xt, out = pick(self.x, n + PAD), D.empty(K, D.ldd)
            m.arrow_scale(ma, xt, n - 1, red, out, self.rr)
            r.update(mv_red=red.cpu().numpy(), mv_out=out.cpu().numpy(), mv_x=xt.cpu().numpy())
        # 2. J' w after cols mode 0
        c0 = D.cols(ks, 0)
        redc, yout = up(c0["red"], 5 * Cn + 1 + PAD), up(c0["yout"])
        wt, out = pick(D.w), pick(self.out0, n + PAD)
        m.arrow_tfix(M, Cn, saa, n, qz, redc, ma, wt, self.rr, yout, out)
        r.update(t_red=c0["red"], t_yout=c0["yout"], t_out=out.cpu().numpy(), t_w=wt.cpu().numpy(), t_redp=redc.cpu().numpy())
        # 3. kk and beta after the reduction (saa only)
        R0, _ = D.reduce(ks)
        e = up(R0["e"])
        kk = beta = None
        if saa:
            redr, d = up(R0["red"], D.npart + PAD), pick(D.d)
            kk, beta = D.empty(K), D.empty(K)
            m.arrow_kkbeta(Cn, d, self.rr, redr, ma, kk, beta)
            r.update(k_red=R0["red"], kk=kk.cpu().numpy(), beta=beta.cpu().numpy(), k_d=d.cpu().numpy())
        else:
            beta = pick(self.beta0)
        # 4. E^-1 with kappa formed on the device
        dot = None
        if saa:                                                      # the existing chunked edot on the device's own e
            p, dot = _lib.ptr, D.empty(K)
            assert D.call("rato_hopper_arrow_edot_f64", K, M, p(e), p(pick(D.t)), p(D.empty(D.nch, K)), p(dot)) == 0
        v, out = pick(D.t, M + PAD), D.empty(K, M + PAD)
        m.arrow_einv(e, v, kk, dot, out)
        r.update(e=R0["e"], e_dot=None if dot is None else dot.cpu().numpy(), e_out=out.cpu().numpy(), e_v=v.cpu().numpy())
        # 5. the right-hand side of the solve after cols mode 1
        c1 = D.cols(ks, 1)
        redc, rc = up(c1["red"], 5 * Cn + 1 + PAD), pick(self.rc0, nc + PAD)
        m.arrow_rhsfix(Cn, nc, qcol, redc, beta, rc)
        r.update(r_red=c1["red"], r_rc=rc.cpu().numpy(), r_beta=beta.cpu().numpy())
        # 6. addc of rows mode 1
        xc, addc = pick(self.xc, nc + PAD), D.empty(K)
        m.arrow_scale(beta, xc, nc - 1, None, addc, 0)
        r.update(addc=addc.cpu().numpy(), a_xc=xc.cpu().numpy())
        torch.cuda.synchronize()
        return r


def same_runs(a, b, rows=None):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        x = np.asarray(a[k]) if rows is None else np.asarray(a[k])[rows]
        assert np.ascontiguousarray(x).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("saa", [True, False], ids=["saa", "baseline"])
@pytest.mark.parametrize("M,Cn", shapes([1, 2, 32, 33, 65, 161]))
def test_fixup_kernels_on_designed_buffers(M, Cn, saa):
    from riskaversetrajopt_amd import _lib
    assert int(_lib.load().rato_hopper_arrow_chunk()) == 32           # M: under, at and over one chunk boundary, and several
    F = Fixups(M, Cn, saa)
    D, n, nc, q, y0, rr = F.D, F.n, F.nc, F.q, F.y0, F.rr
    everyone = list(range(K3))
    r = F.run(everyone)
    same_runs(r, F.run(everyone))                                     # a second launch gives the same bits
    for k in everyone:
        same_runs(r, F.run([k]), [k])                                 # the batch is bitwise the K = 1 launches
    nan_pad = lambda a, length: np.all(np.isnan(a[:, length:]))
    ma = D.malpha

    def minus_fx_total(red):
        tot = np.zeros(red.shape[0])
        for c in range(Cn):
            tot -= red[:, 5 * c + 3]
        return tot
    # 1. o[:, rr] = malpha * x[:, n - 1] + red
    if saa:
        assert r["mv_out"][:, rr].tobytes() == (ma * F.x[:, n - 1] + r["mv_red"]).tobytes()
        assert np.all(np.isnan(np.delete(r["mv_out"], rr, axis=1))) and nan_pad(r["mv_x"], n)
    # 2. the transposed product's finish, in the host's order
    red, o = r["t_red"], F.out0.copy()
    tot = minus_fx_total(red)
    o[:, F.qz[:5 * Cn]] += red[:, :5 * Cn]
    o[:, n - 2] += tot
    if saa:
        o[:, n - 1] += ma * D.w[:, rr] + tot
        o[:, y0:y0 + M] = r["t_yout"]
    assert r["t_out"][:, :n].tobytes() == o.tobytes() and nan_pad(r["t_out"], n)
    assert nan_pad(r["t_redp"], 5 * Cn + 1) and np.array_equal(np.isnan(r["t_w"]), np.isnan(D.w))
    # 3. kk = d0 / (1 + d0 s), beta = d0 malpha
    if saa:
        d0, s = D.d[:, rr], r["k_red"][:, q * (q + 1) // 2 + 2 * q]
        assert r["kk"].tobytes() == (d0 / (1.0 + d0 * s)).tobytes() and r["beta"].tobytes() == (d0 * ma).tobytes()
        assert np.array_equal(np.isnan(r["k_d"]), np.isnan(D.d))
    # 4. out = (1 / e) o (v - kk red)
    u = 1.0 / r["e"]
    kappa = r["kk"] * r["e_dot"] if saa else np.zeros(K3)
    assert r["e_out"][:, :M].tobytes() == (u * (D.t - kappa[:, None])).tobytes()
    assert nan_pad(r["e_out"], M) and nan_pad(r["e_v"], M)
    # 5. rc[qcol] -= red, rc[nc - 2] -= tot, rc[nc - 1] -= tot + beta red[5C]
    red, rc, beta = r["r_red"], F.rc0.copy(), r["r_beta"]
    tot = minus_fx_total(red)
    rc[:, F.qcol[:5 * Cn]] -= red[:, :5 * Cn]
    rc[:, -2] -= tot
    rc[:, -1] -= tot + beta * red[:, 5 * Cn]
    assert r["r_rc"][:, :nc].tobytes() == rc.tobytes() and nan_pad(r["r_rc"], nc)
    # 6. addc = beta * xc[:, nc - 1]
    assert r["addc"].tobytes() == (beta * F.xc[:, -1]).tobytes() and nan_pad(r["a_xc"], nc)


@pytest.mark.parametrize("K", [256, 257, 600])
def test_lane_numbered_fixups_past_their_first_block(K):
    """``arrow_scale_kernel`` and ``arrow_kkbeta_kernel`` take the problem number from the lane, 256 problems a block: a full
    block, one problem into the second, and a ragged third.  Graded inputs on padded strides, NaN wherever no kernel may read or
    write; every problem bitwise the NumPy line of ``test_fixup_kernels_on_designed_buffers``"""
    import torch
    m = bind()
    rng = np.random.RandomState(K)
    g12 = lambda *s: rng.randn(*s) * 10.0 ** rng.uniform(-6, 6, s)
    pos12 = lambda *s: 10.0 ** rng.uniform(-6, 6, s)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=DEV)
    # out[k][ocol] = a[k] x[k][col] + add[k], and without add into a vector
    nx, col, ldo, ocol = 7, 6, 5, 2
    a, x, add = g12(K), g12(K, nx), g12(K)
    xt, out, vec = up(x, nx + PAD), nan(K, ldo), nan(K)
    m.arrow_scale(up(a), xt, col, up(add), out, ocol)
    m.arrow_scale(up(a), xt, col, None, vec, 0)
    oh = out.cpu().numpy()
    assert oh[:, ocol].tobytes() == (a * x[:, col] + add).tobytes() and np.all(np.isnan(np.delete(oh, ocol, axis=1)))
    assert vec.cpu().numpy().tobytes() == (a * x[:, col]).tobytes()
    assert np.all(np.isnan(xt.cpu().numpy()[:, nx:]))
    # kk = d0 / (1 + d0 s), beta = d0 malpha: d0 in column rr of d, s behind G, w and a in red
    Cn, rr = 1, 4
    q = 5 * Cn + 2
    npart, at = q * (q + 1) // 2 + 2 * q + 1 + 15 * Cn, q * (q + 1) // 2 + 2 * q
    d0, s, ma = pos12(K), pos12(K), K * rng.uniform(0.05, 0.75, K)
    dh, redh = np.full((K, rr + 1 + PAD), np.nan), np.full((K, npart + PAD), np.nan)
    dh[:, rr], redh[:, at] = d0, s
    kk, beta = nan(K), nan(K)
    m.arrow_kkbeta(Cn, up(dh), rr, up(redh), up(ma), kk, beta)
    assert kk.cpu().numpy().tobytes() == (d0 / (1.0 + d0 * s)).tobytes() and beta.cpu().numpy().tobytes() == (d0 * ma).tobytes()


def test_fixup_entry_points_answer_bad_arguments_with_einval():
    import torch
    from riskaversetrajopt_amd import _lib
    L, p = _lib.load(), _lib.ptr
    buf = torch.zeros(8192, dtype=torch.float64, device=DEV)
    qi = torch.zeros(256, dtype=torch.int32, device=DEV)
    b, qp, s = p(buf), p(qi), _lib.current_stream()
    M, Cn, n, nc, ldr, rr, ldw = 5, 2, 30, 14, 11, 3, 40
    npart = int(L.rato_hopper_arrow_npart(Cn))

    def scale(K=1, a=b, x=b, ldx=n, col=n - 1, add=b, out=b, ldo=n, ocol=2):
        return L.rato_hopper_arrow_scale_f64(K, a, x, ldx, col, add, out, ldo, ocol, s)

    def tfix(K=1, M=M, C=Cn, saa=1, n=n, qz=qp, red=b, ldr=ldr, malpha=b, w=b, ldw=ldw, rr=rr, yout=b, out=b, ldo=n):
        return L.rato_hopper_arrow_tfix_f64(K, M, C, saa, n, qz, red, ldr, malpha, w, ldw, rr, yout, out, ldo, s)

    def kkbeta(K=1, C=Cn, d=b, ldd=ldw, rr=rr, red=b, ldr=npart, malpha=b, kk=b, beta=b):
        return L.rato_hopper_arrow_kkbeta_f64(K, C, d, ldd, rr, red, ldr, malpha, kk, beta, s)

    def einv(K=1, M=M, e=b, v=b, ldv=M, kk=b, red=b, out=b, ldo=M):
        return L.rato_hopper_arrow_einv_f64(K, M, e, v, ldv, kk, red, out, ldo, s)

    def rhsfix(K=1, C=Cn, nc=nc, qcol=qp, red=b, ldr=ldr, beta=b, rc=b, ldrc=nc):
        return L.rato_hopper_arrow_rhsfix_f64(K, C, nc, qcol, red, ldr, beta, rc, ldrc, s)
    assert scale() == 0 and scale(add=None) == 0 and tfix() == 0 and tfix(saa=0, malpha=None, w=None, yout=None) == 0
    assert kkbeta() == 0 and einv() == 0 and einv(kk=None, red=None) == 0 and rhsfix() == 0
    bad = [scale(K=0), scale(K=65536), scale(a=None), scale(x=None), scale(out=None), scale(col=n), scale(col=-1), scale(ocol=n),
           scale(ocol=-1),
           tfix(K=0), tfix(K=65536), tfix(M=0), tfix(C=0), tfix(C=51), tfix(n=M + 1), tfix(ldo=n - 1), tfix(qz=None), tfix(red=None),
           tfix(ldr=5 * Cn), tfix(out=None), tfix(malpha=None), tfix(w=None), tfix(yout=None), tfix(rr=-1), tfix(rr=ldw),
           kkbeta(K=0), kkbeta(K=65536), kkbeta(C=0), kkbeta(C=51), kkbeta(d=None), kkbeta(rr=-1), kkbeta(rr=ldw), kkbeta(red=None),
           kkbeta(ldr=npart - 1), kkbeta(malpha=None), kkbeta(kk=None), kkbeta(beta=None),
           einv(K=0), einv(K=65536), einv(M=0), einv(e=None), einv(v=None), einv(ldv=M - 1), einv(red=None), einv(out=None),
           einv(ldo=M - 1),
           rhsfix(K=0), rhsfix(K=65536), rhsfix(C=0), rhsfix(C=51), rhsfix(nc=5 * Cn + 1), rhsfix(qcol=None), rhsfix(red=None),
           rhsfix(ldr=5 * Cn), rhsfix(beta=None), rhsfix(rc=None), rhsfix(ldrc=nc - 1)]
    assert all(v == EINVAL for v in bad), bad
    torch.cuda.synchronize()


# ---- the backend on device tensors against its list methods -------------------------------------------------------------------
@pytest.mark.parametrize("method", ["saa", "baseline"])
@pytest.mark.parametrize("S,M", [(2, 4), (2, 65), (6, 4), (6, 65)])
def test_backend_on_tensors_against_the_list_methods(S, M, method, monkeypatch):
    import torch
    from riskaversetrajopt_amd import hopper_arrow, hopper_ipm, ipm
    flds = H.fields(M)
    models = [device_model(S, M, method, a, flds) for a in ALPHAS]
    be, bt = hopper_arrow.ArrowDeviceBackend(models), hopper_arrow.ArrowDeviceBackend(models)
    st, lay = be.st, models[0].nlp_layout()
    n, ncon, nc, y0, saa = st["n"], st["ncon"], st["nc"], st["y0"], method == 'saa'
    everyone = list(range(K3))
    Z0s = [R.problem(S, M, k) for k in everyone]
    ps = [ipm.Problem(mm, Z0, g0, H.TOL) for mm, Z0, g0 in zip(models, Z0s, be.eval_g(everyone, Z0s))]   # pushed into the interior
    Zs = [p.z.copy() for p in ps]
    rng = np.random.RandomState(600 + S + M)
    lams = list(rng.uniform(-1, 1, (K3, ncon)))
    G = np.stack(be.eval_full(everyone, Zs, lams, [0.0] * K3))        # obj_factor 0: the blocks of the constraints alone
    G1 = np.stack(be.eval_g(everyone, Zs))
    X, W, B = rng.randn(K3, n), rng.randn(K3, ncon), rng.randn(K3, n)
    D = 10.0 ** rng.uniform(-3, 3, (K3, ncon))
    diags = np.stack([gershgorin(st["hess"], be.hess_host[k]) for k in everyone]) + 10.0 ** rng.uniform(-3, 3, (K3, n))
    Jx, JTw = np.stack(be.matvec(everyone, list(X))), np.stack(be.tmatvec(everyone, list(W)))
    Sh, e, _, _, _ = be.schur(everyone, list(D), list(diags))
    Sh, e = Sh.cpu().numpy(), e.cpu().numpy()
    assert be.factor(everyone, list(D), list(diags)) == [0] * K3      # positive definite by design
    sol = np.stack(be.solve(everyone, list(B)))
    assert np.all(np.isfinite(sol))

    kept = []
    factor_all = bt.factor_all

    def keep_then_factor(Kc):                                         # the Schur complement before it is factored in place
        kept.append(Kc.clone())
        return factor_all(Kc)
    bt.factor_all = keep_then_factor

    def tensors():
        return dict(Z=up(np.stack(Zs)), Y=up(np.stack(lams), ncon + PAD), X=up(X, n + PAD), W=up(W, ncon + PAD), d=up(D, ncon + PAD),
                    dg=up(diags), B=up(B, n + PAD))

    def calls(t):
        out = dict(g=bt.eval_full_t(t["Z"], t["Y"]), g1=bt.eval_g_t(t["Z"]), Jx=bt.matvec_t(t["X"]), JTw=bt.tmatvec_t(t["W"]),
                   Wx=bt.hess_apply_t(t["X"]), info=bt.factor_t(t["d"], t["dg"]))
        out["x"] = bt.solve_t(t["B"])
        return out
    calls(tensors())                                                  # warm: the maps and the work buffers are made once
    work = {k: v.data_ptr() for k, v in bt._work().items()}
    t = tensors()
    del kept[:]
    with nothing_moves_to_the_host(monkeypatch):
        got = calls(t)
    assert {k: v.data_ptr() for k, v in bt._work().items()} == work   # allocated once per group, not per call
    assert got["x"] is t["B"] and got["info"].shape == (K3,) and got["info"].dtype == torch.int32
    assert not np.any(got["info"].cpu().numpy())
    for name, length in (("Y", ncon), ("X", n), ("W", ncon), ("d", ncon), ("B", n)):
        assert np.all(np.isnan(t[name].cpu().numpy()[:, length:])), name
    # g: bitwise but for the SAA sum row, whose sum the device orders differently
    keep = np.ones(ncon, dtype=bool)
    if saa:
        keep[lay["off"]["risk"]] = False
        assert lay["off"]["risk"] == st["rr"]
    for name, g, ref in (("eval_full_t", got["g"].cpu().numpy(), G), ("eval_g_t", got["g1"].cpu().numpy(), G1)):
        assert g.shape == (K3, ncon)
        assert np.ascontiguousarray(g[:, keep]).tobytes() == np.ascontiguousarray(ref[:, keep]).tobytes(), name
        if saa:
            for k in everyone:
                val, mag = HD.g_sum_row(models[0], Zs[k], M * ALPHAS[k])
                within((name, "sum row", k), g[k, st["rr"]], val, gamma(M + 2) * mag)
    # the values left behind
    for name in ("vals0", "dx", "dfz"):
        assert getattr(bt, name).cpu().numpy().tobytes() == getattr(be, name).cpu().numpy().tobytes(), name
    assert np.array_equal(bt.hessd.cpu().numpy(), be.hessd.cpu().numpy())     # + 0.0 of the host's add: equal, a zero's sign aside
    # the products, the Schur complement, e, kk, beta and the solve: bitwise the list methods'
    assert got["Jx"].cpu().numpy().tobytes() == Jx.tobytes() and got["JTw"].cpu().numpy().tobytes() == JTw.tobytes()
    low = np.tril(np.ones((nc, nc), dtype=bool))
    assert len(kept) == 1 and np.where(low, kept[0].cpu().numpy()[:, :, :nc], 0.0).tobytes() == np.where(low, Sh[:, :, :nc], 0.0).tobytes()
    assert bt.e.cpu().numpy().tobytes() == e.tobytes()
    if saa:
        assert bt.kk.cpu().numpy().tobytes() == be.kk.cpu().numpy().tobytes()
        assert bt.beta.cpu().numpy().tobytes() == be.beta.cpu().numpy().tobytes()
    assert got["x"].cpu().numpy()[:, :n].tobytes() == sol.tobytes()
    # W x: both within gamma_13 of the exact sum
    Wx = got["Wx"].cpu().numpy()
    assert Wx.shape == (K3, n)
    for k in everyone:
        want = hopper_ipm._hess_apply(st["hess"], be.hess_host[k], X[k])
        Bf = np.abs(R.untril78(be.hess_host[k]))
        magw = np.zeros(n + 1)
        magw[st["hess"]["block_vars"]] = np.einsum("tab,tb->ta", Bf, np.abs(np.append(X[k], 0.0))[st["hess"]["block_vars"]])
        assert np.all(np.abs(Wx[k] - want) <= 2 * gamma(13) * magw[:-1]), k


# ---- one Newton step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,M", [(2, 4), (6, 65)])
def test_one_newton_step_of_the_device_driver(S, M, alpha=0.2):
    """the NumPy arrow backend on the restatement's callbacks under the host driver, the device arrow backend under the device
    driver, from the same designed interior state -> the same delta_w and factorization count, and relative residuals in the
    uncondensed KKT system on the restatement's J and W with device <= 100 x NumPy (the project's margin for this pairing)"""
    from riskaversetrajopt_amd import hopper_arrow as m, ipm
    flds = H.fields(M)
    host = H.host_model('saa', alpha, S, M)
    model = device_model(S, M, 'saa', alpha, flds)
    be_np, be_dev = m.ArrowNumpyBackend([host], [H.RestatementCallbacks(host, flds)]), m.ArrowDeviceBackend([model])
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
    assert q.mu == 0.1 and q.status is None
    print(f"arrow newton step S={S} M={M}: numpy backend, host driver {res_np:.3e} ({p.factorizations} fact, dw {p.dw:g}); "
          f"device backend, device driver {residual(q):.3e} ({fact[0]} fact, dw {q.dw:g})")
    assert fact[0] == p.factorizations and q.dw == p.dw              # the same ladder
    res_dev = residual(q)
    assert np.isfinite(res_dev) and res_dev <= 100.0 * res_np, (res_np, res_dev)


# ---- end to end --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problems(M, Zb_bytes):
    """the SAA problems at alphas 0.1 / 0.3 from the S = 6, M = 4 arrow baseline, and their host-driver arrow solutions (the
    yardstick; computed once, do not modify)"""
    from riskaversetrajopt_amd import hopper_ipm
    Zb = np.frombuffer(Zb_bytes)
    flds = H.fields(M)
    models = [device_model(H.S_SMALL, M, 'saa', a, flds) for a in (0.1, 0.3)]
    Z0s = [H.warm_start(mm, Zb) for mm in models]
    return dict(fields=flds, models=models, Z0s=Z0s, host=hopper_ipm.solve_batch(models, Z0s, newton='arrow'))


@functools.lru_cache(maxsize=None)
def device_solutions(M, Zb_bytes, which, run=0):
    """``which`` of the problems as one batch under the device driver, max_iter = 10 x the host driver's iterations"""
    from riskaversetrajopt_amd import hopper_ipm
    e = problems(M, Zb_bytes)
    return hopper_ipm.solve_batch([e["models"][k] for k in which], [e["Z0s"][k] for k in which], newton='arrow', driver='device',
                                  max_iter=10 * max(e["host"][k][1]["iterations"] for k in which))


def report(tag, ih, info):
    print(f"{tag}: host driver {ih['status']} {ih['iterations']} it / {ih['factorizations']} fact, device driver {info['status']} "
          f"{info['iterations']} it / {info['factorizations']} fact, |f_device_driver - f_host_driver| {abs(ih['f'] - info['f']):.3e}")


@pytest.mark.parametrize("M", [4, 130])
def test_end_to_end_under_the_device_driver(baseline_small, M):
    Zb = baseline_small["Zb"].tobytes()
    e = problems(M, Zb)
    batch = device_solutions(M, Zb, (0, 1))
    for k, (Z, info) in enumerate(batch):
        Zh, ih = e["host"][k]
        report(f"S=6 M={M} alpha={e['models'][k].alpha:g} (bound {baseline_small['f_bound']:.3e})", ih, info)
        assert ih["status"] == "converged" and "driver" not in ih    # the yardstick itself converged
        assert info["status"] == "converged" and info["driver"] == "device" and info["backend"] == "device"
        assert set(info) == set(ih) | {"driver"}
        H.check_solution(e["models"][k], e["fields"], Z, info)
        assert abs(info["f"] - ih["f"]) <= baseline_small["f_bound"]


def test_baseline_under_the_device_driver(baseline_small):
    flds = H.fields(H.M_SMALL)
    base = device_model(H.S_SMALL, H.M_SMALL, 'baseline', 0.1, flds)
    Zh, ih = base.solve(newton='arrow')
    assert Zh.tobytes() == baseline_small["Zb"].tobytes() and ih["status"] == "converged"
    Z, info = base.solve(newton='arrow', driver='device', max_iter=10 * ih["iterations"])
    report(f"S=6 M={H.M_SMALL} baseline (bound {baseline_small['f_bound']:.3e})", ih, info)
    assert info["status"] == "converged" and info["driver"] == "device"
    H.check_solution(base, flds, Z, info)
    assert abs(info["f"] - ih["f"]) <= baseline_small["f_bound"]


@pytest.mark.parametrize("M", [4, 130])
def test_device_driver_batch_is_bitwise_the_solo_runs_and_repeats(baseline_small, M):
    Zb = baseline_small["Zb"].tobytes()
    batch = device_solutions(M, Zb, (0, 1))
    for k in (0, 1):
        solo, = device_solutions(M, Zb, (k,))
        assert batch[k][1]["status"] == "converged"
        assert bitwise(batch[k], solo), ("the batch differs from the solo run", k)      # max_iter differs: it must not matter
    for r0, r1 in zip(batch, device_solutions(M, Zb, (0, 1), run=1)):
        assert bitwise(r0, r1)


def test_entry_points_agree_with_solve_batch(baseline_small, tmp_path):
    from riskaversetrajopt_amd import hopper_ipm, scp
    M, Zb0 = H.M_SMALL, baseline_small["Zb"].tobytes()
    e = problems(M, Zb0)
    cap = 10 * max(ih["iterations"] for _, ih in e["host"])
    flds = H.fields(M)
    base = device_model(H.S_SMALL, M, 'baseline', 0.1, flds)
    (Zb, ib), = hopper_ipm.solve_batch([base], newton='arrow', driver='device', max_iter=cap)
    assert ib["status"] == "converged"
    assert bitwise(base.solve(max_iter=cap, newton='arrow', driver='device'), (Zb, ib))
    r = scp.run_hopper(e["models"][1], e["Z0s"][1], max_iter=cap, newton='arrow', driver='device')
    want, = hopper_ipm.solve_batch([e["models"][1]], [e["Z0s"][1]], newton='arrow', driver='device', max_iter=cap)
    assert bitwise((r["Z"], r["info"]), want) and r["status"] == "converged"
    # the experiment: its SAA starts are the DEVICE driver's baseline, so its batch is compared with a batch from that start
    out = scp.hopper_experiment(alphas=(0.1, 0.3), M=M, S=H.S_SMALL, seed=1, results_dir=str(tmp_path), max_iter=cap,
                                newton='arrow', driver='device')
    assert bitwise((out["base"]["Z"], out["base"]["info"]), (Zb, ib))
    assert list(out["status"]) == ["converged", "converged"]
    starts = [H.warm_start(mm, Zb) for mm in e["models"]]
    want = hopper_ipm.solve_batch(e["models"], starts, newton='arrow', driver='device', max_iter=cap)
    for sol, ref in zip(out["results"], want):
        assert bitwise((sol["Z"], sol["info"]), ref) and sol["info"]["driver"] == "device"
