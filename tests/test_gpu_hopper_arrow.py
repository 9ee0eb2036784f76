"""GPU: the kernels of csrc/hopper_arrow.hip on designed buffers, and the device backend of the arrowhead Newton step
(``hopper_arrow.ArrowDeviceBackend``, newton='arrow').

Kernel bounds: |device - np.longdouble| <= gamma_(len + 1) sum |terms|, gamma_k = k u / (1 - k u), u = 2^-53, where len counts
the terms of the sum plus the roundings inside one term (b_i = -d_ic g_ic, the slack entry of b_i a sum over C contacts, u_i =
1 / e_i with the DEVICE's e_i, the products); each ``len`` is written where it is used.  The bound holds for any summation
order, so it covers the chunked two-level sums.  Solves: 100 x what the NumPy twin reaches."""
import numpy as np
import pytest

import _hopper_ipm as H
from _hopper_ipm import gamma

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAN = float("nan")
K3 = 3


def ipm():
    from riskaversetrajopt_amd import hopper_ipm
    return hopper_ipm


def arrow():
    from riskaversetrajopt_amd import hopper_arrow
    return hopper_arrow


def lib():
    from riskaversetrajopt_amd import _lib
    return _lib, _lib.load()


def chunk():
    return int(lib()[1].rato_hopper_arrow_chunk())


def sample_counts():
    ch = 32                                                          # asserted against the library's in the test
    return [1, 2, 63, 64, 65, 130, 257, 5 * ch - 1, 5 * ch + 1]


class Designed:
    """K problems' buffers: partials and d graded over 12 decades, NaN in every element no kernel may read or write"""

    def __init__(self, M, Cn, saa, seed):
        import torch
        self.torch = torch
        rng = np.random.RandomState(seed)
        self.M, self.Cn, self.saa, self.q = M, Cn, saa, 5 * Cn + 2
        pre, post = 5, 3
        self.r0 = pre + (1 + M if saa else 0)
        self.ldd = self.r0 + M * Cn + post
        g12 = lambda *s: 10.0 ** rng.uniform(-6, 6, s)
        d = np.full((K3, self.ldd), NAN)
        if saa:
            d[:, pre:self.r0] = g12(K3, 1 + M)
        d[:, self.r0:self.r0 + M * Cn] = g12(K3, M * Cn)
        self.d = d
        self.dx = rng.uniform(-1, 1, (K3, Cn, 3, M)) * g12(K3, Cn, 3, M)
        self.dfz = rng.uniform(-1, 1, (K3, Cn, M)) * g12(K3, Cn, M)
        self.ydiag = g12(K3, M)
        self.malpha = M * np.array([0.05, 0.3, 0.75])
        self.nc = self.q + 7
        self.qcol = rng.permutation(self.nc)[:self.q].astype(np.int32)
        self.lda = self.nc + 3
        Sh = np.full((K3, self.nc, self.lda), NAN)
        r, c = np.tril_indices(self.nc)
        Sh[:, r, c] = rng.randn(K3, r.size) * g12(K3, r.size)
        self.Sh = Sh
        self.w = np.full((K3, self.ldd), NAN)                         # a vector over the rows of g
        self.w[:, (pre if saa else self.r0):self.r0 + M * Cn] = rng.randn(K3, self.r0 - (pre if saa else self.r0) + M * Cn)
        self.t = rng.randn(K3, M) * g12(K3, M)
        self.xq = rng.randn(K3, self.q)
        self.xy = rng.randn(K3, M)
        self.addc = rng.randn(K3)
        self.kappa = rng.randn(K3)
        self.nch = int(lib()[1].rato_hopper_arrow_nchunks(M))
        self.npart = int(lib()[1].rato_hopper_arrow_npart(Cn))

    def dev(self, a, ks, dtype=np.float64):
        return self.torch.as_tensor(np.ascontiguousarray(np.asarray(a)[ks], dtype=dtype), device="cuda:0")

    def empty(self, *shape):
        return self.torch.full(shape, NAN, dtype=self.torch.float64, device="cuda:0")

    def call(self, name, *args):
        _lib, L = lib()
        with self.torch.cuda.device("cuda:0"):
            return getattr(L, name)(*args, _lib.current_stream())

    # each runner -> dict of host arrays, for the problems ``ks``
    def reduce(self, ks):
        p = lib()[0].ptr
        K = len(ks)
        dx, dfz, d, yd = self.dev(self.dx, ks), self.dev(self.dfz, ks), self.dev(self.d, ks), self.dev(self.ydiag, ks)
        e, part, red = self.empty(K, self.M), self.empty(self.nch, K, self.npart), self.empty(K, self.npart)
        assert self.call("rato_hopper_arrow_reduce_f64", K, self.M, self.Cn, int(self.saa), p(dx), p(dfz), p(d), self.ldd, self.r0,
                         p(yd), p(e), p(part), p(red)) == 0
        return dict(e=e.cpu().numpy(), red=red.cpu().numpy()), red

    def assemble(self, ks, red):
        p = lib()[0].ptr
        K = len(ks)
        Sh, d, ma = self.dev(self.Sh, ks), self.dev(self.d, ks), self.dev(self.malpha, ks)
        qc = self.torch.as_tensor(self.qcol, device="cuda:0")
        assert self.call("rato_hopper_arrow_assemble_f64", K, self.M, self.Cn, int(self.saa), self.nc, self.lda, p(qc), p(red), p(d),
                         self.ldd, self.r0, p(ma), p(Sh)) == 0
        return Sh.cpu().numpy()

    def cols(self, ks, mode):
        p = lib()[0].ptr
        K = len(ks)
        dx, dfz = self.dev(self.dx, ks), self.dev(self.dfz, ks)
        w, t = self.dev(self.d if mode else self.w, ks), (self.dev(self.t, ks) if mode else None)
        yout = None if mode else self.empty(K, self.M)
        part, red = self.empty(self.nch, K, 5 * self.Cn + 1), self.empty(K, 5 * self.Cn + 1)
        assert self.call("rato_hopper_arrow_cols_f64", K, self.M, self.Cn, int(self.saa), mode, p(dx), p(dfz), p(w), self.ldd,
                         self.r0, p(t), p(yout), p(part), p(red)) == 0
        return dict(red=red.cpu().numpy(), yout=None if mode else yout.cpu().numpy())

    def rows(self, ks, mode):
        p = lib()[0].ptr
        K = len(ks)
        dx, dfz, xq, xy = self.dev(self.dx, ks), self.dev(self.dfz, ks), self.dev(self.xq, ks), self.dev(self.xy, ks)
        part, red = self.empty(self.nch, K), self.empty(K)
        if mode == 0:
            out = self.empty(K, self.ldd)
            assert self.call("rato_hopper_arrow_rows_f64", K, self.M, self.Cn, int(self.saa), 0, p(dx), p(dfz), p(xq), p(xy), None, 0,
                             self.r0, None, p(out), self.ldd, p(part), p(red)) == 0
        else:
            out, d, addc = self.empty(K, self.M + 2), self.dev(self.d, ks), self.dev(self.addc, ks)
            assert self.call("rato_hopper_arrow_rows_f64", K, self.M, self.Cn, int(self.saa), 1, p(dx), p(dfz), p(xq), p(xy), p(d),
                             self.ldd, self.r0, p(addc), p(out), self.M + 2, None, None) == 0
        return dict(out=out.cpu().numpy(), red=red.cpu().numpy())

    def einv(self, ks, e):
        p = lib()[0].ptr
        K = len(ks)
        ed, v, kappa = self.dev(e, ks), self.dev(self.t, ks), self.dev(self.kappa, ks)
        part, red, out = self.empty(self.nch, K), self.empty(K), self.empty(K, self.M)
        assert self.call("rato_hopper_arrow_edot_f64", K, self.M, p(ed), p(v), p(part), p(red)) == 0
        assert self.call("rato_hopper_arrow_eapply_f64", K, self.M, p(ed), p(v), p(kappa), p(out)) == 0
        return dict(dot=red.cpu().numpy(), out=out.cpu().numpy())


def close(dev, ref, mag, length, what):
    assert np.all(np.isfinite(dev)), what
    bound = gamma(length + 1) * mag
    bad = np.abs(dev.astype(LD) - ref) > bound
    assert not np.any(bad), (what, float(np.max(np.abs(dev.astype(LD) - ref) / (bound + np.finfo(LD).tiny))))


def same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a if a[k] is not None)


def shapes(Ms, at_the_limit=(33, 65)):
    """(M, Cn): every M at Cn = 1, 4, 20, and Cn = 50, the entry points' limit, at M = 33 and 65 (two and three chunks, the last
    of one sample).  At Cn = 50 the reduction asks for 32 (5 Cn + 3) doubles = 64,768 bytes of dynamic LDS and the right-hand
    side's fix-up uses 252 of its 256 lanes"""
    return [(M, Cn) for Cn in (1, 4, 20) for M in Ms] + [(M, 50) for M in at_the_limit]


@pytest.mark.parametrize("saa", [True, False], ids=["saa", "baseline"])
@pytest.mark.parametrize("M,Cn", shapes(sample_counts()))
def test_kernels_on_designed_buffers(M, Cn, saa):
    assert chunk() == 32 and int(lib()[1].rato_hopper_arrow_nchunks(M)) == -(-M // 32)
    D = Designed(M, Cn, saa, 1000 * Cn + M)
    q, r0, all_k = D.q, D.r0, list(range(K3))
    nent = q * (q + 1) // 2
    assert D.npart == nent + 2 * q + 1 + 15 * Cn
    # ---- launches: the batch, a second time, and each problem alone (bitwise) ------------------------------------------------
    R, red_dev = D.reduce(all_k)
    Sh = D.assemble(all_k, red_dev)
    runs = dict(c0=D.cols(all_k, 0), c1=D.cols(all_k, 1), r0=D.rows(all_k, 0), r1=D.rows(all_k, 1), ei=D.einv(all_k, R["e"]))
    R2, red2 = D.reduce(all_k)
    assert same(R, R2) and Sh.tobytes() == D.assemble(all_k, red2).tobytes()
    assert same(runs["c0"], D.cols(all_k, 0)) and same(runs["r1"], D.rows(all_k, 1)) and same(runs["ei"], D.einv(all_k, R["e"]))
    for k in all_k:
        Rk, redk = D.reduce([k])
        assert all(Rk[n].tobytes() == R[n][k:k + 1].tobytes() for n in Rk)
        assert D.assemble([k], redk).tobytes() == Sh[k:k + 1].tobytes()
        for name, one in (("c0", D.cols([k], 0)), ("c1", D.cols([k], 1)), ("r0", D.rows([k], 0)), ("r1", D.rows([k], 1)),
                          ("ei", D.einv([k], R["e"]))):
            assert all(one[n].tobytes() == runs[name][n][k:k + 1].tobytes() for n in one if one[n] is not None), (name, k)
    # ---- references ------------------------------------------------------------------------------------------------------------
    slack, tq = 5 * Cn, 5 * Cn + 1
    for k in all_k:
        d = D.d[k].astype(LD)
        dic = d[r0:r0 + M * Cn].reshape(M, Cn)
        g = np.stack([D.dx[k, :, 0].T, D.dx[k, :, 1].T, D.dx[k, :, 2].T, np.ones((M, Cn)), D.dfz[k].T], axis=2).astype(LD)   # (M, C, 5)
        dsum = dic.sum(1)
        B = np.zeros((M, q), dtype=LD)
        B[:, :slack] = (-dic[:, :, None] * g).reshape(M, slack)
        B[:, slack] = dsum
        if saa:
            B[:, tq] = dsum
        aB = np.abs(B)
        e_ref = D.ydiag[k].astype(LD) + ((d[r0 - M:r0] + dsum) if saa else 0)
        close(R["e"][k], e_ref, e_ref, Cn + 2, "e")                                    # C + 2 positive terms
        u = 1 / R["e"][k].astype(LD)                                                   # the device's e: one rounding in 1 / e
        red = R["red"][k]
        r, c = np.tril_indices(q)
        G, aG = (B.T * u) @ B, (aB.T * u) @ aB
        close(red[:nent], G[r, c], aG[r, c], M + 2 * Cn + 3, "G")                      # M terms; b_p, b_r (<= C each), u, 2 products
        w, a, s = B.T @ u, B.sum(0), u.sum()
        close(red[nent:nent + q], w, aB.T @ u, M + Cn + 2, "w")
        close(red[nent + q:nent + 2 * q], a, aB.sum(0), M + Cn, "a")
        close(red[nent + 2 * q:nent + 2 * q + 1], s, s, M + 1, "s")
        P = np.einsum("mc,mcj,mcl->cjl", dic, g, g)
        aP = np.einsum("mc,mcj,mcl->cjl", dic, np.abs(g), np.abs(g))
        r5, c5 = np.tril_indices(5)
        close(red[nent + 2 * q + 1:].reshape(Cn, 15), P[:, r5, c5], aP[:, r5, c5], M + 2, "P")
        # Shat: the slip rows' share, then the elimination's terms; 13 more roundings than G's chain (beta, k, v, the products, the sums)
        A, aA = np.zeros((q, q), dtype=LD), np.zeros((q, q), dtype=LD)
        for cc in range(Cn):
            N = np.zeros((M, q), dtype=LD)
            N[:, 5 * cc:5 * cc + 5], N[:, slack] = g[:, cc], -1
            if saa:
                N[:, tq] = -1
            A += N.T @ (dic[:, cc, None] * N)
            aA += np.abs(N).T @ (dic[:, cc, None] * np.abs(N))
        T, aT = A, aA
        if saa:
            d0, ma = d[r0 - M - 1], LD(D.malpha[k])
            beta, kk = d0 * ma, d0 / (1 + d0 * s)
            et = np.zeros(q, dtype=LD)
            et[tq] = 1
            v, av = w + beta * s * et, aB.T @ u + beta * s * et
            T = A - (G + beta * (np.outer(w, et) + np.outer(et, w)) + beta * beta * s * np.outer(et, et)) + kk * np.outer(v, v)
            aT = aA + aG + beta * (np.outer(aB.T @ u, et) + np.outer(et, aB.T @ u)) + beta * beta * s * np.outer(et, et) + kk * np.outer(av, av)
            T[tq, tq] += d0 * ma * ma
            aT[tq, tq] += d0 * ma * ma
        want = np.tril(D.Sh[k][:, :D.nc]).astype(LD)
        mag = np.abs(want)
        hi, lo = np.maximum(D.qcol[r], D.qcol[c]), np.minimum(D.qcol[r], D.qcol[c])
        want[hi, lo] += T[r, c]
        mag[hi, lo] += aT[r, c]
        low = np.tril(np.ones((D.nc, D.nc), dtype=bool))
        got = Sh[k][:, :D.nc]
        close(got[low], want[low], mag[low], M + 2 * Cn + 16, "Shat")
        touched = np.zeros((D.nc, D.nc), dtype=bool)
        touched[hi, lo] = True
        if not saa:
            touched[D.qcol[tq], :] = touched[:, D.qcol[tq]] = False
        keep = low & ~touched
        assert got[keep].tobytes() == D.Sh[k][:, :D.nc][keep].tobytes()              # nothing else of the triangle is written
        assert np.all(np.isnan(got[~low])) and np.all(np.isnan(Sh[k][:, D.nc:]))     # nor the upper triangle and the padding
        # ---- products ------------------------------------------------------------------------------------------------------------
        wv = D.w[k].astype(LD)
        wic = wv[r0:r0 + M * Cn].reshape(M, Cn)
        c0 = runs["c0"]
        close(c0["red"][k][:slack].reshape(Cn, 5), np.einsum("mc,mcj->cj", wic, g), np.einsum("mc,mcj->cj", np.abs(wic), np.abs(g)),
              M + 1, "J_risk' w")
        assert c0["red"][k][slack] == 0.0
        if saa:
            yref = wv[r0 - M - 1] - wv[r0 - M:r0] - wic.sum(1)
            close(c0["yout"][k], yref, np.abs(wv[r0 - M - 1]) + np.abs(wv[r0 - M:r0]) + np.abs(wic).sum(1), Cn + 2, "J_risk' w on y")
        else:
            assert not np.any(c0["yout"][k])
        t = D.t[k].astype(LD)
        om = -t[:, None] * dic
        c1 = runs["c1"]["red"][k]
        close(c1[:slack].reshape(Cn, 5), np.einsum("mc,mcj->cj", om, g), np.einsum("mc,mcj->cj", np.abs(om), np.abs(g)), M + 2, "B_s' t")
        close(c1[slack:], t.sum(keepdims=True), np.abs(t).sum(keepdims=True), M, "1' t")
        xq, xy = D.xq[k].astype(LD), D.xy[k].astype(LD)
        gx = np.einsum("mcj,cj->mc", g, xq[:slack].reshape(Cn, 5))
        agx = np.einsum("mcj,cj->mc", np.abs(g), np.abs(xq[:slack].reshape(Cn, 5)))
        lin = gx - xq[slack] - (xq[tq] + xy[:, None] if saa else 0)
        alin = agx + np.abs(xq[slack]) + (np.abs(xq[tq]) + np.abs(xy[:, None]) if saa else 0)
        o0 = runs["r0"]["out"][k]
        close(o0[r0:r0 + M * Cn].reshape(M, Cn), lin, alin, 8 + 5, "J_risk v")        # 8 terms, 5 products
        written = np.zeros(D.ldd, dtype=bool)
        written[r0:r0 + M * Cn] = True
        if saa:
            written[r0 - M:r0] = True
            assert np.array_equal(o0[r0 - M:r0], -D.xy[k])
            close(runs["r0"]["red"][k:k + 1], xy.sum(keepdims=True), np.abs(xy).sum(keepdims=True), M, "1' v_y")
        assert np.all(np.isnan(o0[~written]))
        lin1 = gx - xq[slack] - (xq[tq] if saa else 0)
        alin1 = agx + np.abs(xq[slack]) + (np.abs(xq[tq]) if saa else 0)
        bx = -(dic * lin1).sum(1) + LD(D.addc[k])
        abx = (dic * alin1).sum(1) + np.abs(D.addc[k])
        o1 = runs["r1"]["out"][k]
        close(o1[:M], xy - bx, np.abs(xy) + abx, 7 * Cn + 2 + 7, "r_y - B x_c")        # 7 C + 2 terms, <= 7 roundings inside one
        assert np.all(np.isnan(o1[M:]))
        ei = runs["ei"]
        close(ei["dot"][k:k + 1], (u * t).sum(keepdims=True), (u * np.abs(t)).sum(keepdims=True), M + 2, "u' v")
        close(ei["out"][k], u * (t - LD(D.kappa[k])), u * (np.abs(t) + np.abs(D.kappa[k])), 2 + 3, "E^-1 apply")


def test_bad_arguments_return_einval():
    import torch
    _lib, L = lib()
    D = Designed(5, 2, True, 1)
    p = _lib.ptr
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda:0")
    qc = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    b, s = p(buf), _lib.current_stream()
    EINVAL = -1
    assert L.rato_hopper_arrow_nchunks(0) == 0 and L.rato_hopper_arrow_npart(0) == 0 and L.rato_hopper_arrow_npart(51) == 0
    good = dict(K=1, M=5, C=2, ldd=D.ldd, r0=D.r0)
    for bad in (dict(K=0), dict(K=65536), dict(M=0), dict(C=0), dict(C=51), dict(ldd=D.r0 + 9), dict(r0=5)):
        a = dict(good, **bad)
        assert L.rato_hopper_arrow_reduce_f64(a["K"], a["M"], a["C"], 1, b, b, b, a["ldd"], a["r0"], b, b, b, b, s) == EINVAL, bad
        assert L.rato_hopper_arrow_cols_f64(a["K"], a["M"], a["C"], 1, 0, b, b, b, a["ldd"], a["r0"], None, b, b, b, s) == EINVAL, bad
        assert L.rato_hopper_arrow_assemble_f64(a["K"], a["M"], a["C"], 1, 12, 12, p(qc), b, b, a["ldd"], a["r0"], b, b, s) == EINVAL, bad
    assert L.rato_hopper_arrow_reduce_f64(1, 5, 2, 1, None, b, b, D.ldd, D.r0, b, b, b, b, s) == EINVAL
    assert L.rato_hopper_arrow_assemble_f64(1, 5, 2, 1, 11, 11, p(qc), b, b, D.ldd, D.r0, b, b, s) == EINVAL      # nc < q
    assert L.rato_hopper_arrow_assemble_f64(1, 5, 2, 1, 12, 11, p(qc), b, b, D.ldd, D.r0, b, b, s) == EINVAL      # lda < nc
    assert L.rato_hopper_arrow_cols_f64(1, 5, 2, 1, 2, b, b, b, D.ldd, D.r0, b, b, b, b, s) == EINVAL             # mode
    assert L.rato_hopper_arrow_cols_f64(1, 5, 2, 1, 1, b, b, b, D.ldd, D.r0, None, b, b, b, s) == EINVAL          # mode 1 without t
    assert L.rato_hopper_arrow_rows_f64(1, 5, 2, 1, 0, b, b, b, b, None, 0, D.r0, None, b, D.r0 + 9, b, b, s) == EINVAL   # ldo
    assert L.rato_hopper_arrow_rows_f64(1, 5, 2, 1, 1, b, b, b, b, None, D.ldd, D.r0, b, b, 5, None, None, s) == EINVAL   # no d
    assert L.rato_hopper_arrow_rows_f64(1, 5, 2, 1, 0, b, b, b, b, None, 0, D.r0, None, b, D.ldd, b, b, s) == 0          # C = 2 is served,
    assert L.rato_hopper_arrow_rows_f64(1, 5, 51, 1, 0, b, b, b, b, None, 0, D.r0, None, b, D.r0 + 5 * 51, b, b, s) == EINVAL   # 51 is not
    assert L.rato_hopper_arrow_rows_f64(1, 5, 51, 1, 1, b, b, b, b, b, D.r0 + 5 * 51, D.r0, b, b, 5, None, None, s) == EINVAL
    assert L.rato_hopper_arrow_edot_f64(1, 0, b, b, b, b, s) == EINVAL and L.rato_hopper_arrow_eapply_f64(1, 5, b, b, None, b, s) == EINVAL
    torch.cuda.synchronize()


# ---- the backend ---------------------------------------------------------------------------------------------------------------
def device_model(S, M, method, alpha=0.2, flds=None):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=H.fields(M) if flds is None else flds, precision='f64')


@pytest.mark.parametrize("S,M", [(2, 4), (2, 65), (6, 4), (6, 65)])
def test_one_newton_step_residual(S, M):
    """the device arrow step's relative residual in the UNCONDENSED regularised KKT system (the restatement's dense J and W) is at
    most 100 x the NumPy arrow backend's at the same designed interior iterate"""
    m = arrow()
    flds = H.fields(M)
    host = H.host_model('saa', 0.2, S, M)
    r_np, dw_np = H.newton_residual(m.ArrowNumpyBackend([host], [H.RestatementCallbacks(host, flds)]), host, flds, S, M)
    model = device_model(S, M, 'saa', flds=flds)
    r_dev, dw_dev = H.newton_residual(m.ArrowDeviceBackend([model]), model, flds, S, M)
    print("arrow newton residual S=%d M=%d: device %.3e numpy %.3e (delta_w %g / %g)" % (S, M, r_dev, r_np, dw_dev, dw_np))
    assert dw_dev == dw_np
    assert r_dev <= 100.0 * r_np


@pytest.mark.parametrize("S,M", [(2, 4), (2, 65)])
def test_list_methods_on_a_subset_of_the_group(S, M):
    """"nothing a kernel computes for a problem depends on the others": after one eval_full of the K = 3 problems of a group
    (alphas differ) at the designed interior iterates of ``_hopper_ipm.newton_residual``, matvec, tmatvec and schur for
    idx = [2, 0] are bitwise rows 2 and 0 of the calls for idx = [0, 1, 2].  M = 65 crosses one chunk boundary of the sample
    reduction (32 samples a chunk, two chunks' partials summed), M = 4 stays under it."""
    import _hopper_nlp as R
    from riskaversetrajopt_amd import ipm as method
    m = arrow()
    flds = H.fields(M)
    models = [device_model(S, M, 'saa', a, flds) for a in (0.1, 0.2, 0.3)]
    be = m.ArrowDeviceBackend(models)
    everyone, sub = list(range(K3)), [2, 0]
    Z0s = [R.problem(S, M, k) for k in everyone]
    ps = [method.Problem(mm, Z0, g0, H.TOL) for mm, Z0, g0 in zip(models, Z0s, be.eval_g(everyone, Z0s))]
    rng = np.random.RandomState(500 + S + M)
    n, ncon, nc = ps[0].n, ps[0].m, be.st["nc"]
    lams = list(rng.uniform(-1, 1, (K3, ncon)))
    be.eval_full(everyone, [p.z.copy() for p in ps], lams, [p.sf for p in ps])
    X, W = list(rng.randn(K3, n)), list(rng.randn(K3, ncon))
    D, diags = list(10.0 ** rng.uniform(-3, 3, (K3, ncon))), list(10.0 ** rng.uniform(-3, 3, (K3, n)))
    pick = lambda rows: [rows[i] for i in sub]
    low = np.tril(np.ones((nc, nc), dtype=bool))

    def schur(idx, d, dg):
        Sh, e, _, red, _ = be.schur(idx, d, dg)
        return np.where(low, Sh.cpu().numpy(), 0.0), e.cpu().numpy(), red

    full = dict(matvec=(np.stack(be.matvec(everyone, X)),), tmatvec=(np.stack(be.tmatvec(everyone, W)),), schur=schur(everyone, D, diags))
    part = dict(matvec=(np.stack(be.matvec(sub, pick(X))),), tmatvec=(np.stack(be.tmatvec(sub, pick(W))),),
                schur=schur(sub, pick(D), pick(diags)))
    assert full["matvec"][0].shape == (K3, ncon) and full["tmatvec"][0].shape == (K3, n) and full["schur"][0].shape == (K3, nc, nc)
    for name in full:
        for a, b in zip(full[name], part[name]):
            assert np.all(np.isfinite(a)), name
            assert np.ascontiguousarray(a[sub]).tobytes() == b.tobytes(), name


def gershgorin(st, blocks):
    """per variable the absolute row sum of W given as step blocks (S+1, 78): W + diag is positive definite for diag above it"""
    import _hopper_nlp as R
    Bf = np.abs(R.untril78(blocks))
    mag = np.zeros(st["n"] + 1)
    mag[st["block_vars"]] = Bf.sum(axis=2)
    return mag[:-1]


@pytest.mark.parametrize("S,M,method", [(2, 4, 'saa'), (2, 65, 'saa'), (2, 4, 'baseline')])
def test_refactoring_a_subset_leaves_the_others_factors(S, M, method):
    """the ladder of ``ipm.newton_steps``: everyone is factored, [2, 0] are factored again with other weights, then everyone is
    solved for.  What is kept per problem (e, d, kk, beta, L) is addressed by problem number: problem 1's solution does not move
    by a bit, alone or in the batch, and problems 2 and 0 get bitwise what a fresh backend gives that factored everyone with the
    new weights in their rows.  Diagonals above W's Gershgorin radius: every factorization succeeds by design."""
    import _hopper_nlp as R
    from riskaversetrajopt_amd import ipm as method_ipm
    m = arrow()
    flds = H.fields(M)
    models = [device_model(S, M, method, a, flds) for a in (0.1, 0.2, 0.3)]
    everyone, sub = list(range(K3)), [2, 0]
    Z0s = [R.problem(S, M, k) for k in everyone]
    rng = np.random.RandomState(700 + S + M)
    lay = models[0].nlp_layout()
    n, ncon = lay["nvar"], lay["ncon"]
    lams = list(rng.uniform(-1, 1, (K3, ncon)))

    def backend():
        be = m.ArrowDeviceBackend(models)
        ps = [method_ipm.Problem(mm, Z0, g0, H.TOL) for mm, Z0, g0 in zip(models, Z0s, be.eval_g(everyone, Z0s))]
        be.eval_full(everyone, [p.z.copy() for p in ps], lams, [p.sf for p in ps])
        return be
    be = backend()
    radius = np.stack([gershgorin(be.st["hess"], be.hess_host[k]) for k in everyone])
    B = list(rng.randn(K3, n))
    D, diags = 10.0 ** rng.uniform(-3, 3, (K3, ncon)), radius + 10.0 ** rng.uniform(-3, 3, (K3, n))
    D2, diags2 = D.copy(), diags.copy()
    D2[sub], diags2[sub] = 10.0 ** rng.uniform(-3, 3, (2, ncon)), radius[sub] + 10.0 ** rng.uniform(-3, 3, (2, n))
    assert be.factor(everyone, list(D), list(diags)) == [0] * K3
    X = np.stack(be.solve(everyone, B))
    assert be.factor(sub, list(D2[sub]), list(diags2[sub])) == [0, 0]
    X2, X3 = np.stack(be.solve(everyone, B)), np.stack(be.solve([1], [B[1]]))
    fresh = backend()
    assert fresh.factor(everyone, list(D2), list(diags2)) == [0] * K3
    Xf = np.stack(fresh.solve(everyone, B))
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(X2))
    assert X2[1].tobytes() == X[1].tobytes() and X3[0].tobytes() == X[1].tobytes()
    for k in sub:
        assert X2[k].tobytes() == Xf[k].tobytes(), k
        assert X2[k].tobytes() != X[k].tobytes(), k                   # the new weights did arrive


@pytest.fixture(scope="module")
def baseline_small():
    """the S = 6, M = 4 baseline by the device arrow step, and the largest |f_device - f_numpy| of the DENSE step over the
    baseline and the two alphas (what the existing dense device / NumPy end-to-end test compares)"""
    flds = H.fields(H.M_SMALL)
    base = device_model(H.S_SMALL, H.M_SMALL, 'baseline', 0.1, flds)
    Zb, ib = base.solve(newton='arrow')
    assert ib["status"] == "converged"
    H.check_solution(base, flds, Zb, ib)
    diff = 0.0
    for method, a in (('baseline', 0.1), ('saa', 0.1), ('saa', 0.3)):
        m = device_model(H.S_SMALL, H.M_SMALL, method, a, flds)
        Z0 = None if method == 'baseline' else H.warm_start(m, Zb)
        fd, fn = m.solve(Z0)[1]["f"], m.solve(Z0, backend='numpy')[1]["f"]
        diff = max(diff, abs(fd - fn))
    print("dense device / numpy at S=6 M=4: max |f_device - f_numpy| = %.3e" % diff)
    return dict(Zb=Zb, f_bound=max(10.0 * diff, 1e-12))


@pytest.mark.parametrize("M", [4, 130])
def test_end_to_end_on_the_device(baseline_small, M):
    m = ipm()
    flds = H.fields(M)
    models = [device_model(H.S_SMALL, M, 'saa', a, flds) for a in (0.1, 0.3)]
    Z0s = [H.warm_start(mm, baseline_small["Zb"]) for mm in models]
    batch = m.solve_batch(models, Z0s, newton='arrow')
    for mm, Z0, (Z, info) in zip(models, Z0s, batch):
        assert info["status"] == "converged" and info["backend"] == "device"
        H.check_solution(mm, flds, Z, info)
        Z1, i1 = mm.solve(Z0, newton='arrow')                                          # Model.solve = the K = 1 batch, bitwise
        assert Z.tobytes() == Z1.tobytes() and (info["iterations"], info["factorizations"]) == (i1["iterations"], i1["factorizations"])
        Zn, inn = mm.solve(Z0, backend='numpy', newton='arrow')
        assert inn["status"] == "converged"
        print("S=6 M=%d alpha=%g: device %d it / %d fact, numpy %d it; |f_device - f_numpy| = %.3e (bound %.3e)" %
              (M, mm.alpha, info["iterations"], info["factorizations"], inn["iterations"], abs(info["f"] - inn["f"]),
               baseline_small["f_bound"]))
        assert abs(info["f"] - inn["f"]) <= baseline_small["f_bound"]
