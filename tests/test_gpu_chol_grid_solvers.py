"""GPU: the solvers under ``chol='grid'`` (csrc/chol_grid.hip).  The grid Cholesky returns the bits of the workgroup
one, so nothing here has a tolerance of its own: every factor, every solution of a Newton system and every (Z, info) of a whole
solve under ``chol='grid'`` is held BITWISE to the ``chol='workgroup'`` one, the batch to its solo runs, and the returned points
to the independent checks of tests/_hopper_ipm.py and tests/_drone_gaussian_ipm.py."""
import functools

import numpy as np
import pytest

import _drone_gaussian_ipm as T
import _hopper_ipm as H
import _hopper_nlp as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 3
K3 = 3
ALPHAS = (0.05, 0.2, 0.6)
METHODS = ("workgroup", "grid")


def up(a, ld=None):
    import torch
    a = np.asarray(a, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(a if ld is None else T.padded(a, ld)), device=DEV)


def lower_bytes(L, n):
    """the bytes of the lower triangles of L (K, n, lda): what a factorization defines"""
    r, c = np.tril_indices(n)
    return np.ascontiguousarray(L.cpu().numpy()[:, r, c]).tobytes()


def bitwise(r0, r1):
    (Z0, i0), (Z1, i1) = r0, r1
    same = lambda a, b: a.tobytes() == b.tobytes() if isinstance(a, np.ndarray) else a == b
    return Z0.tobytes() == Z1.tobytes() and set(i0) == set(i1) and all(same(i0[k], i1[k]) for k in i0)


def hopper_model(S, M, method, alpha, flds):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=flds, precision='f64')


def check_backends(make, n, ncon, Zs, rng):
    """one backend per method on the same evaluation (multipliers 0 and objective factor 0: the normal matrix is
    diag + J' D J, positive definite by design): the list methods at idx = [0, 2] and the tensor methods on the whole group,
    twice each; factors and solutions bitwise across the methods, the grid form's scratch allocated once"""
    everyone, idx = list(range(K3)), [0, 2]
    D, diags = 10.0 ** rng.uniform(-2, 2, (K3, ncon)), 10.0 ** rng.uniform(-1, 2, (K3, n))
    B = rng.randn(K3, n)
    lams = np.zeros((K3, ncon))
    got = {}
    for method in METHODS:
        be = make(method)
        assert be.chol == method
        be.eval_full(everyone, list(Zs), list(lams), [0.0] * K3)
        rec = []
        for _ in range(2):                                           # two iterations
            info = be.factor(idx, list(D[idx]), list(diags[idx]))
            x = np.stack(be.solve(idx, list(B[idx])))
            assert [int(v) for v in info] == [0, 0] and np.all(np.isfinite(x))
            rec.append((lower_bytes(be.L[idx], be.L.shape[1]), x.tobytes(), None if be.chol_work is None else be.chol_work.data_ptr()))
        bt = make(method)
        bt.eval_full_t(up(Zs), up(lams, ncon + PAD))
        for _ in range(2):
            info = bt.factor_t(up(D, ncon + PAD), up(diags))
            xt = bt.solve_t(up(B, n + PAD))
            assert info.cpu().tolist() == [0] * K3
            xh = xt.cpu().numpy()
            assert np.all(np.isfinite(xh[:, :n])) and np.all(np.isnan(xh[:, n:]))
            rec.append((lower_bytes(bt.L, bt.L.shape[1]), xh[:, :n].tobytes(), None if bt.chol_work is None else bt.chol_work.data_ptr()))
        got[method] = rec
        for b in (be, bt):
            if method == 'grid':
                from riskaversetrajopt_amd import _lib
                assert b.chol_work is not None and b.chol_work.numel() == K3 * _lib.load().rato_chol_grid_work_doubles(b.L.shape[1])
            else:
                assert b.chol_work is None
    for (Lw, xw, _), (Lg, xg, _) in zip(got["workgroup"], got["grid"]):
        assert Lg == Lw and xg == xw
    g = got["grid"]
    assert g[0][2] == g[1][2] and g[2][2] == g[3][2]                 # the scratch's address: unchanged across the iterations
    assert g[0][:2] == g[1][:2] and g[2][:2] == g[3][:2]             # and the second iteration is bitwise the first


@pytest.mark.parametrize("newton", ["dense", "arrow"])
@pytest.mark.parametrize("S,M", [(2, 4), (6, 65)])
def test_hopper_backends_are_bitwise_under_the_grid_cholesky(S, M, newton):
    from riskaversetrajopt_amd import hopper_arrow, hopper_ipm
    flds = H.fields(M)
    models = [hopper_model(S, M, 'saa', a, flds) for a in ALPHAS]
    cls = hopper_ipm.DeviceBackend if newton == 'dense' else hopper_arrow.ArrowDeviceBackend
    st = hopper_ipm.structure(models[0])
    Zs = np.stack([R.problem(S, M, k) for k in range(K3)])
    check_backends(lambda method: cls(models, chol=method), st["n"], st["ncon"], Zs, np.random.RandomState(10 * S + M))


@pytest.mark.parametrize("S", sorted(T.CASES))
def test_drone_gaussian_backend_is_bitwise_under_the_grid_cholesky(S):
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm as m
    alphas = (0.05, 0.1, 0.3)
    nlps = [m.Nlp(dg.Model(S, alpha=a, device=DEV)) for a in alphas]
    Zs = np.stack(T.starts(S, alphas))
    check_backends(lambda method: m.DeviceBackend(nlps, chol=method), nlps[0].num_vars, nlps[0].n_nl + 1, Zs,
                   np.random.RandomState(S))


def test_an_unknown_method_is_refused_by_the_backends():
    from riskaversetrajopt_amd import ipm
    import torch
    with pytest.raises(ValueError):
        ipm.DeviceBase(torch.device(DEV), 1, chol='panel')


def test_device_base_scatters_a_failed_retry_and_gathers_a_subset_under_the_grid_cholesky():
    """the twin of test_hopper_ipm_gpu.py::test_device_base_scatters_a_retry_and_gathers_a_subset, made harsher: all four problems
    factored at n = 65, problem 2 again with an indefinite matrix (info != 0, the other three factors survive), then with a
    definite one as a delta_w retry does, then a solve for problems 0, 2, 3.  The factors and X bitwise those of a
    ``chol='workgroup'`` DeviceBase fed the same sequence; the scratch made once for four problems and reused for the subsets"""
    import torch
    from riskaversetrajopt_amd import _lib, ipm
    from test_gpu_chol_grid import padded as tri_padded, spd
    n_all, n, j_bad = 4, 65, 40
    lda = n + PAD
    As = [spd("bbt", n, 650 + k) for k in range(n_all)]
    indefinite = spd("bbt", n, 658)
    indefinite[j_bad, j_bad] = -1.0
    first, bad, retry = tri_padded(As, lda), tri_padded([indefinite], lda), tri_padded([spd("graded", n, 659)], lda)
    B = list(np.random.RandomState(65).uniform(-1, 1, (3, n)))
    got = {}
    for method in METHODS:
        be = ipm.DeviceBase(torch.device(DEV), n_all, chol=method)
        assert be.factor_device([0, 1, 2, 3], first.clone()) == [0] * n_all
        kept = be.L.cpu().numpy().copy()
        ptrs = [None if be.chol_work is None else be.chol_work.data_ptr()]
        info_bad = be.factor_device([2], bad.clone())
        assert info_bad[0] != 0
        after = be.L.cpu().numpy()
        assert all(after[k].tobytes() == kept[k].tobytes() for k in (0, 1, 3))   # the failure stays in row 2
        ptrs.append(None if be.chol_work is None else be.chol_work.data_ptr())
        assert be.factor_device([2], retry.clone()) == [0]
        ptrs.append(None if be.chol_work is None else be.chol_work.data_ptr())
        Lh = be.L.cpu().numpy()
        assert all(Lh[k].tobytes() == kept[k].tobytes() for k in (0, 1, 3)) and Lh[2].tobytes() != kept[2].tobytes()
        X = be.solve_device([0, 2, 3], B)
        assert X.shape == (3, n) and np.all(np.isfinite(X))
        got[method] = (info_bad, lower_bytes(be.L, n), X.tobytes())
        if method == 'grid':
            assert be.chol_work.numel() == n_all * _lib.load().rato_chol_grid_work_doubles(n)
            assert ptrs[0] is not None and ptrs[0] == ptrs[1] == ptrs[2]     # allocated once, for four problems
        else:
            assert be.chol_work is None
    assert got["grid"] == got["workgroup"]
    one = retry.clone()                                               # row 2 is the retry's factor, not the failed one's
    assert ipm.chol_factor(one).cpu().tolist() == [0]
    r, c = np.tril_indices(n)
    assert np.ascontiguousarray(one.cpu().numpy()[:, r, c]).tobytes() == np.frombuffer(got["grid"][1]).reshape(n_all, -1)[2:3].tobytes()


# ---- end to end --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hopper_problems():
    """saa 0.1 and 0.5 at S = 6, M = 4 from the baseline's solution (computed once; do not modify)"""
    flds = H.fields(H.M_SMALL)
    base = hopper_model(H.S_SMALL, H.M_SMALL, 'baseline', 0.1, flds)
    Zb, ib = base.solve()
    assert ib["status"] == "converged"
    models = [hopper_model(H.S_SMALL, H.M_SMALL, 'saa', a, flds) for a in (0.1, 0.5)]
    return dict(fields=flds, models=models, Z0s=[H.warm_start(mm, Zb) for mm in models])


@pytest.mark.parametrize("newton,driver", [("dense", "host"), ("dense", "device"), ("arrow", "device")])
def test_hopper_solve_is_bitwise_under_the_grid_cholesky(newton, driver):
    from riskaversetrajopt_amd import hopper_ipm
    e = hopper_problems()
    kw = dict(newton=newton, driver=driver, max_iter=1000)
    ref = hopper_ipm.solve_batch(e["models"], e["Z0s"], chol='workgroup', **kw)
    got = hopper_ipm.solve_batch(e["models"], e["Z0s"], chol='grid', **kw)
    retries = [info["factorizations"] - info["iterations"] for _, info in ref]
    print(f"newton={newton} driver={driver}: delta_w retries of the chol='workgroup' run per problem {retries}")
    # the reference run met failed factorizations, so the bitwise match below covers the grid form's failing path and the delta_w
    # retry on its kept scratch; no problem had to be added for it: alpha 0.1 / 0.5 show 40 / 60 retries (32 / 34 iterations)
    assert max(retries) > 0
    for k, (mm, Z0) in enumerate(zip(e["models"], e["Z0s"])):
        assert got[k][1]["status"] == "converged"
        assert bitwise(got[k], ref[k]), ("chol='grid' differs from chol='workgroup'", k)
        assert bitwise(got[k], mm.solve(Z0, chol='grid', **kw)), ("the batch differs from the solo run", k)
        H.check_solution(mm, e["fields"], *got[k])


@pytest.mark.parametrize("driver", ["host", "device"])
def test_drone_gaussian_solve_is_bitwise_under_the_grid_cholesky(driver):
    from riskaversetrajopt_amd import drone_gaussian as dg, drone_gaussian_ipm as m
    S = min(T.CASES)
    alphas = T.CASES[S]
    models = [dg.Model(S, alpha=a, device=DEV) for a in alphas]
    kw = dict(tol=T.TOL, max_iter=300, backend='device', driver=driver)
    ref = m.solve_batch(models, T.starts(S, alphas), chol='workgroup', **kw)
    got = m.solve_batch(models, T.starts(S, alphas), chol='grid', **kw)
    for k, a in enumerate(alphas):
        assert got[k][1]["status"] == "converged"
        assert bitwise(got[k], ref[k]), ("chol='grid' differs from chol='workgroup'", a)
        solo, = m.solve_batch([models[k]], T.starts(S, [a]), chol='grid', **kw)
        assert bitwise(got[k], solo), ("the batch differs from the solo run", a)
        T.check_solution(S, a, *got[k])
