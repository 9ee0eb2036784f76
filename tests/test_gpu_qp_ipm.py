"""GPU: rato_qp_ipm_batch_f64 (csrc/qp_ipm.hip) and the 'device' backend of ``qp_ipm``; the driving Gaussian SCP through it.

Solutions are judged as in tests/test_qp_ipm_cpu.py: KKT residuals recomputed in NumPy fp64 from the returned (z, y) and the
original data, each <= 2 tol.  Sizes straddle the kernel's internal boundaries:
  * the Cholesky's panel width 32 (n = 31, 32, 33) and its 64 x 64 trailing tiles, which start at row 32 (n = 64, 65: one
    tile; n = 121, 193: two and three tile rows);
  * the wave size 64 (n = 64, 65: the column-per-lane products spill into a second wave) and the workgroup's 256 lanes
    (m = 255, 256, 257, 261: the row-per-lane loops take a second trip);
  * there is NO LDS-versus-workspace switch: the condensed matrix always lives in the caller's workspace.
No case is meant to fault: the not-'solved' cases are ordinary inputs whose expected outcome is a status within the cap."""
import ctypes as C

import numpy as np
import pytest

import _qp_ipm as H

pytestmark = pytest.mark.gpu
TOL = H.TOL
INF = np.inf
SIZES = [(1, 0), (1, 1), (2, 3), (31, 40), (32, 64), (33, 65), (61, 85), (64, 130), (65, 255), (121, 256), (121, 257), (193, 261)]


def ipm():
    from riskaversetrajopt_amd import qp_ipm
    return qp_ipm


def status_of(info_row):
    return ipm().STATUSES[int(info_row[0])]


@pytest.mark.parametrize("K,pad", [(1, 0), (3, 3)])
@pytest.mark.parametrize("n,m", SIZES)
def test_constructed_qps_on_the_device(n, m, K, pad):
    """the designed solution is recovered within ``_qp_ipm.constructed_bound``; lda = n + 3 pads A's rows with NaN and the
    outputs are pre-filled with NaN (``solve_device`` does both)"""
    probs = [H.constructed(n, m, 1000 * n + 10 * m + k) for k in range(K)]
    P, q, A, l, u = (np.stack([p[i] for p in probs]) for i in range(5))
    Z, Y, info = ipm().solve_device(P, q, A.reshape(K, m, n), l.reshape(K, m), u.reshape(K, m), TOL, 100, lda=n + pad)
    assert Z.shape == (K, n) and Y.shape == (K, m) and np.all(np.isfinite(Z)) and np.all(np.isfinite(Y)) and np.all(np.isfinite(info))
    for k in range(K):
        print(f"n={n} m={m} k={k}: {status_of(info[k])} in {int(info[k, 1])} iterations, {int(info[k, 2])} factorizations")
        assert status_of(info[k]) == "solved" and info[k, 1] <= H.ITER_CAP
        H.assert_kkt(P[k], q[k], A[k].reshape(m, n), l[k], u[k], Z[k], Y[k], what=f"device n={n} m={m} k={k}")
        zs = probs[k][5]
        assert np.max(np.abs(Z[k] - zs)) <= H.constructed_bound(P[k], A[k].reshape(m, n), zs)


@pytest.mark.parametrize("l,u", [(-INF, INF), (-INF, 0.5), (1.5, INF), (0.2, 0.6), (1.5, 4.0), (-4.0, -2.0), (0.7, 0.7), (np.nan, 0.5)])
def test_scalar_qp_on_the_device(l, u):
    Z, Y, info = ipm().solve_batch(np.array([[2.0]]), np.array([-2.0]), np.array([[[1.0]]]), np.array([[l]]), np.array([[u]]))
    lo, up = (-INF if np.isnan(l) else l), (INF if np.isnan(u) else u)
    assert info["status"] == ["solved"]
    H.assert_kkt([[2.0]], [-2.0], [[1.0]], [l], [u], Z[0], Y[0], what=f"scalar [{l}, {u}]")
    assert abs(Z[0, 0] - np.clip(1.0, lo, up)) <= 1e-6


@pytest.mark.parametrize("n", [33, 61])
def test_box_and_equality_qps_on_the_device(n):
    P, q, A, l, u, zs = H.box_qp(n, seed=n)
    Z, Y, info = ipm().solve_batch(P, q, A[None], l[None], u[None])
    assert info["status"] == ["solved"] and info["iterations"][0] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, Z[0], Y[0], what=f"box n={n}")
    assert np.max(np.abs(Z[0] - zs)) <= 1e-6
    P, q, A, l, u, zs, ys = H.equality_qp(n, n // 3, seed=100 + n)
    Z, Y, info = ipm().solve_batch(P, q, A[None], l[None], u[None])
    assert info["status"] == ["solved"] and info["iterations"][0] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, Z[0], Y[0], what=f"equality n={n}")
    assert np.max(np.abs(Z[0] - zs)) <= 1e-5 and np.max(np.abs(Y[0] - ys)) <= 1e-5


def driving_cases():
    return [(20, 0.05, "scp_iter0"), (20, 0.05, "warmup1"), (40, 0.01, "main1")] + [(5, a, "main1") for a in H.ALPHAS]


@pytest.mark.parametrize("S,alpha,name", driving_cases())
def test_driving_qps_device_against_twin(S, alpha, name):
    """identical inputs through both backends: the same status, both within the KKT limit, <= 40 iterations; the iteration
    counts may differ (the summation orders do) and the difference is printed"""
    P, q, A, l, u = qp = dict(H.warmup_qps(S, alpha))[name]
    Zd, Yd, idev = ipm().solve_batch(P, q, A[None], l[None], u[None], TOL, 100, backend='device')
    zt, yt, itw = H.twin_solve(qp)
    print(f"S={S} alpha={alpha} {name}: device {idev['status'][0]} in {idev['iterations'][0]}, twin {itw['status']} in "
          f"{itw['iterations']} (difference {int(idev['iterations'][0]) - int(itw['iterations'])})")
    assert idev["status"][0] == itw["status"] == "solved"
    assert idev["iterations"][0] <= H.ITER_CAP and itw["iterations"] <= H.ITER_CAP
    H.assert_kkt(*qp, Zd[0], Yd[0], what="device")
    H.assert_kkt(*qp, zt, yt, what="twin")


def three_problems():
    """a solvable QP, one with the infeasible pair a'z <= -1, a'z >= 1, one with a NaN in A"""
    Pa, qa, Aa, la, ua, _, _ = H.constructed(33, 40, 11)
    Ab, lb, ub = Aa.copy(), la.copy(), ua.copy()
    Ab[1] = Ab[0]
    lb[0], ub[0], lb[1], ub[1] = -INF, -1.0, 1.0, INF
    Ac = Aa.copy()
    Ac[7, 5] = np.nan
    return np.stack([Pa] * 3), np.stack([qa] * 3), np.stack([Aa, Ab, Ac]), np.stack([la, lb, la]), np.stack([ua, ub, ua])


def test_batch_of_three_equals_the_solo_launches_bitwise():
    P, q, A, l, u = three_problems()
    Z, Y, info = ipm().solve_device(P, q, A, l, u, TOL, 100)
    st = [status_of(r) for r in info]
    assert st[0] == "solved" and st[1] in ("max_iter", "numerical") and st[2] == "invalid"
    assert 0 <= info[1, 1] <= 100 and np.all(np.isnan(Z[2])) and np.all(np.isnan(Y[2])) and np.all(np.isfinite(Z[:2]))
    for k in range(3):
        z1, y1, i1 = ipm().solve_device(P[k:k + 1], q[k:k + 1], A[k:k + 1], l[k:k + 1], u[k:k + 1], TOL, 100)
        assert z1.tobytes() == Z[k:k + 1].tobytes() and y1.tobytes() == Y[k:k + 1].tobytes()
        assert i1.tobytes() == info[k:k + 1].tobytes()
    # a stride of 0 shares the objective: the same bits as three copies of it
    Z0, Y0, info0 = ipm().solve_device(P[0], q[0], A, l, u, TOL, 100, shared_objective=True)
    assert Z0.tobytes() == Z.tobytes() and Y0.tobytes() == Y.tobytes() and info0.tobytes() == info.tobytes()


def test_argument_checks_return_einval_without_a_launch():
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    n, m, K = 4, 3, 2
    d = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda:0")
    P, q, A, l, u, z, y = d(K, n, n), d(K, n), d(K, m, n), d(K, m), d(K, m), d(K, n), d(K, m)
    info = torch.full((K, 8), -7.0, dtype=torch.float64, device="cuda:0")
    nbytes = lib.rato_qp_ipm_workspace_bytes(K, n, m)
    assert nbytes == K * n * n * 8 and lib.rato_qp_ipm_workspace_bytes(0, n, m) == 0
    work = d(nbytes // 8)

    def call(K=K, n=n, m=m, P=P, q=q, A=A, lda=n, l=l, u=u, z=z, y=y, info=info, work=work, nbytes=nbytes):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return lib.rato_qp_ipm_batch_f64(K, n, m, p(P), n * n, p(q), n, p(A), lda, m * lda, p(l), p(u), m, TOL, 100, p(z), n, p(y), m,
                                         p(info), p(work), nbytes, _lib.current_stream())
    EINVAL = -1
    for kw in (dict(P=None), dict(q=None), dict(A=None), dict(l=None), dict(u=None), dict(z=None), dict(y=None), dict(info=None),
               dict(work=None), dict(n=0), dict(m=-1), dict(lda=n - 1), dict(K=0), dict(K=65536), dict(nbytes=nbytes - 8),
               dict(n=257), dict(m=385)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert torch.all(info == -7.0)                                # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.all(info[:, 0] == 0.0)                           # z = 0 solves the all-zero problem


@pytest.mark.parametrize("S", [5, 20])
def test_driving_gaussian_scp_through_the_device_solver(S):
    """run_driving_gaussian_batch(solver='ipm'), four alphas, 60 iterations: every solve 'solved', the final L2 step <= 1e-5 per
    alpha, the final controls within 1e-5 of the twin's run (define step of tests/_car_gaussian there, the kernel's here)"""
    from riskaversetrajopt_amd import driving_gaussian as DG
    from riskaversetrajopt_amd import scp
    models = [DG.Model(alpha=a, S=S) for a in H.ALPHAS]
    assert all(m.solver == "osqp" for m in models)
    res = scp.run_driving_gaussian_batch(models, 60, solver='ipm')
    for a, r in zip(H.ALPHAS, res):
        tw = H.twin_scp(S, a)
        diff = float(np.max(np.abs(r["us"] - tw["us"])))
        print(f"S={S} alpha={a}: final L2 step {r['L2_error'][-1]:.3e}, |us - twin| {diff:.3e}, "
              f"statuses {sorted(set(r['status']))}, solve_s {r['solve_s'].sum():.3f}")
        assert r["status"] == ["solved"] * 60
        assert r["L2_error"][-1] <= 1e-5
        assert diff <= 1e-5
