"""GPU: the branches of rato_qp_ipm_batch_f64 (csrc/qp_ipm.hip) that the inputs of tests/test_gpu_qp_ipm.py never take -- there
every iteration factors once.

  * the retry ladder: the restore of the lower triangle from the strict upper triangle and ``diag``, the rung arithmetic, the
    factorization count, info[6] (the last delta_w) and the exhausted exit, by ``_qp_ipm.saddle`` (a rung count fixed by the
    design, not by rounding) and ``_qp_ipm.deficient`` (reached by rounding); both proven on the host twin in
    tests/test_qp_ipm_cpu.py;
  * a batch whose workgroups leave the loop at different places;
  * tol <= 0, max_iter <= 0, a max_iter exit with an exact count, and max_iter above the kernel's cap of 200 on an input that
    runs all 200 iterations (``_qp_ipm.CAP_QP``: a tolerance no fp64 residual reaches);
  * padded strides of every array, by raw calls (``solve_device`` only passes tight ones);
  * the entry point's largest shapes, n = 256 and m = 384 (107,856 bytes of dynamic LDS).
No case is meant to fault: the loops have compile-time caps and every exit here is an ordinary status.

Measured on the MI355X (iterations / factorizations; the host twin gives the same counts on every one of these inputs):
  saddle (70, 85)        c = 1e-11   c = 1e-7   c = 1e-3        saddle (33, 40), j = 32, c = 1e-7:   15 / 60
    j = 0                16 / 32     16 / 64    16 / 96         saddle (130, 85), j = 96, c = 1e-7:  13 / 52
    j = 31               14 / 28     14 / 56    14 / 84
    j = 32               14 / 28     14 / 56    14 / 84
    j = 69               13 / 26     13 / 52    13 / 78
  deficient (n, r, m, scale): (33, 10, 20, 1) 11 / 18, last delta_w 1e-8; (65, 20, 40, 1e4) 17 / 48, last delta_w 1e-2;
    (70, 35, 50, 1e6) 20 / 72, last delta_w 1
  constructed, k = 0, 1: (256, 384) 18, 18; (255, 383) 19, 17; (256, 0) 1, 1; (1, 384) 9, 6 -- one factorization each
  cap (``_qp_ipm.CAP_QP``, tol 1e-17): ``max_iter`` at 150 / 1356 for max_iter = 150, at 200 / 1856 for 200 and for 10**6
What each saddle position pins: a failure in the first panel (j = 0, 31) leaves the matrix as it was, so those two pin the
counts and delta_w; at j >= 32 a panel has been factored before the failure, and a kernel that restored the diagonal on top of
the previous rung's, or did not restore the lower triangle, ends ``numerical`` or ``max_iter`` there.
"""
import numpy as np
import pytest

import _qp_ipm as H
from test_gpu_qp_ipm import ipm, status_of, three_problems

pytestmark = pytest.mark.gpu
TOL = H.TOL


def solve1(P, q, A, l, u, tol=TOL, max_iter=100):
    """one problem straight to the kernel (``solve_device`` skips the presolve) -> z, y, info row"""
    Z, Y, info = ipm().solve_device(P[None], q[None], A[None], l[None], u[None], tol, max_iter)
    return Z[0], Y[0], info[0]


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. the deterministic ladder ------------------------------------------------------------------------------------------------
def saddle_cases():
    cases = [(70, 85, j, c) for j in (0, 31, 32, 69) for c in (1e-11, 1e-7, 1e-3)]   # first pivot, panel edge, panel 2, last pivot
    return cases + [(33, 40, 32, 1e-7), (130, 85, 96, 1e-7)]                          # j = 96: behind two trailing-tile updates


@pytest.mark.parametrize("n,m,j,c", saddle_cases())
def test_saddle_climbs_the_designed_rungs_on_the_device(n, m, j, c):
    """every iteration fails at pivot j exactly RUNGS[c] - 1 times: the counts, the last delta_w bitwise, z_j exactly 0, and the
    other variables at ``constructed``'s solution -- which they reach only if every rung restored the matrix it factors"""
    P, q, A, l, u, zs, _, keep = H.saddle(n, m, j, c, 1000 * n + 10 * m + j)
    z, y, info = solve1(P, q, A, l, u)
    rungs = H.RUNGS[c]
    print(f"saddle n={n} m={m} j={j} c={c:g}: {status_of(info)} in {int(info[1])} iterations, {int(info[2])} factorizations, "
          f"delta_w {info[6]:g}")
    assert status_of(info) == "solved" and 0 < info[1] <= H.ITER_CAP
    assert info[2] == rungs * info[1]
    assert np.float64(info[6]).tobytes() == np.float64(H.rung(rungs - 1)).tobytes()
    assert z[j] == 0.0
    H.assert_kkt(P, q, A, l, u, z, y, what=f"saddle n={n} m={m} j={j} c={c:g}")
    assert np.max(np.abs(z[keep] - zs[keep])) <= H.constructed_bound(P[np.ix_(keep, keep)], A[:, keep], zs[keep])


# ---- 2. the exhausted ladder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [0, 32])
def test_exhausted_ladder_ends_numerical_at_the_start_point(j):
    P, q, A, l, u, _, _, _ = H.saddle(70, 85, j, 1e13, 1000 * 70 + 10 * 85 + j)
    z, y, info = solve1(P, q, A, l, u)
    assert status_of(info) == "numerical"
    assert info[1] == 0 and info[2] == 13
    assert np.float64(info[6]).tobytes() == np.float64(H.rung(12)).tobytes()
    assert np.all(z == 0.0)                                          # the last finite iterate: the start
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(info))


# ---- 3. the ladder reached by rounding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r,m,scale", H.DEFICIENT)
def test_deficient_qps_retry_and_solve_on_the_device(n, r, m, scale):
    """rank r < n: at least 20 surplus pivots are rounding noise, about 1e3 delta_w in size, so a solve without a single retry
    is not a credible outcome; the solution is not unique and the KKT residuals judge it"""
    P, q, A, l, u = H.deficient(n, r, m, n, scale)
    z, y, info = solve1(P, q, A, l, u)
    print(f"deficient n={n} r={r} m={m} scale={scale:g}: {status_of(info)}, {int(info[2])} factorizations in {int(info[1])} "
          f"iterations, last delta_w {info[6]:g}")
    assert status_of(info) == "solved" and info[1] <= H.ITER_CAP
    H.assert_kkt(P, q, A, l, u, z, y, what=f"deficient n={n} r={r}")
    assert info[2] > info[1]


# ---- 4. workgroups that diverge ---------------------------------------------------------------------------------------------------
def test_diverging_batch_equals_the_solo_launches_bitwise():
    """one shape, three fates: one factorization per iteration, four per iteration, and out after 13 attempts"""
    n, m, j = 70, 85, 32
    seed = 1000 * n + 10 * m + j                                      # the saddles proven on the twin
    probs = [H.constructed(n, m, seed)[:5], H.saddle(n, m, j, 1e-7, seed)[:5], H.saddle(n, m, j, 1e13, seed)[:5]]
    P, q, A, l, u = (np.stack([p[i] for p in probs]) for i in range(5))
    Z, Y, info = ipm().solve_device(P, q, A, l, u, TOL, 100)
    assert [status_of(r) for r in info] == ["solved", "solved", "numerical"]
    assert info[0, 2] == info[0, 1] and info[1, 2] == 4 * info[1, 1] and info[2, 2] == 13
    for k in range(3):
        z1, y1, i1 = solve1(P[k], q[k], A[k], l[k], u[k])
        assert same_bytes((z1, y1, i1), (Z[k], Y[k], info[k])), k


# ---- 5. caps and defaults -----------------------------------------------------------------------------------------------------------
def test_defaults_and_caps_bitwise():
    P, q, A, l, u, _, _ = H.constructed(33, 65, 33065)
    ref = solve1(P, q, A, l, u, 1e-8, 100)
    assert status_of(ref[2]) == "solved"
    for tol in (0.0, -1.0):
        assert same_bytes(solve1(P, q, A, l, u, tol, 100), ref), tol
    for max_iter in (0, -5):
        assert same_bytes(solve1(P, q, A, l, u, 1e-8, max_iter), ref), max_iter
    z, y, info = solve1(P, q, A, l, u, 1e-8, 3)
    assert ref[2][1] > 3                                              # (the cap binds)
    assert status_of(info) == "max_iter" and info[1] == 3 and info[2] == 3 and np.all(np.isfinite(z))
    # the infeasible pair never ends 'solved'; it may leave early as 'numerical', so this is NOT the test of the cap (the next is)
    Pb, qb, Ab, lb, ub = (a[1] for a in three_problems())
    capped = solve1(Pb, qb, Ab, lb, ub, 1e-8, 200)
    assert status_of(capped[2]) in ("max_iter", "numerical") and capped[2][1] <= 200
    assert same_bytes(solve1(Pb, qb, Ab, lb, ub, 1e-8, 10 ** 6), capped)


def test_max_iter_above_the_hard_cap_is_clamped_to_200():
    """``_qp_ipm.CAP_QP`` at tol = 1e-17 never meets the stop rule and keeps finite iterates (proven on the twin), so max_iter is
    the only exit: 200 iterations for max_iter = 200, the same bytes for 10**6 (without the clamp the loop's own bound would
    end it at 201), other bytes for 150"""
    P, q, A, l, u, _, _ = H.constructed(*H.CAP_QP)
    at200, above, at150 = (solve1(P, q, A, l, u, H.CAP_TOL, mi) for mi in (200, 10 ** 6, 150))
    print(f"cap: {status_of(at200[2])} in {int(at200[2][1])} iterations, {int(at200[2][2])} factorizations; "
          f"max_iter=150: {status_of(at150[2])} in {int(at150[2][1])}")
    assert status_of(at200[2]) == "max_iter" and at200[2][1] == 200 and np.all(np.isfinite(at200[0]))
    assert status_of(at150[2]) == "max_iter" and at150[2][1] == 150
    assert same_bytes(above, at200)
    assert at150[0].tobytes() != at200[0].tobytes()                   # the last 50 iterations move the point: the cap is what binds


# ---- 6. padded strides ---------------------------------------------------------------------------------------------------------------
def test_padded_strides_equal_the_tight_call_bitwise():
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    K, n, m = 3, 33, 65
    lda = n
    probs = [H.constructed(n, m, 700 + k) for k in range(K)]
    data = dict(P=[p[0].reshape(-1) for p in probs], q=[p[1] for p in probs], A=[p[2].reshape(-1) for p in probs],
                l=[p[3] for p in probs], u=[p[4] for p in probs])
    tight = dict(P=n * n, q=n, A=m * lda, lu=m, z=n, y=m)
    loose = dict(P=n * n + 7, q=n + 1, A=m * lda + 5, lu=m + 3, z=n + 2, y=m + 4)
    nbytes = lib.rato_qp_ipm_workspace_bytes(K, n, m)

    def call(s):
        def up(rows, stride):                                         # (K, stride), every gap NaN
            buf = np.full((K, stride), np.nan)
            for k, r in enumerate(rows):
                buf[k, :r.size] = r
            return torch.as_tensor(buf, device="cuda:0")
        P, q, A = up(data["P"], s["P"]), up(data["q"], s["q"]), up(data["A"], s["A"])
        l, u = up(data["l"], s["lu"]), up(data["u"], s["lu"])
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
        z, y, info, work = nan(K, s["z"]), nan(K, s["y"]), nan(K, 8), nan(nbytes // 8)
        p = _lib.ptr
        assert lib.rato_qp_ipm_batch_f64(K, n, m, p(P), s["P"], p(q), s["q"], p(A), lda, s["A"], p(l), p(u), s["lu"], TOL, 100,
                                         p(z), s["z"], p(y), s["y"], p(info), p(work), nbytes, _lib.current_stream()) == 0
        torch.cuda.synchronize()
        return z.cpu().numpy(), y.cpu().numpy(), info.cpu().numpy()
    zt, yt, it = call(tight)
    zl, yl, il = call(loose)
    assert [status_of(r) for r in it] == ["solved"] * K
    for k in range(K):
        H.assert_kkt(*probs[k][:5], zt[k], yt[k], what=f"tight strides k={k}")
    assert same_bytes((zl[:, :n], yl[:, :m], il), (zt, yt, it))
    assert np.all(np.isnan(zl[:, n:])) and np.all(np.isnan(yl[:, m:]))


# ---- 7. the largest shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(256, 384), (255, 383), (256, 0), (1, 384)])
def test_constructed_qps_at_the_largest_shapes(n, m):
    """the assertions of test_constructed_qps_on_the_device at the limits of the entry point (one more of either is EINVAL)"""
    K = 2
    probs = [H.constructed(n, m, 1000 * n + 10 * m + k) for k in range(K)]
    P, q, A, l, u = (np.stack([p[i] for p in probs]) for i in range(5))
    Z, Y, info = ipm().solve_device(P, q, A.reshape(K, m, n), l.reshape(K, m), u.reshape(K, m), TOL, 100, lda=n + 3)
    assert Z.shape == (K, n) and Y.shape == (K, m) and np.all(np.isfinite(Z)) and np.all(np.isfinite(Y)) and np.all(np.isfinite(info))
    for k in range(K):
        print(f"n={n} m={m} k={k}: {status_of(info[k])} in {int(info[k, 1])} iterations, {int(info[k, 2])} factorizations")
        assert status_of(info[k]) == "solved" and info[k, 1] <= H.ITER_CAP
        H.assert_kkt(P[k], q[k], A[k].reshape(m, n), l[k], u[k], Z[k], Y[k], what=f"device n={n} m={m} k={k}")
        zs = probs[k][5]
        assert np.max(np.abs(Z[k] - zs)) <= H.constructed_bound(P[k], A[k].reshape(m, n), zs)
