"""GPU: the grid-parallel Cholesky of csrc/chol_grid.hip (``ipm.chol_factor`` / ``chol_solve`` with ``method='grid'``).

Two yardsticks.  The one that is independent of both kernels: the textbook elementwise backward-error bounds (Higham, Accuracy
and Stability of Numerical Algorithms, Thm 10.3 / 10.4), |L L' - A| <= gamma_(n+1) |L| |L'| and
|b - A x| <= gamma_(3n+1) |L| |L'| |x|, the left sides in extended precision.  And the one the solvers' guarantees rest on:
L and X are BITWISE those of the workgroup kernels (csrc/chol.hip) on the same input.  ``spd``, ``padded`` and ``untouched``
are the constructions of tests/test_hopper_ipm_gpu.py."""
import numpy as np
import pytest

from _hopper_ipm import gamma

pytestmark = pytest.mark.gpu
LD = np.longdouble
EINVAL, OK = -1, 0


def chol():
    from riskaversetrajopt_amd import ipm as method
    return method


def spd(kind, n, seed):
    rng = np.random.RandomState(seed)
    if kind == "bbt":
        B = rng.uniform(-1, 1, (n, n))
        A = B @ B.T + np.eye(n)
    else:                                                             # graded: diag(10^(-6 i / n)) Q-conjugated
        Q, _ = np.linalg.qr(rng.randn(n, n))
        A = (Q * 10.0 ** (-6.0 * np.arange(n) / n)) @ Q.T
    return (A + A.T) / 2


def padded(As, lda):
    """(K, n, lda) device tensor: the lower triangles of As, NaN in the strict upper triangle and in the padding"""
    import torch
    K, n = len(As), As[0].shape[0]
    buf = np.full((K, n, lda), np.nan)
    r, c = np.tril_indices(n)
    for k, A in enumerate(As):
        buf[k, r, c] = A[r, c]
    return torch.as_tensor(buf, device="cuda:0")


def untouched(out, n):
    """the strict upper triangle and the padding still hold NaN"""
    o = out.cpu().numpy()
    r, c = np.triu_indices(n, 1)
    return np.all(np.isnan(o[:, r, c])) and np.all(np.isnan(o[:, :, n:]))


def lower(Lh, n):
    L = np.zeros((n, n))
    r, c = np.tril_indices(n)
    L[r, c] = Lh[r, c]
    return L


def same(a, b):
    return a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def check_factor_and_solve(n, pad, kind, K, factor_calls):
    import torch
    m = chol()
    assert m.chol_panel_width() == 32
    lda = n + pad
    As = [spd(kind, n, 10 * n + k) for k in range(K)]
    A0 = padded(As, lda)
    Lold = A0.clone()
    assert m.chol_factor(Lold, method='workgroup').cpu().tolist() == [0] * K
    work = m.chol_grid_work(n, K, A0.device)
    Ls = [A0.clone() for _ in range(factor_calls)]
    for i, Lg in enumerate(Ls):                                       # fresh copies; the last call allocates its own scratch
        info = m.chol_factor(Lg, method='grid', work=work if i + 1 < factor_calls else None)
        assert info.cpu().tolist() == [0] * K
    L1 = Ls[0]
    assert all(same(L1, Lg) for Lg in Ls[1:])                        # repeated calls are bitwise equal
    assert same(L1, Lold)                                            # and bitwise the workgroup kernel's (NaN bytes included)
    assert untouched(L1, n)
    Lh = L1.cpu().numpy()
    Lk = [lower(Lh[k], n) for k in range(K)]
    LLs = [np.abs(L) @ np.abs(L).T for L in Lk]
    for k in range(K):
        err = np.abs(Lk[k].astype(LD) @ Lk[k].T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * LLs[k].astype(LD)), (k, float(err.max()))
        single = A0[k:k + 1].clone()                                 # problem k of the batch is bitwise its K = 1 call
        assert m.chol_factor(single, method='grid').cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == Lh[k:k + 1].tobytes()
    rng = np.random.RandomState(n)
    for nrhs in (1, 3):
        ldb = n + 2
        bh = np.full((K, nrhs, ldb), np.nan)
        bh[:, :, :n] = rng.uniform(-1, 1, (K, nrhs, n))
        X1, X2, Xold = (torch.as_tensor(bh, device="cuda:0") for _ in range(3))
        m.chol_solve(L1, X1, method='grid')
        m.chol_solve(L1, X2, method='grid')
        m.chol_solve(L1, Xold, method='workgroup')
        xh = X1.cpu().numpy()
        assert same(X1, X2) and same(X1, Xold) and np.all(np.isnan(xh[:, :, n:]))
        for k in range(K):
            for j in range(nrhs):
                x = xh[k, j, :n]
                res = np.abs(bh[k, j, :n].astype(LD) - As[k].astype(LD) @ x.astype(LD))
                assert np.all(res <= gamma(3 * n + 1) * (LLs[k] @ np.abs(x)).astype(LD)), (k, j, float(res.max()))
            one = torch.as_tensor(bh[k:k + 1], device="cuda:0")
            m.chol_solve(L1[k:k + 1].contiguous(), one, method='grid')
            assert one.cpu().numpy().tobytes() == xh[k:k + 1].tobytes()


@pytest.mark.parametrize("kind", ["bbt", "graded"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 96, 97, 130])
def test_grid_cholesky_and_solve(n, pad, kind):
    check_factor_and_solve(n, pad, kind, K=3, factor_calls=2)


@pytest.mark.parametrize("kind", ["bbt", "graded"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [288, 289, 321, 400])
def test_grid_cholesky_and_solve_at_the_workloads_sizes(n, pad, kind):
    """the sizes at which the workgroup kernels' one-lane-per-row loops take a second trip, and the workload's own; three
    factorizations of fresh copies, bitwise each other's and the workgroup kernel's: the check on the in-place hazard rule
    (a workgroup that read an entry another one of its launch had already overwritten would differ from it, or from run to run)"""
    check_factor_and_solve(n, pad, kind, K=2, factor_calls=3)


@pytest.mark.parametrize("j,what", [(0, "negative"), (31, "negative"), (32, "negative"), (69, "negative"), (32, "nan")])
def test_grid_pivot_failure(j, what):
    """info = j + 1 for the middle problem, its neighbours bitwise their solo factorizations, the padding untouched"""
    m = chol()
    n = 70
    rng = np.random.RandomState(j)
    As = []
    for k in range(3):
        A = rng.uniform(-1, 1, (n, n))
        As.append((A + A.T) / 2 + n * np.eye(n))                     # diagonally dominant
    As[1][j, j] = -1.0 if what == "negative" else np.nan
    buf = padded(As, n + 3)
    ref = [buf[k:k + 1].clone() for k in (0, 2)]
    old = buf.clone()
    info = m.chol_factor(buf, method='grid')                          # raises on a non-zero status
    assert info.cpu().tolist() == [0, j + 1, 0]
    assert m.chol_factor(old, method='workgroup').cpu().tolist() == [0, j + 1, 0]
    for k, single in zip((0, 2), ref):
        assert m.chol_factor(single, method='grid').cpu().tolist() == [0]
        assert same(single, buf[k:k + 1]) and same(single, old[k:k + 1])
    assert untouched(buf, n)


def test_grid_arguments_are_refused_without_a_launch():
    """valid device buffers, the status only: RATO_EINVAL, and nothing is written"""
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    n, K, nrhs = 40, 2, 2
    A = torch.full((K, n, n), 7.0, dtype=torch.float64, device="cuda:0")
    B = torch.full((K, nrhs, n), 5.0, dtype=torch.float64, device="cuda:0")
    info = torch.full((K,), -3, dtype=torch.int32, device="cuda:0")
    assert lib.rato_chol_grid_work_doubles(n) > 0
    work = torch.full((K * lib.rato_chol_grid_work_doubles(n),), 9.0, dtype=torch.float64, device="cuda:0")
    p = _lib.ptr

    def fac(A_=p(A), n_=n, lda=n, K_=K, info_=p(info), work_=p(work)):
        return lib.rato_chol_factor_grid_batch_f64(A_, n_, lda, K_, info_, work_, None)

    def sol(L=p(A), n_=n, lda=n, K_=K, B_=p(B), nrhs_=nrhs, ldb=n):
        return lib.rato_chol_solve_grid_batch_f64(L, n_, lda, K_, B_, nrhs_, ldb, None)
    for status in (fac(A_=None), fac(info_=None), fac(work_=None), fac(n_=0), fac(lda=n - 1), fac(K_=0), fac(K_=65536),
                   sol(L=None), sol(B_=None), sol(n_=0), sol(n_=8001, lda=8001, ldb=8001), sol(lda=n - 1), sol(ldb=n - 1),
                   sol(K_=0), sol(K_=65536), sol(nrhs_=0)):
        assert status == EINVAL
    torch.cuda.synchronize()
    assert bool((A == 7.0).all()) and bool((B == 5.0).all()) and bool((info == -3).all()) and bool((work == 9.0).all())
    small = torch.eye(32, dtype=torch.float64, device="cuda:0")[None].contiguous()   # the query is 0: work may be NULL
    assert lib.rato_chol_grid_work_doubles(32) == 0
    assert lib.rato_chol_factor_grid_batch_f64(p(small), 32, 32, 1, p(info), None, _lib.current_stream()) == OK
    assert info.cpu().tolist() == [0, -3]
