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
@pytest.mark.parametrize("n", [288, 289, 321, 400, 545, 577])
def test_grid_cholesky_and_solve_at_the_workloads_sizes(n, pad, kind):
    """the sizes at which the workgroup kernels' one-lane-per-row loops take a second trip, and the workload's own; three
    factorizations of fresh copies, bitwise each other's and the workgroup kernel's: the check on the in-place hazard rule
    (a workgroup that read an entry another one of its launch had already overwritten would differ from it, or from run to run;
    on a free chip only -- tests/test_gpu_chol_grid_schedule.py takes the launch off the co-resident schedule).  545 / 577: the
    one-lane-per-row loops of the solve take a third trip (from row 32 + 512); 577 ends in a diagonal block of one row"""
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


# ---- failing in company ----------------------------------------------------------------------------------------------------------
# n = 330: launch 0 has five row blocks, so five panel workgroups of the failing problem meet the pivot and each must find it for
# itself; later launches have trailing tiles, which the return at the top of a launch skips once info[k] is set.
N_COMPANY = 330
BAD_PIVOTS = [(j, "negative") for j in (0, 31, 32, 95, 96, 288, 300, 329)] + [(32, "nan"), (300, "nan")]
ALL_FAIL = (5, 100, 329)


def dominant(n, K, seed):
    rng = np.random.RandomState(seed)
    As = []
    for k in range(K):
        A = rng.uniform(-1, 1, (n, n))
        As.append((A + A.T) / 2 + n * np.eye(n))                     # diagonally dominant
    return As


def all_fail_batch():
    """three diagonally dominant problems of n = 330, pad 3, with a negative pivot at j = 5, 100 and 329"""
    As = dominant(N_COMPANY, 3, 5100329)
    for A, j in zip(As, ALL_FAIL):
        A[j, j] = -1.0
    return padded(As, N_COMPANY + 3)


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("j,what", BAD_PIVOTS)
def test_grid_pivot_failure_in_company(j, what, pos):
    """info = j + 1 for the bad problem wherever it stands in the batch, under both methods; the healthy problems bitwise their
    solo grid factorizations and the workgroup kernel's; the strict upper triangles and the padding untouched, the failed
    problem's included"""
    m = chol()
    n = N_COMPANY
    As = dominant(n, 3, j)
    As[pos][j, j] = -1.0 if what == "negative" else np.nan
    buf = padded(As, n + 3)
    healthy = [k for k in range(3) if k != pos]
    ref = [buf[k:k + 1].clone() for k in healthy]
    old = buf.clone()
    want = [j + 1 if k == pos else 0 for k in range(3)]
    assert m.chol_factor(buf, method='grid').cpu().tolist() == want
    assert m.chol_factor(old, method='workgroup').cpu().tolist() == want
    for k, single in zip(healthy, ref):
        assert m.chol_factor(single, method='grid').cpu().tolist() == [0]
        assert same(single, buf[k:k + 1]) and same(single, old[k:k + 1])
    assert untouched(buf, n)


def test_grid_pivot_failure_of_every_problem():
    m = chol()
    buf = all_fail_batch()
    old = buf.clone()
    want = [j + 1 for j in ALL_FAIL]
    assert m.chol_factor(buf, method='grid').cpu().tolist() == want
    assert m.chol_factor(old, method='workgroup').cpu().tolist() == want
    assert untouched(buf, N_COMPANY)


# ---- hostile leftovers: what outlives a call ------------------------------------------------------------------------------------
def grid_factor_direct(A, info, work):
    """rato_chol_factor_grid_batch_f64 on the caller's own info and work -> the status"""
    from riskaversetrajopt_amd import _lib
    p = _lib.ptr
    return _lib.load().rato_chol_factor_grid_batch_f64(p(A), A.shape[1], A.shape[2], A.shape[0], p(info), p(work), _lib.current_stream())


def test_grid_overwrites_a_stale_info():
    import torch
    m = chol()
    n, K = 130, 3
    A0 = padded([spd("bbt", n, 1300 + k) for k in range(K)], n + 3)
    Lw, Lg = A0.clone(), A0.clone()
    assert m.chol_factor(Lw, method='workgroup').cpu().tolist() == [0] * K
    info = torch.full((K,), 7, dtype=torch.int32, device=A0.device)
    assert grid_factor_direct(Lg, info, m.chol_grid_work(n, K, A0.device)) == OK
    assert info.cpu().tolist() == [0] * K and same(Lg, Lw) and untouched(Lg, n)


@pytest.mark.parametrize("fill", [None, float("nan")], ids=["as-left", "nan"])
def test_grid_on_the_scratch_and_info_a_failed_call_left(fill):
    """the all-fail batch, then, on the same ``work`` and ``info`` untouched in between, a healthy batch of the same shape: what a
    delta_w retry meets.  ``nan``: the scratch holds NaN before the first call"""
    import torch
    m = chol()
    n, K = N_COMPANY, 3
    bad = all_fail_batch()
    work = m.chol_grid_work(n, K, bad.device)
    if fill is not None:
        work.fill_(fill)
    info = torch.empty(K, dtype=torch.int32, device=bad.device)
    assert grid_factor_direct(bad, info, work) == OK
    assert info.cpu().tolist() == [j + 1 for j in ALL_FAIL]
    A0 = padded(dominant(n, K, 330), n + 3)
    Lw, Lg = A0.clone(), A0.clone()
    assert m.chol_factor(Lw, method='workgroup').cpu().tolist() == [0] * K
    assert grid_factor_direct(Lg, info, work) == OK
    assert info.cpu().tolist() == [0] * K and same(Lg, Lw) and untouched(Lg, n)


@pytest.mark.parametrize("n", [33, 400])
def test_grid_stays_inside_its_scratch(n):
    """``work`` is the middle of a buffer of a sentinel: K * rato_chol_grid_work_doubles(n) doubles between two guards"""
    import torch
    from riskaversetrajopt_amd import _lib
    m = chol()
    K, guard, sentinel = 3, 4096, -12345.678
    need = K * int(_lib.load().rato_chol_grid_work_doubles(n))
    assert need > 0
    whole = torch.full((guard + need + guard,), sentinel, dtype=torch.float64, device="cuda:0")
    work = whole[guard:guard + need]
    assert work.is_contiguous() and work.data_ptr() == whole.data_ptr() + 8 * guard
    A0 = padded([spd("bbt", n, 10 * n + k) for k in range(K)], n + 3)
    Lw, Lg = A0.clone(), A0.clone()
    assert m.chol_factor(Lw, method='workgroup').cpu().tolist() == [0] * K
    info = torch.empty(K, dtype=torch.int32, device="cuda:0")
    assert grid_factor_direct(Lg, info, work) == OK
    assert info.cpu().tolist() == [0] * K and same(Lg, Lw)
    assert bool((whole[:guard] == sentinel).all()) and bool((whole[guard + need:] == sentinel).all())


# ---- the batch axis --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [120, 400])
def test_grid_cholesky_and_solve_of_a_large_batch(K):
    """K = 120 is the workload's batch (the SAA grid); K = 400 makes launch 1 about 2000 workgroups, more than the chip holds at
    once.  The whole batch bitwise the workgroup kernels', problems 0, K / 2 and K - 1 bitwise their K = 1 calls and within
    the two bounds"""
    import torch
    m = chol()
    n, pad = 130, 3
    As = [spd("bbt" if k % 2 == 0 else "graded", n, 7000 + k) for k in range(K)]
    A0 = padded(As, n + pad)
    bh = np.full((K, 1, n + 2), np.nan)
    bh[:, :, :n] = np.random.RandomState(K).uniform(-1, 1, (K, 1, n))
    Lg, Lw = A0.clone(), A0.clone()
    Xg, Xw = (torch.as_tensor(bh, device="cuda:0") for _ in range(2))
    assert m.chol_factor(Lg, method='grid').cpu().tolist() == [0] * K
    assert m.chol_factor(Lw, method='workgroup').cpu().tolist() == [0] * K
    m.chol_solve(Lg, Xg, method='grid')
    m.chol_solve(Lw, Xw, method='workgroup')
    assert same(Lg, Lw) and same(Xg, Xw) and untouched(Lg, n)
    Lh, xh = Lg.cpu().numpy(), Xg.cpu().numpy()
    assert np.all(np.isnan(xh[:, :, n:]))
    for k in (0, K // 2, K - 1):
        single, one = A0[k:k + 1].clone(), torch.as_tensor(bh[k:k + 1], device="cuda:0")
        assert m.chol_factor(single, method='grid').cpu().tolist() == [0]
        m.chol_solve(single, one, method='grid')
        assert single.cpu().numpy().tobytes() == Lh[k:k + 1].tobytes() and one.cpu().numpy().tobytes() == xh[k:k + 1].tobytes()
        Lk = lower(Lh[k], n)
        LL = np.abs(Lk) @ np.abs(Lk).T
        err = np.abs(Lk.astype(LD) @ Lk.T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * LL.astype(LD)), (k, float(err.max()))
        x = xh[k, 0, :n]
        res = np.abs(bh[k, 0, :n].astype(LD) - As[k].astype(LD) @ x.astype(LD))
        assert np.all(res <= gamma(3 * n + 1) * (LL @ np.abs(x)).astype(LD)), (k, float(res.max()))
