"""GPU: the kernels of csrc/hopper_ipm.hip and csrc/chol.hip (``ipm.chol_factor`` / ``chol_solve``) and the device backend of
``hopper_ipm``.

The Cholesky and its solve are held to the textbook elementwise backward-error bounds (Higham, Accuracy and Stability of
Numerical Algorithms, Thm 10.3 / 10.4), which hold for any summation order: |L L' - A| <= gamma_(n+1) |L| |L'| and
|b - A x| <= gamma_(3n+1) |L| |L'| |x|, gamma_k = k u / (1 - k u), u = 2^-53; the left sides are evaluated in extended
precision.  The normal matrix is held to gamma_(T+2) sum |terms| per entry (T triples), as on the CPU."""
import numpy as np
import pytest

import _hopper_ipm as H
from _hopper_ipm import dense_reference, designed_values, gamma, map_cases

pytestmark = pytest.mark.gpu
LD = np.longdouble


def ipm():
    from riskaversetrajopt_amd import hopper_ipm
    return hopper_ipm


def chol():
    from riskaversetrajopt_amd import ipm as method
    return method


def NB():
    return chol().chol_panel_width()


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


def sizes():
    nb = 32                              # asserted against the kernel's in the test; 3 nb: the trailing tiles' first edge
    return [1, 2, nb - 1, nb, nb + 1, 2 * nb, 2 * nb + 1, 3 * nb, 3 * nb + 1, 130]


@pytest.mark.parametrize("kind", ["bbt", "graded"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", sizes())
def test_cholesky_and_solve_backward_error(n, pad, kind):
    import torch
    m = chol()
    assert NB() == 32
    K, lda = 3, n + pad
    As = [spd(kind, n, 10 * n + k) for k in range(K)]
    A0 = padded(As, lda)
    L1, L2 = A0.clone(), A0.clone()
    info = m.chol_factor(L1)
    m.chol_factor(L2)
    assert info.cpu().tolist() == [0] * K
    assert L1.cpu().numpy().tobytes() == L2.cpu().numpy().tobytes()  # two calls are bitwise equal
    assert untouched(L1, n)
    Lh = L1.cpu().numpy()
    r, c = np.tril_indices(n)
    for k in range(K):
        L = np.zeros((n, n))
        L[r, c] = Lh[k, r, c]
        err = np.abs(L.astype(LD) @ L.T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * (np.abs(L) @ np.abs(L).T).astype(LD)), (k, float(err.max()))
        single = A0[k:k + 1].clone()                                 # problem k of the batch is bitwise its K = 1 call
        assert m.chol_factor(single).cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == Lh[k:k + 1].tobytes()
    rng = np.random.RandomState(n)
    for nrhs in (1, 3):
        ldb = n + 2
        bh = np.full((K, nrhs, ldb), np.nan)
        bh[:, :, :n] = rng.uniform(-1, 1, (K, nrhs, n))
        X1, X2 = torch.as_tensor(bh, device="cuda:0"), torch.as_tensor(bh, device="cuda:0")
        m.chol_solve(L1, X1)
        m.chol_solve(L1, X2)
        xh = X1.cpu().numpy()
        assert xh.tobytes() == X2.cpu().numpy().tobytes() and np.all(np.isnan(xh[:, :, n:]))
        for k in range(K):
            L = np.zeros((n, n))
            L[r, c] = Lh[k, r, c]
            LL = np.abs(L) @ np.abs(L).T
            for j in range(nrhs):
                x = xh[k, j, :n]
                res = np.abs(bh[k, j, :n].astype(LD) - As[k].astype(LD) @ x.astype(LD))
                assert np.all(res <= gamma(3 * n + 1) * (LL @ np.abs(x)).astype(LD)), (k, j, float(res.max()))
            one = torch.as_tensor(bh[k:k + 1], device="cuda:0")
            m.chol_solve(L1[k:k + 1].contiguous(), one)
            assert one.cpu().numpy().tobytes() == xh[k:k + 1].tobytes()


@pytest.mark.parametrize("what", ["negative", "nan"])
@pytest.mark.parametrize("jname", ["0", "NB-1", "NB", "n-1"])
def test_indefinite_input_is_reported_not_faulted(jname, what):
    """what the solver meets on every delta_w retry: info = j + 1, the neighbours bitwise unaffected, the call returns 0"""
    m = chol()
    n = 70
    j = {"0": 0, "NB-1": NB() - 1, "NB": NB(), "n-1": n - 1}[jname]
    rng = np.random.RandomState(j)
    As = []
    for k in range(3):
        A = rng.uniform(-1, 1, (n, n))
        A = (A + A.T) / 2 + n * np.eye(n)                            # diagonally dominant
        As.append(A)
    As[1][j, j] = -1.0 if what == "negative" else np.nan
    buf = padded(As, n + 3)
    ref = [buf[k:k + 1].clone() for k in (0, 2)]
    info = m.chol_factor(buf)                                         # raises on a non-zero status
    assert info.cpu().tolist() == [0, j + 1, 0]
    for k, single in zip((0, 2), ref):
        assert m.chol_factor(single).cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == buf[k:k + 1].cpu().numpy().tobytes()
    assert untouched(buf, n)


# ---- the Cholesky at the workload's sizes ---------------------------------------------------------------------------------------
# n = 400 is the hopper's dense step at S = M = 30, 370 its arrow core, 387 the drone at S = 64.  With 256 lanes the three
# one-lane-per-row loops (step 2 of chol_factor, "rows below" and "rows above" of chol_solve) take a second trip from n = 289
# on (row 32 + 256), which the sizes above never reach.
def lower(Lh, n):
    L = np.zeros((n, n))
    r, c = np.tril_indices(n)
    L[r, c] = Lh[r, c]
    return L


@pytest.mark.parametrize("kind", ["bbt", "graded"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [288, 289, 321, 400, 545, 577])
def test_cholesky_and_solve_backward_error_at_the_workloads_sizes(n, pad, kind):
    """the assertions of test_cholesky_and_solve_backward_error with K = 2: 288 is the last size of one trip, 289 the first of
    two in all three loops, 321 one panel more, 400 the workload's; 545 and 577 take a third trip (from row 32 + 512), and 577
    ends in a diagonal block of one row"""
    import torch
    m = chol()
    assert NB() == 32
    K, lda = 2, n + pad
    As = [spd(kind, n, 10 * n + k) for k in range(K)]
    A0 = padded(As, lda)
    L1, L2 = A0.clone(), A0.clone()
    info = m.chol_factor(L1)
    m.chol_factor(L2)
    assert info.cpu().tolist() == [0] * K
    assert L1.cpu().numpy().tobytes() == L2.cpu().numpy().tobytes()  # two calls are bitwise equal
    assert untouched(L1, n)
    Lh = L1.cpu().numpy()
    Ls = [lower(Lh[k], n) for k in range(K)]
    LLs = [np.abs(L) @ np.abs(L).T for L in Ls]
    for k in range(K):
        err = np.abs(Ls[k].astype(LD) @ Ls[k].T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * LLs[k].astype(LD)), (k, float(err.max()))
        single = A0[k:k + 1].clone()                                 # problem k of the batch is bitwise its K = 1 call
        assert m.chol_factor(single).cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == Lh[k:k + 1].tobytes()
    rng = np.random.RandomState(n)
    for nrhs in (1, 3):
        ldb = n + 2
        bh = np.full((K, nrhs, ldb), np.nan)
        bh[:, :, :n] = rng.uniform(-1, 1, (K, nrhs, n))
        X1, X2 = torch.as_tensor(bh, device="cuda:0"), torch.as_tensor(bh, device="cuda:0")
        m.chol_solve(L1, X1)
        m.chol_solve(L1, X2)
        xh = X1.cpu().numpy()
        assert xh.tobytes() == X2.cpu().numpy().tobytes() and np.all(np.isnan(xh[:, :, n:]))
        for k in range(K):
            for j in range(nrhs):
                x = xh[k, j, :n]
                res = np.abs(bh[k, j, :n].astype(LD) - As[k].astype(LD) @ x.astype(LD))
                assert np.all(res <= gamma(3 * n + 1) * (LLs[k] @ np.abs(x)).astype(LD)), (k, j, float(res.max()))
            one = torch.as_tensor(bh[k:k + 1], device="cuda:0")
            m.chol_solve(L1[k:k + 1].contiguous(), one)
            assert one.cpu().numpy().tobytes() == xh[k:k + 1].tobytes()


@pytest.mark.parametrize("what", ["negative", "nan"])
@pytest.mark.parametrize("j", [288, 300, 329])
def test_indefinite_input_behind_a_second_trip_row(j, what):
    """n = 330: the failing pivot sits in a row that only a second-trip lane of step 2 has solved (row >= 32 + 256);
    info = j + 1, the neighbours bitwise unaffected"""
    m = chol()
    n = 330
    rng = np.random.RandomState(j)
    As = []
    for k in range(3):
        A = rng.uniform(-1, 1, (n, n))
        As.append((A + A.T) / 2 + n * np.eye(n))                     # diagonally dominant
    As[1][j, j] = -1.0 if what == "negative" else np.nan
    buf = padded(As, n + 3)
    ref = [buf[k:k + 1].clone() for k in (0, 2)]
    info = m.chol_factor(buf)
    assert info.cpu().tolist() == [0, j + 1, 0]
    for k, single in zip((0, 2), ref):
        assert m.chol_factor(single).cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == buf[k:k + 1].cpu().numpy().tobytes()
    assert untouched(buf, n)


def test_more_workgroups_than_compute_units():
    """K = 300 problems in one launch (256 compute units): every info word 0, problems 0, 150 and 299 bitwise their K = 1 calls,
    and their factors within the bound"""
    m = chol()
    K, n = 300, 33
    rng = np.random.RandomState(300)
    As = []
    for k in range(K):
        B = rng.uniform(-1, 1, (n, n))
        A = B @ B.T + np.eye(n)
        As.append((A + A.T) / 2)
    A0 = padded(As, n + 3)
    L = A0.clone()
    assert m.chol_factor(L).cpu().tolist() == [0] * K
    assert untouched(L, n)
    Lh = L.cpu().numpy()
    for k in (0, 150, 299):
        single = A0[k:k + 1].clone()
        assert m.chol_factor(single).cpu().tolist() == [0]
        assert single.cpu().numpy().tobytes() == Lh[k:k + 1].tobytes()
        Lk = lower(Lh[k], n)
        err = np.abs(Lk.astype(LD) @ Lk.T.astype(LD) - As[k].astype(LD))
        assert np.all(err <= gamma(n + 1) * (np.abs(Lk) @ np.abs(Lk).T).astype(LD)), (k, float(err.max()))


def test_device_base_scatters_a_retry_and_gathers_a_subset():
    """``ipm.DeviceBase`` on its own (no model): all four problems factored, problem 2 factored again with another matrix as a
    delta_w retry does, then a solve for problems 0, 2, 3 -- row 2 must come from the SECOND factor, problem 1's factor must
    survive the scatter"""
    import torch
    m = chol()
    n_all, n = 4, 65
    lda = n + 3
    As = [spd("bbt", n, 650 + k) for k in range(n_all)]
    A2 = spd("graded", n, 659)
    first, second = padded(As, lda), padded([A2], lda)
    Lref, Lref2 = first.clone(), second.clone()
    assert m.chol_factor(Lref).cpu().tolist() == [0] * n_all and m.chol_factor(Lref2).cpu().tolist() == [0]
    be = m.DeviceBase(torch.device("cuda:0"), n_all)
    assert be.factor_device([0, 1, 2, 3], first) == [0] * n_all
    assert be.L.shape == (n_all, n, lda) and be.L.cpu().numpy().tobytes() == Lref.cpu().numpy().tobytes()
    keep1 = be.L[1].cpu().numpy().tobytes()
    assert be.factor_device([2], second) == [0]
    Lh = be.L.cpu().numpy()
    assert Lh[1].tobytes() == keep1                                   # untouched by the scatter
    assert Lh[2].tobytes() == Lref2[0].cpu().numpy().tobytes()
    assert Lh[0].tobytes() == Lref[0].cpu().numpy().tobytes() and Lh[3].tobytes() == Lref[3].cpu().numpy().tobytes()
    rng = np.random.RandomState(65)
    B = [rng.uniform(-1, 1, n) for _ in range(3)]
    X = be.solve_device([0, 2, 3], B)
    assert X.shape == (3, n)

    def within_bound(A, Ldev, b, x):                                  # |b - A x| <= gamma_(3n+1) |L| |L'| |x| for factor Ldev of A
        Lk = lower(Ldev.cpu().numpy(), n)
        res = np.abs(b.astype(LD) - A.astype(LD) @ x.astype(LD))
        return bool(np.all(res <= gamma(3 * n + 1) * ((np.abs(Lk) @ np.abs(Lk).T) @ np.abs(x)).astype(LD)))
    for row, (Ldev, A) in enumerate(((Lref[0:1], As[0]), (Lref2, A2), (Lref[3:4], As[3]))):
        b = torch.as_tensor(B[row][None, None, :].copy(), device="cuda:0")
        m.chol_solve(Ldev.contiguous(), b)
        assert b[0, 0].cpu().numpy().tobytes() == X[row].tobytes(), row
        assert within_bound(A, Ldev[0], B[row], X[row]), row          # row 1: the retry's matrix, not the first one


def device_model(S, M, method, phases, alpha=0.2):
    from riskaversetrajopt_amd import hopper
    return hopper.Model(M, method, alpha, S=S, fields=H.fields(M), phases=phases, precision='f64')


@pytest.mark.parametrize("S,M,method,phases", map_cases())
def test_normal_matrix_and_matvecs_on_the_device(S, M, method, phases):
    import torch
    m = ipm()
    model = device_model(S, M, method, phases)
    st = m.structure(model)
    be = m.DeviceBackend([model] * 3)
    K, n = 3, st["n"]
    designed = [designed_values(st, 7 + S + 10 * M + 100 * k) for k in range(K)]
    vals, d = np.stack([v for v, _ in designed]), [w for _, w in designed]
    rng = np.random.RandomState(2)
    hess, diag = rng.randn(K, S + 1, 78), rng.rand(K, n)
    be.set_values(vals, hess)
    out = torch.full((K, n, n + 3), float("nan"), dtype=torch.float64, device=model.device)
    Kc = be.normal_matrix([0, 1, 2], d, None, with_hess=False, out=out).cpu().numpy()
    low = np.tril(np.ones((n, n), dtype=bool))
    assert np.all(np.isnan(Kc[:, :, :n][:, ~low])) and np.all(np.isnan(Kc[:, :, n:]))          # upper triangle and padding untouched
    structural = np.zeros(n * n, dtype=bool)
    structural[st["ent_keys"]] = True
    full = be.normal_matrix([0, 1, 2], d, list(diag)).cpu().numpy()
    for k in range(K):
        ref, mag, T = dense_reference(st, vals[k], d[k])
        bound = np.array([gamma(int(t) + 2) for t in T.reshape(-1)], dtype=LD).reshape(T.shape) * mag
        A = Kc[k, :, :n]
        assert np.all((np.abs(A.astype(LD) - ref) <= bound)[low])                                   # dense NumPy
        host = m.normal_matrix_host(st, vals[k], d[k])
        assert np.all((np.abs(A.astype(LD) - host.astype(LD)) <= bound)[low])                   # the CPU product map
        outside = low & ~structural.reshape(n, n)
        assert not np.any(A[outside]) and not np.any(np.signbit(A[outside]))                        # zero fill
        Wd = m.normal_matrix_host(st, np.zeros(st["nnz"]), np.zeros(st["ncon"]), hess[k])
        want = (np.where(low, A, 0.0) + np.tril(Wd)) + np.diag(diag[k])
        assert np.array_equal(np.where(low, full[k], 0.0), want)                                    # W, then the diagonal
    be1 = m.DeviceBackend([model])
    x, w = rng.randn(K, n), rng.randn(K, st["ncon"])
    Jx, JTw = np.stack(be.matvec([0, 1, 2], list(x))), np.stack(be.tmatvec([0, 1, 2], list(w)))
    for k in range(K):                                                # K = 3 against singles is bitwise
        be1.set_values(vals[k:k + 1], hess[k:k + 1])
        one = be1.normal_matrix([0], [d[k]], [diag[k]]).cpu().numpy()
        assert np.where(low, one[0], 0.0).tobytes() == np.where(low, full[k], 0.0).tobytes()
        assert be1.matvec([0], [x[k]])[0].tobytes() == Jx[k].tobytes()
        assert be1.tmatvec([0], [w[k]])[0].tobytes() == JTw[k].tobytes()
        J = np.zeros((st["ncon"], n), dtype=LD)
        J[st["rows"], st["cols"]] = vals[k]
        aJ = np.abs(J)
        nr, nc = np.diff(st["row_ptr"]), np.diff(st["indptr"])
        assert np.all(np.abs(Jx[k] - J @ x[k]) <= np.array([gamma(int(t) + 1) for t in nr]) * (aJ @ np.abs(x[k])))
        assert np.all(np.abs(JTw[k] - J.T @ w[k]) <= np.array([gamma(int(t) + 1) for t in nc]) * (aJ.T @ np.abs(w[k])))


@pytest.mark.parametrize("S", [2, 6])
def test_one_newton_step_residual(S):
    """The device step's relative residual in the UNCONDENSED regularised KKT system (dense J and W of the restatement) is at
    most 10 x what backend='numpy' leaves on the same system at the same designed interior iterate.  The margin of 10 covers a
    different summation order, nothing else.  Measured on the host (backend='numpy', 'saa', M = 4, two refinement steps):
    3.4e-11 at S = 2, 1.0e-13 at S = 6; without refinement 1.1e-2 and 6.0e-7, so the refinement is what the bound tests."""
    m = ipm()
    M, flds = 4, H.fields(4)
    host = H.host_model('saa', 0.2, S, M)
    r_np, dw_np = H.newton_residual(m.NumpyBackend([host], [H.RestatementCallbacks(host, flds)]), host, flds, S, M)
    model = device_model(S, M, 'saa', None)
    r_dev, dw_dev = H.newton_residual(m.DeviceBackend([model]), model, flds, S, M)
    print("newton residual S=%d: device %.3e numpy %.3e (delta_w %g / %g)" % (S, r_dev, r_np, dw_dev, dw_np))
    assert dw_dev == dw_np
    assert r_dev <= 10.0 * r_np


@pytest.fixture(scope="module")
def end_to_end():
    from riskaversetrajopt_amd import hopper
    flds = H.fields(H.M_SMALL)
    mk = lambda method, a: hopper.Model(H.M_SMALL, method, a, S=H.S_SMALL, fields=flds, precision='f64')
    base = mk('baseline', 0.1)
    Zb, ib = base.solve()
    models = [base, mk('saa', 0.1), mk('saa', 0.3)]
    Z0s = [None, H.warm_start(models[1], Zb), H.warm_start(models[2], Zb)]
    return dict(fields=flds, models=models, Z0s=Z0s, base=(Zb, ib))


@pytest.mark.parametrize("k", [0, 1, 2], ids=["baseline", "saa0.1", "saa0.3"])
def test_end_to_end_solve_on_the_device(end_to_end, k):
    e = end_to_end
    model = e["models"][k]
    Z, info = e["base"] if k == 0 else model.solve(e["Z0s"][k])
    print("device", k, info["status"], info["iterations"], info["factorizations"], info["E0"])
    assert info["status"] == "converged" and info["backend"] == "device" and info["iterations"] <= 3000
    H.check_solution(model, e["fields"], Z, info)
    Zn, inn = model.solve(e["Z0s"][k], backend='numpy')               # the step on the host, the Model's callbacks
    print("numpy ", k, inn["status"], inn["iterations"], inn["factorizations"], inn["E0"])
    assert inn["status"] == "converged" and inn["backend"] == "numpy"
    H.check_solution(model, e["fields"], Zn, inn)


def test_device_batch_is_bitwise_the_solo_runs(end_to_end):
    """the two SAA problems in one lockstep batch (one group: alpha differs) against their own K = 1 runs"""
    e = end_to_end
    batch = ipm().solve_batch(e["models"][1:], e["Z0s"][1:])
    for k, (Z, info) in zip((1, 2), batch):
        Z1, i1 = e["models"][k].solve(e["Z0s"][k])
        assert info["status"] == i1["status"] == "converged"
        assert Z.tobytes() == Z1.tobytes() and info["iterations"] == i1["iterations"]


def test_run_hopper_and_experiment_write_the_scripts_files(tmp_path):
    """scp.run_hopper on one model, and scp.hopper_experiment at S = 6, M = 4: baseline first, then the alphas in one batch from
    its solution; the files hold xs then us of the returned solutions"""
    from riskaversetrajopt_amd import hopper, scp
    flds = H.fields(H.M_SMALL)
    model = hopper.Model(H.M_SMALL, 'baseline', S=H.S_SMALL, fields=flds, precision='f64')
    r = scp.run_hopper(model)
    assert r["status"] == "converged" and r["xs"].shape == (H.S_SMALL + 1, 8) and r["us"].shape == (H.S_SMALL, 4)
    H.check_solution(model, flds, r["Z"], r["info"])
    out = scp.hopper_experiment(alphas=(0.1, 0.3), M=H.M_SMALL, S=H.S_SMALL, seed=1, results_dir=str(tmp_path))
    assert out["base"]["Z"].tobytes() == r["Z"].tobytes()             # the fields of RandomState(1), the same start
    assert list(out["status"]) == ["converged", "converged"] and out["alphas"] == [0.1, 0.3]
    for name, sol in (("hopper_base_results.npy", out["base"]), ("hopper_saa_alpha=0.1_results.npy", out["results"][0]),
                      ("hopper_saa_alpha=0.3_results.npy", out["results"][1])):
        xs, us = scp.load_results(str(tmp_path / name), 2)
        assert np.array_equal(xs, sol["xs"]) and np.array_equal(us, sol["us"])
    for a, sol in zip((0.1, 0.3), out["results"]):
        H.check_solution(hopper.Model.host_only(H.M_SMALL, method='saa', alpha=a, S=H.S_SMALL), flds, sol["Z"], sol["info"])
