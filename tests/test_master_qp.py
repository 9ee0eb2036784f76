"""CPU: the master QP of the cutting-plane loop (csrc/master.hip, csrc/rato_nnls.h; host code) against references that do
not share its NNLS formulation (tests/_master_designs.py): the enumeration of every active set in fp64 for up to 10 rows, and
the KKT certificate of the returned (z, lam) for longer sequences.  ``dense_qp.MasterPy``, the NumPy twin the other tests
compare the native master with, shares its formulas -- and shared its defect: a row that vanishes in the null space of the
equalities, or a very loose one, put a huge entry into the NNLS problem whose 1-norm scaled the KKT tolerance of every column
beyond every dual, and status 1 came back with all rows ignored.

Measured here (native master against the enumeration, every healthy design, chunked and in one go):
  |z - z_ref| / max(1, |z_ref|_inf)  <= 3.4e-15  (more rows than n - m_eq + 1, all ten rows)
  |R'lam - R'mu_ref| / max(1, |R'mu_ref|_inf) <= 9.2e-15  (the same design; lam itself is not unique with duplicate rows)
  certificate of the returned (z, lam), worst part <= 2.2e-15; over the 300 solves of the churn sequence <= 3.1e-15
Z_TOL, LAM_TOL and CERT_TOL are 100 x those; Z_TOL stays far under the 1e-8 max(1, |z|) that
test_dense_qp.py::test_native_master_equals_the_numpy_master grants the twin comparison, so that cap is not reached."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import nnls

import _master_designs as md
from riskaversetrajopt_amd import dense_qp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

Z_TOL = 3.4e-13       # 100 x 3.4e-15 (measured, above)
LAM_TOL = 9.2e-13     # 100 x 9.2e-15
CERT_TOL = 3.1e-13    # 100 x 3.1e-15
assert Z_TOL <= 1e-8

HEALTHY = md.healthy_designs()
VANISHING = md.vanishing_designs()
LOOSE = md.loose_designs()
_WORST = {"z": 0.0, "lam": 0.0, "cert": 0.0}


@pytest.fixture(scope="module")
def lib():
    from riskaversetrajopt_amd import _build, _lib
    _build.build()
    return _lib.load()


def _ptr(a):
    return a.ctypes.data if a.size else None


def run_lib(lib, d, chunks=None):
    """the sequence through the library -> (create status, [(status, rows, z, lam) per solve])"""
    chunks = d.chunks if chunks is None else chunks
    pd, q, A, b, R, r = (np.ascontiguousarray(a, dtype=np.float64) for a in (d.pd, d.q, d.A, d.b, d.R, d.r))
    n = q.shape[0]
    h = C.c_void_p()
    rc = lib.rato_master_create(C.byref(h), n, pd.ctypes.data, q.ctypes.data, A.shape[0], _ptr(A), _ptr(b))
    if rc != 0:
        assert not h.value
        return rc, []
    out, done = [], 0
    try:
        for upto in chunks:
            assert lib.rato_master_add_rows(h, int(upto - done), R[done:].ctypes.data, r[done:].ctypes.data) == 0
            done = int(upto)
            z, lam = np.zeros(n), np.zeros(done)
            st = lib.rato_master_solve(h, z.ctypes.data, _ptr(lam))
            out.append((st, lib.rato_master_rows(h), z, lam))
    finally:
        lib.rato_master_destroy(h)
    return rc, out


def _against_enumeration(d, rows, st, z, lam, what):
    ref = md.enumerate_reference(d.pd, d.q, d.A, d.b, d.R[:rows], d.r[:rows])
    assert ref is not None, (what, "the design is infeasible")
    z_ref, mu = ref
    assert st == 1, (what, st)
    ez = np.abs(z - z_ref).max() / max(1.0, np.abs(z_ref).max())
    gl, gr = d.R[:rows].T @ lam, d.R[:rows].T @ mu
    el = np.abs(gl - gr).max() / max(1.0, np.abs(gr).max())
    ec = md.certificate_worst(md.certificate(d.pd, d.q, d.A, d.b, d.R[:rows], d.r[:rows], z, lam))
    return ez, el, ec


def _check_healthy(lib, d, chunks):
    rc, solves = run_lib(lib, d, chunks)
    assert rc == 0 and len(solves) == len(chunks)
    for upto, (st, rows, z, lam) in zip(chunks, solves):
        assert rows == upto
        ez, el, ec = _against_enumeration(d, upto, st, z, lam, (d.name, upto))
        for k, e in (("z", ez), ("lam", el), ("cert", ec)):
            _WORST[k] = max(_WORST[k], e)
        print(f"{d.name!r} rows={upto}: z {ez:.2e} lam {el:.2e} certificate {ec:.2e}; worst so far {_WORST}")
        assert ez <= Z_TOL and el <= LAM_TOL and ec <= CERT_TOL, (d.name, upto, ez, el, ec)
        assert lam.min(initial=0.0) >= 0.0


@pytest.mark.parametrize("d", HEALTHY, ids=lambda d: d.name)
def test_healthy_designs_equal_the_enumeration(lib, d):
    """status 1, the enumeration's z and R'lam and a clean certificate at every solve of the chunked sequence and with all rows
    added at once (plain random with and without active rows, m_eq = 1 and n - 1, rows scaled 1e-8 .. 1e8, optima at |v| ~ 1e3
    and 1e6, exact duplicates, more rows than n - m_eq + 1, n = 24 with a 1e4 penalty entry)"""
    _check_healthy(lib, d, d.chunks)
    _check_healthy(lib, d, (len(d.r),))


def test_churn_sequence_keeps_a_clean_certificate(lib):
    """300 solves, one new tangent plane of a growing ball per solve: the passive set turns over, the kept factor is updated and
    downdated past FACTOR_REFRESH; every solve returns 1 with a clean certificate, and the last 10 rows' active set is the
    enumeration's when restricted to the rows that carry a multiplier"""
    d = md.churn_design()
    rc, solves = run_lib(lib, d)
    assert rc == 0
    worst, turned = 0.0, 0
    prev = None
    for upto, (st, rows, z, lam) in zip(d.chunks, solves):
        assert st == 1 and rows == upto, (upto, st)
        c = md.certificate_worst(md.certificate(d.pd, d.q, d.A, d.b, d.R[:upto], d.r[:upto], z, lam))
        worst = max(worst, c)
        assert c <= CERT_TOL, (upto, c)
        act = frozenset(np.flatnonzero(lam > 0.0))
        turned += prev is not None and not (prev <= act)         # a row left the passive set
        prev = act
    print(f"churn: worst certificate {worst:.2e}, solves at which a row left the passive set: {turned}")
    assert turned >= 97, turned                                  # more downdates than FACTOR_REFRESH
    # the final solve against the enumeration over its active rows plus the newest ones (<= 10)
    act = sorted(prev)
    assert len(act) <= 8
    keep = sorted(set(act) | set(range(len(d.r) - (10 - len(act)), len(d.r))))
    z_ref, _ = md.enumerate_reference(d.pd, d.q, d.A, d.b, d.R[keep], d.r[keep])
    z = solves[-1][2]
    assert np.all(d.R @ z_ref - d.r <= 1e-9 * (np.linalg.norm(d.R, axis=1) * np.linalg.norm(z_ref) + np.abs(d.r)))
    assert np.abs(z - z_ref).max() <= Z_TOL * max(1.0, np.abs(z_ref).max())


def _without(d, upto):
    idx = [j for j in range(upto) if j not in d.without]
    return md.enumerate_reference(d.pd, d.q, d.A, d.b, d.R[idx], d.r[idx])[0]


@pytest.mark.parametrize("d", VANISHING, ids=lambda d: d.name)
def test_a_row_that_vanishes_in_the_null_space_of_the_equalities(lib, d):
    """a combination of equality rows / an all-zero row.  With slack: the solution is what it is without the row, the row's
    multiplier is 0, the certificate of the whole problem is clean.  Violated: RATO_EINFEASIBLE from the solve after the row
    was added, and from every later one.  (The parent commit returned status 1 with every row ignored: rows violated by 6.5.)"""
    for chunks in (d.chunks, (len(d.r),)):
        rc, solves = run_lib(lib, d, chunks)
        assert rc == 0
        for upto, (st, rows, z, lam) in zip(chunks, solves):
            gone = [j for j in d.without if j < upto]
            if d.kind == "infeasible" and gone:
                assert st == md.EINFEASIBLE, (d.name, upto, st)
                assert md.enumerate_reference(d.pd, d.q, d.A, d.b, d.R[:upto], d.r[:upto]) is None
                continue
            ez, el, ec = _against_enumeration(d, upto, st, z, lam, (d.name, upto))
            assert ez <= Z_TOL and el <= LAM_TOL and ec <= CERT_TOL, (d.name, upto, ez, el, ec)
            z0 = _without(d, upto)
            assert np.abs(z - z0).max() <= Z_TOL * max(1.0, np.abs(z0).max()), (d.name, upto)
            assert np.all(lam[gone] == 0.0)


@pytest.mark.parametrize("d", LOOSE, ids=lambda d: d.name)
def test_a_very_loose_row_changes_nothing(lib, d):
    """one row with offset 1e6 .. 1e18 (in units of its own norm), as the last row and as the first: status 1, the enumeration's
    z, which is the z without the row, and a clean certificate.  (Parent commit: violation 6.6e-2 at 1e14, 6.5 at 1e15.)"""
    rc, solves = run_lib(lib, d)
    assert rc == 0
    for upto, (st, rows, z, lam) in zip(d.chunks, solves):
        ez, el, ec = _against_enumeration(d, upto, st, z, lam, (d.name, upto))
        assert ez <= Z_TOL and el <= LAM_TOL and ec <= CERT_TOL, (d.name, upto, ez, el, ec)
        idx = [j for j in range(upto) if j not in d.without]
        if idx:
            z0 = _without(d, upto)
            assert np.abs(z - z0).max() <= Z_TOL * max(1.0, np.abs(z0).max()), (d.name, upto)
        assert np.all(lam[[j for j in d.without if j < upto]] == 0.0)


@pytest.mark.parametrize("d", VANISHING + LOOSE[::3] + HEALTHY[:2], ids=lambda d: d.name)
def test_the_numpy_twin_treats_those_rows_the_same_way(d):
    """``dense_qp.MasterPy`` on the vanishing and loose rows (and two healthy designs): the enumeration's z or InfeasibleError.
    Its tolerance is the one test_dense_qp.py grants the twin, 1e-8 max(1, |z|)."""
    m = dense_qp.MasterPy(np.diag(d.pd), d.q, d.A, d.b)
    done = 0
    for upto in d.chunks:
        m.add_rows(d.R[done:upto], d.r[done:upto])
        done = upto
        ref = md.enumerate_reference(d.pd, d.q, d.A, d.b, d.R[:upto], d.r[:upto])
        if ref is None:
            with pytest.raises(dense_qp.InfeasibleError):
                m.solve()
            continue
        z, lam = m.solve()
        assert np.abs(z - ref[0]).max() <= 1e-8 * max(1.0, np.abs(ref[0]).max()), (d.name, upto)
        assert lam.shape == (upto,) and lam.min() >= 0.0
        assert md.certificate_worst(md.certificate(d.pd, d.q, d.A, d.b, d.R[:upto], d.r[:upto], z, lam)) <= 1e-8


def test_native_and_twin_agree_through_the_facade():
    """``dense_qp.Master`` (the factory the SCP uses) picks the native master for these designs, and it raises / returns what
    MasterPy does on a vacuous and on a violated vanishing row"""
    for d in VANISHING[:2]:
        nat, ref = dense_qp.Master(np.diag(d.pd), d.q, d.A, d.b), dense_qp.MasterPy(np.diag(d.pd), d.q, d.A, d.b)
        assert isinstance(nat, dense_qp.MasterNative)
        for m in (nat, ref):
            m.add_rows(d.R, d.r)
        if d.kind == "infeasible":
            for m in (nat, ref):
                with pytest.raises(dense_qp.InfeasibleError):
                    m.solve()
        else:
            (zn, ln), (zr, lr) = nat.solve(), ref.solve()
            np.testing.assert_allclose(zn, zr, rtol=0, atol=1e-8 * max(1.0, np.abs(zr).max()))
            np.testing.assert_allclose(ln, lr, rtol=1e-6, atol=1e-8 * max(1.0, lr.max()))


def test_create_refusals(lib):
    """rank-deficient equalities, m_eq >= n, a non-positive (or NaN) diagonal entry: RATO_EINVAL and no handle"""
    rng, pd, q, A, b, R, r, xf = md._base(0, 12, 3, 2)
    ok = md.Design("ok", pd, q, A, b, R, r, ())
    assert run_lib(lib, ok)[0] == 0
    dep = np.vstack([A, 2.0 * A[0] - A[2]])
    cases = {"dependent equality rows": (pd, dep, dep @ xf), "a zero equality row": (pd, np.vstack([A, np.zeros(12)]), np.append(b, 0.0)),
             "m_eq = n": (pd, rng.randn(12, 12), rng.randn(12)), "m_eq > n": (pd, rng.randn(13, 12), rng.randn(13))}
    for bad in (0.0, -1.0, np.nan):
        p2 = pd.copy()
        p2[5] = bad
        cases[f"diagonal entry {bad}"] = (p2, A, b)
    for name, (p_, A_, b_) in cases.items():
        assert run_lib(lib, md.Design(name, p_, q, A_, b_, R, r, ()))[0] == -1, name
    h = C.c_void_p()
    assert lib.rato_master_create(None, 12, pd.ctypes.data, q.ctypes.data, 3, A.ctypes.data, b.ctypes.data) == -1
    assert lib.rato_master_create(C.byref(h), 0, pd.ctypes.data, q.ctypes.data, 0, None, None) == -1
    assert lib.rato_master_create(C.byref(h), 12, pd.ctypes.data, q.ctypes.data, 3, None, None) == -1 and not h.value


def test_entry_point_edges(lib):
    """rato_master_solve before any row is the equality-constrained minimiser (lam may be NULL); rato_master_add_rows with
    k = 0 changes nothing; rato_master_rows counts; NULL handles and negative k are RATO_EINVAL; no equalities at all"""
    rng, pd, q, A, b, R, r, xf = md._base(0, 12, 3, 8)
    d = md.Design("edges", pd, q, A, b, R, r, (0, 0, 8, 8))
    rc, solves = run_lib(lib, d)
    z_eq = md._eq_minimiser(pd, q, A, b)
    assert rc == 0 and [s[1] for s in solves] == [0, 0, 8, 8] and all(s[0] == 1 for s in solves)
    assert np.abs(solves[0][2] - z_eq).max() <= Z_TOL * max(1.0, np.abs(z_eq).max())
    assert np.array_equal(solves[0][2], solves[1][2])
    assert np.array_equal(solves[2][2], solves[3][2]) and np.array_equal(solves[2][3], solves[3][3])   # a repeated solve
    assert lib.rato_master_rows(None) == -1 and lib.rato_master_add_rows(None, 0, None, None) == -1
    assert lib.rato_master_solve(None, None, None) == -1
    h = C.c_void_p()
    assert lib.rato_master_create(C.byref(h), 12, pd.ctypes.data, q.ctypes.data, 3, A.ctypes.data, b.ctypes.data) == 0
    try:
        z = np.zeros(12)
        assert lib.rato_master_add_rows(h, -1, R.ctypes.data, r.ctypes.data) == -1
        assert lib.rato_master_add_rows(h, 1, None, r.ctypes.data) == -1 and lib.rato_master_rows(h) == 0
        assert lib.rato_master_solve(h, None, None) == -1
        assert lib.rato_master_add_rows(h, 1, R.ctypes.data, r.ctypes.data) == 0
        assert lib.rato_master_solve(h, z.ctypes.data, None) == -1             # a row, but nowhere to put its multiplier
    finally:
        lib.rato_master_destroy(h)
    lib.rato_master_destroy(None)
    free = md.Design("no equalities", pd, q, np.zeros((0, 12)), np.zeros(0), R, r, (0, 8))
    rc, solves = run_lib(lib, free)
    assert rc == 0 and np.abs(solves[0][2] + q / pd).max() <= 1e-15 * max(1.0, np.abs(q / pd).max())
    ez, el, ec = _against_enumeration(free, 8, *solves[1][0:1], *solves[1][2:], "no equalities")
    assert ez <= Z_TOL and el <= LAM_TOL and ec <= CERT_TOL


# ---- rato_nnls_warm alone ------------------------------------------------------------------------------------------------
def nnls_cases():
    rng = np.random.RandomState(11)
    out = []
    A = rng.randn(6, 9)
    out.append(("every column independent, n > m: the factor fills up", A, A[:, :6] @ (0.5 + rng.rand(6)) + 0.0, None, 0))
    A = rng.randn(8, 6)
    A[:, 3] = A[:, 0] + A[:, 1]
    A[:, 5] = 2.0 * A[:, 2]
    out.append(("a warm guess with dependent columns", A, rng.randn(8), np.ones(6, dtype=np.int64), 0))
    A = rng.randn(7, 5)
    A[:, 2] = 0.0
    out.append(("a zero column, in the guess", A, rng.randn(7), np.array([0, 1, 1, 0, 0]), 0))
    out.append(("m = 1", np.array([[1.0, -2.0, 3.0, 0.5]]), np.array([2.0]), None, 0))
    out.append(("n = 1, positive", rng.rand(5, 1) + 0.1, np.ones(5), None, 0))
    out.append(("n = 1, clamped at 0", rng.rand(5, 1) + 0.1, -np.ones(5), np.array([1]), 0))
    out.append(("m = n = 1", np.array([[2.0]]), np.array([3.0]), None, 0))
    A = rng.randn(12, 8)
    out.append(("maxiter = 1", A, A @ rng.rand(8), None, 1))
    return out


NNLS_CASES = nnls_cases()


def run_nnls(lib, A, b, passive, maxiter):
    m, n = A.shape
    Af = np.asfortranarray(A, dtype=np.float64)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    P = np.zeros(n, dtype=np.uint8) if passive is None else np.asarray(passive, dtype=np.uint8).copy()
    y = np.zeros(n)
    st = lib.rato_nnls_warm(Af.ctypes.data, m, n, bb.ctypes.data, P.ctypes.data, y.ctypes.data, int(maxiter))
    return st, y, P


@pytest.mark.parametrize("name,A,b,passive,maxiter", NNLS_CASES, ids=[c[0] for c in NNLS_CASES])
def test_nnls_alone_against_scipy(lib, name, A, b, passive, maxiter):
    """residual and dual A'(b - A y) against scipy.optimize.nnls: |A y - b| equal to 1e-12 (1 + |b|), the dual <= 1e-12 |A|_1 |b|
    off the passive set and |.| <= that on it, the passive flags are y > 0.  maxiter = 1 returns 0 with y >= 0."""
    st, y, P = run_nnls(lib, A, b, passive, maxiter)
    assert np.all(y >= 0.0) and np.all(np.isfinite(y))
    if maxiter == 1:
        assert st == 0
        return
    y_ref, rn = nnls(A, b, maxiter=50 * A.shape[1])
    assert st == 1 and np.array_equal(P.astype(bool), y > 0.0)
    assert abs(np.linalg.norm(A @ y - b) - rn) <= 1e-12 * (1.0 + np.linalg.norm(b))
    w = A.T @ (b - A @ y)
    bound = 1e-12 * max(np.abs(A).sum(axis=0).max(), 1e-300) * max(np.linalg.norm(b), 1.0)
    assert np.all(w[~P.astype(bool)] <= bound) and np.all(np.abs(w[P.astype(bool)]) <= bound), (name, w)
    if "fills up" in name:
        assert int(P.sum()) == A.shape[0]                          # k == m: b is reproduced exactly
        assert np.abs(A @ y - b).max() <= 1e-12 * (1.0 + np.abs(b).max())


# ---- the same entry points under the address and undefined-behaviour sanitizers ------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("master_host") / "master_host")
    csrc = os.path.join(ROOT, "riskaversetrajopt_amd", "csrc")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(HERE, "host", "master_host.hip"), os.path.join(csrc, "master.hip"), os.path.join(csrc, "nnls.hip"), "-o", path]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return path


def _run_host(exe, tmp_path, write):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write(fin)
    env = dict(os.environ, LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    run = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "master host ok" in run.stdout, (run.returncode, run.stdout, run.stderr[-3000:])
    return np.fromfile(fout)


def _refused():
    rng, pd, q, A, b, R, r, xf = md._base(0, 12, 3, 2)
    return md.Design("rank-deficient equalities", pd, q, np.vstack([A, A[1]]), np.append(b, b[1]), R, r, (2,))


HOST_DESIGNS = HEALTHY + VANISHING + LOOSE + [md.churn_design(), _refused(),
                                              md.Design("k = 0 and no row", *md._base(0, 12, 3, 8)[1:7], (0, 0, 8, 8))]


@needs_hipcc
@pytest.mark.parametrize("d", HOST_DESIGNS, ids=lambda d: d.name)
def test_sanitized_host_program_equals_the_library_bitwise(lib, exe, tmp_path, d):
    """tests/host/master_host.hip + master.hip + nnls.hip under -fsanitize=address,undefined, every array at exactly its size:
    no report, and status, row count, z and lam of every solve are the library's bit for bit"""
    got = _run_host(exe, tmp_path, lambda f: md.write_sequence(f, d))
    rc, solves = run_lib(lib, d)
    want = md.flat_sequence(rc, solves, len(d.q), len(d.r))
    assert got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64)), \
        (d.name, np.flatnonzero(got.view(np.int64) != want.view(np.int64))[:8])


@needs_hipcc
@pytest.mark.parametrize("name,A,b,passive,maxiter", NNLS_CASES, ids=[c[0] for c in NNLS_CASES])
def test_sanitized_nnls_equals_the_library_bitwise(lib, exe, tmp_path, name, A, b, passive, maxiter):
    p = np.zeros(A.shape[1], dtype=np.int64) if passive is None else passive
    got = _run_host(exe, tmp_path, lambda f: md.write_nnls(f, A, b, p, maxiter))
    st, y, P = run_nnls(lib, A, b, passive, maxiter)
    want = np.concatenate([[float(st)], y, P.astype(np.float64)])
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), name
