"""GPU: the interior-point driver's vector kernels spread over the rows (csrc/ipm_driver_grid.hip, ``ipm.DeviceState(vec='grid')``;
DESIGN §7.al).  The grid form returns the bits of the one-workgroup-per-problem form, so nothing here has a tolerance: after
every phase of the driver's chain every array of the state (with its three NaN columns of padding), ``diag`` and ``rec`` under
``vec='grid'`` are the BYTES under ``vec='workgroup'``, for the designed batch of four kinds of problem
(tests/_ipm_driver.py) and for each problem alone, and a second run repeats them.  What the workgroup form computes is held
to its references by test_gpu_ipm_driver.py."""
import ctypes as C

import numpy as np
import pytest

import _drone_gaussian_ipm as T
import _ipm_driver as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 3
VECS = ("workgroup", "grid")


def method():
    from riskaversetrajopt_amd import ipm
    return ipm


def rows():
    from riskaversetrajopt_amd import _lib
    return int(_lib.load().rato_ipm_grid_rows())


def up(a, ld=None):
    import torch
    a = np.asarray(a, dtype=np.float64)
    return torch.as_tensor(np.ascontiguousarray(a if ld is None else T.padded(a, ld)), device=DEV)


def raw(st):
    """every array of the state as it lies on the device"""
    names = st.NV + st.N + st.M + ("diag", "rec")
    return {k: getattr(st, k).cpu().numpy().copy() for k in names}


def differing(a, b):
    """the arrays whose bytes differ"""
    return [k for k in a if a[k].tobytes() != b[k].tobytes()]


def shapes():
    """(n, mE, mI): the smallest sizes at which block boundaries, the last partial block and the n / nv split of the sums can
    go wrong, R rows to a workgroup: nv = n + mI and m = mE + mI at R - 1, R, R + 1, 2 R + 1; n < R < nv; n = R with mI = 0"""
    R = rows()
    return [(1, 0, 1), (1, 1, 0), (5, 2, 3), (300, 10, 700)] + [(5, 5, x - 5) for x in (R - 1, R, R + 1, 2 * R + 1)] + \
        [(R - 6, 3, 20), (R, 7, 0)]


def chain(des, sel, vec, ps=None, keep=None, upto=None):
    """``test_gpu_ipm_driver.device_chain`` with the form as a parameter: residuals, rhs, two ladder attempts, q / r / update
    twice, finish, setup and two trial / accept rounds for the problems ``sel`` of the designed batch, the other kernels'
    results replaced by the designed vectors -> [(phase, raw state)] after each phase.  ``keep``: the phases to take a snapshot
    after (None: all); ``upto='setup'``: the chain ends after the step setup"""
    import torch
    n, m = des["n"], des["m"]
    ps = [D.problems(des)[k] for k in sel] if ps is None else ps
    st = method().DeviceState(ps, DEV, ldv=n + des["nI"] + PAD, ldm=m + PAD, vec=vec)
    assert (st.work is not None) == (vec == "grid")
    pick = lambda a, length: up(np.asarray(a)[sel], length + PAD)
    trail = []
    snap = lambda phase: trail.append((phase, raw(st))) if keep is None or phase in keep else None

    def put(name, a):
        rws = [i for i, k in enumerate(sel) if k < 2]
        if rws:
            getattr(st, name)[rws, :a.shape[1]] = up(np.asarray(a)[[sel[i] for i in rws]])

    snap("start")
    st.residuals(pick(des["g"], m), pick(des["JTy"], n))
    snap("residuals")
    st.newton("rhs", pick(des["JTw"], n))
    snap("rhs")
    for attempt in (1, 2):                                           # problem 0's factorization fails twice: dw = 1e-4, 8e-4
        st.newton("ladder", info=torch.as_tensor([int(k == 0) for k in sel], dtype=torch.int32, device=DEV), flag=attempt)
        snap("ladder")
    put("dz", des["dz0"])
    for r in range(2):
        st.newton("q", pick(des["Jdz"][r], m), flag=r == 0)
        snap("q")
        st.newton("r", pick(des["Wdz"][r], n), pick(des["JTq"][r], n))
        snap("r")
        put("ez", des["ez"][r])
        st.newton("update", pick(des["Jez"][r], m))
        snap("update")
    st.newton("finish", pick(des["Jdz"][2], m))
    snap("finish")
    put("dv", des["dv"])
    st.step_setup(pick(des["Hdv"], n))
    snap("setup")
    if upto == "setup":
        return trail
    factors = dict(des, ct_factor=[f[sel] for f in des["ct_factor"]])
    for r in range(2):
        st.trial()
        snap("trial")
        got = [D.problems(des)[k] for k in sel]
        st.download(got)
        st.accept(up(D.trial_g(factors, got, r), m + PAD))
        snap("accept")
    return trail


def assert_same_trails(what, got, ref):
    assert [p for p, _ in got] == [p for p, _ in ref]
    for step, ((phase, a), (_, b)) in enumerate(zip(got, ref)):
        assert not differing(a, b), (what, step, phase, differing(a, b))


@pytest.mark.parametrize("pattern", D.PATTERNS)
@pytest.mark.parametrize("shape", range(10), ids=lambda i: "shape%d" % i)
def test_every_phase_is_bitwise_the_workgroup_form(shape, pattern):
    n, mE, mI = shapes()[shape]
    des = D.designed(n, mE, mI, pattern)
    everyone = list(range(D.K))
    grid = chain(des, everyone, "grid")
    assert_same_trails("batch", grid, chain(des, everyone, "workgroup"))
    assert_same_trails("second run", chain(des, everyone, "grid"), grid)
    for k in everyone:
        assert_same_trails(("solo", D.KINDS[k]), chain(des, [k], "grid"), chain(des, [k], "workgroup"))
    # the chain went where it was designed to go: two problems ended in the residual phase, problem 0 took both ladder steps
    from riskaversetrajopt_amd import _lib
    F = {f: i for i, f in enumerate(_lib.IPM_FIELDS)}
    rec = grid[-1][1]["rec"]
    assert rec[:, F["status"]].tolist() == [-1.0, -1.0, 2.0, 0.0]
    assert rec[0, F["dw"]] == 8.0 * 1e-4 and rec[1, F["dw"]] == 0.0 and np.all(rec[:2, F["trials"]] >= 1.0)


def test_an_accepted_step_is_applied_once():
    """Where problem 0 accepts in round 0 and problem 1 is rejected there (its trial residual is 1e3 c) and accepts in round 1,
    the launches of round 1 serve problem 0 again: its v, y, zl, zu must be what round 0 left.  Whether the Armijo test
    rejects problem 1 in round 0 depends on the designed values (nu stays 0 where the nu rule does not fire), so the cases are
    taken from the workgroup form's own record; one of them must have more rows than a workgroup takes."""
    from riskaversetrajopt_amd import _lib
    F = {f: i for i, f in enumerate(_lib.IPM_FIELDS)}
    rounds = lambda des, vec: [s for p, s in chain(des, list(range(D.K)), vec) if p == "accept"]
    found = []
    for n, mE, mI in shapes():
        for pattern in ("both", "mixed"):
            des = D.designed(n, mE, mI, pattern)
            r0, r1 = (s["rec"] for s in rounds(des, "workgroup"))
            if not (r0[0, F["accepted"]] == 1.0 and r0[1, F["accepted"]] == 0.0 and r0[1, F["searching"]] == 1.0 and
                    r1[1, F["accepted"]] == 1.0):
                continue
            found.append((n, mE, mI, pattern))
            for vec in VECS:
                a0, a1 = rounds(des, vec)
                r0, r1 = a0["rec"], a1["rec"]
                assert (r0[0, F["accepted"]], r0[0, F["searching"]], r0[0, F["trials"]]) == (1.0, 0.0, 1.0), vec
                assert (r0[1, F["accepted"]], r0[1, F["searching"]], r0[1, F["trials"]]) == (0.0, 1.0, 1.0), vec
                assert (r1[1, F["accepted"]], r1[1, F["searching"]], r1[1, F["trials"]]) == (1.0, 0.0, 2.0), vec
                assert r1[0].tobytes() == r0[0].tobytes(), vec
                for name in ("v", "y", "zl", "zu"):
                    assert a1[name][0].tobytes() == a0[name][0].tobytes(), (vec, name, "problem 0 moved in round 1")
                    assert a1[name][1].tobytes() != a0[name][1].tobytes(), (vec, name, "problem 1 did not move")
    print("accept in round 0 / round 1:", found)
    assert any(n + mI > rows() for n, mE, mI, _ in found), found


@pytest.mark.parametrize("where", ["zl", "zu", "zl_slack"])
@pytest.mark.parametrize("shape,at", [(2, None), (6, None), (6, "R"), (6, "last"), (7, "R"), (7, "last")],
                         ids=["2", "6", "6-R", "6-last", "7-R", "7-last"])
def test_a_nan_multiplier(shape, at, where):
    """one NaN in zl (zu) of a bounded variable of the mu_loop problem: E0 is NaN and the status 'line_search'.  In zl of a
    bounded SLACK the host's max(a, b) rules drop the NaN from dual and from the complementarity, the problem keeps running
    and the mu loop meets the side's NaN at every pass.  Either way the state is the workgroup form's, byte for byte.
    ``at``: the entry that holds the NaN -- None: the middle of the variables (of the slacks), which is block 0; 'R': the first
    entry of block 1; 'last': the last entry, in the last, partial block.  Both are slacks' entries (n = 5), of zu for 'zu'
    and of zl otherwise.  At shape 6 (nv = R + 1) the two are one entry, the only row of block 1; at shape 7 (nv = 2 R + 1)
    block 1 is a whole block and the last entry is the only row of block 2."""
    from riskaversetrajopt_amd import _lib
    F = {f: i for i, f in enumerate(_lib.IPM_FIELDS)}
    n, mE, mI = shapes()[shape]
    des = D.designed(n, mE, mI, "both")
    got = {}
    for vec in VECS:
        ps = D.problems(des)
        if at is not None:
            pos = rows() if at == "R" else n + mI - 1
            assert n <= rows() <= pos < n + mI
            (ps[0].zu if where == "zu" else ps[0].zl)[pos] = np.nan
        elif where == "zl_slack":
            ps[0].zl[n + mI // 2] = np.nan
        else:
            getattr(ps[0], where)[n // 2] = np.nan
        st = method().DeviceState(ps, DEV, ldv=n + mI + PAD, ldm=des["m"] + PAD, vec=vec)
        st.residuals(up(des["g"], des["m"] + PAD), up(des["JTy"], n + PAD))
        got[vec] = raw(st)
    assert not differing(got["grid"], got["workgroup"]), differing(got["grid"], got["workgroup"])
    rec = got["grid"]["rec"]
    if where == "zl_slack" or at is not None:
        assert rec[0, F["status"]] == -1.0 and np.isfinite(rec[0, F["E0"]])
    else:
        assert np.isnan(rec[0, F["E0"]]) and rec[0, F["status"]] == 2.0
    assert rec[1:, F["status"]].tolist() == [-1.0, 2.0, 0.0]


def test_the_sixtieth_failed_factorization_ends_the_problem():
    import torch
    des = D.designed(5, 2, 3, "mixed")
    info = torch.as_tensor([1, 0, 1, 1], dtype=torch.int32, device=DEV)
    got = {}
    for vec in VECS:
        ps = D.problems(des)
        st = method().DeviceState(ps, DEV, vec=vec)
        st.residuals(up(des["g"]), up(des["JTy"]))
        trail = []
        for flag in (1, 2, 3, 59):
            st.newton("ladder", info=info, flag=flag)
            trail.append(raw(st))
        st.download(ps)
        assert [p.status for p in ps] == [None, None, "line_search", "converged"] and ps[0].dw == 1e-4 * 8.0 ** 3 and ps[1].dw == 0.0
        st.newton("ladder", info=info, flag=60)
        trail.append(raw(st))
        st.download(ps)
        assert [p.status for p in ps] == ["line_search", None, "line_search", "converged"] and ps[0].dw == 1e-4 * 8.0 ** 3
        assert differing(trail[-1], trail[-2]) == ["rec"]            # the sixtieth failure writes the status and nothing else
        got[vec] = trail
    for a, b in zip(got["grid"], got["workgroup"]):
        assert not differing(a, b), differing(a, b)


def test_work_query():
    from riskaversetrajopt_amd import _lib
    q = _lib.load().rato_ipm_grid_work_doubles
    R = rows()
    assert R >= 64 and R % 64 == 0
    for n, nI, m, K in ((1, 0, 1, 1), (5, 3, 5, 4), (R, 0, 7, 2), (R - 1, 1, R + 1, 3), (3 * R, 2 * R, 2 * R + 1, 7)):
        base = q(n, nI, m, K)
        assert base >= K * (2 * (n + nI))                            # the two barrier terms of every entry, at least
        assert q(n + 1, nI, m, K) >= base and q(n, nI + 1, max(m, nI + 1), K) >= base and q(n, nI, m + 1, K) >= base
        assert q(n + R, nI, m, K) > base and q(n, nI, m, K + 1) > base
        assert q(n, nI, m, K) == K * q(n, nI, m, 1)
    assert q(0, 0, 1, 1) == 0 and q(1, -1, 1, 1) == 0 and q(1, 0, 0, 1) == 0 and q(1, 0, 1, 0) == 0


def test_argument_errors():
    """RATO_EINVAL without a launch, the state's bytes untouched: a NULL work, a work one double short, and every case of
    test_gpu_ipm_driver.test_argument_errors through the grid entry points"""
    import torch
    from riskaversetrajopt_amd import _lib
    lib = _lib.load()
    des = D.designed(5, 2, 3, "mixed")
    st = method().DeviceState(D.problems(des), DEV, vec="grid")
    n, m = des["n"], des["m"]
    g, jt, info = up(des["g"]), up(des["JTy"]), torch.zeros(D.K, dtype=torch.int32, device=DEV)
    P, s = _lib.ptr, _lib.current_stream()
    need = lib.rato_ipm_grid_work_doubles(n, des["nI"], m, D.K)
    assert st.work.numel() == need
    W = dict(work=st.work, wl=need)

    def variant(**kw):
        c = _lib.IpmState.from_buffer_copy(st.c_state)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    res = lambda c=st.c_state, g=g, ldg=m, jt=jt, ldj=n, work=W["work"], wl=W["wl"]: \
        lib.rato_ipm_residuals_grid_f64(c, P(g), ldg, P(jt), ldj, 0, P(work), wl, s)
    newton = lambda phase, a=jt, lda=n, b=jt, ldb=n, info=info, flag=1, c=st.c_state, work=W["work"], wl=W["wl"]: \
        lib.rato_ipm_newton_grid_f64(c, phase, P(a), lda, P(b), ldb, P(info), flag, P(work), wl, s)
    setup = lambda h=jt, ldh=n, c=st.c_state, work=W["work"], wl=W["wl"]: lib.rato_ipm_step_setup_grid_f64(c, P(h), ldh, P(work), wl, s)
    trial = lambda c=st.c_state, work=W["work"], wl=W["wl"]: lib.rato_ipm_trial_grid_f64(c, P(work), wl, s)
    accept = lambda gt=g, ldg=m, c=st.c_state, work=W["work"], wl=W["wl"]: lib.rato_ipm_accept_grid_f64(c, P(gt), ldg, P(work), wl, s)
    before = raw(st)
    states = [variant(K=0), variant(K=65536), variant(n=0), variant(nI=-1), variant(m=0), variant(nI=m + 1), variant(ldv=n + 2),
              variant(ldm=m - 1)] + [variant(**{f: None}) for f, t in _lib.IpmState._fields_ if t is C.c_void_p]
    bad = []
    for c in states:
        bad += [res(c=c), newton(0, c=c), setup(c=c), trial(c=c), accept(c=c)]
    bad += [res(g=None), res(ldg=m - 1), res(jt=None), res(ldj=n - 1), newton(6), newton(-1), newton(0, a=None), newton(0, lda=n - 1),
            newton(1, info=None), newton(1, flag=0), newton(2, a=g, lda=m - 1), newton(3, b=None), newton(3, ldb=n - 1),
            newton(4, a=None), newton(5, a=g, lda=m - 1), setup(h=None), setup(ldh=n - 1), accept(gt=None), accept(ldg=m - 1)]
    for short in (dict(work=None), dict(wl=need - 1), dict(wl=0), dict(wl=-1)):
        bad += [res(**short), setup(**short), trial(**short), accept(**short)] + \
            [newton(ph, a=(g if ph in (2, 4, 5) else jt), lda=(m if ph in (2, 4, 5) else n), **short) for ph in range(6)]
    assert all(v == -1 for v in bad), bad                            # RATO_EINVAL
    torch.cuda.synchronize()
    assert not differing(raw(st), before)
    assert res() == 0 and newton(0) == 0 and newton(1) == 0 and newton(2, a=g, lda=m) == 0 and newton(3) == 0 and \
        newton(4, a=g, lda=m) == 0 and newton(5, a=g, lda=m) == 0 and setup() == 0 and trial() == 0 and accept() == 0
    bigger = torch.empty(need + 5, dtype=torch.float64, device=DEV)   # a longer work is as good
    assert res(work=bigger, wl=need + 5) == 0
    torch.cuda.synchronize()


def test_an_unknown_form_is_refused():
    des = D.designed(1, 0, 1, "both")
    with pytest.raises(ValueError):
        method().DeviceState(D.problems(des), DEV, vec="rows")
