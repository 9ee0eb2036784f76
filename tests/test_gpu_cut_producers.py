"""GPU: the producers of the cut oracle -- rato_drone_rowmax_rollout, rato_car_rowmax_rollout, rato_drone_rowmax_implicit,
rato_drone_linearize_generators and the by-value | device-memory switch of rato_cut_oracle_rollout -- at every horizon edge
of their control flow, on designed inputs with closed-form answers and on random samples against the fp64 oracle.

Horizons, from the kernels' arithmetic (csrc/cvar.hip, csrc/drone.hip):
  drone rowmax rollout   double batches of 16 steps unguarded, the last S mod 16 behind guards, loads past the horizon clamped
                         to row S - 1: S mod 16 = 0 (16, 32, 64), a remainder of 1 .. 8 (1, 2, 8, 17, 24, 33, 65: the second
                         guarded batch is empty), 9 .. 15 (9: exactly one step in it; 15, 25, 31)
  driving rowmax rollout the same batches, every step guarded; ego tables of 8 (14 S + 10) bytes of LDS: S = 584 (65488) runs,
                         S = 585 (65600) is refused
  rato_cut_oracle_rollout x by value while S n_u <= 192 doubles: drone 64 | 65, driving 96 | 97
  implicit rowmax        batches of 8: S in {1, 7, 8, 9, 16, 17}; a22_axes 2 and 3; both signs
  generators             forward in guarded double batches of 16, backward in groups of 4 parked in LDS (S mod 4, S mod 16,
                         S < 4); LDS 32 (6 (S + 1) + 1560) bytes: beyond the default 64 KiB between S = 80 (65472) and 81
                         (65664), refused beyond 160 KiB between S = 592 (163776) and 593 (163968)
Batches M in {1, 255, 256, 257, 513} (generators: 1, 5, 255, 256, 257): the row stride ld = 4 ceil(M / 4) exceeds M for all
but 256.  Every output buffer is filled with NaN / -1 first and nothing at an index >= M may change.

Designed cases (tests/_cut_designs.py; tests/test_cut_designs.py shows on the CPU that their expectations are the oracle's and
that every mistake below changes an arg-max row or moves m by >= 1000 tolerances) have NO tolerance: m is the float of an
exact number and the arg-max row an integer.  Random cases are held to bounds that are derived, not fitted: every output is
fp64 arithmetic rounded once to fp32, so
    |device - ref| <= 2^-24 |ref| + 8 spread (+ e22 term)
where ``spread`` is max |oracle's dense form - the direct tangent recursion in np.longdouble| over the case (two evaluations
of the same rows on the CPU; 8 x because the kernel's fma order is a third one), and the e22 term -- g_up and the final rows
of the generators kernel only -- is twice the measured effect of a22 = 1 - float(e22), the table rounding that kernel
documents.  The constants of the parameter struct the fp64 kernels read (dt64, kp64, ...) are the oracle's doubles
(asserted): they add nothing.  No bound is looser than what tests/test_gpu_scp.py holds the same quantity to (m: 6e-8 |m| +
2e-9 scale; g: rtol 1e-6 atol 5e-6; g_up: rtol 5e-5 atol 2e-4; Z: rtol 1e-6 atol 1e-6): the smaller of the two applies.
Arg-max rows are compared wherever the reference's top two rows differ by more than 1e-8 scale, as there.

Measured on the MI355X (RATO_TOL_REPORT=1; profiles/cut_producers_tolerances.txt has every case).  The limit is the final
rounding to within 1e-3 of itself, so a correct kernel comes close to it (records, not tolerances):
  quantity                                   spread (max over the class)   limit at |ref| = 1   worst error / limit
  drone rowmax rollout, random samples       6.3e-13 .. 7.0e-10 (S = 2)    5.96e-8 .. 6.2e-8    0.981
  drone rowmax rollout, standing-still batch <= 4.3e-14                    5.96e-8              0.769
  driving rowmax rollout, random samples     <= 5.4e-13                    5.96e-8              0.978 (S = 584: 0.318)
  driving rowmax rollout, standing still     <= 2.8e-14                    5.96e-8              0.991
  one-call round trip, m                     <= 8.5e-13                    5.96e-8              0.981 (cut gradient 0.003 and
                                                                                                offset 0.026 of their bounds)
  implicit rowmax vs fp64 on its own tables  <= 7.3e-11                    5.96e-8              0.975 (vs the oracle: < 1e-3 of
                                                                                                2e-4 scale)
  generators e22 | W | g | g_up | Z          8.9e-16 | 3.6e-12 | 7.0e-10 | 7.0e-10 | 2.7e-15    0.998 | 0.997 | 0.997 | 0.996 | 0.981
  generators part: Jacobian sums | rhs       2.7e-12 | 2.2e-12 (e22 term <= 2.8e-7 | 1.7e-6 a sample)   0.991 | 0.944
At S <= 8 the random drone samples have their maximum at step 0 (dt = 50 / S is long: the drone has left the obstacles after
one step), where no control enters: there the designs carry the test, not the random samples.

One kernel had to change.  drone_rowmax_rollout_block DROPPED a NaN row (v_max_f64 returns its other operand, the strict >
is false): a sample with a NaN noise value reported the finite maximum of its earlier rows, where the driving kernel and the
oracle report NaN.  It now reports NaN (test_a_nan_row_is_reported_and_touches_no_other_sample[drone] fails on the parent).

Mutation check (scratch builds, one mistake per kernel and build, arithmetic or control only -- never an address; this file
once per build).  Cases that fail, by their horizon S:
  drone rollout    last step dropped                   all 14 S -- S >= 2 ONLY through the 'last_row' design (the random
                                                       samples' maxima are never in the last step), S = 1 through every sample
                   remainder (S mod 16 steps) skipped  every S but 16, 32, 64
                   second guarded batch skipped        9, 15, 25, 31 (S mod 16 in 9 .. 15) and no other
                   >= for > over t                     every S >= 2;     >= for > over the obstacles: all 14
                   control of step t enters row t      all 14, and both drone cases of the one-call round trip
                   no NaN report (the parent commit)   the drone NaN case alone
  driving rollout  last step dropped                   all 9 S;          >= for >: every S >= 7
                   second batch of a pair skipped      9, 16, 17, 33, 96, 97, 584 and both driving one-call cases; not 1, 7, 8
                   NaN row dropped                     the driving NaN case
  implicit rowmax  last step dropped | >= | largest    exact tables at all 6 S
                   partial batch of 8 skipped          exact tables at 1, 7, 9, 17 and not at 8, 16
                   the other table layout              exact and real tables at every S >= 7 (a22 meets v = 0 at S = 1)
  generators       flush_group skipped for a short     1, 2, 3, 5, 15, 17, 31, 33, 81 (S mod 4 != 0) and not 4, 16, 32, 80, 592
                   group
                   forward: last step dropped          all 14 S;         adjoint stops one step early: every S >= 2
A clamped load CONSUMED (the guard of a step past the horizon lost) cannot be built without reading u_k and x past their
ends, so it was not run: tests/test_cut_designs.py models it on the CPU ('last_noise': the noise of step S - 1 is aimed at
the best obstacle / at the ego, so consuming it once more moves m by far more than 1000 tolerances).
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import _cut_designs as cd
from tests import _tail_patterns as tp

pytestmark = pytest.mark.gpu

RATO_EINVAL = -1                                  # rato_saa.h
M_ALL = (1, 255, 256, 257, 513)
POOL = 513
PAD = 8                                           # sentinel entries behind the last lane of a row


def _report(what, spread, err_over_limit, note=""):
    if os.environ.get("RATO_TOL_REPORT"):
        print(f"[tol] {what}: spread {spread:.2e}; worst error / limit {err_over_limit:.3f}{note}")


def _ptr(t):
    from riskaversetrajopt_amd import _lib
    return _lib.ptr(t)


def _f64(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev).contiguous()


def _sentinels(n, dev):
    import torch
    return (torch.full((n,), float("nan"), dtype=torch.float32, device=dev),
            torch.full((n,), -1, dtype=torch.int32, device=dev))


def _untouched(m, a, M):
    import torch
    return bool(torch.isnan(m[M:]).all()) and bool((a[M:] == -1).all())


# ---- the two rollout kernels ----------------------------------------------------------------------------------------
class _Rollout:
    """one system at one (S, M): the device Model on the first M samples of a pool, its parameter struct (with the constants
    of a design written over it) and a launcher that returns (m fp32 (M,), arg (M,)) after checking the sentinels"""

    def __init__(self, system, S, M, samples, const, designed):
        import torch
        from riskaversetrajopt_amd import _lib
        self.system, self.S, self.M = system, S, M
        smp = [a[:M] for a in samples]
        if system == "drone":
            from riskaversetrajopt_amd import drone_risk
            d = drone_risk.Model(S, *smp, 'saa', 0.2)
            dW, mass, Qsym, _ = d._inputs(None)
            self.ld = mass.numel()
            self.p, self.inputs, self.n_u = d._params(M, self.ld), (dW, mass, Qsym), 3
            assert self.ld == (M + 3) // 4 * 4
            if designed:
                cd.apply_drone_const(self.p, const)
            assert (self.p.dt64, self.p.beta64, self.p.kp64, self.p.kd64, self.p.drag64) == (const.dt, const.beta, const.kp, const.kd, const.drag)
            assert all(self.p.x_init64[i] == const.x_init[i] for i in range(6))
            assert all(self.p.obs_xy64[j][a] == const.obs_xy[j, a] for j in range(3) for a in range(2))
            self.name = "rato_drone_rowmax_rollout"
        else:
            from riskaversetrajopt_amd import driving
            d = driving.Model(M, 'saa', 0.2, S=S, samples=smp)
            self.ld = M
            self.p, self.inputs, self.n_u = d._params(M), (d._dW, d._x0, d._ws, d._wr), 2
            if designed:
                cd.apply_car_const(self.p, const)
            assert (self.p.dt64, self.p.beta64, self.p.speed_ped_des64, self.p.d_min64) == (const.dt, const.beta, const.v_des, const.d_min)
            assert all(self.p.ego_init64[i] == smp[0][0, i] for i in range(4))
            self.name = "rato_car_rowmax_rollout"
        self.d, self.dev, self.lib, self._lib, self.torch = d, d.device, d._lib, _lib, torch

    def status(self, uk, x, m, a):
        uk_d, x_d = _f64(uk, self.dev), _f64(x, self.dev)
        rc = getattr(self.lib, self.name)(C.byref(self.p), _ptr(uk_d), *[_ptr(t) for t in self.inputs], _ptr(x_d), _ptr(m), _ptr(a),
                                          self._lib.current_stream())
        self.torch.cuda.synchronize()
        return rc

    def __call__(self, uk, x):
        m, a = _sentinels(self.ld + PAD, self.dev)
        assert self.status(uk, x, m, a) == 0, self.name
        assert _untouched(m, a, self.M), "an index >= M was written"
        return m[:self.M].cpu().numpy(), a[:self.M].cpu().numpy()


def _reference(system, const, samples, uk, x):
    """-> (rows (M, R S) of the fp64 oracle, spread = max |oracle - the direct recursion in long double|)"""
    M = samples[0].shape[0]
    if system == "drone":
        rows = cd.drone_dense(const, samples, uk, x)["rows"].reshape(M, -1)
        ld = cd.drone_direct(const, samples, uk, x, dtype=np.longdouble)["rows"].reshape(M, -1)
    else:
        rows = cd.car_dense(const, samples, uk, x)["rows"]
        ld = cd.car_direct(const, samples, uk, x, dtype=np.longdouble)
    return rows, float(np.abs(rows - ld.astype(np.float64)).max())


def _check_against_rows(what, m32, arg, rows, spread, worst):
    m, m_o, a_o = m32.astype(np.float64), rows.max(axis=1), rows.argmax(axis=1)
    scale = max(1.0, np.abs(rows).max())
    limit = cd.m_limit(m_o, scale, spread)
    ratio = float(np.max(np.abs(m - m_o) / np.maximum(limit, 1e-300)))
    worst.append(ratio)
    assert np.all(np.abs(m - m_o) <= limit), (what, ratio, float(np.abs(m - m_o).max()), spread)
    clear = cd.clear_rows(rows, scale)
    assert np.array_equal(arg[clear], a_o[clear]), (what, np.flatnonzero(arg[clear] != a_o[clear]))
    assert np.all((arg >= 0) & (arg < rows.shape[1])), what


def _random_inputs(system, S):
    rng = np.random.RandomState(4)
    if system == "drone":
        from oracle import drone as od
        samples = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=POOL, S=S)]
        return cd.drone_const(S), samples, tp.graze(S), 0.3 * rng.randn(S, 3)
    from oracle import driving as ocar
    samples = [cd.r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(0), POOL, 'saa', S)]
    return cd.car_const(S), samples, tp.driving_uk(S), 0.3 * rng.randn(S, 2) * np.array([1.0, 0.05])


def _rollout_case(system, S):
    # (a) random samples at the problem's own constants against the fp64 oracle
    const, samples, uk, x = _random_inputs(system, S)
    rows, spread = _reference(system, const, samples, uk, x)
    x_other = x.copy()
    x_other[S - 1] += 1.0                                         # the control of step S - 1 enters no row
    worst = []
    for M in M_ALL:
        run = _Rollout(system, S, M, samples, const, designed=False)
        m, a = run(uk, x)
        _check_against_rows(f"{system} S={S} M={M}", m, a, rows[:M], spread, worst)
        m2, a2 = run(uk, x_other)
        assert np.array_equal(m.view(np.int32), m2.view(np.int32)) and np.array_equal(a, a2), "x at step S - 1 changed a result"
    _report(f"{system} rowmax rollout, random samples, S={S}", spread, max(worst),
            f" (limit at |m| = 1: {float(cd.m_limit(np.array(1.0), 1.0, spread)):.2e})")
    # (b) standing still: exact expectations for the designed samples, the oracle for the others
    d = (cd.drone_still if system == "drone" else cd.car_still)(S, M=POOL)
    ref = {k: _reference(system, d.const, d.samples, uk_, x_) for k, (uk_, x_) in (("zero", (d.uk0, d.x0)), ("step", (d.uk0, d.x_step)))}
    worst = []
    for M in M_ALL:
        run = _Rollout(system, S, M, d.samples, d.const, designed=True)
        out = {"zero": run(d.uk0, d.x0), "last": run(d.uk_last, d.x_last), "step": run(d.uk0, d.x_step)}
        here = d.idx < M
        idx, m_exp, a_exp, st = d.idx[here], d.m[here].astype(np.float32), d.arg[here], d.still[d.idx[here]]
        for k, (m, a) in out.items():
            sel = np.ones(len(idx), bool) if k != "step" else st          # (x at step s moves the one sample that moves)
            assert np.array_equal(m[idx][sel].view(np.int32), m_exp[sel].view(np.int32)), (k, M, m[idx], m_exp, np.array(d.kind)[here])
            assert np.array_equal(a[idx][sel], a_exp[sel]), (k, M, a[idx], a_exp, np.array(d.kind)[here])
        # nothing of step S - 1 (u_k or x) reaches a row: every sample bit for bit
        assert np.array_equal(out["last"][0].view(np.int32), out["zero"][0].view(np.int32)) and np.array_equal(out["last"][1], out["zero"][1])
        for k in ("zero", "step"):
            _check_against_rows(f"{system} still/{k} S={S} M={M}", *out[k], ref[k][0][:M], ref[k][1], worst)
    _report(f"{system} rowmax rollout, standing-still batch, S={S}", max(ref["zero"][1], ref["step"][1]), max(worst))


DRONE_S = (1, 2, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 64, 65)
CAR_S = (1, 7, 8, 9, 16, 17, 33, 96, 97)


@pytest.mark.parametrize("S", DRONE_S)
def test_drone_rowmax_rollout(S):
    _rollout_case("drone", S)


@pytest.mark.parametrize("S", CAR_S)
def test_driving_rowmax_rollout(S):
    _rollout_case("driving", S)


def test_driving_rowmax_rollout_at_the_lds_limit():
    """S = 584: the ego tables take 65488 of the 65536 bytes; S = 585 (65600) is refused and writes nothing"""
    from oracle import driving as ocar
    rng = np.random.RandomState(4)
    for S, M in ((584, 3), (585, 3)):
        samples = [cd.r32(a) for a in ocar.sample_uncertain_parameters(np.random.RandomState(0), M, 'saa', S)]
        const, uk, x = cd.car_const(S), tp.driving_uk(S), 0.3 * rng.randn(S, 2) * np.array([1.0, 0.05])
        run = _Rollout("driving", S, M, samples, const, designed=False)
        if S == 585:
            m, a = _sentinels(M + PAD, run.dev)
            assert run.status(uk, x, m, a) == RATO_EINVAL and _untouched(m, a, 0)
            continue
        rows = cd.car_dense(const, samples, uk, x, chunk=1)["rows"]
        spread = float(np.abs(rows - cd.car_direct(const, samples, uk, x, dtype=np.longdouble).astype(np.float64)).max())
        worst = []
        _check_against_rows(f"driving S={S} M={M}", *run(uk, x), rows, spread, worst)
        _report(f"driving rowmax rollout, random samples, S={S}", spread, max(worst))


# ---- the NaN contract --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["drone", "driving"])
def test_a_nan_row_is_reported_and_touches_no_other_sample(system):
    S, M, k = 20, 300, 70
    const, samples, uk, x = _random_inputs(system, S)
    samples = [a[:M].copy() for a in samples]
    clean = _Rollout(system, S, M, samples, const, designed=False)(uk, x)
    if system == "drone":
        samples[0][k, 3, 3] = np.nan                              # one noise value of sample k
    else:
        samples[0][k, 4:6] = samples[0][k, 0:2]                   # the pedestrian starts where the ego is: |d| = 0
    m, a = _Rollout(system, S, M, samples, const, designed=False)(uk, x)
    others = np.arange(M) != k
    assert not np.isfinite(m[k])
    assert np.array_equal(m[others].view(np.int32), clean[0][others].view(np.int32)) and np.array_equal(a[others], clean[1][others])


# ---- one oracle round trip on both sides of 192 doubles -------------------------------------------------------------------
@pytest.mark.parametrize("system,S", [("drone", 64), ("drone", 65), ("driving", 96), ("driving", 97)])
def test_one_call_round_trip_by_value_and_through_memory(system, S):
    """x rides in the kernel arguments while S n_u <= 192 (drone 64, driving 96) and goes through device memory beyond: either
    way m, arg, the statistics record and the cut sums equal the stepwise calls bit for bit, and the fp64 reference"""
    import torch
    from riskaversetrajopt_amd import stats
    M, alpha = POOL, 0.2                                          # three workgroups, the last one a single sample
    const, samples, uk, x = _random_inputs(system, S)
    run = _Rollout(system, S, M, samples, const, designed=False)
    d, n_u = run.d, run.n_u
    d.alpha = alpha
    cs = d._reduced_cut_solver(M, run.ld) if system == "drone" else d._reduced_cut_solver(M)
    cs.rollout = (system, run.p) + tuple(run.inputs)
    cs.set_linearization_point(uk)
    by_value = S * n_u <= 192
    torch.cuda.synchronize()
    cs.x_dev.fill_(float("nan"))
    u = (uk + x).reshape(-1)
    x_eff = (u - cs.u_lin).reshape(S, n_u)
    phi, t, grad = cs.evaluate(None, None, 0, None, u, slot=3)
    assert bool(torch.isnan(cs.x_dev).all()) == by_value            # by value: x_dev is neither written nor read
    one = (cs.ring_m[3].clone(), cs.ring_arg[3].clone(), cs.ring_res[3].clone(), cs.res_host.clone())
    sign, x0 = cs._form()
    cs._evaluate_stepwise(None, None, 0, None, np.ascontiguousarray(u - x0), sign, cs.ring_m[4], cs.ring_arg[4], cs.ring_res[4])
    assert torch.equal(one[0].view(torch.int32), cs.ring_m[4].view(torch.int32)) and torch.equal(one[1], cs.ring_arg[4])
    assert torch.equal(one[2], cs.ring_res[4]) and np.array_equal(one[3].numpy(), one[2].cpu().numpy())
    # ... and the fp64 reference
    m32, arg, rec = one[0].cpu().numpy(), one[1].cpu().numpy(), one[2].cpu().numpy()
    rows, spread = _reference(system, const, samples, uk, x_eff)
    worst = []
    _check_against_rows(f"one call {system} S={S}", m32, arg, rows, spread, worst)
    w, thr, n_gt, n_eq, lam = tp.weights(m32, alpha, M)
    td, lam_d = np.float32(rec[10]), (min(max((alpha * M - rec[8]) / rec[9], 0.0), 1.0) if rec[9] > 0 else 0.0)
    assert np.array_equal((m32 > td) * 1.0 + (m32 == td) * lam_d, w) and t == rec[0]
    dense = (cd.drone_dense if system == "drone" else cd.car_dense)(const, samples, uk, x_eff, arg=arg.astype(np.int64))
    nw = 2 * (S - 1)
    cols = dense["G_arg"].reshape(M, S, n_u)[:, :S - 1, :2].reshape(M, nw)
    ref = tp.cut_sums(cols[:, None, :], dense["g_arg"][:, None], w, np.zeros(M, dtype=np.int64), m32 == np.float32(thr), lam)
    tol_grad, tol_off = tp.rollout_tolerance(ref)
    sums = rec[stats.N_STATS:]
    e_grad, e_off = np.abs(sums[:nw] - ref["grad"]), abs(sums[nw] - ref["off"])
    assert np.all(e_grad <= tol_grad) and e_off <= tol_off, (float(np.max(e_grad / tol_grad)), e_off / tol_off)
    _report(f"one-call round trip {system} S={S} ({'by value' if by_value else 'device memory'})", spread, max(worst),
            f"; cut gradient err/bound {float(np.max(e_grad / tol_grad)):.3f}, offset {e_off / tol_off:.3f}")


# ---- rato_drone_rowmax_implicit ------------------------------------------------------------------------------------------
def _implicit_launch(d, p, mass, A22, axes, W, base, sign, xs, M, n):
    from riskaversetrajopt_amd import _lib
    import torch
    m, a = _sentinels(n, d.device)
    _lib.check(d._lib.rato_drone_rowmax_implicit(C.byref(p), _ptr(mass), _ptr(A22), axes, _ptr(W), _ptr(base), sign, _ptr(xs), _ptr(m),
                                                 _ptr(a), _lib.current_stream()), "rato_drone_rowmax_implicit")
    torch.cuda.synchronize()
    assert _untouched(m, a, M), "an index >= M was written"
    return m[:M].cpu().numpy(), a[:M].cpu().numpy()


IMPLICIT_S = (1, 7, 8, 9, 16, 17)


@pytest.mark.parametrize("S", IMPLICIT_S)
def test_implicit_rowmax_on_exact_tables(S):
    """a21 = 0, a22 = 1 in either layout, dyadic dt and masses, small integers: m is the float of an integer and every tie an
    exact one -- the last row of group 0 against the first of group 1, all rows equal, a maximum that only the final
    partial batch of 8 reaches, a tie the loop meets in the other order than the row index"""
    import torch
    from riskaversetrajopt_amd import drone_risk
    d = drone_risk.Model(S, None, None, None, 'saa', 0.2)
    for axes in (2, 3):
        for sign in (1.0, -1.0):
            des = cd.implicit_design(S, axes, sign)
            p = d._params(des.M, des.ld)
            p.dt, p.dt64, p.kp, p.kp64 = cd.IMPLICIT_DT, cd.IMPLICIT_DT, 0.0, 0.0
            t = lambda a: torch.as_tensor(a, device=d.device).contiguous()
            m, a = _implicit_launch(d, p, t(des.mass), t(des.A22), axes, t(des.W), t(des.base), sign, _f64(des.xs, d.device), des.M,
                                    des.ld + PAD)
            assert np.array_equal(m.view(np.int32), des.m.astype(np.float32).view(np.int32)), (axes, sign, m, des.m, des.kind)
            assert np.array_equal(a, des.arg), (axes, sign, a, des.arg, des.kind)


@pytest.mark.parametrize("S", IMPLICIT_S)
def test_implicit_rowmax_on_real_tables(S):
    """the tables of rato_drone_linearize_generators (a22_axes 3: 1 - a22) and the same numbers as a22 (a22_axes 2), base = g
    with sign +1 and base = g_up with sign -1: against the recursion on the device's own fp32 tables in fp64 (what is left is
    fp64 rounding and the final rounding of m) and against the fp64 oracle's dense rows under the bound the table form has in
    tests/test_gpu_scp.py (2e-4 of the rows' scale: the tables are fp32)"""
    import torch
    from oracle import drone as od
    from riskaversetrajopt_amd import drone_risk
    M = 257
    samples = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S)]
    const = cd.drone_const(S)
    d = drone_risk.Model(S, *samples, 'saa', 0.2)
    uk = cd.r32(tp.graze(S))
    x = 0.3 * np.random.RandomState(4).randn(S, 3)
    mass = d._inputs(None)[1]
    ld = mass.numel()
    p = d._params(M, ld)
    assert (p.dt64, p.kp64) == (const.dt, const.kp)
    worst_t, worst_o, spreads = [], [], []
    rows_o = cd.drone_dense(const, samples, uk, x)["rows"].reshape(M, -1)         # g + G x = G (u_k + x) - g_up
    for sign, rows_out, xs in ((1.0, 1, x), (-1.0, 0, uk + x)):
        gen = d.linearize_generators_device(uk, rows_out=rows_out)
        e22 = gen["_A22"]
        tables = {3: e22, 2: (1.0 - e22.double()).float()[:, :2].contiguous()}
        for axes, A22 in tables.items():
            m, a = _implicit_launch(d, p, mass, A22, axes, gen["_W"], gen["_g_up"], sign, _f64(xs, d.device), M, M)
            args = (A22.cpu().numpy(), axes, gen["_W"].cpu().numpy(), gen["_g_up"].cpu().numpy(), mass.cpu().numpy(), xs, sign,
                    p.dt64, p.kp64, M)
            r64 = cd.implicit_rows(*args).reshape(M, -1)
            spread = float(np.abs(r64 - cd.implicit_rows(*args, dtype=np.longdouble).reshape(M, -1).astype(np.float64)).max())
            spreads.append(spread)
            _check_against_rows(f"implicit S={S} axes={axes} sign={sign}", m, a, r64, spread, worst_t)
            scale = max(1.0, np.abs(rows_o).max())
            err = np.abs(m.astype(np.float64) - rows_o.max(axis=1)).max()
            worst_o.append(err / (2e-4 * scale))
            assert err < 2e-4 * scale
            clear = (np.sort(rows_o, axis=1)[:, -1] - np.sort(rows_o, axis=1)[:, -2]) > 1e-3 * scale if 3 * S > 1 else np.ones(M, bool)
            assert np.array_equal(a[clear], rows_o.argmax(axis=1)[clear])
    _report(f"implicit rowmax on real tables S={S}", max(spreads), max(worst_t), f"; against the oracle (2e-4 scale): {max(worst_o):.3f}")


# ---- rato_drone_linearize_generators -----------------------------------------------------------------------------------
GEN_M = (1, 5, 255, 256, 257)
GEN_S = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 80, 81)
# what tests/test_gpu_scp.py already holds the same quantities to (rtol, atol): the derived bound may only be tighter
GEN_EXISTING = {"g": (1e-6, 5e-6), "g_up": (5e-5, 2e-4), "Z": (1e-6, 1e-6)}


class _Generators:
    def __init__(self, S, M, samples):
        from riskaversetrajopt_amd import drone_risk
        self.d = drone_risk.Model(S, *[a[:M] for a in samples], 'saa', 0.2)
        self.S, self.M = S, M
        self.dW, self.mass, self.Qsym, _ = self.d._inputs(None)
        self.ld = self.mass.numel()
        self.nblk = (M + 255) // 256

    def launch(self, us, tables, want_z, rows_out=0):
        """-> (status, dict of NaN-prefilled buffers as the kernel left them)"""
        import torch
        from riskaversetrajopt_amd import _lib
        S, ld, dev = self.S, self.ld, self.d.device
        nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
        b = {"A22": nan(S, 3, ld), "W": nan(3, S, 2, ld), "g_up": nan(3, S, ld), "Z": nan(ld), "part": nan(self.nblk, 6 * S + 6)}
        p = self.d._params(self.M, ld, rows_out)
        rc = self.d._lib.rato_drone_linearize_generators(
            C.byref(p), _ptr(self.d._us_device(us)), _ptr(self.dW), _ptr(self.mass), _ptr(self.Qsym), _ptr(b["A22"]),
            _ptr(b["W"] if tables else None), _ptr(b["g_up"] if tables else None), _ptr(b["Z"] if want_z else None), _ptr(b["part"]),
            _lib.current_stream())
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in b.items()}, p


def _gen_reference(S, samples, us):
    """the oracle's quantities per sample, the spreads against the long-double recursion and the effect of the e22 rounding"""
    const = cd.drone_const(S)
    M = samples[0].shape[0]
    ref = cd.drone_dense(const, samples, us, chunk=max(1, min(257, 300000 // (S * S))))
    ld = cd.drone_direct(const, samples, us, dtype=np.longdouble)
    a, b = cd.drone_direct(const, samples, us), cd.drone_direct(const, samples, us, round_e22=True)
    return const, ref, ld, {k: np.abs(a[k] - b[k]) for k in ("g_up", "fdu", "rhs")}


def _gen_check(what, dev, ref, spread, extra, worst, existing=None):
    limit = cd.once_rounded_bound(ref, spread, 2.0 * extra)
    if existing is not None:
        limit = np.minimum(limit, existing[1] + existing[0] * np.abs(ref))
    err = np.abs(dev.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(limit, 1e-300)))
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert np.all(err <= limit), (what, ratio, float(err.max()), spread, float(np.max(extra)))


def _generators_case(S, Ms, pool):
    from oracle import drone as od
    samples = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=pool, S=S)]
    us = cd.r32(tp.graze(S))                                       # the kernel reads the controls as floats
    const, ref, ld, e22_fx = _gen_reference(S, samples, us)
    sp = {k: float(np.abs(ref[k] - ld[k].astype(np.float64)).max()) for k in ("e22", "W", "g", "g_up", "Z")}
    worst = {}
    for M in Ms:
        gk = _Generators(S, M, samples)
        rc, full, p = gk.launch(us, True, True)
        assert rc == 0 and (p.dt64, p.kp64, p.kd64, p.drag64, p.tol64) == (const.dt, const.kp, const.kd, const.drag, const.tol)
        rc1, rows1, _ = gk.launch(us, True, True, rows_out=1)
        rc2, only_z, _ = gk.launch(us, False, True)
        rc3, neither, _ = gk.launch(us, False, False)
        assert (rc1, rc2, rc3) == (0, 0, 0)
        for name, out, wrote in (("full", full, ("A22", "W", "g_up", "Z")), ("rows_out", rows1, ("A22", "W", "g_up", "Z")),
                                 ("only Z", only_z, ("A22", "Z")), ("neither", neither, ("A22",))):
            for k in ("A22", "W", "g_up", "Z"):
                if k in wrote:                                    # lanes >= M of every row keep their sentinel
                    assert np.isnan(out[k][..., M:]).all() and np.isfinite(out[k][..., :M]).all(), (name, k)
                else:
                    assert np.isnan(out[k]).all(), (name, k)
            assert np.isfinite(out["part"]).all(), name
            # the instantiations without W / g_up (and without Z) leave the same table and bit-identical sample sums
            assert np.array_equal(out["part"].view(np.int32), full["part"].view(np.int32)), name
            assert np.array_equal(out["A22"][..., :M].view(np.int32), full["A22"][..., :M].view(np.int32)), name
            if "Z" in wrote:
                assert np.array_equal(out["Z"][:M].view(np.int32), full["Z"][:M].view(np.int32)), name
        assert np.array_equal(rows1["W"][..., :M].view(np.int32), full["W"][..., :M].view(np.int32))
        _gen_check("e22", full["A22"][..., :M].transpose(2, 0, 1), ref["e22"][:M], sp["e22"], 0.0, worst)
        _gen_check("W", full["W"][..., :M].transpose(3, 0, 1, 2), ref["W"][:M], sp["W"], 0.0, worst)
        _gen_check("g", rows1["g_up"][..., :M].transpose(2, 0, 1), ref["g"][:M], sp["g"], 0.0, worst, GEN_EXISTING["g"])
        _gen_check("g_up", full["g_up"][..., :M].transpose(2, 0, 1), ref["g_up"][:M], sp["g_up"], e22_fx["g_up"][:M], worst, GEN_EXISTING["g_up"])
        _gen_check("Z", full["Z"][:M], ref["Z"][:M], sp["Z"], 0.0, worst, GEN_EXISTING["Z"])
        # every block row of part: the sums over the block's samples of the final-state Jacobian and of the rhs
        blk = lambda v: cd.block_sums(v[:M], M)
        du_ref, du_ld = blk(ref["fdu"]).reshape(gk.nblk, 6 * S), blk(ld["fdu"]).astype(np.float64).reshape(gk.nblk, 6 * S)
        rhs_ref, rhs_ld = blk(ref["rhs"]), blk(ld["rhs"]).astype(np.float64)
        sp["du"], sp["rhs"] = max(sp.get("du", 0.0), float(np.abs(du_ref - du_ld).max())), max(sp.get("rhs", 0.0), float(np.abs(rhs_ref - rhs_ld).max()))
        _gen_check("part: final-state Jacobian", full["part"][:, :6 * S], du_ref, float(np.abs(du_ref - du_ld).max()),
                   blk(e22_fx["fdu"]).reshape(gk.nblk, 6 * S), worst)
        _gen_check("part: rhs", full["part"][:, 6 * S:], rhs_ref, float(np.abs(rhs_ref - rhs_ld).max()), blk(e22_fx["rhs"]), worst)
    for k, v in worst.items():
        key = {"part: final-state Jacobian": "du", "part: rhs": "rhs"}.get(k, k)
        fx = {"g_up": "g_up", "du": "fdu", "rhs": "rhs"}.get(key)
        _report(f"generators S={S} {k}", sp[key], v, f"; e22 term (per sample) {float(e22_fx[fx].max()):.2e}" if fx else "")


@pytest.mark.parametrize("S", GEN_S)
def test_generators_linearization(S):
    _generators_case(S, GEN_M, 257)


def test_generators_linearization_at_the_lds_limit():
    """S = 592 takes 163776 of the 163840 bytes of LDS a workgroup can have; S = 593 (163968) is refused and writes nothing"""
    from oracle import drone as od
    _generators_case(592, (3,), 3)
    S, M = 593, 3
    samples = [cd.r32(a) for a in od.sample_uncertain_parameters(np.random.RandomState(0), 'saa', M=M, S=S)]
    rc, out, _ = _Generators(S, M, samples).launch(cd.r32(tp.graze(S)), True, True)
    assert rc == RATO_EINVAL and all(np.isnan(v).all() for v in out.values())
